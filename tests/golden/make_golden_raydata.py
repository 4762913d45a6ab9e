#!/usr/bin/env python3
"""Generate tests/golden/g8_raydata.npz by IMPORTING the reference's LLFFDataset (as make_golden.py does; nothing of it
is copied): what the reference's data layer holds for a tiny forward-facing scene.

    python tests/golden/make_golden_raydata.py        (build container only: needs the reference)

Contents (data only):
  imgs                 uint8 [3, 6, 8, 3], seeded; every byte value is not needed here (tests/test_raydata_gpu.py covers
                       all 256 against the restated arithmetic), the bytes go through the reference's own path:
                       `/ 255.0` in float64 as its image reader's caller does, then torch.tensor(..., float32)
  poses                float32 [3, 4, 4]: rotations a few degrees off identity, small translations (forward facing: no
                       NDC ray comes near the singular set d_z = 0 documented in tests/test_gpu_parity.py)
  hwf                  (6, 8, focal), min_bound, max_bound
  ndc1_* / ndc0_*      for ndc True / False: rays_o, rays_d, rgb [144, 3], aabb [6], near, far of the constructed dataset

The reference's modules import `imageio` and `nerfacc`, which this container does not have; empty placeholder modules
stand in for them at import time (neither is reached by LLFFDataset)."""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def main():
    sys.path.insert(0, REF)
    placeholders = {}
    for name in ("nerfacc", "nerfacc.volrend", "nerfacc.estimators", "nerfacc.estimators.occ_grid", "imageio"):
        m = types.ModuleType(name)
        m.rendering = m.OccGridEstimator = None
        placeholders[name] = m
    sys.modules.update(placeholders)
    try:
        from nerfdata.datasets.llff import LLFFDataset
    finally:
        for name in placeholders:
            sys.modules.pop(name, None)
    torch.set_num_threads(1)
    rng = np.random.default_rng(8)
    n, H, W, focal = 3, 6, 8, 7.5
    imgs = rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    poses = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    deg = math.pi / 180.0
    for k, (ang, t) in enumerate((((2.0, -3.0, 1.0), (0.10, -0.05, 0.02)), ((-4.0, 1.5, -2.0), (-0.12, 0.08, -0.03)),
                                  ((1.0, 5.0, 3.0), (0.03, 0.11, 0.05)))):
        poses[k, :3, :3] = rot(*(a * deg for a in ang)).astype(np.float32)
        poses[k, :3, 3] = t
    min_bound, max_bound = 1.25, 9.5
    out = {"imgs": imgs, "poses": poses, "hwf": np.array([H, W, focal], dtype=np.float64),
           "min_bound": np.float64(min_bound), "max_bound": np.float64(max_bound)}
    for ndc in (True, False):
        ds = LLFFDataset(imgs / 255.0, poses, min_bound, max_bound, (H, W, focal), False, False, ndc)
        assert len(ds) == n * H * W and torch.equal(ds[5][2], ds.rgb[5])
        tag = f"ndc{int(ndc)}_"
        out[tag + "rays_o"] = ds.rays_o.contiguous().numpy()
        out[tag + "rays_d"] = ds.rays_d.contiguous().numpy()
        out[tag + "rgb"] = ds.rgb.contiguous().numpy()
        out[tag + "aabb"] = ds.aabb.numpy()
        out[tag + "near"], out[tag + "far"] = np.float64(ds.near), np.float64(ds.far)
        assert np.isfinite(out[tag + "rays_o"]).all() and np.isfinite(out[tag + "rays_d"]).all()
        if ndc:
            assert np.abs(out[tag + "rays_d"][:, 2]).min() > 0.1  # far from d_z = 0
    path = os.path.join(HERE, "g8_raydata.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
