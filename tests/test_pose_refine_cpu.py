"""CPU: the learnable-pose layer's C-ABI (declared, bound, exported; argument validation without a device), pose_error,
and the float64 reference of tests/pose_refine_ref.py recovering a known correction (the bound the GPU test holds the
loaders to)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L

import pose_refine_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fsn_pose_compose", "fsn_ray_pose_grad")


def test_the_two_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "fsnerf_hip.h")).read()
    lib = L.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    from fs_nerf_amd import nerfdata, ops
    assert callable(ops.pose_compose) and callable(ops.ray_pose_grad)
    assert nerfdata.CameraRefiner is not None and callable(nerfdata.pose_error)


def test_argument_validation_without_gpu():
    lib = L.lib()
    p = C.c_void_p(64)  # never dereferenced: every call below is refused (or is empty) before any HIP call
    assert lib.fsn_pose_compose(None, p, 3, p, None) == -1 and b"fsn_pose_compose" in lib.fsn_last_error()
    assert lib.fsn_pose_compose(p, None, 3, p, None) == -1
    assert lib.fsn_pose_compose(p, p, 3, None, None) == -1
    assert lib.fsn_pose_compose(p, p, -1, p, None) == -1
    assert lib.fsn_pose_compose(p, p, 0, p, None) == 0  # no view: nothing to do

    def grad(poses0=p, xi=p, n=3, H=8, W=8, focal=10.0, index=p, count=5, grad_xi=p):
        return lib.fsn_ray_pose_grad(poses0, xi, n, H, W, focal, 0, 1.0, index, p, p, count, grad_xi, None, None)

    assert grad(poses0=None) == -1 and b"fsn_ray_pose_grad" in lib.fsn_last_error()
    assert grad(xi=None) == -1
    assert grad(grad_xi=None) == -1
    assert grad(index=None) == -1
    assert grad(n=-1) == -1
    assert grad(H=0) == -1 and grad(H=-4) == -1 and grad(W=0) == -1
    assert grad(focal=0.0) == -1
    assert grad(count=-1) == -1
    assert grad(H=1 << 16, W=1 << 16) == -2  # a view of 2^32 pixels: refused by name
    assert grad(n=0) == 0  # no view: nothing to write


def exact_poses(n, seed):
    """[n,4,4] float64 with rotations orthonormal to float64 rounding (world_poses rounds its own to float32)."""
    rng = np.random.default_rng(seed)
    out = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1)
    out[:, :3, :3] = torch.from_numpy(PR.random_rotations(n, rng))
    out[:, :3, 3] = 4.0 * out[:, :3, 2]
    return out


def similarity(rng):
    Rg = torch.from_numpy(PR.random_rotations(1, rng)[0])
    return float(rng.uniform(0.5, 2.0)), Rg, torch.from_numpy(rng.standard_normal(3))


def test_pose_error_is_zero_for_poses_moved_by_a_similarity_transform():
    from fs_nerf_amd.nerfdata import pose_error
    rng = np.random.default_rng(0)
    for n in (3, 8, 30):
        truth = exact_poses(n, seed=n)
        s, Rg, tg = similarity(rng)
        moved = truth.clone()
        moved[:, :3, :3] = Rg @ truth[:, :3, :3]
        moved[:, :3, 3] = s * (truth[:, :3, 3] @ Rg.T) + tg
        rot, trans = pose_error(moved, truth)
        assert rot.shape == trans.shape == (n,) and rot.dtype == trans.dtype == torch.float64
        assert float(rot.abs().max()) <= 1e-9 and float(trans.abs().max()) <= 1e-9, (n, rot, trans)
        rot, trans = pose_error(moved[:, :3], truth.float())  # [n,3,4] and float32 inputs are taken too
        assert float(rot.abs().max()) <= 1e-4 and float(trans.abs().max()) <= 1e-5


@pytest.mark.parametrize("angle_deg", [1e-3, 0.5, 30.0, 170.0])
def test_pose_error_returns_the_injected_angle(angle_deg):
    from fs_nerf_amd.nerfdata import pose_error
    rng = np.random.default_rng(1)
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    E = torch.linalg.matrix_exp(PR.skew(torch.from_numpy(axis * math.radians(angle_deg))))
    # one camera alone: its centre fixes the translation only
    truth = exact_poses(1, seed=2)
    turned = truth.clone()
    turned[0, :3, :3] = E @ truth[0, :3, :3]
    rot, trans = pose_error(turned, truth)
    assert abs(float(rot[0]) - angle_deg) <= 1e-9 * max(1.0, angle_deg) and float(trans[0]) <= 1e-12
    # one camera of five turned in place: the centres align by the identity, the others stay at 0
    truth = exact_poses(5, seed=3)
    turned = truth.clone()
    turned[2, :3, :3] = E @ truth[2, :3, :3]
    rot, trans = pose_error(turned, truth)
    assert abs(float(rot[2]) - angle_deg) <= 1e-9 * max(1.0, angle_deg)
    assert float(rot[[0, 1, 3, 4]].abs().max()) <= 1e-9 and float(trans.abs().max()) <= 1e-9


# ---------------------------------------------------------------- recovery: the geometry of the GPU test
REC_H, REC_W, REC_FOCAL, REC_VIEWS, REC_STEPS, REC_BOUND = 8, 8, 10.0, 3, 300, 1e-3


def recovery_case(ndc):
    """(stored poses [3,4,4] float32, xi* [3,6] float64 with entries ~0.1, all ray indices)."""
    rng = np.random.default_rng(11 if ndc else 12)
    poses = PR.forward_poses(REC_VIEWS, seed=5) if ndc else PR.world_poses(REC_VIEWS, seed=5)
    return poses, torch.from_numpy(rng.standard_normal((REC_VIEWS, 6)) * 0.1), torch.arange(REC_VIEWS * REC_H * REC_W)


def ray_loss(o, d, to, td):
    return ((o - to) ** 2).sum() + ((d - td) ** 2).sum()


@pytest.mark.parametrize("ndc", [False, True])
def test_the_float64_reference_recovers_the_correction(ndc):
    poses, xi_star, index = recovery_case(ndc)
    P0 = PR.poses12(poses).double()
    if ndc:  # the fixture's promise: the NDC map stays far from its singular set
        o, d = PR.rays(PR.compose(P0, xi_star), index, REC_H, REC_W, REC_FOCAL, False)
        assert float(d[:, 2].abs().min()) > 0.5
    to, td = PR.rays(PR.compose(P0, xi_star), index, REC_H, REC_W, REC_FOCAL, ndc)
    xi = PR.recover(lambda x: ray_loss(*PR.rays(PR.compose(P0, x), index, REC_H, REC_W, REC_FOCAL, ndc), to, td),
                    torch.zeros(REC_VIEWS, 6, dtype=torch.float64), REC_STEPS)
    ratio = float((xi - xi_star).abs().max() / xi_star.abs().max())
    print(f"float64 reference, ndc={ndc}: max |xi - xi*| = {ratio:.2e} x its initial value after {REC_STEPS} steps")
    assert ratio <= REC_BOUND, ratio
