#!/usr/bin/env python3
"""Time one next() of nerfdata.UnseenPatchLoader (fsn_unseen_patch_batch, csrc/unseen_views.hip: ONE launch from a step
counter to the rays of --patches 64 patches of --patch 32 x 32 on --hw 800 x 800 intrinsics) against the torch spelling
a user writes without it, as examples/train_synthetic.py did: random numbers from torch.rand on the device, the shell
point and the look-at with torch ops, utilities.get_rays of the whole frame per pose (its pose goes through the host, as
get_rays takes it), and the windows sliced out with index tensors.  Both serve the same distribution (fitted to eight
orbit cameras), not the same random numbers.  --poses-per-batch: 1 and 8 poses shared by the batch's patches.  Schedule:
interleaved (tools/benchlib.py), --rounds 3 rounds, us. There is no pass or fail on these times.  Appends one JSON line
to profiles/bench_unseen.jsonl (--out) and prints it.

    timeout -k 10 300 python tools/bench_unseen.py [--iters 20] [--warmup 5] [--patches 64] [--patch 32] [--hw 800] [--tag NAME]
"""
import argparse
import math

import benchlib


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=20, warmup=5, rounds=3, out="bench_unseen.jsonl")
    ap.add_argument("--patches", type=int, default=64)
    ap.add_argument("--patch", type=int, default=32)
    ap.add_argument("--hw", type=int, default=800)
    args = ap.parse_args()
    import torch
    benchlib.package()
    from fs_nerf_amd.nerfdata import UnseenPatchLoader, UnseenViewSampler
    from fs_nerf_amd.utils import utilities as U
    from oracle import fsnerf_oracle as O
    dev = torch.device("cuda:0")
    H = W = args.hw
    hwf = (H, W, 0.5 * W / math.tan(0.5 * 0.6911112))
    B, P = args.patches, args.patch
    train_poses = torch.stack([O.pose_from_spherical(4.0311289, 50.0, float(phi)) for phi in range(0, 360, 45)])
    sampler = UnseenViewSampler.from_poses(train_poses, "shell", device=dev)
    ds = sampler.dist
    centre, up = torch.tensor(list(ds.centre), device=dev), torch.tensor(list(ds.up), device=dev)
    e1, e2 = torch.tensor(list(ds.e1), device=dev), torch.tensor(list(ds.e2), device=dev)
    focus = torch.tensor(list(ds.focus), device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    window = torch.arange(P, device=dev)

    def torch_batch(n_poses):
        u = torch.rand(n_poses, 6, device=dev, generator=gen)
        z = ds.z_lo + u[:, 0] * (ds.z_hi - ds.z_lo)
        r = ds.r_lo + u[:, 1] * (ds.r_hi - ds.r_lo)
        phi, h = 2.0 * math.pi * u[:, 2], torch.sqrt(1.0 - z * z)
        origin = centre + r[:, None] * ((h * torch.cos(phi))[:, None] * e1 + (h * torch.sin(phi))[:, None] * e2 + z[:, None] * up)
        target = focus + ds.jitter * (2.0 * u[:, 3:] - 1.0)
        zc = torch.nn.functional.normalize(origin - target, dim=-1)
        xc = torch.nn.functional.normalize(torch.linalg.cross(up.expand_as(zc), zc), dim=-1)
        yc = torch.linalg.cross(zc, xc)
        poses = torch.stack([xc, yc, zc, origin], dim=-1)  # [n,3,4]
        corner = torch.randint(0, H - P + 1, (B, 2), device=dev, generator=gen)
        rows = (corner[:, :1] + window)[:, :, None].expand(-1, -1, P)
        cols = (corner[:, 1:] + window)[:, None, :].expand(-1, P, -1)
        per = B // n_poses
        os_, ds_ = [], []
        for k in range(n_poses):
            o, d = U.get_rays(poses[k], hwf, dev)
            os_.append(o[rows[k * per:(k + 1) * per], cols[k * per:(k + 1) * per]].reshape(-1, 3))
            ds_.append(d[rows[k * per:(k + 1) * per], cols[k * per:(k + 1) * per]].reshape(-1, 3))
        return torch.cat(os_), torch.cat(ds_)

    variants = {}
    for n_poses in (1, 8):
        loader = UnseenPatchLoader(sampler, hwf, P, B, patches_per_pose=B // n_poses, seed=0)
        variants[f"{n_poses}pose_kernel"] = loader.next
        variants[f"{n_poses}pose_torch"] = (lambda n: lambda: torch_batch(n))(n_poses)
    for name, fn in variants.items():  # both spellings serve B * P * P rays
        o, d = fn()
        assert o.shape == d.shape == (B * P * P, 3) and bool(torch.isfinite(o).all()) and bool(torch.isfinite(d).all()), name
    rounds = benchlib.interleaved(variants, args.iters, args.warmup, args.rounds)
    out = {**benchlib.header("bench_unseen", args.tag), "patches": [B, P, P],
           "image": [H, W], "iters": args.iters, "rounds": args.rounds,
           "what": "one batch of unseen-view patch rays (rays_o, rays_d), device events with the host path, us",
           "variants": {name: benchlib.rounds_summary(r, "us") for name, r in rounds.items()}}
    benchlib.emit(out, args.out)


if __name__ == "__main__":
    main()
