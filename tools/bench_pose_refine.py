#!/usr/bin/env python3
"""Time one training batch with learnable poses - the batch and the backward from the rays' gradients to dL/dxi - through
nerfdata.CameraRefiner (RayLoader(cameras=): fsn_pose_compose when xi changed, fsn_ray_batch, fsn_ray_pose_grad;
csrc/pose_refine.hip) against the torch spelling a user writes without it: the index and colours from the plain loader's
launch, then matrix_exp of the skew matrices, a gather of the corrected poses by view, an einsum with the pixel's camera
direction, the NDC map under autograd, and autograd's backward of all that (index_add_ per view: float atomics, not
reproducible).  Shapes: --rays 4096 per batch over 8 and 100 views of --hw 64 x 64 pixels, world and NDC rays.  xi is
changed before every batch, as an optimizer step does.  The timed call is batch + backward.  Schedule: interleaved
(tools/benchlib.py), --rounds 3 rounds, us. There is no pass or fail on these times.  Appends one JSON line to
profiles/bench_pose_refine.jsonl (--out) and prints it.

    timeout -k 10 300 python tools/bench_pose_refine.py [--iters 20] [--warmup 5] [--rays 4096] [--hw 64] [--tag NAME]
"""
import argparse
import os
import sys

import benchlib


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=20, warmup=5, rounds=3, out="bench_pose_refine.jsonl")
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--hw", type=int, default=64)
    args = ap.parse_args()
    import torch
    sys.path.insert(0, os.path.join(benchlib.package(), "tests"))
    from fs_nerf_amd.nerfdata import CameraRefiner, RayDataset, RayLoader
    import pose_refine_ref as PR  # the fixtures' poses
    dev = torch.device("cuda:0")
    H = W = args.hw
    focal, B = 1.1 * W, args.rays
    gen = torch.Generator(device=dev).manual_seed(0)
    co, cd = torch.randn(B, 3, device=dev, generator=gen), torch.randn(B, 3, device=dev, generator=gen)
    pix = torch.arange(H * W, device=dev)
    c_table = torch.stack([((pix % W).float() - W * 0.5) / focal, -((pix // W).float() - H * 0.5) / focal,
                           -torch.ones(H * W, device=dev)], -1)
    c_table = c_table / c_table.norm(dim=-1, keepdim=True)
    sx, sy = -1.0 / (W / (2.0 * focal)), -1.0 / (H / (2.0 * focal))

    def case(n_views, ndc):
        imgs = torch.zeros(n_views, H, W, 3, dtype=torch.uint8)
        poses = PR.forward_poses(n_views, 1) if ndc else PR.world_poses(n_views, 1)
        ds = RayDataset(imgs, poses, (H, W, focal), near=0.0 if ndc else 2.0, far=1.0 if ndc else 6.0, ndc=ndc, device=dev)
        cam = CameraRefiner(ds)
        xi_t = torch.zeros(n_views, 6, device=dev, requires_grad=True)
        P0 = ds.poses12.view(-1, 3, 4)
        step = 1e-4 * torch.randn(n_views, 6, device=dev, generator=gen)
        state = {"kernel": None, "torch": None}
        loaders = {"kernel": RayLoader(ds, B, seed=0, cameras=cam), "torch": RayLoader(ds, B, seed=0, with_index=True)}

        def batch(which):
            try:
                return next(state[which])
            except (StopIteration, TypeError):
                state[which] = iter(loaders[which])
                return next(state[which])

        def kernel():
            with torch.no_grad():
                cam.xi.add_(step)
            o, d, _ = batch("kernel")
            return torch.autograd.grad([o, d], [cam.xi], [co[:o.shape[0]], cd[:o.shape[0]]])[0]

        def spelled():
            with torch.no_grad():
                xi_t.add_(step)
            _, _, _, index = ds.batch("permuted", start=0, count=B, seed=0, epoch=0, want_rays=False, want_index=True)
            view, p = index // (H * W), index % (H * W)
            R = torch.linalg.matrix_exp(PR.skew(xi_t[:, :3])) @ P0[:, :, :3]
            t = P0[:, :, 3] + xi_t[:, 3:]
            d = torch.einsum("bij,bj->bi", R[view], c_table[p])
            o = t[view]
            if ndc:
                tt = -(1.0 + o[:, 2]) / d[:, 2]
                q = o + tt[:, None] * d
                o, d = (torch.stack([sx * q[:, 0] / q[:, 2], sy * q[:, 1] / q[:, 2], 1.0 + 2.0 / q[:, 2]], -1),
                        torch.stack([sx * (d[:, 0] / d[:, 2] - q[:, 0] / q[:, 2]), sy * (d[:, 1] / d[:, 2] - q[:, 1] / q[:, 2]),
                                     -2.0 / q[:, 2]], -1))
            return torch.autograd.grad([o, d], [xi_t], [co, cd])[0]

        return {"kernel": kernel, "torch": spelled}

    cases = {f"{'ndc' if ndc else 'world'}_{n}views": case(n, ndc) for n in (8, 100) for ndc in (False, True)}
    variants = {f"{c}_{which}": fn for c, fns in cases.items() for which, fn in fns.items()}
    rounds = benchlib.interleaved(variants, args.iters, args.warmup, args.rounds)
    out = {**benchlib.header("bench_pose_refine", args.tag), "rays": B,
           "image": [H, W], "iters": args.iters, "rounds": args.rounds,
           "what": "xi update + batch + backward to dL/dxi, device events, us",
           "variants": {name: benchlib.rounds_summary(r, "us") for name, r in rounds.items()}}
    benchlib.emit(out, args.out)


if __name__ == "__main__":
    main()
