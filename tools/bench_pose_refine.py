#!/usr/bin/env python3
"""Time one training batch with learnable poses - the batch and the backward from the rays' gradients to dL/dxi - through
nerfdata.CameraRefiner (RayLoader(cameras=): fsn_pose_compose when xi changed, fsn_ray_batch, fsn_ray_pose_grad;
csrc/pose_refine.hip) against the torch spelling a user writes without it: the index and colours from the plain loader's
launch, then matrix_exp of the skew matrices, a gather of the corrected poses by view, an einsum with the pixel's camera
direction, the NDC map under autograd, and autograd's backward of all that (index_add_ per view: float atomics, not
reproducible).  Shapes: --rays 4096 per batch over 8 and 100 views of --hw 64 x 64 pixels, world and NDC rays.  xi is
changed before every batch, as an optimizer step does.  Device events around batch + backward; the two spellings
alternate run by run, three rounds of --iters runs, the median of each round and the median of those.  There is no pass
or fail on these times.  Appends one JSON line to profiles/bench_pose_refine.jsonl (--out) and prints it.

    timeout -k 10 300 python tools/bench_pose_refine.py [--iters 20] [--warmup 5] [--rays 4096] [--hw 64] [--tag NAME]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--hw", type=int, default=64)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_pose_refine.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fs_nerf_amd  # noqa: F401
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
    rounds = {k: [] for k in variants}
    for _ in range(args.rounds):
        times = {k: [] for k in variants}
        for it in range(args.warmup + args.iters):
            for name, fn in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if it >= args.warmup:
                    times[name].append(a.elapsed_time(b) * 1e3)
        for name in variants:
            rounds[name].append(float(np.median(times[name])))
    out = {"tool": "bench_pose_refine", "tag": args.tag, "device": torch.cuda.get_device_name(0), "rays": B,
           "image": [H, W], "iters": args.iters, "rounds": args.rounds,
           "what": "xi update + batch + backward to dL/dxi, device events, us",
           "variants": {name: {"us_median": round(float(np.median(r)), 2), "us_rounds": [round(x, 2) for x in r]}
                        for name, r in rounds.items()}}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
