#!/usr/bin/env python3
"""Time forward + backward of the depth-warp consistency term (core.loss.WarpConsistencyLoss over nerfdata.WarpSource:
csrc/warp.hip, one launch each way over the resident uint8 images) against the torch spelling a user writes today: float
copies of the images (here 12 bytes per pixel beside the dataset's 4), the projection as torch ops, one
F.grid_sample(align_corners=True) over the view stack (the view index as the third grid coordinate, so that rays with
different source views share one call without a host synchronisation), the same masked mean, autograd. Shapes: --views 8
views of --hw 800 x 800 RGBA bytes on an orbit; --rays 4096 scattered rays (random pixels of random views, depth 4 +-
0.5) and --patches 64 patches of --patch 32 x 32, each against the view nearest to its own. The timed call is loss +
backward to the depth.  Schedule: interleaved (tools/benchlib.py), --rounds 3 rounds, us.  There is no pass or fail on
these times.  Appends one JSON line to profiles/bench_warp.jsonl (--out) and prints it.

    timeout -k 10 300 python tools/bench_warp.py [--iters 20] [--warmup 5] [--tag NAME]
"""
import argparse
import math

import benchlib


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=20, warmup=5, rounds=3, out="bench_warp.jsonl")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--patches", type=int, default=64)
    ap.add_argument("--patch", type=int, default=32)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    benchlib.package()
    from fs_nerf_amd.core.loss import WarpConsistencyLoss
    from fs_nerf_amd.nerfdata import RayDataset, WarpSource
    dev = torch.device("cuda:0")
    V, H, W = args.views, args.hw, args.hw
    focal = 0.5 * W / math.tan(0.5 * 0.6911112)
    gen = torch.Generator(device=dev).manual_seed(0)
    images = torch.randint(0, 256, (V, H, W, 4), device=dev, dtype=torch.uint8, generator=gen)
    poses = torch.zeros(V, 4, 4)
    for i in range(V):  # an orbit of radius 4 around the origin, the cameras looking at it (down their own -z, z up)
        a = 2.0 * math.pi * i / V
        c = torch.tensor([4.0 * math.cos(a), 4.0 * math.sin(a), 1.0])
        zc = c / c.norm()
        xc = torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0]), zc)
        xc = xc / xc.norm()
        poses[i, :3, :3] = torch.stack([xc, torch.linalg.cross(zc, xc), zc], 1)
        poses[i, :3, 3], poses[i, 3, 3] = c, 1.0
    ds = RayDataset.blender(images, poses, (H, W, focal), white_bkgd=True, device=dev)
    source = WarpSource(ds)
    loss = WarpConsistencyLoss("l1", border=0.5)
    border, z_min = 0.5, 1e-3
    # the torch spelling's float tables [1,3,V,H,W] and cameras
    rgba = images.float() / 255.0
    table = (rgba[..., :3] * rgba[..., 3:] + (1.0 - rgba[..., 3:])).permute(3, 0, 1, 2)[None].contiguous()
    c2w = ds.poses12.view(V, 3, 4)

    def torch_loss(rgb, depth, o, d, s):
        X = o + depth[:, None] * d
        cam = torch.einsum("nkj,nk->nj", c2w[s, :, :3], X - c2w[s, :, 3])
        z = -cam[:, 2]
        u = W * 0.5 + focal * cam[:, 0] / z
        v = H * 0.5 - focal * cam[:, 1] / z
        valid = (torch.isfinite(depth) & (depth > 0) & (z >= z_min) & (u >= border) & (u <= W - 1 - border) & (v >= border)
                 & (v <= H - 1 - border))
        grid = torch.stack([2.0 * u / (W - 1) - 1.0, 2.0 * v / (H - 1) - 1.0, 2.0 * s.float() / max(V - 1, 1) - 1.0], -1)
        colour = F.grid_sample(table, grid.view(1, 1, 1, -1, 3), mode="bilinear", padding_mode="border",
                               align_corners=True)[0, :, 0, 0, :].T
        per_row = (rgb - colour).abs().mean(dim=1)
        return torch.where(valid, per_row, torch.zeros_like(per_row)).sum() / valid.sum().clamp(min=1).to(per_row.dtype)

    def batch(o, d, index):
        n = o.shape[0]
        view = torch.div(index, H * W, rounding_mode="floor")
        depth = (3.5 + torch.rand(n, device=dev, generator=gen)).requires_grad_(True)
        return torch.rand(n, 3, device=dev, generator=gen), depth, o, d, source.other_views(1)[view, 0]

    o, d, _, index = ds.batch("permuted", start=0, count=args.rays, seed=1, want_rgb=False, want_index=True)
    rays = batch(o, d, index)
    o, d, _, index = ds.patch_batch("permuted", args.patch, start=0, count=args.patches, seed=2, want_rgb=False, want_index=True)
    patches = batch(o, d, index)
    variants = {
        "rays_kernel": (lambda: loss(*rays, source), rays[1]),
        "rays_torch": (lambda: torch_loss(*rays), rays[1]),
        "patches_kernel": (lambda: loss(*patches, source), patches[1]),
        "patches_torch": (lambda: torch_loss(*patches), patches[1]),
    }
    agree, valid_rows = {}, {}
    for name, b in (("rays", rays), ("patches", patches)):  # the two spellings compute the same loss
        x, y = float(variants[name + "_kernel"][0]().detach()), float(variants[name + "_torch"][0]().detach())
        agree[name] = abs(x - y) / max(abs(y), 1e-12)
        valid_rows[name] = int(source.sample(b[2], b[3], b[1].detach(), b[4], border=border)[1].sum())
    rounds = benchlib.interleaved({name: (lambda fn=fn, leaf=leaf: torch.autograd.grad(fn(), leaf))
                                   for name, (fn, leaf) in variants.items()}, args.iters, args.warmup, args.rounds)
    out = {**benchlib.header("bench_warp", args.tag), "views": [V, H, W, 4],
           "rays": args.rays, "patches": [args.patches, args.patch, args.patch], "valid_rows": valid_rows,
           "iters": args.iters, "rounds": args.rounds, "what": "loss forward + backward to the depth, device events, us",
           "float_table_bytes": table.numel() * 4, "uint8_image_bytes": images.numel(),
           "relative_difference_of_the_two_spellings": agree,
           "variants": {name: benchlib.rounds_summary(r, "us") for name, r in rounds.items()}}
    benchlib.emit(out, args.out)


if __name__ == "__main__":
    main()
