#!/usr/bin/env python3
"""Time the monocular-depth-prior feature against the torch spelling a user writes without it.

  ssi_kernel / ssi_torch      loss + backward of core.loss.ScaleShiftDepthLoss on --patches 64 patches of --patch 32 x 32
                              (a tenth of the prior NaN) against batched float32 sums with the closed-form (s, t) inside
                              autograd
  rank_kernel / rank_torch    the same for core.loss.DepthRankingLoss against a [B, N, N] broadcast of all pairs
  aux_loader / index_gather   one PatchLoader next() with with_aux=True against with_index=True plus one torch gather
                              from a float table (the LLFF few-shot shape 8 x 378 x 504, --patches patches of --patch)

Schedule: interleaved (tools/benchlib.py), --rounds 3 rounds, us.  There is no pass or fail on these times.  Appends one
JSON line to profiles/bench_depth_prior.jsonl (--out) and prints it.

    timeout -k 10 300 python tools/bench_depth_prior.py [--iters 20] [--warmup 5] [--patches 64] [--patch 32] [--tag NAME]
"""
import argparse

import benchlib


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=20, warmup=5, rounds=3, out="bench_depth_prior.jsonl")
    ap.add_argument("--patches", type=int, default=64)
    ap.add_argument("--patch", type=int, default=32)
    args = ap.parse_args()
    import torch
    benchlib.package()
    from fs_nerf_amd.core.loss import DepthRankingLoss, ScaleShiftDepthLoss
    from fs_nerf_amd.nerfdata import PatchLoader, RayDataset
    dev = torch.device("cuda:0")
    B, P = args.patches, args.patch
    gen = torch.Generator(device=dev).manual_seed(0)
    depth = (2.0 + 4.0 * torch.rand(B, P, P, device=dev, generator=gen)).requires_grad_(True)
    prior = 0.7 * (depth.detach() + 2.0 * torch.rand(B, P, P, device=dev, generator=gen)) - 1.3
    prior = torch.where(torch.rand(B, P, P, device=dev, generator=gen) < 0.1, torch.full_like(prior, float("nan")), prior)
    ssi, rank = ScaleShiftDepthLoss(), DepthRankingLoss(margin=1e-4)

    def torch_ssi():
        ok = torch.isfinite(prior) & torch.isfinite(depth)
        w = ok.float()
        x, p = torch.where(ok, depth, torch.ones_like(depth)), torch.where(ok, prior, torch.zeros_like(prior))
        M = w.sum((1, 2)).clamp(min=1.0)
        mx, mp = (w * x).sum((1, 2)) / M, (w * p).sum((1, 2)) / M
        dx, dp = x - mx[:, None, None], p - mp[:, None, None]
        vx, cxp = (w * dx * dx).sum((1, 2)) / M, (w * dx * dp).sum((1, 2)) / M
        deg = (ok.sum((1, 2)) < 2) | ~(vx > 1e-10 * mx * mx)
        s = cxp / torch.where(deg, torch.ones_like(vx), vx)
        r = s[:, None, None] * dx - dp
        L = torch.where(deg, torch.zeros_like(vx), (w * r * r).sum((1, 2)) / M)
        return L.sum() / (~deg).sum().clamp(min=1)

    def torch_rank():
        ok = (torch.isfinite(prior) & torch.isfinite(depth)).reshape(B, -1)
        d, p = depth.reshape(B, -1), torch.where(ok, prior.reshape(B, -1), torch.zeros_like(ok, dtype=prior.dtype))
        ranked = (p[:, :, None] < p[:, None, :]) & ok[:, :, None] & ok[:, None, :]
        hinge = (d[:, :, None] - d[:, None, :] + 1e-4).clamp(min=0.0)
        return (hinge * ranked).sum() / ranked.sum().clamp(min=1)

    # the loaders: the prior as an aux plane, against the index and one gather from a float table
    n, H, W = 8, 378, 504
    imgs = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    table = torch.rand(n, H, W, 1, generator=torch.Generator().manual_seed(2))
    poses = torch.eye(4).repeat(n, 1, 1)
    ds = RayDataset(imgs, poses, (H, W, 407.6), near=2.0, far=6.0, device=dev, aux=table)
    flat = ds.aux.reshape(-1, 1)
    aux_it = iter(PatchLoader(ds, P, B, shuffle=True, seed=3, with_aux=True))
    idx_it = iter(PatchLoader(ds, P, B, shuffle=True, seed=3, with_index=True))

    def aux_loader():
        return next(aux_it)[3]

    def index_gather():
        return flat[next(idx_it)[3]]

    assert torch.equal(aux_loader(), index_gather())
    variants = {
        "ssi_kernel": lambda: torch.autograd.grad(ssi(depth, prior), depth),
        "ssi_torch": lambda: torch.autograd.grad(torch_ssi(), depth),
        "rank_kernel": lambda: torch.autograd.grad(rank(depth, prior), depth),
        "rank_torch": lambda: torch.autograd.grad(torch_rank(), depth),
        "aux_loader": aux_loader,
        "index_gather": index_gather,
    }
    agree = {}
    for name, a, b in (("ssi", ssi(depth, prior), torch_ssi()), ("rank", rank(depth, prior), torch_rank())):
        agree[name] = abs(float(a.detach()) - float(b.detach())) / max(abs(float(b.detach())), 1e-12)
    rounds = benchlib.interleaved(variants, args.iters, args.warmup, args.rounds)
    out = {**benchlib.header("bench_depth_prior", args.tag),
           "patches": [B, P, P], "loader_dataset": [n, H, W], "iters": args.iters, "rounds": args.rounds,
           "what": "loss forward + backward / one loader next(), device events with the host path, us",
           "relative_difference_of_the_two_spellings": agree,
           "variants": {name: benchlib.rounds_summary(r, "us") for name, r in rounds.items()}}
    benchlib.emit(out, args.out)


if __name__ == "__main__":
    main()
