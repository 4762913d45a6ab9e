#!/usr/bin/env python3
"""Time forward + backward of the few-shot geometry losses (core.loss.RayEntropyLoss, DepthKLLoss,
PatchDepthSmoothnessLoss: csrc/ray_losses.hip) against the torch spelling a user writes without the kernels: clamp /
index_add_ / log over the packed samples for the two ray losses (float atomics: not reproducible), slicing for the patch
loss.  Shapes: --rays 4096 rays with ragged spans (about --samples 150 samples per ray: a uniform count in [samples/2, 3
samples/2], every 64th ray empty), and --patches 64 patches of --patch 32 x 32.  The timed call is loss + backward.
Schedule: interleaved (tools/benchlib.py), --rounds 3 rounds, us.  There is no pass or fail on these times.  Appends one
JSON line to profiles/bench_ray_losses.jsonl (--out) and prints it.

    timeout -k 10 300 python tools/bench_ray_losses.py [--iters 20] [--warmup 5] [--rays 4096] [--samples 150] [--tag NAME]
"""
import argparse
import math

import benchlib


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=20, warmup=5, rounds=3, out="bench_ray_losses.jsonl")
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=150)
    ap.add_argument("--patches", type=int, default=64)
    ap.add_argument("--patch", type=int, default=32)
    args = ap.parse_args()
    import torch
    benchlib.package()
    from fs_nerf_amd import ops
    from fs_nerf_amd.core.loss import DepthKLLoss, PatchDepthSmoothnessLoss, RayEntropyLoss
    dev = torch.device("cuda:0")
    R, S = args.rays, args.samples
    gen = torch.Generator(device=dev).manual_seed(0)
    counts = torch.randint(S // 2, S + S // 2 + 1, (R,), device=dev, generator=gen)
    counts[::64] = 0
    ri = torch.repeat_interleave(torch.arange(R, device=dev), counts)
    N = ri.numel()
    first = torch.cumsum(counts, 0) - counts
    pos = (torch.arange(N, device=dev) - first[ri]).float()
    dt = (4.0 / counts.clamp(min=1).float())[ri]
    t0 = 2.0 + pos * dt
    t1 = t0 + dt
    sig = torch.rand(N, device=dev, generator=gen) * 3.0
    sig = torch.where(torch.rand(N, device=dev, generator=gen) < 0.05, -0.1 * sig, sig)
    rgb = torch.rand(N, 3, device=dev, generator=gen)
    _, opacity, depth, ex = ops.composite_packed(sig, rgb, t0, t1, ri, R, [1.0, 1.0, 1.0])
    alphas, weights = ex["alphas"].clone().requires_grad_(True), ex["weights"].clone().requires_grad_(True)
    target = depth.reshape(-1) + 0.1 * torch.randn(R, device=dev, generator=gen)
    var = torch.full((R,), 0.01, device=dev)
    patches = (2.0 + 4.0 * torch.rand(args.patches, args.patch, args.patch, device=dev, generator=gen)).requires_grad_(True)
    entropy, kl, smooth = RayEntropyLoss(), DepthKLLoss(), PatchDepthSmoothnessLoss()
    scale = 1.0 / math.log(2.0)

    def torch_entropy():
        c = (opacity.detach().reshape(-1) > 0.1).float()
        u = alphas.clamp(min=0.0)
        p = u / (torch.zeros(R, device=dev).index_add_(0, ri, u) + 1e-10)[ri]
        per_ray = torch.zeros(R, device=dev).index_add_(0, ri, p * torch.log(p + 1e-10))
        return (-scale * c * per_ray).mean()

    def torch_kl():
        ok = torch.isfinite(target) & (target > 0) & torch.isfinite(var) & (var > 0)
        m = (t0 + t1) / 2.0
        gauss = torch.exp(-(m - target[ri]) ** 2 / (2.0 * var[ri])) * (t1 - t0)
        per_ray = torch.zeros(R, device=dev).index_add_(0, ri, -torch.log(weights.clamp(min=0.0) + 1e-5) * gauss)
        return (per_ray * ok).sum() / ok.sum().clamp(min=1)

    def torch_smooth():
        a = patches[:, :-1, :-1]
        tv = ((a - patches[:, :-1, 1:]) ** 2 + (a - patches[:, 1:, :-1]) ** 2).sum(dim=(1, 2))
        return tv.mean() / float((args.patch - 1) ** 2)

    # name -> (loss closure, the leaf it differentiates)
    variants = {
        "entropy_kernel": (lambda: entropy(alphas, ri, R, opacity=opacity), alphas),
        "entropy_torch": (torch_entropy, alphas),
        "depth_kl_kernel": (lambda: kl(weights, t0, t1, ri, R, target, var), weights),
        "depth_kl_torch": (torch_kl, weights),
        "smooth_kernel": (lambda: smooth(patches), patches),
        "smooth_torch": (torch_smooth, patches),
    }
    agree = {}
    for name in ("entropy", "depth_kl", "smooth"):  # the two spellings compute the same loss
        a, b = float(variants[name + "_kernel"][0]().detach()), float(variants[name + "_torch"][0]().detach())
        agree[name] = abs(a - b) / max(abs(b), 1e-12)
    rounds = benchlib.interleaved({name: (lambda fn=fn, leaf=leaf: torch.autograd.grad(fn(), leaf))
                                   for name, (fn, leaf) in variants.items()}, args.iters, args.warmup, args.rounds)
    out = {**benchlib.header("bench_ray_losses", args.tag), "rays": R, "samples": N,
           "patches": [args.patches, args.patch, args.patch], "iters": args.iters, "rounds": args.rounds,
           "what": "loss forward + backward, device events, us", "relative_difference_of_the_two_spellings": agree,
           "variants": {name: benchlib.rounds_summary(r, "us") for name, r in rounds.items()}}
    benchlib.emit(out, args.out)


if __name__ == "__main__":
    main()
