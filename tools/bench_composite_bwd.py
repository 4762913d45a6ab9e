#!/usr/bin/env python3
"""Time the backward of the packed compositor at the training step's shape (4096 rays x 192 samples): the lean entry point
(fsn_composite_packed_bwd: colours and opacity, the default training step) and the full one
(fsn_composite_packed_bwd_full) with the same two cotangents, with d_depth, with d_weights and with all six (one kernel
behind both entry points: "lean" and "full_colors_opacity" differ in the host call only; lines recorded before the merge
timed a separate lean kernel); and the distortion loss's two kernels.  The timed call is the ops-level call (its two
memsets and the kernel). Schedule: interleaved (tools/benchlib.py), one round, median and minimum in us.  GB/s is
against the byte model: 40 B per sample for the lean backward (sigma, rgb, t0, t1 read; d_sigma, d_rgb written) plus 4 B
per sample for each per-sample cotangent present; the per-ray arrays and the binary search over ray_indices are not
counted.  Prints one JSON line.

    timeout -k 10 120 python tools/bench_composite_bwd.py [--iters 20] [--warmup 5] [--rays 4096] [--samples 192] [--tag NAME]
"""
import argparse

import benchlib


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=20, warmup=5)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=192)
    args = ap.parse_args()
    import numpy as np
    import torch
    benchlib.package()
    from fs_nerf_amd import ops
    dev = torch.device("cuda:0")
    R, S = args.rays, args.samples
    N = R * S
    gen = torch.Generator(device=dev).manual_seed(0)
    edges = ops.stratified_edges(2.0, 6.0, S, R, torch.rand(R, device=dev, generator=gen), dev)
    ri, t0, t1 = ops.edges_to_packed(edges)
    sig = torch.rand(N, device=dev, generator=gen) * (0.15 * S)
    rgb = torch.rand(N, 3, device=dev, generator=gen)
    bk = [1.0, 1.0, 1.0]
    _, opacity, depth, ex = ops.composite_packed(sig, rgb, t0, t1, ri, R, bk)
    dc, dop, dd = (torch.randn(R, k, device=dev, generator=gen) for k in (3, 1, 1))
    dw, da, dt = (torch.randn(N, device=dev, generator=gen) for _ in range(3))
    dray = torch.randn(R, 1, device=dev, generator=gen)

    def full(**kw):
        return lambda: ops.composite_packed_bwd_full(sig, rgb, t0, t1, ri, R, bk, dc, dop, opacity=opacity, depth=depth, **kw)

    # name -> (call, bytes per sample)
    variants = {
        "lean": (lambda: ops.composite_packed_bwd(sig, rgb, t0, t1, ri, R, bk, dc, dop), 40),
        "full_colors_opacity": (full(), 40),
        "full_depth": (full(d_depth=dd), 40),
        "full_weights": (full(d_weights=dw), 44),
        "full_all_six": (full(d_depth=dd, d_weights=dw, d_alphas=da, d_trans=dt), 52),
        "distortion_fwd": (lambda: ops._DistortionFn.apply(ex["weights"], t0, t1, ri, R), 12),
    }
    wg = ex["weights"].clone().requires_grad_(True)
    dist = ops.distortion(wg, t0, t1, ri, R)
    variants["distortion_bwd"] = (lambda: torch.autograd.grad(dist, wg, dray, retain_graph=True), 16)
    times = benchlib.interleaved({name: fn for name, (fn, _) in variants.items()}, args.iters, args.warmup, keep="samples")
    out = {**benchlib.header("bench_composite_bwd", args.tag), "rays": R,
           "samples_per_ray": S, "iters": args.iters, "variants": {}}
    for name, (_, bps) in variants.items():
        med = float(np.median(times[name])) * 1e3  # us
        out["variants"][name] = {"us_median": round(med, 2), "us_min": round(float(np.min(times[name])) * 1e3, 2),
                                 "bytes_per_sample": bps, "gb_per_s": round(N * bps / (med * 1e-6) / 1e9, 1)}
    benchlib.emit(out)


if __name__ == "__main__":
    main()
