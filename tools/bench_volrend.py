#!/usr/bin/env python3
"""Time the packed volume-rendering primitives against the plain torch ops a user writes without them: 4096 rays at about
40 and about 150 kept samples per ray (counts uniform in [m/2, 3m/2], seeded), render_weight_from_density +
accumulate_along_rays(C = 3), forward alone and forward + backward (gradients to sigmas and rgbs through a loss on the
colours).

  hip     render/volrend.py: one launch for the weights, one for the accumulation, one each for their backwards
  torch   the same results from torch ops on the device: a GLOBAL cumsum of sigma dt minus its value at each ray's
          first sample, exp, index_add_ - and the autograd nodes behind them

Schedule: windows (tools/benchlib.py), three runs of --iters calls each, ms.  The results are compared first (max |hip -
torch| / max |torch|), so that the times are of the same answer.  One JSON line per case, printed and appended to --out.
Run it under a time limit of its own:

    timeout -k 10 300 python tools/bench_volrend.py [--iters 500] [--warmup 20] [--out profiles/bench_volrend.jsonl]
"""
import argparse

import torch

import benchlib

benchlib.package()
from fs_nerf_amd.render import volrend as V  # noqa: E402

RAYS, RUNS = 4096, 3


def make_case(mean, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    counts = torch.randint(mean // 2, mean + mean // 2 + 1, (RAYS,), generator=gen)
    ri = torch.repeat_interleave(torch.arange(RAYS), counts)
    N = ri.numel()
    starts = torch.cumsum(counts, 0) - counts
    k = torch.arange(N) - starts[ri]
    dt = 4.0 / (mean + mean // 2)
    t0 = 2.0 + k.float() * dt
    sig = torch.rand(N, generator=gen) * (6.0 / (mean * dt))
    rgb = torch.rand(N, 3, generator=gen)
    g = torch.randn(RAYS, 3, generator=gen)
    return dict(N=N, ri=ri.to(dev), first=starts[ri].to(dev), t0=t0.to(dev), t1=(t0 + dt).to(dev), sig=sig.to(dev),
                rgb=rgb.to(dev), g=g.to(dev))


def hip_forward(c, sig, rgb):
    w, _, _ = V.render_weight_from_density(c["t0"], c["t1"], sig, ray_indices=c["ri"], n_rays=RAYS)
    return V.accumulate_along_rays(w, rgb, c["ri"], RAYS)


def torch_forward(c, sig, rgb):
    sdt = sig * (c["t1"] - c["t0"])
    excl = torch.cumsum(sdt, 0) - sdt
    trans = torch.exp(-(excl - excl[c["first"]]))
    w = trans * (1.0 - torch.exp(-sdt))
    return torch.zeros(RAYS, 3, device=sig.device).index_add_(0, c["ri"], w[:, None] * rgb)


def step(fwd, c, backward):
    if not backward:
        with torch.no_grad():
            return fwd(c, c["sig"], c["rgb"])
    sig, rgb = c["sig"].detach().requires_grad_(True), c["rgb"].detach().requires_grad_(True)
    out = fwd(c, sig, rgb)
    (out * c["g"]).sum().backward()
    return out.detach(), sig.grad, rgb.grad


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp(min=1e-30))


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=500, warmup=20, out="bench_volrend.jsonl")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_volrend needs the GPU: there is nothing to time without one"
    dev = torch.device("cuda:0")
    for mean in (40, 150):
        c = make_case(mean, dev, seed=mean)
        variants = {"hip": hip_forward, "torch": torch_forward}
        for backward in (False, True):
            outs = {name: step(fwd, c, backward) for name, fwd in variants.items()}
            pairs = zip(outs["hip"], outs["torch"]) if backward else [(outs["hip"], outs["torch"])]
            agree = [round(rel(a, b), 9) for a, b in pairs]
            runs = benchlib.windows({name: (lambda fwd=fwd: step(fwd, c, backward)) for name, fwd in variants.items()},
                                    args.iters, args.warmup, RUNS)
            line = {**benchlib.header("bench_volrend", args.tag),
                    "case": "forward+backward" if backward else "forward", "rays": RAYS, "samples": c["N"],
                    "samples_per_ray": round(c["N"] / RAYS, 1), "channels": 3, "iters": args.iters, "runs": RUNS,
                    "max_rel_diff_hip_vs_torch": agree}
            for name in variants:
                line[name] = benchlib.rounds_summary(runs[name], "ms", per="runs")
            benchlib.emit(line, args.out)


if __name__ == "__main__":
    main()
