#!/usr/bin/env python3
"""Time the proposal-network sampler (csrc/propnet.hip, render/propnet.py) at 4096 rays, prop_samples=(128,),
num_samples=64, the profiler off.  Three cases, one JSON line each, printed and
appended to --out:

  level      one level between two network evaluations, 128 intervals in -> 64 out, no gradients:
               fused     fsn_prop_resample, one launch
               composed  render_transmittance_from_density, 1 - cat(trans, 0), fsn_importance_sample
               torch     what a user writes without either: cumsum / exp for the cdf, torch.searchsorted, gather, lerp,
                         midpoints and the transform as torch ops
             (the three are compared first: fused against composed bit for bit, torch by its largest difference)
  sampling   PropNetEstimator.sampling with one 4x128 proposal network (density-only pass): as it is (fused level), and
             with the composed level put in fsn_prop_resample's place by this tool
  step       a training-shaped step through render_rays' "propnet" route with a 4x128 proposal and an 8x256 final
             network: forward, MSE, backward - with the proposal update (proposal graph kept, interlevel loss, its
             backward, both Adam steps) and without it (proposal_requires_grad off, the main Adam step only)

Schedule: windows (tools/benchlib.py), --runs 3 runs of --iters calls each, ms.  Run it under a time limit of its own:

    timeout -k 10 300 python tools/bench_propnet.py [--iters 200] [--warmup 10] [--out profiles/bench_propnet.jsonl]
"""
import argparse

import torch

import benchlib

benchlib.package()
from fs_nerf_amd import ops  # noqa: E402
from fs_nerf_amd.core import models as M  # noqa: E402
from fs_nerf_amd.render import propnet as P  # noqa: E402
from fs_nerf_amd.render import rendering as R  # noqa: E402
from fs_nerf_amd.render import volrend as V  # noqa: E402

RAYS, N_PROP, N_FINAL, NEAR, FAR = 4096, 128, 64, 2.0, 6.0


def alternate(variants, iters, warmup, runs):
    times = benchlib.windows(variants, iters, warmup, runs)
    return {name: benchlib.rounds_summary(t, "ms", per="runs") for name, t in times.items()}


def level_case(dev):
    gen = torch.Generator().manual_seed(0)
    s = torch.cat([torch.zeros(RAYS, 1), torch.sort(torch.rand(RAYS, N_PROP - 1, generator=gen), 1).values,
                   torch.ones(RAYS, 1)], 1).to(dev)
    t = P._transform_stot("lindisp", s, NEAR, FAR)
    sig = (torch.rand(RAYS, N_PROP, generator=gen) ** 4 * 50.0).to(dev)
    return s, t, sig


def level_fused(s, t, sig):
    return ops.prop_resample(s, t, sig, N_FINAL, None, "lindisp", NEAR, FAR)


def level_composed(s, t, sig):
    trans, _ = V.render_transmittance_from_density(t[:, :-1], t[:, 1:], sig)
    cdfs = 1.0 - torch.cat([trans, torch.zeros_like(trans[:, :1])], dim=-1)
    return (cdfs,) + ops.importance_sample(s, cdfs, N_FINAL, None, "lindisp", NEAR, FAR, want_centres=False)


def level_torch(s, t, sig):
    sdt = sig * (t[:, 1:] - t[:, :-1])
    run = torch.cumsum(sdt, 1)
    cdfs = 1.0 - torch.cat([torch.ones_like(run[:, :1]), torch.exp(-run[:, :-1]), torch.zeros_like(run[:, :1])], 1)
    u = ((torch.arange(N_FINAL, device=s.device, dtype=torch.float32) + 0.5) / N_FINAL).expand(RAYS, -1).contiguous()
    k = (torch.searchsorted(cdfs, u, right=True) - 1).clamp(0, N_PROP - 1)
    c0, c1 = cdfs.gather(1, k), cdfs.gather(1, k + 1)
    den = c1 - c0
    frac = torch.where(den > 0, ((u - c0) / den).clamp(0, 1), torch.zeros_like(den))
    v0, v1 = s.gather(1, k), s.gather(1, k + 1)
    x = v0 + frac * (v1 - v0)
    mid = (x[:, :-1] + x[:, 1:]) * 0.5
    e = torch.cat([torch.maximum(2 * x[:, :1] - mid[:, :1], s[:, :1]), mid,
                   torch.minimum(2 * x[:, -1:] - mid[:, -1:], s[:, -1:])], 1)
    return cdfs, e, None, P._transform_stot("lindisp", e, NEAR, FAR)


def nerf(seed, layers, width, skip, dev):
    torch.manual_seed(seed)
    m = M.NeRF(3, 3, layers, width, skip, pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
    with torch.no_grad():
        m.sigma.weight.mul_(16.0)
        m.sigma.bias.add_(1.0)
    return m.to(dev)


def rays(dev):
    gen = torch.Generator().manual_seed(1)
    o = torch.tensor([0.0, 0.0, 4.0]) + 0.1 * torch.randn(RAYS, 3, generator=gen)
    d = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, -1.0]) + 0.2 * torch.randn(RAYS, 3, generator=gen), dim=-1)
    return o.to(dev), d.to(dev)


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=200, warmup=10, runs=3, out="bench_propnet.jsonl")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_propnet needs the GPU: there is nothing to time without one"
    dev = torch.device("cuda:0")
    head = {**benchlib.header("bench_propnet", args.tag), "rays": RAYS,
            "prop_samples": [N_PROP], "num_samples": N_FINAL, "iters": args.iters, "runs": args.runs}

    def emit(case, extra, times):
        benchlib.emit(dict(head, case=case, **extra, **times), args.out)

    # (a) one level
    s, t, sig = level_case(dev)
    with torch.no_grad():
        f, c, th = level_fused(s, t, sig), level_composed(s, t, sig), level_torch(s, t, sig)
        same = all(torch.equal(f[i], c[i]) for i in (0, 1, 3))
        diff = [round(float((f[i] - th[i]).abs().max()), 9) for i in (0, 1, 3)]
        times = alternate({"fused": lambda: level_fused(s, t, sig), "composed": lambda: level_composed(s, t, sig),
                           "torch": lambda: level_torch(s, t, sig)}, args.iters, args.warmup, args.runs)
    emit("level", {"fused_equals_composed": same, "max_abs_diff_fused_vs_torch_cdfs_s_t": diff}, times)

    # (b) estimator.sampling, no gradients
    o, d = rays(dev)
    prop = nerf(11, 4, 128, (), dev).eval()
    est = P.PropNetEstimator(prop_models=[prop], prop_samples=(N_PROP,), num_samples=N_FINAL, near_plane=NEAR, far_plane=FAR)
    fn = P.prop_sigma_fn(prop, o, d)

    fused_level = ops.prop_resample

    def composed_level(s, t, sig, n, b, transform, near, far):
        trans, _ = V.render_transmittance_from_density(t[:, :-1], t[:, 1:], sig)
        cdfs = 1.0 - torch.cat([trans, torch.zeros_like(trans[:, :1])], dim=-1)
        s2, x2, t2 = ops.importance_sample(s, cdfs, n, b, transform, near, far, want_centres=False)
        return cdfs, s2, x2, t2

    def sampling(fused):
        ops.prop_resample = fused_level if fused else composed_level
        try:
            with torch.no_grad():
                return est.sampling([fn], (N_PROP,), N_FINAL, RAYS, NEAR, FAR, "lindisp", device=dev)
        finally:
            ops.prop_resample = fused_level

    same = all(torch.equal(a, b) for a, b in zip(sampling(True), sampling(False)))
    times = alternate({"fused": lambda: sampling(True), "composed": lambda: sampling(False)}, args.iters, args.warmup, args.runs)
    emit("sampling", {"fused_equals_composed": same}, times)

    # (c) a training-shaped step through the route
    from fs_nerf_amd.core.optim import FusedAdam
    prop.train()
    fine = nerf(12, 8, 256, (4,), dev).train()
    est = P.PropNetEstimator(torch.optim.Adam(prop.parameters(), lr=5e-4), prop_models=[prop], prop_samples=(N_PROP,),
                             num_samples=N_FINAL, near_plane=NEAR, far_plane=FAR).train()
    opt = FusedAdam(fine.parameters(), lr=5e-4)
    target = torch.rand(RAYS, 3, device=dev)

    def step(update):
        est.proposal_requires_grad = update
        (rgb, _, _, ex), _, _ = R.render_rays(o, d, est, fine, train=True, white_bkgd=True, device=dev)
        torch.nn.functional.mse_loss(rgb, target).backward()
        opt.step()
        opt.zero_grad()
        if update:
            est.update_every_n_steps(ex["trans"].reshape(RAYS, N_FINAL), requires_grad=True)

    steps = max(args.iters // 10, 5)
    times = alternate({"with_proposal_update": lambda: step(True), "without_proposal_update": lambda: step(False)}, steps,
                      max(args.warmup // 2, 3), args.runs)
    emit("step", {"steps_per_run": steps, "final_network": "8x256", "proposal_network": "4x128"}, times)


if __name__ == "__main__":
    main()
