#!/usr/bin/env python3
"""Time OccGridEstimator.update_every_n_steps (the occupancy refresh of the training loop, run-nerf.py:288-295) per call
(schedule: interleaved, tools/benchlib.py): 128^3 cells at 1 and 4 levels, warm-up phase (every cell) and steady phase
(uniform + occupied draws), one estimator per configuration, three variants:

  closure_parity     the plain closure `model(x) * step`, the model's own (parity) mode: the level loop
  closure_autocast   the same closure under torch.autocast("cuda") with NeRF.autocast_precision set: the level loop in a
                     single-pass mode
  fused              NeRF.occ_eval_fn(step, precision): one launch for all levels

The last two need a build that has them; on an older one they are reported as null and the first variant still runs, so
the same file gives the baseline of an earlier commit.  Prints one JSON line.  Run it under a time limit of its own:

    timeout -k 10 300 python tools/bench_refresh.py [--precision fp16] [--iters 20] [--warmup 3] [--tag NAME]
"""
import argparse

import torch

import benchlib

benchlib.package()
from fs_nerf_amd.core.models import NeRF  # noqa: E402
from fs_nerf_amd.render.occgrid import OccGridEstimator  # noqa: E402

AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
STEP, RES = 5e-3, 128
HAS_SINGLE_PASS = hasattr(NeRF, "occ_eval_fn")


def make_model(dev):
    """8x256 network, seeded; the sigma head scaled and shifted so that about a third of the region of interest ends up
    occupied (median density over the box = 1: occ straddles the refresh threshold)."""
    torch.manual_seed(0)
    m = NeRF(3, 3, 8, 256, (4,), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
    with torch.no_grad():
        m.sigma.weight.mul_(256.0)
    m = m.to(dev).train()
    x = (torch.rand(65536, 3, generator=torch.Generator().manual_seed(1)) * 3 - 1.5).to(dev)
    with torch.no_grad():
        med = float(m(x).median())
        m.sigma.bias.add_(1.0 - med)
    return m


def unused_share(est):
    """Share of a steady-phase refresh's draws that are sentinels (a level with fewer than res^3/4 occupied cells)."""
    n_occ = RES ** 3 // 4
    per_level = est.binaries.reshape(est.levels, -1).sum(dim=1).tolist()
    return sum(max(0, n_occ - int(m)) for m in per_level) / float(est.levels * 2 * n_occ), [int(m) for m in per_level]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp16", choices=["fp16", "bf16"])
    benchlib.common_args(ap, iters=20, warmup=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = make_model(dev)
    closure = lambda x: model(x) * STEP

    def run_parity(est, step):
        est.update_every_n_steps(step, closure, occ_thre=1e-2)

    def run_autocast(est, step):
        model.autocast_precision = args.precision
        with torch.autocast("cuda"):
            est.update_every_n_steps(step, closure, occ_thre=1e-2)
        model.autocast_precision = None

    variants = [("closure_parity", run_parity)]
    if HAS_SINGLE_PASS:
        fused_fn = model.occ_eval_fn(STEP, args.precision)
        variants += [("closure_autocast", run_autocast),
                     ("fused", lambda est, step: est.update_every_n_steps(step, fused_fn, occ_thre=1e-2))]
    out = {**benchlib.header("bench_refresh", args.tag), "resolution": RES,
           "precision": args.precision if HAS_SINGLE_PASS else None, "iters": args.iters, "configs": {}}
    for levels in (1, 4):
        est = OccGridEstimator(AABB, RES, levels).to(dev).train()
        est.generator = torch.Generator().manual_seed(5)
        for phase, step in (("warmup", 0), ("steady", 256)):
            times = benchlib.interleaved({name: (lambda fn=fn: fn(est, step)) for name, fn in variants}, args.iters, args.warmup,
                                         keep="samples")
            cfg = {}
            for name in ("closure_parity", "closure_autocast", "fused"):
                t = times.get(name)
                cfg[name + "_ms"] = None if not t else benchlib.stats(t)
            share, occupied = unused_share(est)
            cfg["occupied_cells_per_level"] = occupied
            if phase == "steady":
                cfg["unused_draw_share"] = round(share, 4)
            out["configs"][f"levels{levels}_{phase}"] = cfg
    if HAS_SINGLE_PASS:
        out["precision_after"] = fused_fn.precision  # ("bf16" here: an fp16 refresh left the range envelope and fell back)
    benchlib.emit(out)


if __name__ == "__main__":
    main()
