#!/usr/bin/env python3
"""Time OccGridEstimator.sampling with and without cone-angle steps (schedule: interleaved, tools/benchlib.py): 4096 rays
through the sphere grid of tests/test_occgrid.py at 128^3 cells, step 5e-3 (the reference's LLFF configuration,
run-nerf.py:92-98), one level and four, cone_angle 0 (the uniform march) against 0.004.  Both go through
fsn_occgrid_march_ex and its one kernel (lines recorded before the plain and the extended kernel were merged timed the
plain kernel as "uniform"):

  march      sampling without sigma_fn: count pass, scan, one host read, fill pass
  sampling   with the model's density pass and the visibility cull behind it (sigma_fn = forward_rays)
  train      a training-shaped step: render_rays(train=True) + loss.backward(), with sampling_kwargs None and
             {"cone_angle": 0.004}; the route each takes is recorded

One JSON line per case, printed and appended to --out.  Run it under a time limit of its own:

    timeout -k 10 300 python tools/bench_march.py [--iters 20] [--warmup 3] [--out profiles/bench_march.jsonl]
"""
import argparse
import os
import sys

import torch

import benchlib

sys.path.insert(0, os.path.join(benchlib.package(), "tests"))
from fs_nerf_amd.core.models import NeRF  # noqa: E402
from fs_nerf_amd.render import rendering as Rm  # noqa: E402
from fs_nerf_amd.render.occgrid import OccGridEstimator  # noqa: E402
from oracle import fsnerf_oracle as O  # noqa: E402
from test_occgrid import AABB, _sphere_binaries  # noqa: E402

STEP, RES, CONE, HW = 5e-3, 128, 0.004, 64  # 64 x 64 pixels: 4096 rays


def make_model(dev):
    """8x256 network, seeded; the sigma head scaled and shifted so that the median density over the box is 1."""
    torch.manual_seed(0)
    m = NeRF(3, 3, 8, 256, (4,), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
    with torch.no_grad():
        m.sigma.weight.mul_(256.0)
    m = m.to(dev)
    x = (torch.rand(65536, 3, generator=torch.Generator().manual_seed(1)) * 3 - 1.5).to(dev)
    with torch.no_grad():
        m.sigma.bias.add_(1.0 - float(m(x).median()))
    return m


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=20, warmup=3, out="bench_march.jsonl")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = make_model(dev)
    o, d = O.get_rays(O.pose_from_spherical(4.0311289, 50.0, 30.0), (HW, HW, HW * 1.39))
    o, d = o.reshape(-1, 3).contiguous().to(dev), d.reshape(-1, 3).contiguous().to(dev)
    target = torch.rand(o.shape[0], 3, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    sigma_fn = lambda a, b, c: model.forward_rays(o, d, c, a, b, full=False).squeeze(-1)

    def emit(case, levels, variants, run):
        """`run(cone)` -> sample count (the last call's is recorded); interleaved schedule."""
        counts = {}
        times = benchlib.interleaved({name: (lambda name=name, cone=cone: counts.__setitem__(name, run(cone)))
                                      for name, cone in variants.items()}, args.iters, args.warmup, keep="samples")
        line = {**benchlib.header("bench_march", args.tag), "case": case,
                "levels": levels, "rays": int(o.shape[0]), "resolution": RES, "step": STEP, "iters": args.iters}
        for name, cone in variants.items():
            line[name] = {"cone_angle": cone, "ms": benchlib.stats(times[name]), **counts[name]}
        line["speedup_median"] = round(line["uniform"]["ms"]["median"] / line["cone"]["ms"]["median"], 3)
        benchlib.emit(line, args.out)

    variants = {"uniform": 0.0, "cone": CONE}
    for levels in (1, 4):
        est = OccGridEstimator(AABB, RES, levels).to(dev)
        est.set_binaries(_sphere_binaries(RES, levels))
        est.generator = torch.Generator(device=dev).manual_seed(5)
        model.eval()
        est.eval()

        def march(cone, fn=None):
            ri, _, _ = est.sampling(o, d, sigma_fn=fn, render_step_size=STEP, stratified=True, cone_angle=cone)
            return {"samples": int(ri.numel()), "max_steps": est.max_steps(STEP, cone)}

        emit("march", levels, variants, march)
        emit("sampling", levels, variants, lambda cone: march(cone, sigma_fn))
        model.train()
        est.train()

        def train(cone):
            opts = {"cone_angle": cone} if cone else None
            (rgb, _, _, _), ri, _ = Rm.render_rays(o, d, est, model, train=True, white_bkgd=True, render_step_size=STEP,
                                                   device=dev, sampling_kwargs=opts)
            torch.nn.functional.mse_loss(rgb, target).backward()
            model.zero_grad(set_to_none=True)
            return {"samples": int(ri.numel()), "route": Rm._rays_route(est, model, None, True, True, o.shape[0], STEP, opts)}

        emit("train", levels, variants, train)


if __name__ == "__main__":
    main()
