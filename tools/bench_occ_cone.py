#!/usr/bin/env python3
"""What cone-angle steps in the one-launch occupancy kernel cost and buy (each child: interleaved, tools/benchlib.py).  The
scene is tools/bench_march.py's: the sphere grid of tests/test_occgrid.py at 128^3 cells over +-1.5, step 5e-3 (the
reference's LLFF configuration, run-nerf.py:92-98), its seeded 8 x 256 network, an orbit camera.

  default-frame   (a) cost to existing users: render_frame at ONE level without sampling options (route
                  camera-occupancy, one launch), this library against the PARENT commit's (--parent-lib, loaded through
                  FSN_LIB_PATH).  The new median may exceed the parent's by no more than the parent's own spread
                  (max - min of its runs); the line records both and the verdict.
  cone-frame      (b) FOUR levels with cone_angle 0.004, an 800 x 800 frame: FUSED_OCC_CONE off (route chunked: march,
                  density pass, cull, full pass, integration as separate launches per chunk) against on
                  (camera-occupancy: one launch).
  cone-train      (c) the same grid, a 4096-ray training call + backward: estimator-sampling against occ-sampler.

Every run of a variant is a fresh child process (the library is chosen when it is loaded); the variants alternate, three
runs each, and a variant's figure is the median of its runs' medians.  Every child runs under a time limit of its own
and the first one that fails ends the tool.  One JSON line per case, printed and appended to --out:

    timeout -k 10 900 python tools/bench_occ_cone.py --parent-lib PATH [--out profiles/bench_occ_cone.jsonl]
"""
import argparse
import json
import os
import sys

import benchlib
from benchlib import ROOT
STEP, RES, CONE, HW, CHUNK = 5e-3, 128, 0.004, 800, 32768
CASES = {"default-frame": dict(levels=1, frame=True, cone=0.0), "cone-frame": dict(levels=4, frame=True, cone=CONE),
         "cone-train": dict(levels=4, frame=False, cone=CONE)}


def child(args):
    """One run of one variant -> one JSON line: per-iteration milliseconds and the route taken."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(benchlib.package(), "tests"))
    from fs_nerf_amd import _lib as L
    from fs_nerf_amd.render import rendering as Rm
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    from oracle import fsnerf_oracle as O
    from bench_march import make_model
    from test_occgrid import AABB, _sphere_binaries
    lib = L.lib()
    if not hasattr(lib, "fsn_render_rays_occgrid_ex"):
        # the parent commit's library: its plain entry points are what the extended ones are with cone_angle 0 and
        # null pointers, which is all the default frame passes
        def render_ex(desc, prec, blob, a, cone, t_min, t_max, t1, stream):
            assert cone == 0.0 and t_min is None and t_max is None and t1 is None
            return lib.fsn_render_rays_occgrid(desc, prec, blob, a, stream)
        lib.fsn_render_rays_occgrid_ex = render_ex
    case = CASES[args.child]
    Rm.FUSED_OCC_CONE = bool(args.cone_switch)
    dev = torch.device("cuda:0")
    model = make_model(dev)
    est = OccGridEstimator(AABB, RES, case["levels"]).to(dev)
    est.set_binaries(_sphere_binaries(RES, case["levels"]))
    est.generator = torch.Generator(device=dev).manual_seed(5)
    opts = {"cone_angle": case["cone"]} if case["cone"] else None
    pose = O.pose_from_spherical(4.0311289, 50.0, 30.0)
    if case["frame"]:
        model.eval()
        est.eval()
        hwf = (HW, HW, HW * 1.39)
        route = Rm._frame_route(est, model, None, False, False, STEP, opts)

        def run():
            with torch.no_grad():
                return Rm.render_frame(hwf, 2.0, 6.0, pose, CHUNK, est, model, white_bkgd=True, render_step_size=STEP,
                                       device=dev, sampling_kwargs=opts)
        rays = HW * HW
    else:
        model.train()
        est.train()
        o, d = O.get_rays(pose, (64, 64, 64 * 1.39))
        o, d = o.reshape(-1, 3).contiguous().to(dev), d.reshape(-1, 3).contiguous().to(dev)
        target = torch.rand(o.shape[0], 3, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        route = Rm._rays_route(est, model, None, True, True, o.shape[0], STEP, opts)

        def run():
            (rgb, _, _, _), ri, _ = Rm.render_rays(o, d, est, model, train=True, white_bkgd=True, render_step_size=STEP,
                                                   device=dev, sampling_kwargs=opts)
            torch.nn.functional.mse_loss(rgb, target).backward()
            model.zero_grad(set_to_none=True)
            return ri
        rays = int(o.shape[0])
    times = benchlib.interleaved({"run": run}, args.iters, args.warmup, keep="samples")["run"]
    print("CHILD " + json.dumps({"ms": [round(t, 4) for t in times], "median": round(float(np.median(times)), 4),
                                 "route": route, "rays": rays, "max_steps": est.max_steps(STEP, case["cone"]),
                                 "lib": os.path.basename(os.path.dirname(L.LIB_PATH)) + "/" + os.path.basename(L.LIB_PATH),
                                 "device": torch.cuda.get_device_name(0)}), flush=True)


def run_child(case, variant, args):
    """A fresh process per run; -> its line, or SystemExit when it fails or runs out of time (nothing more is started)."""
    iters, warmup, limit = (args.train_iters, 3, 240) if case == "cone-train" else (args.frame_iters, 1, 300)
    env = dict(os.environ)
    if variant.get("lib"):
        env.update(FSN_LIB_PATH=variant["lib"], FSN_LIB_PARTIAL="1")  # (the parent exports no *_ex render entry)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", case, "--cone-switch", str(int(variant.get("switch", 0))),
           "--iters", str(iters), "--warmup", str(warmup)]
    return benchlib.run_child(cmd, env, limit, f"bench_occ_cone: {case} / {variant['name']}", "CHILD ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's libfsnerf_hip.so (case default-frame)")
    ap.add_argument("--cases", default="default-frame,cone-frame,cone-train")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--frame-iters", type=int, default=3)
    ap.add_argument("--train-iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bench_occ_cone.jsonl"))
    ap.add_argument("--tag", default="")
    ap.add_argument("--child")
    ap.add_argument("--cone-switch", type=int, default=0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import statistics
    for case in args.cases.split(","):
        if case == "default-frame":
            if not args.parent_lib or not os.path.exists(args.parent_lib):
                raise SystemExit("bench_occ_cone: default-frame needs --parent-lib (the parent commit's library)")
            variants = [dict(name="parent", lib=os.path.abspath(args.parent_lib)), dict(name="new")]
        else:
            variants = [dict(name="switch-off", switch=0), dict(name="switch-on", switch=1)]
        runs = {v["name"]: [] for v in variants}
        for _ in range(args.runs):  # alternate: clock and thermal drift hit both alike
            for v in variants:
                runs[v["name"]].append(run_child(case, v, args))
        line = {"tool": "bench_occ_cone", "tag": args.tag, "case": case, **CASES[case], "resolution": RES, "step": STEP,
                "device": runs[variants[0]["name"]][0]["device"], "rays": runs[variants[0]["name"]][0]["rays"]}
        for name, rs in runs.items():
            meds = [r["median"] for r in rs]
            line[name] = {"route": rs[0]["route"], "max_steps": rs[0]["max_steps"], "lib": rs[0]["lib"], "run_medians_ms": meds,
                          "median_ms": round(statistics.median(meds), 4), "spread_ms": round(max(meds) - min(meds), 4)}
        a, b = (line[v["name"]] for v in variants)
        if case == "default-frame":
            line["excess_ms"] = round(b["median_ms"] - a["median_ms"], 4)
            line["inside_parent_spread"] = line["excess_ms"] <= a["spread_ms"]
        else:
            line["speedup_median"] = round(a["median_ms"] / b["median_ms"], 3)
        benchlib.emit(line, args.out)


if __name__ == "__main__":
    main()
