#!/usr/bin/env python3
"""Time the feed of the training loop: what it costs to get one batch (rays_o, rays_d, rgb) of B rays, and what the
`train-occ` loop body costs when it is fed each way.  Schedule: interleaved (tools/benchlib.py), one round, median / min
/ p90 in ms; B in {1024, 4096, 32768}; two datasets generated from a seed: the LLFF few-shot shape 8x378x504x3 and the
full Blender shape 100x800x800x4 (256 MB of bytes; its float tables are 2.3 GB).

  loader          one RayLoader batch (fs_nerf_amd.nerfdata: uint8 images resident, one fsn_ray_batch launch)
  tables          the feed of examples/train_synthetic.py without --u8-dataset: torch.randint + three gathers from float
                  tables (U.build_rays + float images)
  step_tables     the loop body of bench.py --workload train-occ restated (bench.py is a yardstick and is not imported
                  for its step: one 8x256 network, FusedAdam, the half-full sphere grid at 128^3, 4096 rays per step out
                  of eight 800x800 orbit views, render_step_size 5e-3, the shadow estimator's refresh every 16th step),
                  with that function's own feed line for line; run TWICE (a, b): their difference is the spread
  step_loader     the same body fed by a RayLoader over the bytes of a dataset of that shape
  cpu_dataloader  batches per second of torch.utils.data.DataLoader(TensorDataset(rays_o, rays_d, rgb), batch_size=B,
                  shuffle=True, num_workers=8) on CPU tensors of the LLFF shape: the reference's loader restated
                  (splitter.py:123-128), measured in a CHILD process that is started before this one touches the GPU
                  and that never opens it; first batch to last batch of one epoch (at most --cpu-seconds)

`loader` and `step_loader` need a build that has the data layer; on an older one they are reported as null and the
others still run, so the same file gives the baseline of an earlier commit.  The figures are call times (host launch
path + kernel), not shares of a peak: the kernel is a latency-bound gather of a few hundred KB.  Prints one JSON line.
Run it under a time limit of its own:

    timeout -k 10 600 python tools/bench_loader.py [--iters 50] [--warmup 5] [--steps 48] [--tag NAME] [--skip-blender]
"""
import argparse
import itertools
import json
import math
import os
import subprocess
import sys
import time

import benchlib

BATCHES = (1024, 4096, 32768)
LLFF = (8, 378, 504, 3, 407.6)
BLENDER = (100, 800, 800, 4, 0.5 * 800 / math.tan(0.5 * 0.6911112))


# ------------------------------------------------------------------ the child: CPU only
def cpu_child(seconds: float) -> None:
    import torch
    from torch.utils.data import DataLoader, TensorDataset
    n = LLFF[0] * LLFF[1] * LLFF[2]
    g = torch.Generator().manual_seed(0)
    ds = TensorDataset(torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g))
    out = {}
    for B in BATCHES:
        ld = DataLoader(ds, batch_size=B, shuffle=True, num_workers=8)
        t0 = t1 = None
        k = 0
        for batch in ld:
            now = time.perf_counter()
            if t0 is None:
                t0 = now
            else:
                k += 1
                t1 = now
                if now - t0 > seconds:
                    break
        del ld
        rate = k / (t1 - t0) if k else None
        out[f"B{B}"] = {"batches": k, "batches_per_s": None if rate is None else round(rate, 2),
                        "ms_per_batch": None if rate is None else round(1e3 / rate, 3)}
    print("CPU_DATALOADER " + json.dumps(out), flush=True)


# ------------------------------------------------------------------ the parent: GPU
def stats(t):
    return benchlib.stats(t) if t else None


def orbit_pose(torch, phi_deg):
    th, ph = 50.0 / 180.0 * math.pi, phi_deg / 180.0 * math.pi
    tr = torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0311289], [0, 0, 0, 1.0]])
    rt = torch.tensor([[1, 0, 0, 0], [0, math.cos(th), -math.sin(th), 0], [0, math.sin(th), math.cos(th), 0], [0, 0, 0, 1.0]])
    rp = torch.tensor([[math.cos(ph), -math.sin(ph), 0, 0], [math.sin(ph), math.cos(ph), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    return rp @ (rt @ tr)


def float_images(torch, imgs, white):
    """the float colour table of the bytes, view by view (the temporaries of one view at a time)"""
    out = torch.empty(imgs.shape[0], imgs.shape[1] * imgs.shape[2], 3, device=imgs.device)
    for v in range(imgs.shape[0]):
        f = imgs[v].reshape(-1, imgs.shape[3]).float() / 255.0
        out[v] = f[:, :3] * f[:, 3:] + (1.0 - f[:, 3:]) if white else f[:, :3]
    return out.reshape(-1, 3)


def bench_feed(torch, U, nerfdata, dev, shape, args):
    n, H, W, C, focal = shape
    gen = torch.Generator(device=dev).manual_seed(n * H + C)
    imgs = torch.randint(0, 256, (n, H, W, C), device=dev, dtype=torch.uint8, generator=gen)
    poses = torch.stack([orbit_pose(torch, 360.0 * k / n) for k in range(n)])
    white = C == 4
    ro, rd, _ = U.build_rays(poses, (H, W, focal), dev, False)
    gt = float_images(torch, imgs, white)
    res = {"rays": n * H * W,
           "resident_bytes": {"tables": (ro.numel() + rd.numel() + gt.numel()) * 4,
                              "loader": imgs.numel() + n * 12 * 4 + 6 * 4 if nerfdata else None}}
    ds = nerfdata.RayDataset(imgs, poses, (H, W, focal), near=2.0, far=6.0, white_bkgd=white, device=dev) if nerfdata else None
    for B in BATCHES:
        rgen = torch.Generator(device=dev).manual_seed(0)

        def tables():
            idx = torch.randint(0, ro.shape[0], (B,), device=dev, generator=rgen)
            return ro[idx], rd[idx], gt[idx]

        variants = [("tables", tables)]
        if ds is not None:
            state = {"it": iter(nerfdata.RayLoader(ds, B, seed=1))}
            loader = state["it"].loader

            def from_loader():
                try:
                    return next(state["it"])
                except StopIteration:
                    state["it"] = iter(loader)
                    return next(state["it"])
            variants.append(("loader", from_loader))
        times = benchlib.interleaved(dict(variants), args.iters, args.warmup, keep="samples")
        res[f"B{B}"] = {"tables_ms": stats(times["tables"]), "loader_ms": stats(times.get("loader"))}
    return res


def bench_step(torch, U, nerfdata, dev, args):
    from fs_nerf_amd.core.models import NeRF
    from fs_nerf_amd.core.optim import FusedAdam
    from fs_nerf_amd.render import rendering as Rm
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    H = W = 800
    focal = BLENDER[4]
    RES, STEP, RADIUS, T_RAYS = 128, 5e-3, 1.477, 4096
    box = torch.tensor([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5])
    ax = (torch.arange(RES) + 0.5) / RES * 3.0 - 1.5
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    sphere = ((x * x + y * y + z * z).sqrt() < RADIUS)[None]
    poses = torch.stack([orbit_pose(torch, 45.0 * k) for k in range(8)])
    rays = [U.get_rays(p, (H, W, focal), dev) for p in poses]
    ro = torch.cat([o.reshape(-1, 3) for o, _ in rays])
    rd = torch.cat([d.reshape(-1, 3) for _, d in rays])
    gt = torch.rand(ro.shape[0], 3, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    ds = None
    if nerfdata:
        imgs = torch.randint(0, 256, (8, H, W, 3), device=dev, dtype=torch.uint8, generator=torch.Generator(device=dev).manual_seed(7))
        ds = nerfdata.RayDataset(imgs, poses, (H, W, focal), near=2.0, far=6.0, device=dev)

    def make(feed_kind):
        torch.manual_seed(42)
        model = NeRF(3, 3, 8, 256, (4,), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
        with torch.no_grad():
            model.sigma.weight.mul_(64.0)
            model.sigma.bias.add_(3.0)
        model.to(dev).train()
        est = OccGridEstimator(roi_aabb=box, resolution=RES, levels=1).to(dev)
        est.set_binaries(sphere)
        est.train()
        est.generator = torch.Generator(device=dev).manual_seed(1000)
        shadow = OccGridEstimator(roi_aabb=box, resolution=RES, levels=1).to(dev).train()
        shadow.generator = torch.Generator(device=dev).manual_seed(3000)
        opt = FusedAdam(model.parameters(), lr=5e-4)
        gen = torch.Generator(device=dev).manual_seed(2000)
        if feed_kind == "loader":
            loader = nerfdata.RayLoader(ds, T_RAYS, seed=2000)
            state = {"it": iter(loader)}

        def occ_eval_fn(xx):
            return model(xx) * STEP

        def step(i):
            if feed_kind == "loader":
                try:
                    b_o, b_d, b_gt = next(state["it"])
                except StopIteration:
                    state["it"] = iter(loader)
                    b_o, b_d, b_gt = next(state["it"])
            else:
                idx = torch.randint(0, ro.shape[0], (T_RAYS,), device=dev, generator=gen)
                b_o, b_d, b_gt = ro[idx], rd[idx], gt[idx]
            opt.zero_grad()
            (rgb, _, _, _), ri, _ = Rm.render_rays(b_o, b_d, est, model, train=True, white_bkgd=True, render_step_size=STEP, device=dev)
            loss = torch.nn.functional.mse_loss(rgb, b_gt)
            loss.backward()
            opt.grads.allreduce(average=False)
            opt.step(grad_div=1.0)
            with torch.no_grad():
                shadow.update_every_n_steps(step=256 + i, occ_eval_fn=occ_eval_fn, occ_thre=1e-2)
            return loss
        return step

    variants = [("step_tables_a", make("tables"))]
    if ds is not None:
        variants.append(("step_loader", make("loader")))
    variants.append(("step_tables_b", make("tables")))
    import gc
    gc.collect()
    gc.disable()
    # every step takes its own iteration number (the shadow estimator's refresh period counts it)
    times = benchlib.interleaved({name: (lambda fn=fn, it=itertools.count(): fn(next(it))) for name, fn in variants},
                                 args.steps, args.warmup, keep="samples")
    gc.enable()
    import numpy as np
    out = {name + "_ms": stats(t) for name, t in times.items()}
    out.setdefault("step_loader_ms", None)
    # the refresh steps (every 16th) cost about twice a plain step, so the mean and the median say different things;
    # both are reported, each with the spread between the two repeats of step_tables and the loader's distance from
    # the mean of those two
    for stat, f in (("mean", np.mean), ("median", np.median)):
        v = {name: float(f(t)) for name, t in times.items()}
        cmp = {"per_variant_ms": {k: round(x, 4) for k, x in v.items()},
               "spread_tables_ms": round(abs(v["step_tables_a"] - v["step_tables_b"]), 4)}
        if ds is not None:
            cmp["loader_minus_tables_ms"] = round(v["step_loader"] - 0.5 * (v["step_tables_a"] + v["step_tables_b"]), 4)
        out["by_" + stat] = cmp
    if ds is not None:
        out["resident_bytes"] = {"tables": (ro.numel() + rd.numel() + gt.numel()) * 4, "loader": ds.imgs.numel() + 8 * 12 * 4 + 24}
    out["steps"] = args.steps
    return out


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=50, warmup=5)
    ap.add_argument("--steps", type=int, default=48, help="timed steps per variant of the train-occ body (a multiple of 16: whole refresh periods)")
    ap.add_argument("--cpu-seconds", type=float, default=6.0)
    ap.add_argument("--skip-blender", action="store_true")
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--cpu-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.cpu_child:
        cpu_child(args.cpu_seconds)
        return
    cpu = None
    if not args.skip_cpu:  # first, before this process opens the GPU; the child never does
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-child", "--cpu-seconds", str(args.cpu_seconds)],
                           capture_output=True, text=True, env=env, timeout=60 + 6 * args.cpu_seconds * len(BATCHES))
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("CPU_DATALOADER ")]
        cpu = json.loads(lines[-1][len("CPU_DATALOADER "):]) if r.returncode == 0 and lines else {"error": (r.stdout + r.stderr)[-500:]}
    import torch
    benchlib.package()
    from fs_nerf_amd.utils import utilities as U
    try:
        from fs_nerf_amd import nerfdata
    except ImportError:
        nerfdata = None
    dev = torch.device("cuda:0")
    out = {**benchlib.header("bench_loader", args.tag), "has_loader": nerfdata is not None,
           "iters": args.iters, "cpu_dataloader_llff": cpu, "feed": {}}
    shapes = [("llff_8x378x504x3", LLFF)] + ([] if args.skip_blender else [("blender_100x800x800x4", BLENDER)])
    for name, shape in shapes:
        out["feed"][name] = bench_feed(torch, U, nerfdata, dev, shape, args)
        torch.cuda.empty_cache()
    out["train_occ_step_8x800x800"] = bench_step(torch, U, nerfdata, dev, args)
    benchlib.emit(out)


if __name__ == "__main__":
    main()
