#!/usr/bin/env python3
"""Time the training pair with and without gradients to the rays, from device events after a warm-up: 4096 rays x 192
samples (786,432 samples) through the 8 x 256 network in the ray form, `forward_rays` + `backward` of a fixed
cotangent, three configurations alternated call by call in one process:

  a  parameter gradients only (rays do not require grad: the step every earlier commit ran)
  b  parameters and rays      (fsn_nerf_train_bwd_inputs + fsn_ray_grad_reduce on top of a)
  c  rays only, frozen network in eval mode (the dgrad chain and the input gradient, no weight-gradient launches)

`--configs a` runs on a checkout without input gradients too (`--root` = the checkout whose package is imported), which is
how a is compared with the parent commit: both in one session on one device, alternating process by process.
One JSON line, printed and appended to --out.  Run it under a time limit of its own:

    timeout -k 10 300 python tools/bench_input_grad.py [--iters 20] [--warmup 3] [--out profiles/bench_input_grad.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, S, NEAR, FAR = 4096, 192, 2.0, 6.0


def stats(t):
    return {"median": round(float(np.median(t)), 4), "min": round(float(np.min(t)), 4),
            "p90": round(float(np.percentile(t, 90)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--configs", default="abc")
    ap.add_argument("--root", default=HERE, help="checkout whose package is timed")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "bench_input_grad.jsonl"))
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd.core.models import NeRF
    from oracle import fsnerf_oracle as O

    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    def make(train):
        m = NeRF(3, 3, 8, 256, (4,), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
        m.load_state_dict(O.init_nerf_state_dict(8, 256, [4], 10, 4, seed=42))
        m = m.to(dev)
        if train:
            return m.train()
        for p in m.parameters():
            p.requires_grad_(False)
        return m.eval()

    o, d = O.get_rays(O.pose_from_spherical(4.0311289, 50.0, 30.0), (64, 64, 64 * 1.39))
    o, d = o.reshape(-1, 3).contiguous().to(dev), d.reshape(-1, 3).contiguous().to(dev)
    assert o.shape[0] == R
    edges = NEAR + (FAR - NEAR) * torch.arange(S + 1, device=dev, dtype=torch.float32) / S
    ri = torch.arange(R, device=dev).repeat_interleave(S)
    t0, t1 = edges[:-1].repeat(R).contiguous(), edges[1:].repeat(R).contiguous()
    c = torch.randn(R * S, 4, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    nets = {"a": make(True), "b": None, "c": make(False) if "c" in args.configs else None}
    nets["b"] = nets["a"]

    def step(cfg):
        m = nets[cfg]
        need = cfg != "a"
        og, dg = o.clone().requires_grad_(need), d.clone().requires_grad_(need)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = m.forward_rays(og, dg, ri, t0, t1)
        (out * c).sum().backward()
        b.record()
        b.synchronize()
        if need:
            assert og.grad is not None and dg.grad is not None and bool(torch.isfinite(og.grad).all())
        m.zero_grad(set_to_none=True)
        return a.elapsed_time(b)

    times = {k: [] for k in args.configs}
    for it in range(args.warmup + args.iters):
        for cfg in args.configs:  # alternate call by call: clock and thermal drift hit every configuration alike
            ms = step(cfg)
            if it >= args.warmup:
                times[cfg].append(ms)
    line = {"tool": "bench_input_grad", "tag": args.tag, "device": torch.cuda.get_device_name(0), "rays": R,
            "samples_per_ray": S, "net": "8x256 skip 4", "precision": nets["a"].precision, "iters": args.iters,
            "ms": {k: stats(v) for k, v in times.items()}}
    if "a" in times and "b" in times:
        line["b_over_a"] = round(line["ms"]["b"]["median"] / line["ms"]["a"]["median"], 4)
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
