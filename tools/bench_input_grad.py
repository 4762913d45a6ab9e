#!/usr/bin/env python3
"""Time the training pair with and without gradients to the rays (schedule: interleaved, tools/benchlib.py): 4096 rays x
192 samples (786,432 samples) through the 8 x 256 network in the ray form, `forward_rays` + `backward` of a fixed
cotangent, three configurations alternated call by call in one process:

  a  parameter gradients only (rays do not require grad: the step every earlier commit ran)
  b  parameters and rays      (fsn_nerf_train_bwd_inputs + fsn_ray_grad_reduce on top of a)
  c  rays only, frozen network in eval mode (the dgrad chain and the input gradient, no weight-gradient launches)

`--configs a` runs on a checkout without input gradients too (`--root` = the checkout whose package is imported), which
is how a is compared with the parent commit: both in one session on one device, alternating process by process. One JSON
line, printed and appended to --out.  Run it under a time limit of its own:

    timeout -k 10 300 python tools/bench_input_grad.py [--iters 20] [--warmup 3] [--out profiles/bench_input_grad.jsonl]
"""
import argparse

import torch

import benchlib
from benchlib import ROOT

R, S, NEAR, FAR = 4096, 192, 2.0, 6.0


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=20, warmup=3, out="bench_input_grad.jsonl")
    ap.add_argument("--configs", default="abc")
    ap.add_argument("--root", default=ROOT, help="checkout whose package is timed")
    args = ap.parse_args()
    benchlib.package(args.root)
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

        def pair():
            out = m.forward_rays(og, dg, ri, t0, t1)
            (out * c).sum().backward()
            return out
        ms, _ = benchlib.call_ms(pair)
        if need:
            assert og.grad is not None and dg.grad is not None and bool(torch.isfinite(og.grad).all())
        m.zero_grad(set_to_none=True)
        return ms, None

    # a step brackets its own timed part (the clones before it and the checks after it stay outside): it is its own clock
    times = benchlib.interleaved({cfg: (lambda cfg=cfg: step(cfg)) for cfg in args.configs}, args.iters, args.warmup,
                                 keep="samples", clock=lambda timed_step: timed_step())
    line = {**benchlib.header("bench_input_grad", args.tag), "rays": R,
            "samples_per_ray": S, "net": "8x256 skip 4", "precision": nets["a"].precision, "iters": args.iters,
            "ms": {k: benchlib.stats(v) for k, v in times.items()}}
    if "a" in times and "b" in times:
        line["b_over_a"] = round(line["ms"]["b"]["median"] / line["ms"]["a"]["median"], 4)
    benchlib.emit(line, args.out)


if __name__ == "__main__":
    main()
