#!/usr/bin/env python3
"""Time the LPIPS loss on the GPU.  Schedule: in turns (tools/benchlib.py), warm-up 3, ms:

* forward + backward of core.loss.LPIPSLoss (gradient to the first input) on 64 patches of 32x32, 16 patches of 64x64
  and one 800x800 pair, against the same network written with F.conv2d / F.max_pool2d and torch autograd in float32 -
  what a user would otherwise build next to the package's own VGG16.  Medians of the --rounds 3 rounds'
  medians; the largest gradient difference between them is reported next to the times.
* the evaluation forward (metrics.LPIPS under no_grad) on the 800x800 pair; with --parent-lib LIB (a libfsnerf_hip.so
  built from the parent commit) a child process times the same call through that library, the two processes taking
  turns, to show that the metric's path did not slow down.  Without it that line says "not measured".

    python tools/bench_lpips_loss.py [--iters 20] [--rounds 3] [--parent-lib LIB] [--out profiles/bench_lpips_loss.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import benchlib

sys.path.insert(0, os.path.join(benchlib.package(), "tests"))
import lpips_ref as LR  # noqa: E402
from fs_nerf_amd.core import metrics  # noqa: E402
from fs_nerf_amd.core.loss import LPIPSLoss  # noqa: E402


def alternate(fns, iters, rounds):
    """{name: median over rounds of the round's median ms} and the rounds themselves; schedule: in turns, warm-up 3."""
    per = benchlib.in_turns(fns, iters, 3, rounds)
    return {k: float(np.median(v)) for k, v in per.items()}, {k: [round(t, 4) for t in v] for k, v in per.items()}


class TorchLPIPS:
    """LPIPS-VGG with torch ops in float32 (the formula of tests/lpips_ref.py, with autograd)."""

    def __init__(self, sd, dev):
        self.w = [(sd[f"net.slice{s}.{i}.weight"].to(dev), sd[f"net.slice{s}.{i}.bias"].to(dev), i) for s, i, _, _ in LR.CONVS]
        self.lin = [sd[f"lin{k}.model.1.weight"].to(dev) for k in range(5)]
        self.shift = torch.tensor(LR.SHIFT, device=dev).reshape(1, 3, 1, 1)
        self.scale = torch.tensor(LR.SCALE, device=dev).reshape(1, 3, 1, 1)

    def features(self, t):
        t = (2 * t - 1 - self.shift) / self.scale
        taps = []
        for w, b, i in self.w:
            if i in LR.POOL_BEFORE:
                t = F.max_pool2d(t, 2, 2)
            t = F.relu(F.conv2d(t, w, b, padding=1))
            if i in LR.TAP_AFTER:
                taps.append(t)
        return taps

    def __call__(self, x, y):
        total = 0
        for k, (a, b) in enumerate(zip(self.features(x), self.features(y))):
            na = a / (torch.sqrt(torch.sum(a * a, dim=1, keepdim=True)) + LR.EPS)
            nb = b / (torch.sqrt(torch.sum(b * b, dim=1, keepdim=True)) + LR.EPS)
            total = total + F.conv2d((na - nb) ** 2, self.lin[k]).mean(dim=(1, 2, 3))
        return total.mean()


def eval_forward_ms(iters):
    """The evaluation forward on one 800x800 pair: the median of `iters` device-event timings."""
    dev = torch.device("cuda:0")
    net = metrics.LPIPS()
    net.load_state_dict(LR.random_state_dict(seed=7))
    net = net.to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    x, y = torch.rand(1, 3, 800, 800, device=dev, generator=g), torch.rand(1, 3, 800, 800, device=dev, generator=g)

    def run():
        with torch.no_grad():
            net(x, y, normalize=True)
    return benchlib.in_turns({"eval": run}, iters, 3)["eval"][0]


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=20, rounds=3, tag=False, out="bench_lpips_loss.jsonl")
    ap.add_argument("--parent-lib", default=None, help="libfsnerf_hip.so of the parent commit (evaluation-forward comparison)")
    ap.add_argument("--eval-forward-only", action="store_true", help="(child mode) print the evaluation forward's ms and exit")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips_loss: needs the GPU (a CPU run measures nothing)")
    if a.eval_forward_only:
        print("EVAL_FORWARD_MS " + json.dumps(eval_forward_ms(a.iters)), flush=True)
        return
    dev = torch.device("cuda:0")
    sd = LR.random_state_dict(seed=7)
    net = metrics.LPIPS()
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    loss_fn = LPIPSLoss(net, normalize=True, channel_axis=1)
    ref = TorchLPIPS(sd, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for name, shape, iters in (("64 patches 32x32", (64, 3, 32, 32), a.iters), ("16 patches 64x64", (16, 3, 64, 64), a.iters),
                               ("one 800x800 pair", (1, 3, 800, 800), max(3, a.iters // 4))):
        x = torch.rand(shape, device=dev, generator=g).requires_grad_()
        y = (x.detach() + 0.1 * torch.rand(shape, device=dev, generator=g)).clamp(0, 1)

        def hip():
            x.grad = None
            loss_fn(x, y).backward()

        def conv():
            x.grad = None
            ref(x, y).backward()
        hip()
        g_hip = x.grad.clone()
        conv()
        g_conv = x.grad.clone()
        med, rounds = alternate({"lpips_loss_hip_ms": hip, "conv2d_autograd_f32_ms": conv}, iters, a.rounds)
        lines.append({"case": name, "what": "forward + backward, gradient to one input",
                      **{k: round(v, 4) for k, v in med.items()}, "rounds": rounds,
                      "pairs_per_pass": metrics.lpips_pairs_per_pass(shape[2], shape[3], True, False, loss_fn.max_workspace_bytes),
                      "max_abs_grad_difference_conv2d_f32_vs_hip": float((g_hip - g_conv).abs().max()),
                      "max_abs_grad_hip": float(g_hip.abs().max())})
        benchlib.emit(lines[-1])
        del x, y, g_hip, g_conv
        torch.cuda.empty_cache()

    # the evaluation forward, this library against the parent commit's, each in a process of its own, taking turns
    line = {"case": "one 800x800 pair", "what": "evaluation forward (no_grad)"}
    if a.parent_lib:
        per = {"this_commit_ms": [], "parent_commit_ms": []}
        for _ in range(a.rounds):
            for key, lib in (("this_commit_ms", None), ("parent_commit_ms", a.parent_lib)):
                env = dict(os.environ)
                if lib:  # (an older library exports a subset of the symbols)
                    env["FSN_LIB_PATH"], env["FSN_LIB_PARTIAL"] = os.path.abspath(lib), "1"
                else:
                    env.pop("FSN_LIB_PATH", None)
                per[key].append(benchlib.run_child(
                    [sys.executable, os.path.abspath(__file__), "--eval-forward-only", "--iters", str(a.iters)], env, 600,
                    "bench_lpips_loss: the evaluation-forward child", "EVAL_FORWARD_MS "))
        line.update({k: round(float(np.median(v)), 4) for k, v in per.items()})
        line["rounds"] = {k: [round(t, 4) for t in v] for k, v in per.items()}
    else:
        line.update({"this_commit_ms": round(eval_forward_ms(a.iters), 4), "parent_commit_ms": "not measured"})
    lines.append(line)
    benchlib.emit(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
