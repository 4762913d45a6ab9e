#!/usr/bin/env python3
"""Time the SSIM loss and the patch loader on the GPU.  Schedule: in turns (tools/benchlib.py), warm-up 5, ms:

* forward + backward of core.loss.SSIMLoss on 64 patches of 32x32x3 and on one 800x800x3 pair, against the formulation
  a user would otherwise write - F.conv2d with the 11x11 Gaussian window per channel (float32, no padding: the
  'valid' output is the interior the mean is taken over) + autograd.  Medians of the --rounds 3 rounds' medians;
  the largest gradient difference between them is reported next to the times (the conv2d route is float32).
* one PatchLoader batch (64 patches of 32x32) against the explicit-index route: the anchor -> index arithmetic in torch
  followed by RayDataset.batch("explicit").

    python tools/bench_ssim_loss.py [--iters 50] [--rounds 3] [--out profiles/bench_ssim_loss.jsonl]
"""
import argparse
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import benchlib

benchlib.package()
from fs_nerf_amd.core.loss import SSIMLoss  # noqa: E402
from fs_nerf_amd.nerfdata import PatchLoader, RayDataset  # noqa: E402


def alternate(fns, iters, rounds):
    """{name: median over rounds of the round's median ms} and the rounds themselves; schedule: in turns, warm-up 5."""
    per = benchlib.in_turns(fns, iters, 5, rounds)
    return {k: float(np.median(v)) for k, v in per.items()}, {k: [round(t, 4) for t in v] for k, v in per.items()}


def conv2d_ssim_loss(x, y, window):
    """1 - mean SSIM of (N, C, H, W) float32 tensors, skimage's definition with torch ops (float32)."""
    N, C, H, W = x.shape
    cn = 121.0 / 120.0
    C1, C2 = 0.01 ** 2, 0.03 ** 2

    def filt(t):
        return F.conv2d(t.reshape(N * C, 1, H, W), window)  # 'valid': exactly the interior the mean is taken over
    ux, uy, uxx, uyy, uxy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    return 1.0 - S.reshape(N, -1).mean(dim=1).mean()


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=50, rounds=3, tag=False, out="bench_ssim_loss.jsonl")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim_loss: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    t = torch.arange(-5, 6, dtype=torch.float64)
    taps = torch.exp(-0.5 * (t / 1.5) ** 2)
    taps = taps / taps.sum()
    window = torch.outer(taps, taps).to(dev, torch.float32)[None, None]
    lines = []
    loss_fn = SSIMLoss(channel_axis=1)
    for name, shape, iters in (("64 patches 32x32x3", (64, 3, 32, 32), a.iters), ("one 800x800x3 pair", (1, 3, 800, 800), a.iters)):
        x = torch.rand(shape, device=dev, generator=g).requires_grad_()
        y = (x.detach() + 0.05 * torch.rand(shape, device=dev, generator=g)).clamp(0, 1)

        def hip():
            x.grad = None
            loss_fn(x, y).backward()

        def conv():
            x.grad = None
            conv2d_ssim_loss(x, y, window).backward()
        hip()
        g_hip = x.grad.clone()
        conv()
        g_conv = x.grad.clone()
        med, rounds = alternate({"ssim_loss_hip_ms": hip, "conv2d_autograd_f32_ms": conv}, iters, a.rounds)
        lines.append({"case": name, "what": "forward + backward, gradient to one input", **{k: round(v, 4) for k, v in med.items()},
                      "rounds": rounds, "max_abs_grad_difference_conv2d_f32_vs_hip": float((g_hip - g_conv).abs().max()),
                      "max_abs_grad_hip": float(g_hip.abs().max())})
        benchlib.emit(lines[-1])

    # the loader: 8 views of 400x400, 64 patches of 32x32 per batch
    H = W = 400
    P, B = 32, 64
    imgs = torch.randint(0, 256, (8, H, W, 3), device=dev, dtype=torch.uint8, generator=g)
    poses = torch.eye(4).repeat(8, 1, 1)
    poses[:, 2, 3] = 4.0
    ds = RayDataset(imgs, poses, (H, W, 500.0), near=2.0, far=6.0, device=dev)
    ld = PatchLoader(ds, P, B, seed=0)
    AH, AW = H - P + 1, W - P + 1
    grid = (torch.arange(P, device=dev)[:, None] * W + torch.arange(P, device=dev)[None, :]).reshape(-1)
    state = {"it": iter(ld)}

    def patch_loader():
        try:
            return next(state["it"])
        except StopIteration:
            state["it"] = iter(ld)
            return next(state["it"])

    def explicit_route():
        anchors = torch.randint(0, 8 * AH * AW, (B,), device=dev, generator=g)
        v, rest = anchors // (AH * AW), anchors % (AH * AW)
        top_left = (v * H + rest // AW) * W + rest % AW
        return ds.batch("explicit", indices=(top_left[:, None] + grid[None, :]).reshape(-1))[:3]
    med, rounds = alternate({"patch_loader_ms": patch_loader, "explicit_index_route_ms": explicit_route}, a.iters, a.rounds)
    lines.append({"case": "one batch: 64 patches 32x32 from 8 views 400x400", **{k: round(v, 4) for k, v in med.items()},
                  "rounds": rounds})
    benchlib.emit(lines[-1])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
