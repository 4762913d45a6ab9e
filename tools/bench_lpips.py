#!/usr/bin/env python3
"""Time fs_nerf_amd.core.metrics.LPIPS (VGG16, csrc/lpips.hip; schedule: in turns, tools/benchlib.py, one variant and one
round at a time, warm-up 3): median of --iters calls at 800x800
and 378x504, one pair and eight pairs.  Prints ms per pair and the achieved TFLOP/s of the convolutions (2 * pixels *
Cout * 9 * Cin summed over the 13 layers and both images; 391.6 GFLOP per 800x800 image).  Random weights in the
package's layout (timing does not depend on their values).

    python tools/bench_lpips.py [--n 1 8] [--iters 50]
"""
import argparse
import os
import sys

import numpy as np
import torch

import benchlib

sys.path.insert(0, os.path.join(benchlib.package(), "tests"))
from fs_nerf_amd.core import metrics  # noqa: E402
import lpips_ref as LR  # noqa: E402


def device_ms(fn, iters, warmup=3):
    """(median, min) of the in-turns schedule's samples for one variant."""
    times = benchlib.in_turns({"fn": fn}, iters, warmup, keep="samples")["fn"]
    return float(np.median(times)), float(np.min(times))


def conv_flop(H, W):
    """FLOP of the 13 convolutions on one H x W image."""
    total, h, w = 0, H, W
    for _, idx, cin, cout in LR.CONVS:
        if idx in LR.POOL_BEFORE:
            h, w = h // 2, w // 2
        total += 2 * h * w * cout * 9 * cin
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--sizes", type=str, nargs="+", default=["800x800", "378x504"])
    benchlib.common_args(ap, iters=50, tag=False)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = metrics.LPIPS()
    m.load_state_dict(LR.random_state_dict(seed=0))
    m = m.to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        for n in a.n:
            x = torch.rand(n, 3, H, W, device=dev, generator=g)
            y = (x + 0.05 * torch.rand(n, 3, H, W, device=dev, generator=g)).clamp(0, 1)
            with torch.no_grad():
                med, mn = device_ms(lambda: m(x, y, normalize=True), a.iters)
            flop = 2 * n * conv_flop(H, W)
            benchlib.emit({"hw": f"{H}x{W}", "pairs": n, "ms": round(med, 3), "ms_min": round(mn, 3),
                           "ms_per_pair": round(med / n, 3), "conv_gflop_per_image": round(conv_flop(H, W) / 1e9, 1),
                           "tflops": round(flop / (med * 1e-3) / 1e12, 1)})


if __name__ == "__main__":
    main()
