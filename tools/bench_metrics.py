#!/usr/bin/env python3
"""Time fs_nerf_amd.core.metrics.ssim + psnr on N pairs of 800x800x3 frames (schedule: in turns, tools/benchlib.py, one
variant and one round at a time, warm-up 5), and, for comparison,
the float64 restatement of skimage's SSIM on the host (tests/metrics_ref.py; scipy's filters when scipy is present).

    python tools/bench_metrics.py [--n 1 8] [--iters 50] [--host-iters 1]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

import benchlib

sys.path.insert(0, os.path.join(benchlib.package(), "tests"))
from fs_nerf_amd.core import metrics  # noqa: E402


def device_ms(fn, iters, warmup=5):
    """(median, min) of the in-turns schedule's samples for one variant."""
    times = benchlib.in_turns({"fn": fn}, iters, warmup, keep="samples")["fn"]
    return float(np.median(times)), float(np.min(times))


def host_ssim_s(x, y):
    """One SSIM over the pairs on the host, float64 (scipy's gaussian_filter when available, else the NumPy
    restatement)."""
    try:
        from scipy.ndimage import gaussian_filter
    except ImportError:
        gaussian_filter = None
    import metrics_ref as MR
    t0 = time.perf_counter()
    for n in range(x.shape[0]):
        if gaussian_filter is None:
            MR.ssim(x[n], y[n])
            continue
        for c in range(x.shape[-1]):
            a, b = x[n, ..., c].astype(np.float64), y[n, ..., c].astype(np.float64)
            for m in (a, b, a * a, b * b, a * b):
                gaussian_filter(m, sigma=1.5, truncate=3.5, mode="reflect")
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--hw", type=int, default=800)
    benchlib.common_args(ap, iters=50, tag=False)
    ap.add_argument("--host-iters", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for n in a.n:
        x = torch.rand(n, a.hw, a.hw, 3, device=dev, generator=g)
        y = (x + 0.05 * torch.rand(n, a.hw, a.hw, 3, device=dev, generator=g)).clamp(0, 1)
        s_med, s_min = device_ms(lambda: metrics.ssim(x, y), a.iters)
        p_med, p_min = device_ms(lambda: metrics.psnr(x, y), a.iters)
        b_med, b_min = device_ms(lambda: (metrics.ssim(x, y), metrics.psnr(x, y)), a.iters)
        xh, yh = x.cpu().numpy(), y.cpu().numpy()
        host = min(host_ssim_s(xh, yh) for _ in range(a.host_iters))
        benchlib.emit({"pairs": n, "hw": a.hw, "ssim_ms": round(s_med, 4), "psnr_ms": round(p_med, 4),
                       "ssim_psnr_ms": round(b_med, 4), "ssim_psnr_ms_min": round(b_min, 4),
                       "per_pair_ms": round(b_med / n, 4), "host_filters_s": round(host, 3)})


if __name__ == "__main__":
    main()
