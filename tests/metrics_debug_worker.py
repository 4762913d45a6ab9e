"""Worker of tests/test_metrics_gpu.py: runs the SSIM kernel through the DEBUG library (FSN_LIB_PATH ->
libfsnerf_hip_dbg.so: every LDS index of k_ssim_tile range-checked, csrc/common.hpp) on both windows and on edge sizes
that are not a multiple of the tile, and prints the violation record as JSON."""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd import _lib as L
    from fs_nerf_amd.core import metrics
    assert "dbg" in os.path.basename(L.LIB_PATH), L.LIB_PATH
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for H, W in ((11, 11), (13, 17), (33, 65), (100, 75)):
        x = torch.rand(2, H, W, 3, device=dev, generator=g)
        y = torch.rand(2, H, W, 3, device=dev, generator=g)
        for gw in (True, False):
            metrics.ssim(x, y, gaussian_weights=gw, full=True)
    torch.cuda.synchronize()
    buf = (C.c_uint32 * 4)()
    L.check(L.lib().fsn_debug_report_metrics(buf), "fsn_debug_report_metrics")
    print("METRICS_DEBUG_REPORT " + json.dumps(list(buf)), flush=True)


if __name__ == "__main__":
    main()
