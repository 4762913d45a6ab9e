"""Worker of tests/test_ssim_grad_gpu.py: runs the SSIM gradient through the DEBUG library (FSN_LIB_PATH ->
libfsnerf_hip_dbg.so: every LDS index of k_ssim_grad_maps and k_ssim_grad_filter range-checked, csrc/common.hpp) on the
smallest image (one interior pixel) and on one whose tiles are cut in both directions, with both windows, and prints
the violation record as JSON."""
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
    from fs_nerf_amd.core.loss import SSIMLoss
    assert "dbg" in os.path.basename(L.LIB_PATH), L.LIB_PATH
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for N, Ch, H, W in ((1, 1, 11, 11), (3, 3, 37, 70)):
        x = torch.rand(N, Ch, H, W, device=dev, generator=g).requires_grad_()
        y = torch.rand(N, Ch, H, W, device=dev, generator=g).requires_grad_()
        for gw in (True, False):
            SSIMLoss(gaussian_weights=gw, channel_axis=1)(x, y).backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(y.grad).all())
    buf = (C.c_uint32 * 4)()
    L.check(L.lib().fsn_debug_report_ssim_grad(buf), "fsn_debug_report_ssim_grad")
    print("SSIM_GRAD_DEBUG_REPORT " + json.dumps(list(buf)), flush=True)


if __name__ == "__main__":
    main()
