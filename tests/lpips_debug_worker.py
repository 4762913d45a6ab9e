"""Worker of tests/test_lpips_gpu.py: runs LPIPS-VGG through the DEBUG library (FSN_LIB_PATH -> libfsnerf_hip_dbg.so:
every LDS index of k_lpips_conv range-checked, csrc/common.hpp) on sizes that are not a multiple of the tile, and prints
the violation record as JSON."""
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import fs_nerf_amd  # noqa: F401
    import lpips_ref as LR
    from fs_nerf_amd import _lib as L
    from fs_nerf_amd.core import metrics
    assert "dbg" in os.path.basename(L.LIB_PATH), L.LIB_PATH
    dev = torch.device("cuda:0")
    m = metrics.LPIPS()
    m.load_state_dict(LR.random_state_dict(seed=1))
    m = m.to(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    for H, W in ((16, 16), (37, 53), (40, 70)):
        x = torch.rand(2, 3, H, W, device=dev, generator=g)
        y = torch.rand(2, 3, H, W, device=dev, generator=g)
        m(x, y, normalize=True)
    torch.cuda.synchronize()
    buf = (C.c_uint32 * 4)()
    L.check(L.lib().fsn_debug_report_lpips(buf), "fsn_debug_report_lpips")
    print("LPIPS_DEBUG_REPORT " + json.dumps(list(buf)), flush=True)


if __name__ == "__main__":
    main()
