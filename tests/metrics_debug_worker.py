"""Worker of tests/test_metrics_gpu.py: runs the SSIM kernel through the DEBUG library (FSN_LIB_PATH ->
libfsnerf_hip_dbg.so: every LDS index of k_ssim_tile range-checked, csrc/common.hpp) on both windows and on edge sizes
that are not a multiple of the tile, and prints the violation record as JSON."""
import torch

import debug_lib as D


def main():
    D.open_debug_library()
    from fs_nerf_amd.core import metrics
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for H, W in ((11, 11), (13, 17), (33, 65), (100, 75)):
        x = torch.rand(2, H, W, 3, device=dev, generator=g)
        y = torch.rand(2, H, W, 3, device=dev, generator=g)
        for gw in (True, False):
            metrics.ssim(x, y, gaussian_weights=gw, full=True)
    torch.cuda.synchronize()
    D.emit({"metrics": D.take("metrics"), "all": D.take_all()})


if __name__ == "__main__":
    main()
