"""Worker of tests/test_ssim_grad_gpu.py: runs the SSIM gradient through the DEBUG library (FSN_LIB_PATH ->
libfsnerf_hip_dbg.so: every LDS index of k_ssim_grad_maps and k_ssim_grad_filter range-checked, csrc/common.hpp) on the
smallest image (one interior pixel) and on one whose tiles are cut in both directions, with both windows, and prints
the violation record as JSON."""
import torch

import debug_lib as D


def main():
    D.open_debug_library()
    from fs_nerf_amd.core.loss import SSIMLoss
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for N, Ch, H, W in ((1, 1, 11, 11), (3, 3, 37, 70)):
        x = torch.rand(N, Ch, H, W, device=dev, generator=g).requires_grad_()
        y = torch.rand(N, Ch, H, W, device=dev, generator=g).requires_grad_()
        for gw in (True, False):
            SSIMLoss(gaussian_weights=gw, channel_axis=1)(x, y).backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(y.grad).all())
    D.emit({"ssim_grad": D.take("ssim_grad"), "all": D.take_all()})


if __name__ == "__main__":
    main()
