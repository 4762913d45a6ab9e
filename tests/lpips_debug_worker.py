"""Worker of tests/test_lpips_gpu.py: runs LPIPS-VGG through the DEBUG library (FSN_LIB_PATH -> libfsnerf_hip_dbg.so:
every LDS index of k_lpips_conv range-checked, csrc/common.hpp) on sizes that are not a multiple of the tile, and prints
the violation record as JSON."""
import torch

import debug_lib as D


def main():
    D.open_debug_library()
    import lpips_ref as LR
    from fs_nerf_amd.core import metrics
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
    D.emit({"lpips": D.take("lpips"), "all": D.take_all()})


if __name__ == "__main__":
    main()
