"""Python restatement of the patch geometry of fsn_ray_patch_batch (csrc/raydata.hip) for tests/test_patch_loader_cpu.py
and tests/test_patch_loader_gpu.py: anchors (the patches' top-left pixels) -> flat ray indices."""
import numpy as np


def n_anchors(n_views, H, W, P, dilation):
    ext = (P - 1) * dilation + 1
    return n_views * (H - ext + 1) * (W - ext + 1)


def patch_indices(anchors, H, W, P, dilation):
    """anchors [B] -> flat ray indices [B * P * P], int64: row (b P + i) P + j is pixel (i, j) of patch b."""
    ext = (P - 1) * dilation + 1
    AH, AW = H - ext + 1, W - ext + 1
    out = []
    for a in np.asarray(anchors, dtype=np.int64).tolist():
        v, rest = divmod(a, AH * AW)
        r0, c0 = divmod(rest, AW)
        for i in range(P):
            for j in range(P):
                out.append((v * H + r0 + i * dilation) * W + c0 + j * dilation)
    return np.asarray(out, dtype=np.int64)
