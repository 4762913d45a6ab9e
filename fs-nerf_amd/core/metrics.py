"""Evaluation metrics of the reference's driver loop on the device: PSNR, SSIM and `evaluation()`
(src/run-nerf.py:108-191).

`ssim` takes the keywords of skimage.metrics.structural_similarity (scikit-image 0.22, the version the reference pins) and
restates its arithmetic in HIP (csrc/metrics.hip): the Gaussian window of `gaussian_weights=True` (sigma 1.5, 11 taps) or
the default 7 x 7 box, scipy's `mode='reflect'` edges, the mean of the SSIM map over its interior in float64.  `psnr` is
the reference's `-10 * log10(F.mse_loss(rgbs, rgbs_gt))`.  Both read their inputs in place through their strides (NHWC,
NCHW or a permuted view), return device tensors and never copy a frame to the host.  There is no CPU fallback: CPU
tensors raise.  LPIPS is not provided: the reference computes it and then discards it (`val_lpips = None`, :178)."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from .. import _lib as L
from .. import ops

_GAUSS_WIN, _GAUSS_SIGMA = 11, 1.5
_UNIFORM_WIN = 7


def _check_device(t: Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")


def _as_nchw(t: Tensor, channel_axis: Optional[int]) -> Tensor:
    """(H, W), (H, W, C), (C, H, W), (N, H, W, C) or (N, C, H, W) -> an (N, C, H, W) VIEW of the same storage."""
    if t.dim() == 2:
        if channel_axis not in (None, -1):
            raise ValueError(f"channel_axis={channel_axis} for a 2-D (H, W) image: use None or -1")
        return t[None, None]
    if t.dim() == 3:
        if channel_axis in (-1, 2):
            return t.permute(2, 0, 1)[None]
        if channel_axis in (0, -3):
            return t[None]
        raise ValueError(f"channel_axis={channel_axis} for a 3-D image: expected -1 / 2 (H, W, C) or 0 (C, H, W)")
    if t.dim() == 4:
        if channel_axis in (-1, 3):
            return t.permute(0, 3, 1, 2)
        if channel_axis in (1, -3):
            return t
        raise ValueError(f"channel_axis={channel_axis} for a batch: expected -1 (N, H, W, C) or 1 (N, C, H, W)")
    raise ValueError(f"expected a 2-D, 3-D or 4-D image tensor, got shape {tuple(t.shape)}")


def ssim(im1: Tensor, im2: Tensor, *, data_range: Optional[float] = 1.0, channel_axis: Optional[int] = -1,
         gaussian_weights: bool = True, use_sample_covariance: bool = True, K1: float = 0.01, K2: float = 0.03,
         win_size: Optional[int] = None, sigma: float = _GAUSS_SIGMA, full: bool = False, reduction: str = "mean"):
    """skimage.metrics.structural_similarity on device tensors, for one image or a batch.

    Shapes: (H, W); (H, W, C) with channel_axis=-1 (or (C, H, W) with 0); (N, H, W, C) with channel_axis=-1;
    (N, C, H, W) with channel_axis=1.  Every channel is compared on its own and the channel means are averaged, as
    skimage does.  reduction="mean" -> 0-dim float64 tensor (the mean over the N images, the reference's average over
    frames); "none" -> float64 (N,).  full=True returns (value, S) with the uncropped float32 SSIM map in im1's shape.
    Windows: gaussian_weights=True (sigma 1.5, win_size 11) and the 7 x 7 box (gaussian_weights=False); any other
    win_size / sigma raises ValueError, and so does data_range=None (skimage would guess it from the dtype)."""
    if im1.shape != im2.shape:
        raise ValueError(f"input images must have the same shape: {tuple(im1.shape)} vs {tuple(im2.shape)}")
    if reduction not in ("mean", "none"):
        raise ValueError(f"reduction must be 'mean' or 'none', got {reduction!r}")
    if data_range is None:
        raise ValueError("data_range is required (the reference passes data_range=1.0)")
    if gaussian_weights:
        if win_size not in (None, _GAUSS_WIN) or float(sigma) != _GAUSS_SIGMA:
            raise ValueError(f"only the Gaussian window of sigma {_GAUSS_SIGMA} (win_size {_GAUSS_WIN}) is built")
        window, win = L.FSN_SSIM_GAUSSIAN, _GAUSS_WIN
    else:
        if win_size not in (None, _UNIFORM_WIN):
            raise ValueError(f"only the {_UNIFORM_WIN} x {_UNIFORM_WIN} uniform window is built")
        window, win = L.FSN_SSIM_UNIFORM, _UNIFORM_WIN
    x, y = _as_nchw(im1, channel_axis), _as_nchw(im2, channel_axis)
    H, W = x.shape[2], x.shape[3]
    if H < win or W < win:
        raise ValueError(f"win_size exceeds image extent: {H} x {W} image, {win} x {win} window")
    _check_device(im1, "im1")
    _check_device(im2, "im2")
    smap = smap_nchw = None
    if full:
        smap = torch.empty(im1.shape, dtype=torch.float32, device=im1.device)
        smap_nchw = _as_nchw(smap, channel_axis)
    out = ops.ssim_nchw(x, y, window, use_sample_covariance, float(data_range), float(K1), float(K2), smap_nchw)
    N = x.shape[0]
    val = out[N] if reduction == "mean" else out[:N]
    return (val, smap) if full else val


def _as_batch(t: Tensor) -> Tensor:
    if t.dim() == 2:
        return t[None, None]
    if t.dim() == 3:
        return t[None]
    if t.dim() == 4:
        return t
    raise ValueError(f"expected a 2-D, 3-D or 4-D image tensor, got shape {tuple(t.shape)}")


def psnr(pred: Tensor, gt: Tensor, reduction: str = "stack") -> Tensor:
    """-10 * log10(MSE) on the device, data range 1 (run-nerf.py:160).  reduction="stack": one MSE over every element
    of the batch (the reference's F.mse_loss over the stacked frames) -> 0-dim float32; "none": each image's PSNR ->
    float32 (N,).  A 4-D tensor is a batch of N images along its first dimension; a 2-D or 3-D tensor is one image."""
    if pred.shape != gt.shape:
        raise ValueError(f"pred and gt must have the same shape: {tuple(pred.shape)} vs {tuple(gt.shape)}")
    if reduction not in ("stack", "none"):
        raise ValueError(f"reduction must be 'stack' or 'none', got {reduction!r}")
    x, y = _as_batch(pred), _as_batch(gt)
    _check_device(pred, "pred")
    _check_device(gt, "gt")
    # fsn_psnr walks (h, w, c) with c fastest: as (N, d3, d1, d2) views, each image is summed in its logical row-major
    # order, whatever the storage layout (a permuted view gives the bits of its contiguous copy)
    out = ops.psnr_nchw(x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2))
    N = x.shape[0]
    return out[N] if reduction == "stack" else out[:N]


def evaluation(hwf, model, estimator, lpips_net, data_loader, chunksize: int, device, render_step_size: float = 5e-3, *,
               white_bkgd: bool = False):
    """The reference's evaluation() (run-nerf.py:108-191) on this package: every validation view through render_frame,
    the frames kept on the device, then PSNR over the stack and SSIM per frame averaged over frames, each in one launch.
    data_loader: an iterable of (rgb_gt [1,H,W,3], pose [1,4,4]) whose `.dataset` has near, far and ndc.  lpips_net is
    accepted and ignored (the reference discards LPIPS).  white_bkgd is keyword-only: the reference reads it from its
    global `args`.  Returns (psnr: 0-dim float32 tensor on the device, ssim: float, None)."""
    from ..render import rendering as R

    ds = data_loader.dataset
    rgbs, gts = [], []
    with torch.no_grad():
        for rgb_gt, pose in data_loader:
            gts.append(rgb_gt)
            rgb, _ = R.render_frame(hwf, ds.near, ds.far, pose[0], chunksize, estimator, model, train=False, ndc=ds.ndc,
                                    white_bkgd=white_bkgd, render_step_size=render_step_size, device=device)
            rgbs.append(rgb)
    rgbs = torch.stack(rgbs, dim=0)
    gts = torch.cat(gts, dim=0).to(device=rgbs.device, dtype=torch.float32)
    val_psnr = psnr(rgbs, gts)
    val_ssim = float(ssim(rgbs, gts, channel_axis=-1, data_range=1.0, gaussian_weights=True))
    return val_psnr, val_ssim, None
