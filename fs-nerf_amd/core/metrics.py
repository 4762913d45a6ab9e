"""Evaluation metrics of the reference's driver loop on the device: PSNR, SSIM and `evaluation()`
(src/run-nerf.py:108-191).

`ssim` takes the keywords of skimage.metrics.structural_similarity (scikit-image 0.22, the version the reference pins) and
restates its arithmetic in HIP (csrc/metrics.hip): the Gaussian window of `gaussian_weights=True` (sigma 1.5, 11 taps) or
the default 7 x 7 box, scipy's `mode='reflect'` edges, the mean of the SSIM map over its interior in float64.  `psnr` is
the reference's `-10 * log10(F.mse_loss(rgbs, rgbs_gt))`.  Both read their inputs in place through their strides (NHWC,
NCHW or a permuted view), return device tensors and never copy a frame to the host.  There is no CPU fallback: CPU
tensors raise.

`LPIPS(net="vgg")` is the `lpips` package's LPIPS v0.1 with the VGG16 backbone, as a module with that package's
parameter names, run by csrc/lpips.hip (implicit-GEMM convolutions on the f32 MFMA).  It ships no weights and downloads
nothing: load the package's own state dict (`m.load_state_dict(torch.load("lpips_vgg.pt"))`).  `evaluation()` computes
LPIPS only when it is given this class; the reference computes it and then discards it (`val_lpips = None`, :178).
Called with grad enabled on an input that requires grad it returns a value that carries the gradient to that input
(`_LPIPSFn`; `core.loss.LPIPSLoss` is the training-loop face of it); the weights stay frozen."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

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


# ---------------------------------------------------------------- LPIPS (VGG16, v0.1)
_VGG_CONVS = ((1, 0, 3, 64), (1, 2, 64, 64), (2, 5, 64, 128), (2, 7, 128, 128), (3, 10, 128, 256), (3, 12, 256, 256),
              (3, 14, 256, 256), (4, 17, 256, 512), (4, 19, 512, 512), (4, 21, 512, 512), (5, 24, 512, 512),
              (5, 26, 512, 512), (5, 28, 512, 512))  # (slice, torchvision `features` index, Cin, Cout)
_SLICE_RANGES = {1: range(0, 4), 2: range(4, 9), 3: range(9, 16), 4: range(16, 23), 5: range(23, 30)}
_TAP_CHANNELS = (64, 128, 256, 512, 512)
_SHIFT = (-0.030, -0.088, -0.188)
_SCALE = (0.458, 0.448, 0.450)
_MIN_SIDE = 16  # four 2x2 pools leave relu5_3 at least one pixel


class _ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(_SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(_SCALE)[None, :, None, None])


class _LinLayer(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(c, 1, 1, stride=1, padding=0, bias=False))


class _VGG16Slices(nn.Module):
    """`lpips.pretrained_networks.vgg16`'s module tree: slice1..slice5 hold torchvision's `features` modules under
    their original indices, so the state-dict keys are the package's (net.slice1.0.weight ... net.slice5.28.bias)."""

    def __init__(self):
        super().__init__()
        convs = {idx: (cin, cout) for _, idx, cin, cout in _VGG_CONVS}
        for k, rng in _SLICE_RANGES.items():
            seq = nn.Sequential()
            for i in rng:
                if i in convs:
                    seq.add_module(str(i), nn.Conv2d(convs[i][0], convs[i][1], 3, padding=1))
                elif i in (4, 9, 16, 23):
                    seq.add_module(str(i), nn.MaxPool2d(2, 2))
                else:
                    seq.add_module(str(i), nn.ReLU(inplace=False))
            setattr(self, f"slice{k}", seq)

    def convs(self):
        return [getattr(getattr(self, f"slice{s}"), str(i)) for s, i, _, _ in _VGG_CONVS]


TRAIN_WORKSPACE_BYTES = 1 << 30  # default bound of one training pass's workspace (a setting, not a measurement)


def lpips_pairs_per_pass(H: int, W: int, want_dx: bool, want_dy: bool, max_workspace_bytes: int) -> int:
    """The most pairs whose training workspace (fsn_lpips_train_workspace_floats: linear in the pairs) fits
    `max_workspace_bytes`; at least one, whatever its size."""
    one = 4 * ops._size("fsn_lpips_train_workspace_floats", None, 1, H, W, int(want_dx), int(want_dy))
    return int(max(1, min(max_workspace_bytes // one, 32767)))


class _LPIPSFn(torch.autograd.Function):
    """LPIPS of N pairs with gradients to the images in one node: forward = fsn_lpips_vgg_fwd_save per chunk of
    `pairs_per_pass` pairs (the metric's values bit for bit), backward = fsn_lpips_vgg_bwd per chunk for the inputs
    that need a gradient.  One chunk keeps its activations for the backward; with several the backward runs each
    chunk's forward again (the same bits), so that no more than one chunk's workspace is alive at a time.  The per-tap
    values are returned for reading only (not differentiable)."""

    @staticmethod
    def forward(ctx, in0, in1, net, normalize, pairs_per_pass):
        want_dx, want_dy = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        N = in0.shape[0]
        packed = net.packed()
        vals, pers, ws = [], [], None
        for n0 in range(0, N, pairs_per_pass):
            v, p, ws = ops.lpips_vgg_fwd_save(packed, in0[n0:n0 + pairs_per_pass], in1[n0:n0 + pairs_per_pass], normalize,
                                              want_dx=want_dx, want_dy=want_dy)
            vals.append(v)
            pers.append(p)
        ctx.save_for_backward(in0, in1)
        ctx.net, ctx.normalize, ctx.ppp = net, bool(normalize), pairs_per_pass
        ctx.ws = ws if N <= pairs_per_pass else None
        val, per = torch.cat(vals), torch.cat(pers, dim=1)
        ctx.mark_non_differentiable(per)
        return val, per

    @staticmethod
    @once_differentiable
    def backward(ctx, d_val, _d_per):
        in0, in1 = ctx.saved_tensors
        want_dx, want_dy = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_dx or want_dy):
            return None, None, None, None, None
        net, N = ctx.net, in0.shape[0]
        packed, packed_grad = net.packed(), net.packed_grad()
        d0 = torch.empty_like(in0) if want_dx else None
        d1 = torch.empty_like(in1) if want_dy else None
        for n0 in range(0, N, ctx.ppp):
            sl = slice(n0, n0 + ctx.ppp)
            ws = ctx.ws
            if ws is None:
                _, _, ws = ops.lpips_vgg_fwd_save(packed, in0[sl], in1[sl], ctx.normalize, want_dx=want_dx, want_dy=want_dy)
            ops.lpips_vgg_bwd(packed, packed_grad, ws, in0[sl].shape, ctx.normalize, d_val[sl], want_dx=want_dx,
                              want_dy=want_dy, dx=None if d0 is None else d0[sl], dy=None if d1 is None else d1[sl])
        ctx.ws = None
        return d0, d1, None, None, None


class LPIPS(nn.Module):
    """LPIPS v0.1 with the VGG16 backbone on the device: the `lpips` package's `LPIPS(net="vgg")` forward (no spatial
    map; gradients to the images, not to the weights).  Parameter and buffer names are the package's, so its state dict loads as it is; the
    `lins.K.model.1.weight` aliases of its module list are accepted, and `scaling_layer.*` is optional (the package's
    constants).  The constructor downloads nothing and the module holds no usable weights until `load_state_dict`:
    calling it before raises.  The weights are packed for the kernels once per weight version (csrc/lpips.hip)."""

    def __init__(self, net: str = "vgg", version: str = "0.1"):
        super().__init__()
        if net != "vgg":
            raise NotImplementedError(f"LPIPS(net={net!r}): only the VGG16 backbone is built")
        if version != "0.1":
            raise NotImplementedError(f"LPIPS(version={version!r}): only v0.1 is built")
        self.scaling_layer = _ScalingLayer()
        self.net = _VGG16Slices()
        for k, c in enumerate(_TAP_CHANNELS):
            setattr(self, f"lin{k}", _LinLayer(c))
        for p in self.parameters():
            p.requires_grad_(False)
        self._loaded = False
        self._packed = None
        self._packed_key = None
        self._packed_grad = None
        self._packed_grad_key = None
        self._register_load_state_dict_pre_hook(self._accept_package_keys)

    @staticmethod
    def _accept_package_keys(state_dict, prefix, *args):
        for k in range(len(_TAP_CHANNELS)):
            alias, key = f"{prefix}lins.{k}.model.1.weight", f"{prefix}lin{k}.model.1.weight"
            if alias in state_dict:
                v = state_dict.pop(alias)
                state_dict.setdefault(key, v)
        for name, val in (("shift", _SHIFT), ("scale", _SCALE)):
            state_dict.setdefault(f"{prefix}scaling_layer.{name}", torch.tensor(val)[None, :, None, None])

    def load_state_dict(self, state_dict, strict: bool = True, **kwargs):
        out = super().load_state_dict(state_dict, strict=strict, **kwargs)
        self._loaded = not out.missing_keys
        self._packed_key = None
        self._packed_grad_key = None
        return out

    def _tensors(self):
        return ([c.weight for c in self.net.convs()] + [c.bias for c in self.net.convs()]
                + [getattr(self, f"lin{k}").model[1].weight for k in range(len(_TAP_CHANNELS))]
                + [self.scaling_layer.shift, self.scaling_layer.scale])

    def packed(self) -> Tensor:
        """The kernels' weight blob, re-packed when a parameter or buffer changed (data pointer or version)."""
        ts = self._tensors()
        key = tuple((t.data_ptr(), t._version) for t in ts)
        if self._packed is None or key != self._packed_key:
            self._packed = ops.lpips_pack(ts[:13], ts[13:26], ts[26:31], ts[31], ts[32], out=self._packed)
            self._packed_key = key
        return self._packed

    def packed_grad(self) -> Tensor:
        """The data-gradient kernels' weight blob (the convolutions transposed, csrc/lpips.hip), packed on the first
        loss call and re-packed when a convolution weight changed: keyed like `packed()`."""
        ws = self._tensors()[:13]
        key = tuple((t.data_ptr(), t._version) for t in ws)
        if self._packed_grad is None or key != self._packed_grad_key:
            self._packed_grad = ops.lpips_grad_pack(ws, out=self._packed_grad)
            self._packed_grad_key = key
        return self._packed_grad

    def forward(self, in0: Tensor, in1: Tensor, retPerLayer: bool = False, normalize: bool = False):
        """in0, in1: (N, 3, H, W) device tensors (any strides), in [-1, 1], or in [0, 1] with normalize=True.
        Returns float32 (N, 1, 1, 1), and with retPerLayer the five taps' values as a list of (N, 1, 1, 1) too.
        With grad enabled and an input that requires grad (float32), the value carries the gradient to that input
        (the per-tap values do not); the weights are frozen: a parameter that requires grad raises."""
        if not self._loaded:
            raise RuntimeError("LPIPS: no weights loaded (load the lpips package's VGG state dict with load_state_dict)")
        if in0.shape != in1.shape:
            raise ValueError(f"in0 and in1 must have the same shape: {tuple(in0.shape)} vs {tuple(in1.shape)}")
        if in0.dim() != 4 or in0.shape[1] != 3:
            raise ValueError(f"expected (N, 3, H, W) images, got shape {tuple(in0.shape)}")
        if in0.shape[2] < _MIN_SIDE or in0.shape[3] < _MIN_SIDE:
            raise ValueError(f"LPIPS-VGG needs images of at least {_MIN_SIDE} x {_MIN_SIDE}, got "
                             f"{in0.shape[2]} x {in0.shape[3]}")
        _check_device(in0, "in0")
        _check_device(in1, "in1")
        dev = self.scaling_layer.shift.device
        if in0.device != dev or in1.device != dev:
            raise RuntimeError(f"LPIPS: inputs on {in0.device} / {in1.device}, weights on {dev} (use .to(device))")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("LPIPS: gradients to the weights are not implemented (they are frozen in every use as a "
                               "loss): call requires_grad_(False), or run under torch.no_grad()")
        N = in0.shape[0]
        if N == 0:
            val, per = in0.new_empty(0, dtype=torch.float32), in0.new_empty(5, 0, dtype=torch.float32)
        elif torch.is_grad_enabled() and (in0.requires_grad or in1.requires_grad):
            for t, name in ((in0, "in0"), (in1, "in1")):
                if t.dtype != torch.float32:
                    raise TypeError(f"LPIPS: {name} must be float32, got {t.dtype} (a cast would hide it from autograd)")
            ppp = lpips_pairs_per_pass(in0.shape[2], in0.shape[3], in0.requires_grad, in1.requires_grad,
                                       TRAIN_WORKSPACE_BYTES)
            val, per = _LPIPSFn.apply(in0, in1, self, bool(normalize), ppp)
        else:
            val, per = ops.lpips_vgg(self.packed(), in0.detach(), in1.detach(), normalize)
        val = val.view(N, 1, 1, 1)
        if retPerLayer:
            return val, [per[k].view(N, 1, 1, 1) for k in range(len(_TAP_CHANNELS))]
        return val


def evaluation(hwf, model, estimator, lpips_net, data_loader, chunksize: int, device, render_step_size: float = 5e-3, *,
               white_bkgd: bool = False):
    """The reference's evaluation() (run-nerf.py:108-191) on this package: every validation view through render_frame,
    the frames kept on the device, then PSNR over the stack and SSIM per frame averaged over frames, each in one launch.
    data_loader: an iterable of (rgb_gt [1,H,W,3], pose [1,4,4]) whose `.dataset` has near, far and ndc.  white_bkgd is
    keyword-only: the reference reads it from its global `args`.  Returns (psnr: 0-dim float32 tensor on the device,
    ssim: float, lpips).  lpips: when lpips_net is this package's `LPIPS`, the mean over frames of
    `lpips_net(rgbs, rgbs_gt)` (NCHW, [0, 1] inputs and normalize=False, the reference's call) as a 0-dim float32
    device tensor; for any other lpips_net (None, the `lpips` package's module, ...) None, as the reference returns
    (it computes the value and then discards it).  The reference's formula for 25 views or more (a sum of up to six
    chunk means divided by five) is not restated: the value is always the mean over all frames."""
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
    val_lpips = None
    if isinstance(lpips_net, LPIPS):
        with torch.no_grad():
            val_lpips = lpips_net(rgbs.permute(0, 3, 1, 2), gts.permute(0, 3, 1, 2)).mean()
    return val_psnr, val_ssim, val_lpips
