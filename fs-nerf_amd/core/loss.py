"""Host-side mirror of `src/core/loss.py`: the occlusion regulariser as one
segmented reduction on the GPU instead of a Python loop with one kernel launch per ray; the distortion loss on the
compositor's weights (this package's own, the first consumer of `full_grad`); and the weight-norm
"frequency" regulariser of the training loop (row f1, src/run-nerf.py:266-279) as one reduction over the flat
parameter arena; and the structural (D-SSIM) and perceptual (LPIPS-VGG) terms on rendered patches (this package's own:
the evaluation metrics of core/metrics.py with a backward); and the few-shot geometry losses on the renderer's other
outputs (this package's own definitions of InfoNeRF's ray entropy, DS-NeRF's depth KL term and RegNeRF's patch depth
smoothness: csrc/ray_losses.hip; InfoNeRF's KL between neighbouring rays on per-ray depth histograms:
csrc/ray_hist.hip); and the cross-view reprojection term on nerfdata.WarpSource (depth-warp consistency:
csrc/warp.hip)."""
import ctypes as C
import math
from typing import Optional

import torch
from torch import Tensor
from torch.autograd.function import once_differentiable

from .. import _lib as L
from .. import ops
from . import metrics


class OcclusionRegularizer:
    """Penalises density near the camera: mean over rays of sum_i w(t_i) sigma_i (loss.py:26-42),
    w = -a t + b ('linear') or a exp(-b t) ('exp') (loss.py:44-60).  Differentiable w.r.t. sigmas
    (the reference adds it to the training loss, run-nerf.py:264)."""

    def __init__(self, a: float, b: float, func: str = "linear"):
        assert a >= 0, "a should be non-negative"
        assert b >= 0, "b should be non-negative"
        self.a, self.b, self.func = a, b, func

    def __call__(self, sigmas: Tensor, t_vals: Tensor, ray_idxs: Tensor) -> Tensor:
        return ops.occlusion_reg(sigmas, t_vals, ray_idxs, self.a, self.b, self.func)


class DistortionLoss:
    """Distortion regulariser on the compositor's weights, mip-NeRF 360's interval form: per ray
        L_r = sum_i [ 2 w_i (m_i W_i - V_i) + w_i^2 dt_i / 3 ],   W_i = sum_{j<i} w_j,  V_i = sum_{j<i} w_j m_j,
    which for sorted midpoints m = (t_starts + t_ends)/2 and widths dt = t_ends - t_starts equals
    sum_i sum_j w_i w_j |m_i - m_j| + sum_i w_i^2 dt_i / 3; the call returns the mean over the `n_rays` rays (a ray
    without samples contributes 0).  One segmented reduction on the GPU (ops.distortion), differentiable w.r.t.
    `weights` only - so they must carry a gradient themselves: render_rays(..., full_grad=True), whose extras hold
    "weights", "t_starts" and "t_ends".  This is the package's OWN definition: the reference has no such loss and
    nerfacc's source is absent here, so parity with nerfacc.losses.distortion is UNPINNED."""

    def __call__(self, weights: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, n_rays: int) -> Tensor:
        return ops.distortion(weights, t_starts, t_ends, ray_indices, n_rays).mean()


class RayEntropyLoss:
    """Entropy of each ray's termination distribution (InfoNeRF's ray entropy; this package's OWN definition): with
    u_i = max(v_i, 0), s = sum_i u_i and p_i = u_i / (s + eps) over the ray's samples,
        H_r = -scale c_r sum_i p_i log(p_i + eps),   scale = 1 / ln 2 (`log2`, InfoNeRF's) or 1;
    the call returns the mean over the `n_rays` rays.  `values` [N]: extras["alphas"] of
    render_rays(..., full_grad=True), as InfoNeRF takes them, or extras["weights"]; negative entries (the raw-sigma
    network emits them) count as 0 and receive no gradient.  `opacity` [n_rays] (the renderer's, detached here) masks
    the rays: c_r = (opacity_r > threshold), InfoNeRF's rule - a ray that hits nothing has no distribution to sharpen;
    a masked ray, like a ray without samples, contributes 0 and gets a gradient of exactly 0.  Without `opacity` every
    ray counts.  One segmented reduction on the GPU (ops.ray_entropy), differentiable w.r.t. `values` only.
    InfoNeRF's second term, the KL divergence between the distributions of neighbouring rays, is NeighborRayKLLoss:
    packed rays have differing sample counts, so their samples do not pair up, and it compares the rays' histograms
    over common depth bins instead."""

    def __init__(self, threshold: float = 0.1, eps: float = 1e-10, log2: bool = True):
        self.threshold, self.eps, self.log2 = float(threshold), float(eps), bool(log2)

    def __call__(self, values: Tensor, ray_indices: Tensor, n_rays: int, opacity: Optional[Tensor] = None) -> Tensor:
        c = None if opacity is None else (opacity.detach().reshape(-1) > self.threshold)
        return ops.ray_entropy(values, ray_indices, n_rays, ray_weight=c, eps=self.eps, log2=self.log2).mean()


class NeighborRayKLLoss:
    """KL divergence between the termination distributions of neighbouring rays (InfoNeRF's second term, its
    "information gain reduction"; this package's OWN definition - InfoNeRF's source is absent, parity with it is
    UNPINNED).  The occupancy march emits a different number of samples on every ray, so two rays are compared on a
    common depth axis, not sample by sample: each ray's samples are binned into a histogram over `bins` fixed bins of
    [t_min, t_max] (ops.ray_histogram has the definition: P_rb = sum_i max(v_i, 0) overlap_ib / dt_i / (s_r + 1e-10)),
    and neighbouring pixels of a rendered patch are compared bin by bin (ops.patch_neighbor_kl):
        D(p, q) = sum_b p_b (log(p_b + eps) - log(q_b + eps)),
        out[i,j] = c_ij c_i,j+1 D(P_ij, P_i,j+1) + c_ij c_i+1,j D(P_ij, P_i+1,j)   (each where that neighbour exists).
    The call returns sum(out) / max(number of counted pairs, 1), the count formed on the device (no host sync).
    `patch_shape` = (B, Ph, Pw): the B Ph Pw patch rays are the rays first_ray ... of the `n_rays` (the patches ride
    behind a ray batch: first_ray = the batch's size); the samples of every other ray get a gradient of exactly 0.
    `opacity` (the renderer's, of the patch rays or of all n_rays; detached here) masks pixels: c = opacity > threshold,
    RayEntropyLoss's rule; a pair with a masked pixel is skipped.  Without it every pair counts.  `values` [N]:
    extras["alphas"] or extras["weights"] of render_rays(..., full_grad=True); t_min / t_max: the run's near / far.
    Two launches forward, two backward, differentiable w.r.t. `values` only.  Limits: no gradient to t_starts, t_ends
    or the bin edges; neighbours are patch-adjacent pixels only (InfoNeRF's pose-perturbed partner ray is not built:
    render a second patch and compare two ops.ray_histogram outputs in torch); one direction of KL, InfoNeRF's; with
    disjoint supports D reaches about -log(eps) per unit of mass and its gradient to q reaches p / eps."""

    def __init__(self, bins: int = 64, *, t_min: float, t_max: float, threshold: float = 0.1, eps: float = 1e-5):
        self.bins, self.t_min, self.t_max = ops._hist_axis("NeighborRayKLLoss", bins, t_min, t_max)
        self.threshold, self.eps = float(threshold), float(eps)

    def __call__(self, values: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, n_rays: int, patch_shape,
                 first_ray: int = 0, opacity: Optional[Tensor] = None) -> Tensor:
        B, Ph, Pw = (int(s) for s in patch_shape)
        n_pix = B * Ph * Pw
        if min(B, Ph, Pw) < 0 or Ph < 1 or Pw < 1:
            raise ValueError(f"NeighborRayKLLoss: patch_shape = (B, Ph, Pw) with Ph, Pw >= 1, got {tuple(patch_shape)}")
        c = None
        if opacity is not None:
            c = opacity.detach().reshape(-1)
            if c.numel() == int(n_rays) and c.numel() != n_pix:
                c = c[first_ray:first_ray + n_pix]
            if c.numel() != n_pix:
                raise ValueError(f"NeighborRayKLLoss: opacity has {opacity.numel()} entries for {n_pix} patch rays "
                                 f"(or {int(n_rays)} rays)")
            c = (c > self.threshold).reshape(B, Ph, Pw)
        P = ops.ray_histogram(values, t_starts, t_ends, ray_indices, n_rays, bins=self.bins, t_min=self.t_min,
                              t_max=self.t_max, rays=(int(first_ray), n_pix))
        out = ops.patch_neighbor_kl(P.view(B, Ph, Pw, self.bins), c, eps=self.eps)
        if c is None:
            return out.sum() / float(max(ops.patch_neighbor_pairs(B, Ph, Pw), 1))
        pairs = (c[:, :, :-1] & c[:, :, 1:]).sum() + (c[:, :-1] & c[:, 1:]).sum()
        return out.sum() / pairs.clamp(min=1).to(out.dtype)


class DepthKLLoss:
    """Depth supervision of the termination distribution (DS-NeRF's "sigma loss"; this package's OWN definition): with
    m_i = (t_starts_i + t_ends_i)/2 and dt_i = t_ends_i - t_starts_i, per supervised ray
        L_r = sum_i -log(max(w_i, 0) + eps) exp(-(m_i - depth_r)^2 / (2 var_r)) dt_i,
    the cross entropy between a Gaussian around the known depth and the compositor's weights; the call returns the sum
    over the rays divided by max(number of supervised rays, 1), counted on the device (no host sync).  `depth`
    [n_rays] and `var` [n_rays] (or one float) are per ray; a ray is supervised when both are finite and > 0 - put 0
    or NaN where no depth is known: such a ray contributes 0 and gets a gradient of exactly 0.  `weights` are
    extras["weights"] of render_rays(..., full_grad=True), whose extras hold "t_starts" and "t_ends" as well.  One
    segmented reduction on the GPU (ops.depth_kl), differentiable w.r.t. `weights` only."""

    def __init__(self, eps: float = 1e-5):
        self.eps = float(eps)

    def __call__(self, weights: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, n_rays: int, depth: Tensor,
                 var) -> Tensor:
        per_ray = ops.depth_kl(weights, t_starts, t_ends, ray_indices, n_rays, depth, var, eps=self.eps)
        d = depth.detach().reshape(-1)
        ok = torch.isfinite(d) & (d > 0)
        if isinstance(var, Tensor):
            v = var.detach().reshape(-1)
            ok = ok & torch.isfinite(v) & (v > 0)
        elif not (math.isfinite(var) and var > 0):
            ok = torch.zeros_like(ok)
        return per_ray.sum() / ok.sum().clamp(min=1).to(per_ray.dtype)


class PatchDepthSmoothnessLoss:
    """Smoothness of rendered depth patches (RegNeRF's depth smoothness, compute_tv_norm with the l2 loss; this
    package's OWN definition): for `depth` [B, P, Q], rendered from poses no photograph was taken from,
        S_b = sum_{i < P-1, j < Q-1} (d[i,j] - d[i,j+1])^2 + (d[i,j] - d[i+1,j])^2,
    and the call returns mean_b S_b / ((P-1)(Q-1)) - 0 when P or Q is 1.  One launch forward, one backward
    (ops.patch_depth_smoothness); `depth` must carry a gradient itself: render_rays(..., full_grad=True).  The poses
    are the caller's: nerfdata.UnseenPatchLoader serves such patches, one launch per batch, from a pose distribution
    fitted to the training cameras (nerfdata.UnseenViewSampler.from_poses)."""

    def __call__(self, depth: Tensor) -> Tensor:
        per_patch = ops.patch_depth_smoothness(depth)
        B, P, Q = depth.shape
        return per_patch.sum() / float(max(B, 1) * max((P - 1) * (Q - 1), 1))


def _prior_weight(who: str, weight: Optional[Tensor], opacity: Optional[Tensor], threshold: Optional[float],
                  like: Tensor) -> Optional[Tensor]:
    """The weight of the two prior losses after the opacity mask (RayEntropyLoss's rule, the opacity detached): 0 where
    opacity <= threshold."""
    if threshold is None:
        return weight
    if opacity is None:
        raise ValueError(f"{who}: a threshold needs the renderer's opacity")
    keep = opacity.detach().reshape(like.shape) > threshold
    w = torch.ones_like(like) if weight is None else weight.detach().to(like.dtype)
    return torch.where(keep, w, torch.zeros_like(w))


class ScaleShiftDepthLoss:
    """Rendered depth against a monocular depth prior that is known only up to a scale and a shift per image (the
    scale-and-shift-invariant term of MiDaS, used by MonoSDF; this package's OWN definition - parity with either is
    UNPINNED).  Per patch of `depth`, `prior` [B, P, Q], with x = depth (space="depth") or x = 1 / max(depth, z_min)
    ("disparity": for a prior that is an inverse depth), w the `weight` of a valid pixel (no weight: 1) and every sum in
    float64:
        (s, t) = argmin sum w (s x + t - p)^2 = (cov_w(x, p) / var_w(x),  mean_w(p) - s mean_w(x)),
        L_b = sum w (s x + t - p)^2 / sum w,
    and the call returns the sum of L_b over the non-degenerate patches divided by their number (counted on the device,
    clamped at 1; no host sync).  A pixel is valid iff prior and depth are finite and weight > 0: put NaN in the prior
    where nothing is known; an invalid pixel gets a gradient of exactly 0.  A patch with fewer than two valid pixels,
    sum w <= 0 or var_w(x) <= rel_eps mean_w(x)^2 (a constant patch fixes no scale) is degenerate: value 0, gradient
    exactly 0.  (s, t) minimise L_b, so its gradient is the partial derivative at fixed (s, t) (DESIGN 6.1 has the
    argument); s is not constrained to be positive - return_fit=True also returns fit [B, 4] = (s, t, sum w, degenerate)
    so that the caller can watch its sign.  With `threshold`, `opacity` [B, P, Q] (the renderer's, detached) zeroes the
    weight where opacity <= threshold.  One launch forward, one backward (ops.ssi_depth), P * Q <= 4096; gradients go to
    `depth` only, which must carry one itself: render_rays(..., full_grad=True).  nerfdata.PatchLoader(with_aux=True)
    serves the prior's patches in the batch's own launch."""

    def __init__(self, space: str = "depth", z_min: float = 1e-3, threshold: Optional[float] = None, rel_eps: float = 1e-10):
        if space not in ("depth", "disparity"):
            raise ValueError(f"ScaleShiftDepthLoss: space must be 'depth' or 'disparity', got {space!r}")
        self.space, self.z_min, self.rel_eps = space, float(z_min), float(rel_eps)
        self.threshold = None if threshold is None else float(threshold)

    def __call__(self, depth: Tensor, prior: Tensor, weight: Optional[Tensor] = None, opacity: Optional[Tensor] = None,
                 return_fit: bool = False):
        w = _prior_weight("ScaleShiftDepthLoss", weight, opacity, self.threshold, depth)
        per_patch, fit = ops.ssi_depth(depth, prior, w, inverse=self.space == "disparity", z_min=self.z_min,
                                       rel_eps=self.rel_eps)
        fitted = (fit[:, 3] == 0).sum().clamp(min=1).to(per_patch.dtype)
        loss = per_patch.sum() / fitted
        return (loss, fit) if return_fit else loss


class DepthRankingLoss:
    """Ordinal depth ranking against a prior whose ordering alone is trusted (SparseNeRF's local depth ranking; this
    package's OWN, deterministic definition over ALL pairs of a patch instead of random draws - parity with SparseNeRF
    is UNPINNED).  For `depth`, `prior` [B, P, Q]: an ordered pair (i, j) of valid pixels of one patch counts iff the
    prior puts i nearer, p_i < p_j - prior_gap (with prior_is_disparity: p_i > p_j + prior_gap), and contributes
        max(0, d_i - d_j + margin);
    the call returns the sum over all counted pairs divided by max(their number, 1), counted on the device (no host
    sync; NeighborRayKLLoss's convention).  A pixel is valid iff prior and depth are finite and `weight` > 0 (a mask
    here; no weight: all); an invalid pixel gets a gradient of exactly 0, as does a pair whose hinge is exactly 0.  With
    `threshold`, `opacity` [B, P, Q] (detached) masks the pixels with opacity <= threshold.  One launch forward, one
    backward (ops.depth_rank), P * Q <= 4096 (16.8 M pair tests per patch at the cap); gradients go to `depth` only."""

    def __init__(self, margin: float = 1e-4, prior_gap: float = 0.0, prior_is_disparity: bool = False,
                 threshold: Optional[float] = None):
        self.margin, self.prior_gap, self.prior_is_disparity = float(margin), float(prior_gap), bool(prior_is_disparity)
        self.threshold = None if threshold is None else float(threshold)

    def __call__(self, depth: Tensor, prior: Tensor, weight: Optional[Tensor] = None,
                 opacity: Optional[Tensor] = None) -> Tensor:
        w = _prior_weight("DepthRankingLoss", weight, opacity, self.threshold, depth)
        per_patch, pairs = ops.depth_rank(depth, prior, w, margin=self.margin, prior_gap=self.prior_gap,
                                          prior_is_disparity=self.prior_is_disparity)
        return per_patch.sum() / pairs.sum().clamp(min=1).to(per_patch.dtype)


class WarpConsistencyLoss:
    """Cross-view reprojection (the photometric warping term of GeCoNeRF, SPARF and ConsistentNeRF; this package's OWN
    definition): a rendered ray's colour against the colour that a training photograph shows at the ray's
    rendered 3-D point.  With colour_r, valid_r = source.sample(rays_o, rays_d, depth, src_view) (nerfdata.WarpSource,
    ops.warp_sample: `z_min`, `border` are its keywords), per row
        l_r = mean_c rho(rgb_c - colour_c),   rho = |.| ("l1"; gradient 0 at 0, torch.abs's rule) or (.)^2 ("l2"),
        c_r = valid_r  and, when a `threshold` is given,  opacity_r > threshold  (the opacity detached: RayEntropyLoss's
              rule - a ray that hits nothing has no depth to reproject),
    and the call returns sum_r c_r l_r / max(sum_r c_r, 1), counted on the device (no host sync).  `rgb` [n,3] and
    `depth` [n] come from render_rays(..., full_grad=True), whose depth carries a gradient; `src_view` [n] int64 names
    the source view of each row (WarpSource.other_views for a training batch's own views, nearest_views for the poses of
    an UnseenPatchLoader; -1 = none).  Gradients go to rgb, to depth and to the rays; a row that is invalid or masked
    contributes 0 and gets a gradient of exactly 0.  The reduction is a few torch ops around the operator's one launch
    each way.  Limits: no gradient to the images, to the source poses or to K; one source view per call (call it twice
    for two); no occlusion reasoning beyond the caller's mask and the operator's uvz output; NDC datasets are refused
    by WarpSource."""

    def __init__(self, kind: str = "l1", threshold: Optional[float] = None, z_min: float = 1e-3, border: float = 0.5):
        if kind not in ("l1", "l2"):
            raise ValueError(f"WarpConsistencyLoss: kind must be 'l1' or 'l2', got {kind!r}")
        self.kind, self.threshold = kind, None if threshold is None else float(threshold)
        self.z_min, self.border = float(z_min), float(border)

    def __call__(self, rgb: Tensor, depth: Tensor, rays_o: Tensor, rays_d: Tensor, src_view: Tensor, source,
                 opacity: Optional[Tensor] = None) -> Tensor:
        src_view = src_view.reshape(-1)
        if self.threshold is not None:
            if opacity is None:
                raise ValueError("WarpConsistencyLoss: a threshold needs the renderer's opacity")
            # a masked row goes in without a source view: the operator writes its zeros itself and reads no pixel for it
            src_view = torch.where(opacity.detach().reshape(-1) > self.threshold, src_view, torch.full_like(src_view, -1))
        colour, valid, _ = source.sample(rays_o, rays_d, depth, src_view, z_min=self.z_min, border=self.border)
        diff = rgb.reshape(-1, 3) - colour
        per_row = (diff.abs() if self.kind == "l1" else diff * diff).mean(dim=1)
        # (where, not a product: a masked row's difference may be anything and must not reach the sum)
        total = torch.where(valid, per_row, torch.zeros_like(per_row)).sum()
        return total / valid.sum().clamp(min=1).to(per_row.dtype)


class _SSIMLossFn(torch.autograd.Function):
    """1 - SSIM in one node: forward = fsn_ssim (the evaluation metric's own launch, unchanged), backward = one
    fsn_ssim_grad launch for the inputs that need a gradient."""

    @staticmethod
    def forward(ctx, pred, target, loss):
        x, y = metrics._as_nchw(pred, loss.channel_axis), metrics._as_nchw(target, loss.channel_axis)
        out = ops.ssim_nchw(x, y, loss.window, loss.use_sample_covariance, loss.data_range, loss.K1, loss.K2)
        N = x.shape[0]
        ctx.save_for_backward(pred, target)
        ctx.loss, ctx.N = loss, N
        val = out[N] if loss.reduction == "mean" else out[:N]
        return (1.0 - val).to(torch.float32)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        pred, target = ctx.saved_tensors
        loss, N = ctx.loss, ctx.N
        want_dx, want_dy = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_dx or want_dy):
            return None, None, None
        # loss = 1 - mean_n ssim_n ("mean") or 1 - ssim_n ("none"): dL / d ssim_n
        up = -d_out.to(torch.float64)
        up = (up / N).expand(N) if loss.reduction == "mean" else up
        d_pred = torch.empty_like(pred) if want_dx else None
        d_target = torch.empty_like(target) if want_dy else None
        ca = loss.channel_axis
        ops.ssim_grad_nchw(metrics._as_nchw(pred, ca), metrics._as_nchw(target, ca), loss.window, loss.use_sample_covariance,
                           loss.data_range, loss.K1, loss.K2, up, want_dx=want_dx, want_dy=want_dy,
                           dx=None if d_pred is None else metrics._as_nchw(d_pred, ca),
                           dy=None if d_target is None else metrics._as_nchw(d_target, ca))
        return d_pred, d_target, None


class SSIMLoss:
    """The structural (D-SSIM) term for patch-mode training: `loss(pred, target)` = 1 - metrics.ssim(pred, target, ...)
    with gradients to both inputs - 0-dim float32 (reduction="mean", the mean over the N images or patches) or
    float32 (N,) ("none").  The value is the evaluation metric's own (fsn_ssim, float64; 1 - value is taken in float64
    and rounded once); the backward is one fsn_ssim_grad launch in float64 (csrc/ssim_grad.hip), only for the inputs
    that need a gradient, and cannot be differentiated again.  Shapes and `channel_axis` as metrics.ssim: (H, W),
    (H, W, C), (N, H, W, C) with channel_axis=-1, (N, C, H, W) with 1; float32 GPU tensors of any strides, read in
    place.  Windows: gaussian_weights=True (sigma 1.5, 11 x 11) and the 7 x 7 box; an image must hold one window."""

    def __init__(self, gaussian_weights: bool = True, use_sample_covariance: bool = True, data_range: float = 1.0,
                 K1: float = 0.01, K2: float = 0.03, channel_axis: Optional[int] = -1, reduction: str = "mean"):
        if reduction not in ("mean", "none"):
            raise ValueError(f"reduction must be 'mean' or 'none', got {reduction!r}")
        if data_range is None:
            raise ValueError("data_range is required (the reference passes data_range=1.0)")
        self.window = L.FSN_SSIM_GAUSSIAN if gaussian_weights else L.FSN_SSIM_UNIFORM
        self.win = metrics._GAUSS_WIN if gaussian_weights else metrics._UNIFORM_WIN
        self.use_sample_covariance, self.data_range = bool(use_sample_covariance), float(data_range)
        self.K1, self.K2, self.channel_axis, self.reduction = float(K1), float(K2), channel_axis, reduction

    def __call__(self, pred: Tensor, target: Tensor) -> Tensor:
        if pred.shape != target.shape:
            raise ValueError(f"pred and target must have the same shape: {tuple(pred.shape)} vs {tuple(target.shape)}")
        x = metrics._as_nchw(pred, self.channel_axis)  # (raises ValueError for a shape metrics.ssim does not take)
        if x.shape[2] < self.win or x.shape[3] < self.win:
            raise ValueError(f"win_size exceeds image extent: {x.shape[2]} x {x.shape[3]} image, {self.win} x {self.win} window")
        for t, name in ((pred, "pred"), (target, "target")):
            if not t.is_cuda:
                raise RuntimeError(f"SSIMLoss: {name} is not a GPU tensor (the HIP path has no CPU fallback)")
            if t.dtype != torch.float32:
                raise TypeError(f"SSIMLoss: {name} must be float32, got {t.dtype} (a cast would hide it from autograd)")
        return _SSIMLossFn.apply(pred, target, self)


class LPIPSLoss:
    """The perceptual term for patch-mode training, the sibling of SSIMLoss: `loss(pred, target)` =
    lpips_net(pred, target, normalize=normalize) of `metrics.LPIPS` with gradients to the inputs that need one -
    0-dim float32 (reduction="mean", the mean over the N patches) or float32 (N,) ("none").  Each pair's value is the
    evaluation metric's own, bit for bit; the backward (csrc/lpips.hip: tap backward in float64, the convolutions'
    data gradients on the f32 MFMA) cannot be differentiated again.  The VGG and lin weights are frozen.
    Shapes: (N, H, W, 3) with channel_axis=-1 (render_rays' rows viewed as patches), (N, 3, H, W) with 1; float32 GPU
    tensors of any strides, read in place; H, W >= 16.  normalize=True: inputs in [0, 1] (the renderer's range).
    Definitions where autograd has none or a choice: a pixel whose tap vector is all zero has gradient 0 (autograd:
    NaN); a pooled gradient goes to the first maximum of its 2 x 2 window in row-major order (max_pool2d's rule).

    Memory: a pass keeps about 270 H W floats of activations and 128 H W of gradients per back-propagated image.  N is
    processed in chunks of `pairs_per_pass` pairs, one forward and one backward call each; by default the most pairs
    whose workspace fits `max_workspace_bytes` (1 GiB: a setting, not a measurement; one pair always runs, whatever
    its size).  With more than one chunk the backward runs each chunk's forward again instead of keeping every
    chunk's activations.  The gradients do not depend on the chunking, bit for bit."""

    def __init__(self, lpips_net, normalize: bool = True, channel_axis: int = -1, reduction: str = "mean"):
        if not isinstance(lpips_net, metrics.LPIPS):
            raise TypeError(f"LPIPSLoss: lpips_net must be fs_nerf_amd.core.metrics.LPIPS, got {type(lpips_net).__name__}")
        if reduction not in ("mean", "none"):
            raise ValueError(f"reduction must be 'mean' or 'none', got {reduction!r}")
        if channel_axis not in (-1, 3, 1, -3):
            raise ValueError(f"channel_axis={channel_axis}: expected -1 (N, H, W, 3) or 1 (N, 3, H, W)")
        self.net, self.normalize, self.channel_axis, self.reduction = lpips_net, bool(normalize), channel_axis, reduction
        self.max_workspace_bytes = metrics.TRAIN_WORKSPACE_BYTES
        self.pairs_per_pass: Optional[int] = None  # None: from max_workspace_bytes

    def __call__(self, pred: Tensor, target: Tensor) -> Tensor:
        net = self.net
        if not net._loaded:
            raise RuntimeError("LPIPSLoss: no weights loaded (load the lpips package's VGG state dict with load_state_dict)")
        if pred.shape != target.shape:
            raise ValueError(f"pred and target must have the same shape: {tuple(pred.shape)} vs {tuple(target.shape)}")
        if pred.dim() != 4:
            raise ValueError(f"expected (N, H, W, 3) or (N, 3, H, W) patches, got shape {tuple(pred.shape)}")
        x, y = metrics._as_nchw(pred, self.channel_axis), metrics._as_nchw(target, self.channel_axis)
        if x.shape[1] != 3:
            raise ValueError(f"expected 3 channels on axis {self.channel_axis}, got shape {tuple(pred.shape)}")
        H, W = x.shape[2], x.shape[3]
        if H < metrics._MIN_SIDE or W < metrics._MIN_SIDE:
            raise ValueError(f"LPIPS-VGG needs images of at least {metrics._MIN_SIDE} x {metrics._MIN_SIDE}, got {H} x {W}")
        for t, name in ((pred, "pred"), (target, "target")):
            if t.dtype != torch.float32:
                raise TypeError(f"LPIPSLoss: {name} must be float32, got {t.dtype} (a cast would hide it from autograd)")
        for t, name in ((pred, "pred"), (target, "target")):
            if not t.is_cuda:
                raise RuntimeError(f"LPIPSLoss: {name} is not a GPU tensor (the HIP path has no CPU fallback)")
        dev = net.scaling_layer.shift.device
        if pred.device != dev or target.device != dev:
            raise RuntimeError(f"LPIPSLoss: inputs on {pred.device} / {target.device}, weights on {dev} (use .to(device))")
        N = x.shape[0]
        want_dx, want_dy = pred.requires_grad, target.requires_grad
        if N == 0:
            val = pred.new_empty(0)
        elif torch.is_grad_enabled() and (want_dx or want_dy):
            if any(p.requires_grad for p in net.parameters()):
                raise RuntimeError("LPIPSLoss: the LPIPS weights are frozen (gradients to them are not implemented)")
            ppp = self.pairs_per_pass
            if ppp is None:
                ppp = metrics.lpips_pairs_per_pass(H, W, want_dx, want_dy, int(self.max_workspace_bytes))
            if int(ppp) < 1:
                raise ValueError(f"pairs_per_pass must be at least 1, got {ppp}")
            val, _ = metrics._LPIPSFn.apply(x, y, net, self.normalize, int(ppp))
        else:
            val, _ = ops.lpips_vgg(net.packed(), x.detach(), y.detach(), self.normalize)
        return val.mean() if self.reduction == "mean" else val


class _WeightNormFn(torch.autograd.Function):
    """out = sum over the selected tensors of |w|_1 or |w|_2, one reduction launch over the flat parameter arena
    (`fsn_weight_norm_fwd`); backward accumulates d_out * d(out)/dw into a gradient tensor of the arena's layout
    (`fsn_weight_norm_bwd`) and hands each selected parameter its slice."""

    @staticmethod
    def forward(ctx, reg, *params):
        flat, offs, lens = reg._arena(params)
        n = len(offs)
        off_t, len_t = (C.c_int64 * n)(*offs), (C.c_int64 * n)(*lens)
        nws = ops._size("fsn_weight_norm_workspace_floats", None, n, len_t)
        ws = torch.empty(nws, device=flat.device, dtype=torch.float32)
        out = torch.empty(1, device=flat.device, dtype=torch.float32)
        ops._launch("fsn_weight_norm_fwd", flat.device, flat, n, off_t, len_t, int(reg.l2), ws, out)
        ctx.reg, ctx.flat, ctx.ws, ctx.tabs, ctx.shapes = reg, flat, ws, (n, off_t, len_t, offs, lens), [p.shape for p in params]
        return out.reshape(())

    @staticmethod
    def backward(ctx, d_out):
        n, off_t, len_t, offs, lens = ctx.tabs
        flat = ctx.flat
        g = torch.zeros_like(flat)
        d = d_out.reshape(1).to(torch.float32).contiguous()
        ops._launch("fsn_weight_norm_bwd", flat.device, flat, n, off_t, len_t, int(ctx.reg.l2), ctx.ws, d, g)
        return (None,) + tuple(g[o:o + ln].view(sh) for o, ln, sh in zip(offs, lens, ctx.shapes))


class WeightNormRegularizer:
    """The weight-norm "frequency" regulariser the reference writes inline in its training loop
    (src/run-nerf.py:266-279, flags src/utils/parser.py:141-156): over the parameters whose name contains "weight"
    and whose first dimension exceeds 3 (every Linear weight except the 1- and 3-row heads),
        reg "l1":  sum_t |W_t|_1          reg "l2":  sum_t |W_t|_2   (torch.square(p).sum().sqrt() per tensor).
    `reg()` returns that scalar with gradients to the parameters; the caller multiplies by alpha and applies the
    schedule (`active(k)`: k < int(reg_ratio * Td), run-nerf.py:270-271).  One reduction launch over the flat parameter
    arena when the parameters live in one (core/optim.py: FlatParams / FusedAdam); otherwise they are gathered into a
    temporary flat buffer first."""

    def __init__(self, named_parameters, reg: str = "l1", reg_ratio: float = 0.5, Td: int = 0):
        assert reg in ("l1", "l2")
        self.l2 = reg == "l2"
        self.params = [p for name, p in named_parameters if "weight" in name and p.shape[0] > 3]
        self.Ts = int(reg_ratio * Td)

    def active(self, k: int) -> bool:
        return k < self.Ts

    def _arena(self, params):
        """(flat tensor, offsets, lengths): the parameters' own storage when they are views of one contiguous buffer."""
        base = min(p.data_ptr() for p in params)
        offs = [(p.data_ptr() - base) // 4 for p in params]
        lens = [p.numel() for p in params]
        span = max(o + n for o, n in zip(offs, lens))
        st = params[0].untyped_storage()
        same = all(p.is_contiguous() and p.untyped_storage().data_ptr() == st.data_ptr() for p in params)
        if same and span * 4 <= st.nbytes():
            p0 = min(params, key=lambda p: p.data_ptr())
            flat = torch.as_strided(p0.detach(), (span,), (1,), p0.storage_offset())
            return flat, offs, lens
        flat = torch.cat([p.detach().reshape(-1) for p in params])
        offs, o = [], 0
        for n in lens:
            offs.append(o)
            o += n
        return flat, offs, lens

    def __call__(self) -> Tensor:
        if not self.params:
            raise ValueError("WeightNormRegularizer: no weight tensor selected")
        if not all(p.is_cuda for p in self.params):
            raise RuntimeError("WeightNormRegularizer: GPU parameters expected (the HIP path has no CPU fallback)")
        return _WeightNormFn.apply(self, *self.params)
