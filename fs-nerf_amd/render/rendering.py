"""Host-side mirror of the reference's `render/rendering.py` call surface on HIP kernels.

  render_rays(rays_o, rays_d, estimator, model, train, white_bkgd, render_step_size, device)
      -> ((rgb, opacity, depth, extras), ray_indices, t_vals)           (src/render/rendering.py:25-107)
  render_frame(hwf, near, far, pose, chunksize, estimator, model, ...)  (src/render/rendering.py:110-177)
  rendering(t_starts, t_ends, ray_indices, n_rays, rgb_sigma_fn, render_bkgd)
      the nerfacc.volrend.rendering slot (call site rendering.py:89-96); rgb_alpha_fn: its alpha route
  StratifiedEstimator                     the estimator slot (rendering.py:66-74, run-nerf.py:96-98)

`StratifiedEstimator` is the fixed-count sampler `north_star` asks for (64 coarse + 128
importance samples) with the duck-typed interface the reference expects from its estimator
(`sampling`, `update_every_n_steps`, nn.Module modes).  When `model` is this package's NeRF and
`estimator` a StratifiedEstimator, render_rays runs the single fused launch
(fsn_render_rays_fused); any other callable model goes through the same HIP sampler /
compositor kernels with the model evaluated in between, exactly like the reference's closures.
"""
from typing import Callable, Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from .. import ops
from ..core.models import NeRF
from ..core.range_guard import frame_flagged, guarded_launch, sampler_launch
from ..utils import utilities as U
from . import volrend
from .occgrid import OccGridEstimator
from .propnet import PropNetEstimator, prop_sigma_fn

FUSED_OCC_MAX_STEPS = 2048  # csrc/render_occ.hip: samples of one ray group in LDS


class StratifiedEstimator(nn.Module):
    """Fixed-count stratified sampler with optional hierarchical (inverse-CDF) refinement."""

    def __init__(self, near: float, far: float, n_samples: int = 64, n_importance: int = 0,
                 jitter: str = "ray") -> None:
        super().__init__()
        assert jitter in ("ray", "edge")
        self.near, self.far = float(near), float(far)
        self.n_samples, self.n_importance, self.jitter = int(n_samples), int(n_importance), jitter
        self.generator: Optional[torch.Generator] = None  # optional explicit RNG for the jitter

    def bounds(self, near_plane: float = 0.0, far_plane: float = 1e10) -> Tuple[float, float]:
        return max(self.near, float(near_plane)), min(self.far, float(far_plane))

    def draw_u(self, n_rays: int, device) -> Tensor:
        shape = (n_rays,) if self.jitter == "ray" else (n_rays, self.n_samples + 1)
        return torch.rand(*shape, device=device, generator=self.generator)

    @torch.no_grad()
    def sampling(self, rays_o: Tensor, rays_d: Tensor, sigma_fn: Optional[Callable] = None,
                 render_step_size: float = 5e-3, stratified: bool = False, near_plane: float = 0.0,
                 far_plane: float = 1e10, u: Optional[Tensor] = None, u_fine: Optional[Tensor] = None,
                 cone_angle: float = 0.0, t_min: Optional[Tensor] = None, t_max: Optional[Tensor] = None):
        """-> (ray_indices int64 [N], t_starts [N], t_ends [N]); N = n_rays*(n_samples+n_importance).
        `render_step_size` is accepted for signature compatibility (the step is (far-near)/n_samples).  A fixed-count
        sampler has no cone-angle steps and no per-ray bounds: `cone_angle` / `t_min` / `t_max` are a ValueError."""
        if cone_angle != 0.0 or t_min is not None or t_max is not None:
            raise ValueError("StratifiedEstimator: cone_angle / t_min / t_max belong to the occupancy estimator")
        R = rays_o.shape[0]
        near, far = self.bounds(near_plane, far_plane)
        if u is None and stratified:
            u = self.draw_u(R, rays_o.device)
        edges = ops.stratified_edges(near, far, self.n_samples, R, u, rays_o.device)
        if self.n_importance > 0:
            if sigma_fn is None:
                raise ValueError("hierarchical sampling needs sigma_fn")
            ri, t0, t1 = ops.edges_to_packed(edges)
            sig = sigma_fn(t0, t1, ri).reshape(R, self.n_samples)
            # weights of the density pass = the compositor's weights (colours are irrelevant)
            _, _, _, ex = ops.composite(sig, torch.zeros(R, self.n_samples, 3, device=sig.device),
                                        edges[:, :-1].contiguous(), edges[:, 1:].contiguous(), None)
            if u_fine is None and stratified:
                u_fine = torch.rand(R, self.n_importance, device=rays_o.device, generator=self.generator)
            edges = ops.sample_pdf_merge(edges, ex["weights"], self.n_importance, u_fine)
        return ops.edges_to_packed(edges)

    def update_every_n_steps(self, step: int = 0, occ_eval_fn: Optional[Callable] = None,
                             occ_thre: float = 1e-2, **_) -> None:
        """No occupancy state to refresh (run-nerf.py:292-295 calls this every step)."""
        return None


class _CompositeFn(torch.autograd.Function):
    """Volume integration with gradients to sigmas and rgbs (training step).  Lean form: through colors
    and opacity only.  `full` (`rendering(full_grad=True)`): through ALL six outputs - colors, opacity, depth and the
    per-sample weights / alphas / trans; a cotangent nothing asked for arrives as None and reaches the kernel as a NULL
    pointer (fsn_composite_packed_bwd_full)."""

    @staticmethod
    def forward(ctx, sigmas, rgbs, t_starts, t_ends, ray_indices, n_rays, bkgd, full):
        colors, opacity, depth, ex = ops.composite_packed(sigmas, rgbs, t_starts, t_ends, ray_indices, n_rays, bkgd)
        ctx.save_for_backward(ex["sigmas"], ex["rgbs"], t_starts, t_ends, ray_indices, *((opacity, depth) if full else ()))
        ctx.n_rays, ctx.bkgd, ctx.full = n_rays, bkgd, full
        if full:
            ctx.set_materialize_grads(False)
        else:
            ctx.mark_non_differentiable(depth, ex["weights"], ex["alphas"], ex["trans"])
        return colors, opacity, depth, ex["weights"], ex["alphas"], ex["trans"]

    @staticmethod
    def backward(ctx, d_colors, d_opacity, d_depth, d_weights, d_alphas, d_trans):
        sig, rgb, t0, t1, ri, *fwd = ctx.saved_tensors
        if ctx.full:
            ds, dr = ops.composite_packed_bwd_full(sig, rgb, t0, t1, ri, ctx.n_rays, ctx.bkgd, d_colors, d_opacity,
                                                   opacity=fwd[0], depth=fwd[1], d_depth=d_depth, d_weights=d_weights,
                                                   d_alphas=d_alphas, d_trans=d_trans)
        else:
            ds, dr = ops.composite_packed_bwd(sig, rgb, t0, t1, ri, ctx.n_rays, ctx.bkgd, d_colors.contiguous(),
                                              None if d_opacity is None else d_opacity.contiguous())
        return ds.reshape(sig.shape), dr.reshape(rgb.shape), None, None, None, None, None, None


def _rendering_from_alpha(t_starts, t_ends, ray_indices, n_rays, rgb_alpha_fn, render_bkgd):
    """`rendering`'s alpha route, composed as nerfacc composes it: weights from the alphas, then one accumulation each
    for colours, opacity and depth; every step a differentiable HIP primitive of render/volrend.py."""
    rgbs, alphas = rgb_alpha_fn(t_starts, t_ends, ray_indices)
    assert rgbs.shape[-1] == 3, "rgbs must have 3 channels, got {}".format(rgbs.shape)
    assert alphas.shape == t_starts.shape, "alphas must have shape of (N,)! Got {}".format(alphas.shape)
    weights, trans = volrend.render_weight_from_alpha(alphas, ray_indices=ray_indices, n_rays=n_rays)
    colors = volrend.accumulate_along_rays(weights, rgbs, ray_indices, n_rays)
    opacity = volrend.accumulate_along_rays(weights, None, ray_indices, n_rays)
    mids = ((t_starts + t_ends) / 2.0).detach()[:, None]
    depth = volrend.accumulate_along_rays(weights, mids, ray_indices, n_rays)
    depth = depth / opacity.clamp_min(torch.finfo(torch.float32).eps)
    if render_bkgd is not None:
        colors = colors + render_bkgd.to(colors) * (1.0 - opacity)
    return colors, opacity, depth, {"weights": weights, "trans": trans, "alphas": alphas, "rgbs": rgbs}


def rendering(t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, n_rays: int,
              rgb_sigma_fn: Optional[Callable] = None, render_bkgd: Optional[Tensor] = None, full_grad: bool = False,
              rgb_alpha_fn: Optional[Callable] = None):
    """nerfacc.volrend.rendering's contract: -> (colors [n_rays,3], opacities [n_rays,1],
    depths [n_rays,1], extras).  AssertionError on the same shape violations.  Differentiable with
    respect to the rgbs / sigmas returned by `rgb_sigma_fn`: through colors and opacities by default (the lean
    backward of the timed training step; depth and the extras are detached), through EVERY output - depths and
    extras["weights" | "alphas" | "trans"] as well, as nerfacc's are - with `full_grad=True` (depth supervision,
    distortion / entropy / depth KL losses on the weights and alphas - core.loss.DistortionLoss, RayEntropyLoss,
    DepthKLLoss -, opacity priors).  No gradient goes to t_starts / t_ends.
    Exactly one of `rgb_sigma_fn` and `rgb_alpha_fn` is given (else ValueError).  `rgb_alpha_fn` -> (rgbs [N,3],
    alphas [N]) takes the alpha route (an opacity-valued field): render_weight_from_alpha, then accumulate_along_rays
    for colours, opacity and depth, depth / clamp(opacity, eps), the background; extras hold "weights", "trans",
    "alphas" and "rgbs", and every output is differentiable (`full_grad` has nothing to add there)."""
    if (rgb_sigma_fn is None) == (rgb_alpha_fn is None):
        raise ValueError("rendering: exactly one of rgb_sigma_fn and rgb_alpha_fn must be given")
    if rgb_alpha_fn is not None:
        return _rendering_from_alpha(t_starts, t_ends, ray_indices, n_rays, rgb_alpha_fn, render_bkgd)
    rgbs, sigmas = rgb_sigma_fn(t_starts, t_ends, ray_indices)
    assert rgbs.shape[-1] == 3, "rgbs must have 3 channels, got {}".format(rgbs.shape)
    assert sigmas.shape == t_starts.shape, "sigmas must have shape of (N,)! Got {}".format(sigmas.shape)
    # A background that itself requires grad (the reference builds `render_bkgd` with requires_grad=train,
    # rendering.py:86, which is what keeps loss.backward() legal on an all-background batch) is added with the
    # compositor's own op sequence, colors + bkgd * (1 - opacity), as differentiable torch ops on [n_rays,3].
    bk_grad = render_bkgd is not None and torch.is_grad_enabled() and render_bkgd.requires_grad
    kernel_bk = None if bk_grad else render_bkgd
    if torch.is_grad_enabled() and (rgbs.requires_grad or sigmas.requires_grad):
        bk = None if kernel_bk is None else [float(v) for v in kernel_bk.detach().cpu().tolist()]
        colors, opacity, depth, w, a, tr = _CompositeFn.apply(sigmas, rgbs.contiguous(), t_starts, t_ends, ray_indices,
                                                              n_rays, bk, bool(full_grad))
        ex = {"weights": w, "alphas": a, "trans": tr, "sigmas": sigmas, "rgbs": rgbs}
    else:
        colors, opacity, depth, ex = ops.composite_packed(sigmas, rgbs, t_starts, t_ends, ray_indices, n_rays, kernel_bk)
    if bk_grad:
        colors = colors + render_bkgd.to(colors.dtype) * (1.0 - opacity)
    return colors, opacity, depth, ex


def _probe_on_rays(rays_o, rays_d, camera, t_lo: float, t_hi: float, n_rays: int = 512, n_t: int = 32):
    """Probe batch for NeRF.calibrate (per-layer activation scales of the fp16x3 inference path): positions o + d t on
    an even subset of the call's rays (or of the camera's) at n_t depths across [t_lo, t_hi], with the rays' directions."""
    if rays_o is None:
        pose, H, W, focal, row0, nrows, dev = camera
        rays_o, rays_d = ops.get_rays(pose, int(H), int(W), float(focal), dev, int(row0), int(nrows))
    R, dev = rays_o.shape[0], rays_o.device
    idx = torch.linspace(0, max(R - 1, 0), min(max(R, 1), n_rays), device=dev).long()
    o, d = rays_o.reshape(-1, 3)[idx].float(), rays_d.reshape(-1, 3)[idx].float()
    t = t_lo + (t_hi - t_lo) * (torch.arange(n_t, device=dev, dtype=torch.float32) + 0.5) / n_t
    x = o[:, None, :] + d[:, None, :] * t[None, :, None]
    return x.reshape(-1, 3), d[:, None, :].expand(-1, n_t, -1).reshape(-1, 3)


def _probe_in_box(rays_o, rays_d, camera, estimator, n: int = 16384):
    """Probe batch for the occupancy estimator's path: positions uniform in each of the grid's level boxes, an equal
    share per level (every sample the march produces lies in one of them), directions from an even subset of the call's
    rays - random unit directions when the call has none."""
    if rays_o is None:
        pose, H, W, focal, row0, nrows, dev = camera
        rays_o, rays_d = ops.get_rays(pose, int(H), int(W), float(focal), dev, int(row0), int(nrows))
    dev = rays_d.device
    R = rays_d.reshape(-1, 3).shape[0]
    g = torch.Generator(device="cpu").manual_seed(0)
    levels = estimator.levels
    xs = []
    for lvl in range(levels):
        lo, hi = estimator.level_aabb(lvl)
        lo, hi = torch.tensor(lo, device=dev), torch.tensor(hi, device=dev)
        m = n // levels + (1 if lvl < n % levels else 0)
        xs.append(lo + (hi - lo) * torch.rand(m, 3, generator=g).to(dev))
    if R == 0:
        d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1).to(dev)
    else:
        d = rays_d.reshape(-1, 3)[torch.linspace(0, R - 1, n, device=dev).long()].float()
    return torch.cat(xs), d


def _probe(estimator, rays_o, rays_d, camera=None):
    """The calibration probe of a call on these rays (or this camera), for its estimator."""
    if isinstance(estimator, OccGridEstimator):
        return lambda: _probe_in_box(rays_o, rays_d, camera, estimator)
    if isinstance(estimator, StratifiedEstimator):
        return lambda: _probe_on_rays(rays_o, rays_d, camera, *estimator.bounds())
    return None


def _nerfs(model, fine) -> list:
    """The call's distinct NeRFs: the networks the range guard looks after."""
    return [m for m in {id(model): model, id(fine): fine}.values() if isinstance(m, NeRF)]


def _launch_size(rays_o, camera):
    """(ray count, device) of a launch on ray tensors or on a camera (pose, H, W, focal, row0, nrows, dev)."""
    if camera is not None:
        return int(camera[5]) * int(camera[2]), torch.device(camera[6])
    return rays_o.shape[0], rays_o.device


# `sampling_kwargs` of render_rays / render_frame / render_path: what the reference hard-codes in its estimator.sampling
# call (rendering.py:66-74) plus the occupancy march's cone angle and per-ray bounds.  The four scalars are arguments of
# every occupancy kernel, fused ones included; cone_angle and t_min / t_max are arguments of the standalone march and of
# the one-launch kernel's extended entry point, which the routes use for them when FUSED_OCC_CONE is on (below).
_SAMPLING_DEFAULTS = dict(near_plane=0.0, far_plane=1e10, early_stop_eps=1e-4, alpha_thre=0.0)
_SAMPLING_MARCH_ONLY = ("cone_angle", "t_min", "t_max")


def _sampling_options(sampling_kwargs: Optional[dict], per_ray: bool = True) -> dict:
    """A checked copy of `sampling_kwargs` ({} for None); an unknown key is a TypeError.  Frames (`per_ray=False`)
    accept no per-ray t_min / t_max."""
    opts = dict(sampling_kwargs or {})
    allowed = tuple(_SAMPLING_DEFAULTS) + (_SAMPLING_MARCH_ONLY if per_ray else ("cone_angle",))
    unknown = sorted(k for k in opts if k not in allowed)
    if unknown:
        raise TypeError(f"sampling_kwargs: unexpected key(s) {unknown}; accepted: {list(allowed)}")
    return opts


def _has_march_options(opts: Optional[dict]) -> bool:
    opts = opts or {}
    return opts.get("cone_angle", 0.0) != 0.0 or opts.get("t_min") is not None or opts.get("t_max") is not None


def _march_only(opts: Optional[dict]) -> bool:
    """The options ask for a cone angle or per-ray bounds and the one-launch routes are closed to them (FUSED_OCC_CONE
    off, read at call time): the call goes through the standalone march."""
    return _has_march_options(opts) and not FUSED_OCC_CONE


def _occ_max_steps(estimator, render_step_size: float, opts: Optional[dict]) -> int:
    """Intervals a ray can have under the options: the cone march's count where a cone angle is given."""
    opts = opts or {}
    return estimator.max_steps(render_step_size, float(opts.get("cone_angle", 0.0)), float(opts.get("near_plane", 0.0)))


def _stratified_args(estimator, net: NeRF, R: int, dev, u, u_fine, train: bool, opts: Optional[dict] = None) -> dict:
    """The stratified estimator's launch arguments; a training call draws the jitter the caller did not pass (coarse,
    then fine).  Of the sampling options a fixed-count sampler knows the two planes (`bounds`)."""
    opts = opts or {}
    if any(k not in ("near_plane", "far_plane") for k in opts):
        raise ValueError("StratifiedEstimator: sampling_kwargs may hold near_plane / far_plane only")
    if u is None and train:
        u = estimator.draw_u(R, dev)
    if u_fine is None and train and estimator.n_importance > 0:
        u_fine = torch.rand(R, estimator.n_importance, device=dev, generator=estimator.generator)
    near, far = estimator.bounds(opts.get("near_plane", 0.0), opts.get("far_plane", 1e10))
    return dict(near=near, far=far, n_samples=estimator.n_samples, n_importance=estimator.n_importance, u=u,
                u_fine=u_fine, pos_mask=net._mask(net.pos_mask, dev), dir_mask=net._mask(net.dir_mask, dev))


def _occ_args(estimator, model: NeRF, render_step_size: float, u, dev, opts: Optional[dict] = None) -> dict:
    """The reference's estimator.sampling call (rendering.py:66-74: near_plane 0, far_plane 1e10, early_stop_eps 1e-4,
    alpha_thre 0, unless `opts` moves them) as the occupancy kernels' arguments; `u` = stratified jitter (one value per
    ray) or None.  A cone angle and per-ray bounds (FUSED_OCC_CONE) go through as they are."""
    opts = opts or {}
    scalars = {k: float(opts.get(k, v)) for k, v in _SAMPLING_DEFAULTS.items()}
    return dict(aabb=estimator.aabb, res=estimator.resolution, levels=estimator.levels, bits=estimator.bits,
                step=render_step_size, max_steps=_occ_max_steps(estimator, render_step_size, opts), u=u,
                pos_mask=model._mask(model.pos_mask, dev), dir_mask=model._mask(model.dir_mask, dev),
                cone_angle=float(opts.get("cone_angle", 0.0)), t_min=opts.get("t_min"), t_max=opts.get("t_max"), **scalars)


def _fused_launch(rays_o, rays_d, camera, estimator, model, model_fine, train, bk, render_step_size, u, u_fine,
                  want_extras, opts=None):
    """stratified-fused: ONE fused launch (ops.render_fused) for ray tensors or for a camera (rays generated in the
    launch), under the fp16 range guard -> render_rays' return."""
    fine = model_fine if model_fine is not None else model
    R, dev = _launch_size(rays_o, camera)
    kw = _stratified_args(estimator, fine, R, dev, u, u_fine, train, opts)
    probe = _probe(estimator, rays_o, rays_d, camera)
    launch = lambda: ops.render_fused(model.packed(probe) if estimator.n_importance > 0 else None, fine.packed(probe),
                                      rays_o, rays_d, bkgd=(bk, bk, bk), want_extras=want_extras, camera=camera, **kw)
    rgb, opacity, depth, ex = guarded_launch(_nerfs(model, fine), dev, "render_rays", probe, launch, "render_rays call")
    if not want_extras:  # frame rendering: only rgb / depth are consumed (rendering.py:169-171)
        return (rgb, opacity, depth, ex), None, None
    ray_indices, t_starts, t_ends = ops.edges_to_packed(ex["edges"])
    for k in ("weights", "alphas", "trans", "sigmas"):
        ex[k] = ex[k].reshape(-1)
    ex["rgbs"] = ex["rgbs"].reshape(-1, 3)
    return (rgb, opacity, depth, ex), ray_indices, (t_starts + t_ends) / 2.0


def _fused_occ_launch(rays_o, rays_d, camera, estimator, model, model_fine, train, bk, render_step_size, u, u_fine,
                      want_extras, opts=None):
    """occ-frame / occ-extras: the reference's own render path (occupancy estimator in the slot, rendering.py:58-107)
    as ONE launch (ops.render_occ_fused: march -> density pass -> visibility -> full pass -> packed integration, no host
    sync) under the fp16 range guard -> render_rays' return.  The extras mode (the reference's FULL return contract
    without gradients) is that launch + one gather behind one host read."""
    R, dev = _launch_size(rays_o, camera)
    kw = _occ_args(estimator, model, render_step_size, torch.rand(R, device=dev, generator=estimator.generator)
                   if train else None, dev, opts)
    probe = _probe(estimator, rays_o, rays_d, camera)
    launch = lambda: ops.render_occ_fused(model.packed(probe), rays_o, rays_d, bkgd=(bk, bk, bk), camera=camera,
                                          want_extras=want_extras, **kw)
    out = guarded_launch([model], dev, "render_rays", probe, launch, "render_rays call")
    if not want_extras:
        rgb, opacity, depth, _ = out
        return (rgb, opacity, depth, {}), None, None
    rgb, opacity, depth, _, (ray_indices, t_starts, t_ends, ex) = out
    return (rgb, opacity, depth, ex), ray_indices, (t_starts + t_ends) / 2.0


def _stratified_sampler(rays_o, rays_d, estimator, model, train, render_step_size, u, u_fine, needs_grad, opts=None):
    """The hierarchical sampler as ONE launch (ops.sample_fused) instead of stratified edges -> packed -> density pass
    -> weights -> resampling -> packed: same edges bit for bit."""
    dev = rays_o.device
    kw = _stratified_args(estimator, model, rays_o.shape[0], dev, u, u_fine, train, opts)
    edges = sampler_launch(model, needs_grad, dev, _probe(estimator, rays_o, rays_d),
                           lambda pm, status=None: ops.sample_fused(pm, rays_o, rays_d, status=status, **kw))
    with torch.no_grad():
        return ops.edges_to_packed(edges)


def _occ_sampler(rays_o, rays_d, estimator, model, train, render_step_size, u, u_fine, needs_grad, opts=None):
    """estimator.sampling(..., sigma_fn) of the reference's training step (rendering.py:66-74) as one launch + one
    gather (ops.occ_sample_fused): the same samples bit for bit as march -> density pass -> visibility -> compaction,
    one host read instead of two."""
    dev = rays_o.device
    kw = _occ_args(estimator, model, render_step_size, torch.rand(rays_o.shape[0], device=dev,
                                                                  generator=estimator.generator) if train else None, dev,
                   opts)
    launch = lambda pm, status=None: ops.occ_sample_fused(pm, rays_o, rays_d, status=status, **kw)
    if model.cull_precision is not None:
        # opt-in (NeRF.cull_precision): the cull's density pass in single-pass bf16 - no range flags to guard
        with torch.no_grad():
            return launch(model.packed_cull())
    return sampler_launch(model, needs_grad, dev, _probe(estimator, rays_o, rays_d), launch)


def _propnet_sampler(rays_o, rays_d, estimator, model, train, render_step_size, u, u_fine, needs_grad, opts=None):
    """propnet: PropNetEstimator.sampling with the estimator's own proposal networks, counts, planes and sampling type
    (a near_plane / far_plane among the options overrides the planes), flattened to the packed triple - every ray has
    exactly num_samples samples in order, so extras["trans"].reshape(n_rays, num_samples) is what the estimator's
    update_every_n_steps takes.  `u`: the per-level jitters, len(prop_samples) + 1 tensors [n_rays]."""
    opts = opts or {}
    if any(k not in ("near_plane", "far_plane") for k in opts):
        raise ValueError("PropNetEstimator: sampling_kwargs may hold near_plane / far_plane only")
    near, far = opts.get("near_plane", estimator.near_plane), opts.get("far_plane", estimator.far_plane)
    if near is None or far is None:
        raise ValueError("PropNetEstimator: near_plane and far_plane are needed (the estimator's, or in sampling_kwargs)")
    R, dev = rays_o.shape[0], rays_o.device
    requires_grad = bool(estimator.training and torch.is_grad_enabled() and estimator.proposal_requires_grad)
    t_starts, t_ends = estimator.sampling([prop_sigma_fn(m, rays_o, rays_d) for m in estimator.prop_models],
                                          estimator.prop_samples, estimator.num_samples, R, near, far,
                                          estimator.sampling_type, stratified=train, requires_grad=requires_grad, u=u,
                                          device=dev)
    ray_indices = torch.arange(R, device=dev).repeat_interleave(estimator.num_samples)
    return ray_indices, t_starts.reshape(-1), t_ends.reshape(-1)


def _estimator_sampling(rays_o, rays_d, estimator, model, train, render_step_size, u, u_fine, needs_grad, opts=None):
    def sigma_fn(t_starts, t_ends, ray_indices):
        if isinstance(model, NeRF):  # same values, gathers and midpoints inside the launch (no [N,3] tensors)
            return model.forward_rays(rays_o, rays_d, ray_indices, t_starts, t_ends, full=False).squeeze(-1)
        to, td = rays_o[ray_indices], rays_d[ray_indices]
        x = to + td * (t_starts + t_ends)[:, None] / 2.0
        return model(x).squeeze(-1)

    jitter = {"u": u, "u_fine": u_fine} if isinstance(estimator, StratifiedEstimator) else {}
    planes = {"near_plane": 0.0, "far_plane": 1e10, **(opts or {})}  # (None: the reference's own call)
    return estimator.sampling(rays_o, rays_d, sigma_fn=sigma_fn, render_step_size=render_step_size, stratified=train,
                              **planes, **jitter)


def _render_samples(samples, rays_o, rays_d, fine, train, white_bkgd, needs_grad, device, full_grad=False):
    """The sampler routes' common tail: the fine network's full pass on the packed samples -> `rendering`.  With
    `full_grad` the extras also carry the packed interval edges ("t_starts", "t_ends")."""
    ray_indices, t_starts, t_ends = samples

    def rgb_sigma_fn(t_starts, t_ends, ray_indices):
        if isinstance(fine, NeRF):
            out = fine.forward_rays(rays_o, rays_d, ray_indices, t_starts, t_ends, full=True)
            return out[..., :3], out[..., -1]
        to, td = rays_o[ray_indices], rays_d[ray_indices]
        x = to + td * (t_starts + t_ends)[:, None] / 2.0
        out = fine(x, td)
        return out[..., :3], out[..., -1]

    # rendering.py:86 builds `white_bkgd * torch.ones((3,), device=device, requires_grad=train)`: the background's own
    # requires_grad is what keeps loss.backward() legal when nothing else carries a gradient (an all-background batch,
    # a frozen model).  Whenever the samples themselves carry one, the three values go to the compositor as launch
    # arguments instead (a host tensor: no device round trip to read them, and none of the eight tiny launches that
    # add the background and differentiate it with torch ops sit on the training step's host path).
    if train and torch.is_grad_enabled() and not (needs_grad and ray_indices.numel() > 0):
        render_bkgd = white_bkgd * torch.ones((3,), device=device, requires_grad=True)
    else:
        render_bkgd = torch.full((3,), float(white_bkgd))
    try:
        output = rendering(t_starts, t_ends, ray_indices, n_rays=len(rays_o), rgb_sigma_fn=rgb_sigma_fn,
                           render_bkgd=render_bkgd, full_grad=full_grad)
        if full_grad:  # render_rays returns the midpoints only; a distortion loss needs the widths
            output[3].update(t_starts=t_starts, t_ends=t_ends)
    except AssertionError:  # same fallback as the reference (rendering.py:97-103)
        output = (torch.ones_like(rays_o) * white_bkgd, None,
                  torch.zeros_like(rays_o[:, 0].unsqueeze(1), dtype=torch.float32), None)
    return output, ray_indices, (t_starts + t_ends) / 2.0


# render_rays with gradients / extras: OccGridEstimator.sampling as one launch + one gather (ops.occ_sample_fused), for
# calls with at least this many rays.  Round 3 measured it SLOWER than the unfused sequence on the reference's training
# step (4096 rays, 353 marched samples per ray: 7.8-8.1 against 6.8-7.2 ms per step): the launch handed out rays in
# chunks of eight, 4096 rays are two chunks per workgroup, and a workgroup that drew two dense chunks evaluated 9,000
# candidates while its neighbour had none.  Round 4: the chunk size is guided by what is left in the queue (8 rays down
# to 1, csrc/render_occ.hip) and the tail of the launch is one ray's work: 6.2-6.4 ms per step either way on one device
# (bench.py --workload train-occ with FUSED_OCC_SAMPLER_MIN_RAYS 0 / 32768) - a tie, with one host read per step
# instead of two, so the reference's own batch size takes the fused sampler now.
FUSED_OCC_SAMPLER = True
FUSED_OCC_EXTRAS = True  # render_rays(want_extras=True) without gradients through the occupancy estimator: one launch + one gather
FUSED_OCC_SAMPLER_MIN_RAYS = 4096
FUSED_OCC_EXTRAS_MAX_SLOTS = 1 << 26  # rays x max_steps of the extras mode's per-ray slot rows (8 arrays of that many floats)
# A cone angle or per-ray t_min / t_max on the one-launch routes (fsn_render_rays_occgrid_ex): off, because
# tests/test_occ_cone_cpu.py pins such calls to estimator-sampling / chunked; on, they take the route the same call takes
# without them, sized by the cone march's interval count.  tools/bench_occ_cone.py measures both settings.
FUSED_OCC_CONE = False


def _occ_fusable(estimator, model, model_fine, render_step_size: float, opts: Optional[dict] = None) -> bool:
    return isinstance(estimator, OccGridEstimator) and isinstance(model, NeRF) and model_fine is None and \
        model.precision in ("fp16x3", "bf16x3", "fp16", "bf16") and \
        _occ_max_steps(estimator, render_step_size, opts) <= FUSED_OCC_MAX_STEPS


def _extras_slots_fit(estimator, n_rays: int, render_step_size: float, opts: Optional[dict]) -> bool:
    """The extras mode's per-ray slot rows against FUSED_OCC_EXTRAS_MAX_SLOTS, which counts eight arrays per slot: the
    cone regime holds a ninth (the interval ends)."""
    arrays = 9 if (opts or {}).get("cone_angle", 0.0) > 0.0 else 8
    return n_rays * _occ_max_steps(estimator, render_step_size, opts) * arrays <= FUSED_OCC_EXTRAS_MAX_SLOTS * 8


def _stratified_fusable(estimator, model, fine) -> bool:
    return isinstance(estimator, StratifiedEstimator) and isinstance(model, NeRF) and isinstance(fine, NeRF)


def _rays_route(estimator, model, model_fine, needs_grad: bool, want_extras: bool, n_rays: int,
                render_step_size: float, sampling_kwargs: Optional[dict] = None) -> str:
    """render_rays' launch route, from plain attribute tests (the FUSED_OCC_* switches are read at call time).  The
    scalar sampling options (planes, thresholds) are arguments of every route's kernels and choose nothing; a cone
    angle or per-ray bounds take the standalone march unless FUSED_OCC_CONE opens the one-launch routes to them, which
    then apply the rules below with the cone march's interval count.  A PropNetEstimator always takes its own route
    (it is its own sampler; the options it cannot honour are a ValueError there)."""
    if isinstance(estimator, PropNetEstimator):
        return "propnet"
    if _march_only(sampling_kwargs):
        return "estimator-sampling"
    opts = sampling_kwargs
    # (NeRF.cull_precision, opt-in: the cull's density pass runs as its own launch in that mode - the occupancy sampler)
    own_cull = isinstance(model, NeRF) and model.cull_precision is not None
    if not needs_grad and not own_cull and _occ_fusable(estimator, model, model_fine, render_step_size, opts):
        if not want_extras:
            return "occ-frame"
        if FUSED_OCC_EXTRAS and _extras_slots_fit(estimator, n_rays, render_step_size, opts):
            return "occ-extras"
    # the fused launch is forward-only; a training step goes through sampler -> model(x, d) -> rendering, each
    # differentiable where the reference's is
    if not needs_grad and _stratified_fusable(estimator, model, model_fine if model_fine is not None else model):
        return "stratified-fused"
    if isinstance(estimator, StratifiedEstimator) and estimator.n_importance > 0 and isinstance(model, NeRF) and \
            model.precision in ("fp16x3", "bf16x3", "fp16", "bf16", "fp16x2"):
        return "stratified-sampler"
    if FUSED_OCC_SAMPLER and (n_rays >= max(1, FUSED_OCC_SAMPLER_MIN_RAYS) or own_cull) and \
            _occ_fusable(estimator, model, None, render_step_size, opts):
        return "occ-sampler"
    return "estimator-sampling"


_ONE_LAUNCH = {"occ-frame": _fused_occ_launch, "occ-extras": _fused_occ_launch, "stratified-fused": _fused_launch}
_SAMPLERS = {"stratified-sampler": _stratified_sampler, "occ-sampler": _occ_sampler,
             "estimator-sampling": _estimator_sampling, "propnet": _propnet_sampler}


def render_rays(rays_o: Tensor, rays_d: Tensor, estimator, model: nn.Module, train: bool = False,
                white_bkgd: bool = False, render_step_size: float = 5e-3,
                device: torch.device = torch.device("cuda"), *, model_fine: Optional[nn.Module] = None,
                u: Optional[Tensor] = None, u_fine: Optional[Tensor] = None, want_extras: bool = True,
                full_grad: bool = False, sampling_kwargs: Optional[dict] = None):
    """See module docstring.  Keyword-only extras over the reference: `model_fine` (second network
    of the hierarchical pass; default = `model`, as the reference uses one network for both of
    its passes), explicit jitter tensors `u` / `u_fine`, `want_extras`, and `full_grad`: a training call whose depth,
    opacity and extras["weights" | "alphas" | "trans"] all carry gradients to the model (`rendering(full_grad=True)`;
    the default differentiates through rgb and opacity only), with the packed interval edges as extras["t_starts"] /
    extras["t_ends"].  It is ignored on the forward-only one-launch routes, which have no gradients.
    `sampling_kwargs`: options of the estimator's sampling call the reference hard-codes - `near_plane`, `far_plane`,
    `early_stop_eps`, `alpha_thre` (every occupancy route takes them) - and of the occupancy march: `cone_angle`
    (dt = max(t cone_angle, render_step_size)) and per-ray `t_min` / `t_max` [n_rays], which go through
    `estimator.sampling` (with FUSED_OCC_CONE on: through the route the call takes without them).  None is the
    reference's call; an unknown key is a TypeError.  A `PropNetEstimator` in the estimator slot (render/propnet.py) takes
    the "propnet" route: its own `sampling` (near_plane / far_plane are the only options it knows; `u`: its per-level
    jitters, len(prop_samples) + 1 tensors [n_rays]), then the full pass and `rendering`."""
    opts = _sampling_options(sampling_kwargs)
    rays_o = rays_o.to(device)
    rays_d = rays_d.to(device)
    fine = model_fine if model_fine is not None else model
    # (rays that require grad - camera-pose refinement - take the differentiable route too: forward_rays carries their
    # gradients, with a frozen or an eval-mode network as well)
    needs_grad = torch.is_grad_enabled() and isinstance(fine, nn.Module) and \
        ((fine.training and any(p.requires_grad for p in fine.parameters())) or rays_o.requires_grad or rays_d.requires_grad)
    route = _rays_route(estimator, model, model_fine, needs_grad, want_extras, rays_o.shape[0], render_step_size, opts)
    if route in _ONE_LAUNCH:
        return _ONE_LAUNCH[route](rays_o, rays_d, None, estimator, model, model_fine, train, float(white_bkgd),
                                  render_step_size, u, u_fine, want_extras, opts)
    samples = _SAMPLERS[route](rays_o, rays_d, estimator, model, train, render_step_size, u, u_fine, needs_grad, opts)
    return _render_samples(samples, rays_o, rays_d, fine, train, white_bkgd, needs_grad, device, full_grad)


# A frame under the deferred range check is rendered at most this many times: every repeat follows a re-calibration (at
# most three target moves per set of weights, ActScaling.recalibrate) or the switch to bf16x3, which raises no flags.
_FRAME_RERUNS = 6


def _frame_route(estimator, model, model_fine, training: bool, ndc: bool, render_step_size: float,
                 sampling_kwargs: Optional[dict] = None) -> str:
    """render_frame's launch route, from plain attribute tests (sampling options: as in _rays_route)."""
    if _march_only(sampling_kwargs):
        return "chunked"
    if not training and not ndc and _stratified_fusable(estimator, model, model_fine if model_fine is not None else model):
        # ONE persistent launch per frame - the rays are generated inside it from (pose, pixel
        # index), nothing per sample or per ray is kept in HBM besides the image, so `chunksize` (the reference's
        # memory knob: 313 launches for an 800x800 frame at 2048) is not needed.  Rays are independent: the image is
        # the chunked one.
        return "camera-stratified"
    own_cull = isinstance(model, NeRF) and model.cull_precision is not None  # (opt-in: sampler launch + full pass)
    if not training and not ndc and not own_cull and \
            _occ_fusable(estimator, model, model_fine, render_step_size, sampling_kwargs):
        return "camera-occupancy"  # the reference's own frame path (occupancy estimator): ONE launch
    return "chunked"


def _camera_frame(route, hwf, pose, chunksize, estimator, model, model_fine, training, train, ndc, white_bkgd,
                  render_step_size, device, opts=None):
    """ONE launch with the rays generated inside it -> (rgb, depth, flagged).  The end-of-frame look gets no
    `events_before`: a range event the synchronous guard handled inside the launch leaves nothing to render again."""
    H, W, focal = hwf
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    cam = (pose, H, W, focal, 0, H, dev)
    launch = _fused_launch if route == "camera-stratified" else _fused_occ_launch
    (rgb, _, depth, _), _, _ = launch(None, None, cam, estimator, model, model_fine, train, float(white_bkgd),
                                      render_step_size, None, None, False, opts)
    nets = _nerfs(model, model_fine if model_fine is not None else model)
    return rgb, depth, frame_flagged(nets, dev, probe=_probe(estimator, None, None, cam))


def _chunked_frame(route, hwf, pose, chunksize, estimator, model, model_fine, training, train, ndc, white_bkgd,
                   render_step_size, device, opts=None):
    """get_rays -> (ndc) -> render_rays per chunk -> (rgb, depth, flagged); no image when flagged: some chunk is invalid
    (this look, or an earlier chunk's flag consumed by the next chunk's poll)."""
    fine = model_fine if model_fine is not None else model
    rays_o, rays_d = U.get_rays(pose, hwf, device)
    rays_o, rays_d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
    if ndc:
        rays_o, rays_d = U.to_ndc(rays_o, rays_d, hwf, 1.0)
    if not training and _stratified_fusable(estimator, model, fine):  # (NDC frames: to_ndc, then one fused launch)
        chunksize = max(int(rays_o.shape[0]), 1)
    nets = _nerfs(model, fine)
    events0 = sum(m.range_events for m in nets)
    img, depth = [], []
    for co, cd in zip(U.get_chunks(rays_o, chunksize), U.get_chunks(rays_d, chunksize)):
        (rgb, _, d, _), *_ = render_rays(co, cd, estimator, model, train=train, white_bkgd=white_bkgd,
                                         render_step_size=render_step_size, device=device, model_fine=model_fine,
                                         want_extras=False, sampling_kwargs=opts or None)
        img.append(rgb)
        depth.append(d)
    if img and frame_flagged(nets, img[0].device, events0, _probe(estimator, rays_o, rays_d)):
        return None, None, True
    return torch.cat(img, dim=0), torch.cat(depth, dim=0), False


def render_frame(hwf: Tuple[int, int, float], near: float, far: float, pose: Tensor, chunksize: int, estimator,
                 model: nn.Module, train: bool = False, ndc: bool = False, white_bkgd: bool = False,
                 render_step_size: float = 5e-3, device: torch.device = torch.device("cuda"), *,
                 model_fine: Optional[nn.Module] = None, sampling_kwargs: Optional[dict] = None) -> Tuple[Tensor, Tensor]:
    """One image: get_rays -> (ndc) -> chunks -> render_rays -> cat; depth clamped to [near, far]
    (rendering.py:146-177).  Deliberate difference: the reference passes `white_bkgd` positionally
    into render_rays' `train` slot (rendering.py:160-168), so its frames are always composited on
    black; here `train` and `white_bkgd` go to the parameters they name.  `sampling_kwargs`: as render_rays', without
    the per-ray t_min / t_max."""
    opts = _sampling_options(sampling_kwargs, per_ray=False)
    H, W, _ = hwf
    fine = model_fine if model_fine is not None else model
    training = torch.is_grad_enabled() and isinstance(fine, nn.Module) and fine.training
    for _ in range(_FRAME_RERUNS):
        # deferred range check: one look per frame; a flagged frame is rendered again after the models' re-calibration
        # on the frame's OWN rays (or their switch to bf16x3), and the repeat is looked at as well
        route = _frame_route(estimator, model, model_fine, training, ndc, render_step_size, opts)
        run = _chunked_frame if route == "chunked" else _camera_frame
        rgb, depth, flagged = run(route, hwf, pose, chunksize, estimator, model, model_fine, training, train, ndc,
                                  white_bkgd, render_step_size, device, opts)
        if not flagged:
            break
    return rgb.reshape(H, W, 3), depth.clamp(near, far).reshape(H, W)


def to8b(x):
    """float image(s) in [0,1] -> uint8 (rendering.py:21).  Tensors are converted on the GPU."""
    if isinstance(x, Tensor):
        return ops.to8b(x)
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def render_path(render_poses: Tensor, hwf: Tuple[int, int, float], near: float, far: float, chunksize: int,
                model: nn.Module, estimator, ndc: bool = False, train: bool = False, white_bkgd: bool = False,
                render_step_size: float = 5e-3, device: torch.device = torch.device("cuda"), *,
                model_fine: Optional[nn.Module] = None, sampling_kwargs: Optional[dict] = None):
    """One frame per pose under no_grad -> (frames [N,H,W,3], d_frames [N,H,W]) as numpy arrays, like the
    reference (rendering.py:180-248; no progress bar).  Each frame is get_rays + one fused launch per chunk."""
    H, W, _ = hwf
    frames, d_frames = [], []
    for pose in render_poses:
        with torch.no_grad():
            rgb, depth = render_frame(hwf, near, far, pose, chunksize, estimator, model, train=train, ndc=ndc,
                                      white_bkgd=white_bkgd, render_step_size=render_step_size, device=device,
                                      model_fine=model_fine, sampling_kwargs=sampling_kwargs)
        frames.append(rgb.reshape(H, W, 3).detach().cpu().numpy())
        d_frames.append(depth.reshape(H, W).detach().cpu().numpy())
    return np.stack(frames, 0), np.stack(d_frames, 0)


def render_video(frames, d_frames, cmap: str = "plasma"):
    """Video tensors (rendering.py:240-266): (uint8 [N,3,H,W] colour frames, uint8 [N,3,H,W] colormapped depth frames),
    depth normalised with the minimum / maximum over ALL frames.  The whole assembly (to8b, NHWC -> NCHW, Normalize,
    colormap lookup) runs on the GPU; numpy inputs (what `render_path` returns, like the reference's) are uploaded
    once and numpy arrays are returned, tensors in -> tensors out."""
    as_np = not isinstance(frames, Tensor)
    dev = torch.device("cuda", torch.cuda.current_device()) if as_np else frames.device
    fr = torch.as_tensor(np.ascontiguousarray(frames), dtype=torch.float32).to(dev) if as_np else frames
    dp = torch.as_tensor(np.ascontiguousarray(d_frames), dtype=torch.float32).to(dev) if as_np else d_frames.to(dev)
    f8, d8 = ops.video_tensors(fr, dp, cmap)
    return (f8.cpu().numpy(), d8.cpu().numpy()) if as_np else (f8, d8)
