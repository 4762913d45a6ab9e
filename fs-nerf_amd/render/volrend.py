"""nerfacc's `volrend` / `scan` / `pack` call surface on HIP kernels (csrc/packed_scan.hip): the packed building blocks
of volume rendering, each differentiable one a single autograd Function over one forward / one backward launch.

  pack_info(ray_indices, n_rays=None)
  inclusive_sum / exclusive_sum / inclusive_prod / exclusive_prod (inputs, packed_info=None, indices=None)
  render_transmittance_from_density / render_transmittance_from_alpha
  render_weight_from_density / render_weight_from_alpha
  render_visibility_from_density / render_visibility_from_alpha
  accumulate_along_rays(weights, values=None, ray_indices=None, n_rays=None)

Names, argument names and return orders are nerfacc 0.5.x's.  nerfacc's source is not part of the reference, so the
arithmetic is THIS PACKAGE'S definition of nerfacc's documented semantics ("Packed volume-rendering
primitives"); parity with nerfacc's own kernels is not pinned.

Common rules.  Inputs are GPU float32 tensors (a CPU tensor is a RuntimeError: there is no CPU fallback).  The samples
of a ray are found through exactly one of: `packed_info` int64 [n_rays, 2] = (start, count), as `pack_info` returns it
(no search, no host read; it wins when `ray_indices` is given as well); `ray_indices` / `indices` int64 [N], which MUST
BE SORTED (non-decreasing) - every sampler of this package returns them so - with `n_rays` (None: one host read of
ray_indices.max() + 1); neither: the input is dense, [..., n_samples], every row a ray.  Gradients go to `inputs`,
`sigmas`, `alphas`, `weights` and `values`; none goes to the interval edges, to `prefix_trans` or to indices."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from .. import ops


def _spans(t: Tensor, packed_info: Optional[Tensor], ray_indices: Optional[Tensor], n_rays: Optional[int]) -> ops.RaySpans:
    """The addressing of the N = t.numel() samples of `t` (module docstring)."""
    N = t.numel()
    if packed_info is not None:
        return ops.RaySpans(N, packed_info.shape[0], packed_info=packed_info)
    if ray_indices is not None:
        if n_rays is None:
            n_rays = int(ray_indices.max()) + 1 if N > 0 else 0
        return ops.RaySpans(N, int(n_rays), ray_indices=ray_indices)
    if t.dim() < 1:
        raise ValueError("dense input: expected [..., n_samples]")
    S = int(t.shape[-1])
    return ops.RaySpans(N, N // S if S > 0 else 0, dense_S=S)


def pack_info(ray_indices: Tensor, n_rays: Optional[int] = None) -> Tensor:
    """Sorted `ray_indices` [N] -> packed_info int64 [n_rays, 2] = (start, count) per ray.  A ray without samples has
    count 0 and the start where its samples would be.  `n_rays` None: ray_indices.max() + 1 (one host read)."""
    if n_rays is None:
        n_rays = int(ray_indices.max()) + 1 if ray_indices.numel() > 0 else 0
    return ops.pack_info(ray_indices, int(n_rays))


class _ScanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, spans, prod, exclusive):
        out = ops.packed_scan_fwd(x, spans, prod, exclusive)
        ctx.save_for_backward(*((x,) if prod else ()))
        ctx.spans, ctx.prod, ctx.exclusive = spans, prod, exclusive
        return out.reshape(x.shape)

    @staticmethod
    def backward(ctx, g):
        x = ctx.saved_tensors[0] if ctx.prod else None
        d_x = ops.packed_scan_bwd(x, g, ctx.spans, ctx.prod, ctx.exclusive)
        return d_x.reshape(g.shape), None, None, None


def _scan(inputs, packed_info, indices, prod, exclusive):
    x = ops._gpu_f32(inputs, "inputs")
    return _ScanFn.apply(x, _spans(x, packed_info, indices, None), prod, exclusive)


def inclusive_sum(inputs: Tensor, packed_info: Optional[Tensor] = None, indices: Optional[Tensor] = None) -> Tensor:
    """out[k] = sum of the ray's inputs[j], j <= k.  Flat `inputs` [N] with `packed_info` or sorted `indices`; with
    neither, along the last dimension of a dense tensor.  Differentiable w.r.t. `inputs`."""
    return _scan(inputs, packed_info, indices, False, False)


def exclusive_sum(inputs: Tensor, packed_info: Optional[Tensor] = None, indices: Optional[Tensor] = None) -> Tensor:
    """out[k] = sum of the ray's inputs[j], j < k (0 at a ray's first sample); arguments as `inclusive_sum`."""
    return _scan(inputs, packed_info, indices, False, True)


def inclusive_prod(inputs: Tensor, packed_info: Optional[Tensor] = None, indices: Optional[Tensor] = None) -> Tensor:
    """out[k] = product of the ray's inputs[j], j <= k; arguments as `inclusive_sum`.  The backward is division-free: an
    input of exactly 0 has a finite, correct gradient."""
    return _scan(inputs, packed_info, indices, True, False)


def exclusive_prod(inputs: Tensor, packed_info: Optional[Tensor] = None, indices: Optional[Tensor] = None) -> Tensor:
    """out[k] = product of the ray's inputs[j], j < k (1 at a ray's first sample); arguments and backward as
    `inclusive_prod`."""
    return _scan(inputs, packed_info, indices, True, True)


class _WeightsFn(torch.autograd.Function):
    """(weights, trans, alphas) from sigmas or from alphas: fsn_packed_weights_fwd / _bwd.  An output nobody asked for
    is None and never computed; a cotangent nobody sent is None and reaches the kernel as a NULL pointer."""

    @staticmethod
    def forward(ctx, v, t_starts, t_ends, prefix_trans, spans, from_alpha, want):
        outs = ops.packed_weights_fwd(v, t_starts, t_ends, spans, from_alpha, prefix_trans, want)
        ctx.save_for_backward(v, t_starts, t_ends, prefix_trans)
        ctx.spans, ctx.from_alpha = spans, from_alpha
        ctx.set_materialize_grads(False)
        return tuple(None if o is None else o.reshape(v.shape) for o in outs)

    @staticmethod
    def backward(ctx, d_weights, d_trans, d_alphas):
        v, t0, t1, p = ctx.saved_tensors
        if d_weights is None and d_trans is None and d_alphas is None:
            return (None,) * 7
        d_v = ops.packed_weights_bwd(v, t0, t1, ctx.spans, ctx.from_alpha, p, d_weights, d_trans, d_alphas)
        return d_v.reshape(v.shape), None, None, None, None, None, None


def _weights(v, t_starts, t_ends, packed_info, ray_indices, n_rays, prefix_trans, from_alpha, want):
    v = ops._gpu_f32(v, "alphas" if from_alpha else "sigmas")
    det = lambda t, name: None if t is None else ops._gpu_f32(t.detach(), name)
    return _WeightsFn.apply(v, det(t_starts, "t_starts"), det(t_ends, "t_ends"), det(prefix_trans, "prefix_trans"),
                            _spans(v, packed_info, ray_indices, n_rays), from_alpha, want)


def render_transmittance_from_density(t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, packed_info: Optional[Tensor] = None,
                                      ray_indices: Optional[Tensor] = None, n_rays: Optional[int] = None,
                                      prefix_trans: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """-> (trans, alphas): alpha_i = 1 - exp(-sigma_i (t_ends_i - t_starts_i)), trans_i = exp(-sum_{j<i} sigma_j dt_j)
    within the ray, times prefix_trans_i when given.  The compositor's own values, bit for bit.  Differentiable w.r.t.
    `sigmas`."""
    _, trans, alphas = _weights(sigmas, t_starts, t_ends, packed_info, ray_indices, n_rays, prefix_trans, False,
                                (False, True, True))
    return trans, alphas


def render_transmittance_from_alpha(alphas: Tensor, packed_info: Optional[Tensor] = None, ray_indices: Optional[Tensor] = None,
                                    n_rays: Optional[int] = None, prefix_trans: Optional[Tensor] = None) -> Tensor:
    """-> trans: trans_i = prod_{j<i} (1 - alpha_j) within the ray, times prefix_trans_i when given.  Differentiable
    w.r.t. `alphas`, division-free (alpha == 1 is fine)."""
    return _weights(alphas, None, None, packed_info, ray_indices, n_rays, prefix_trans, True, (False, True, False))[1]


def render_weight_from_density(t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, packed_info: Optional[Tensor] = None,
                               ray_indices: Optional[Tensor] = None, n_rays: Optional[int] = None,
                               prefix_trans: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """-> (weights, trans, alphas): `render_transmittance_from_density`'s values and weights = trans * alphas - what
    `rendering` returns in extras["weights" | "trans" | "alphas"], bit for bit.  Differentiable w.r.t. `sigmas`
    through all three."""
    return _weights(sigmas, t_starts, t_ends, packed_info, ray_indices, n_rays, prefix_trans, False, (True, True, True))


def render_weight_from_alpha(alphas: Tensor, packed_info: Optional[Tensor] = None, ray_indices: Optional[Tensor] = None,
                             n_rays: Optional[int] = None, prefix_trans: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """-> (weights, trans): `render_transmittance_from_alpha`'s trans and weights = trans * alphas.  Differentiable
    w.r.t. `alphas` through both."""
    return _weights(alphas, None, None, packed_info, ray_indices, n_rays, prefix_trans, True, (True, True, False))[:2]


@torch.no_grad()
def render_visibility_from_density(t_starts: Tensor, t_ends: Tensor, sigmas: Tensor, packed_info: Optional[Tensor] = None,
                                   ray_indices: Optional[Tensor] = None, n_rays: Optional[int] = None,
                                   early_stop_eps: float = 1e-4, alpha_thre: float = 0.0) -> Tensor:
    """-> bool, shaped like `sigmas`: trans_i >= early_stop_eps and alpha_i >= alpha_thre, on
    `render_transmittance_from_density`'s values (the occupancy sampler's rule, bit for bit)."""
    trans, alphas = render_transmittance_from_density(t_starts, t_ends, sigmas.detach(), packed_info, ray_indices, n_rays)
    return (trans >= early_stop_eps) & (alphas >= alpha_thre)


@torch.no_grad()
def render_visibility_from_alpha(alphas: Tensor, packed_info: Optional[Tensor] = None, ray_indices: Optional[Tensor] = None,
                                 n_rays: Optional[int] = None, early_stop_eps: float = 1e-4,
                                 alpha_thre: float = 0.0) -> Tensor:
    """-> bool, shaped like `alphas`: trans_i >= early_stop_eps and alpha_i >= alpha_thre with
    trans_i = prod_{j<i} (1 - alpha_j).  For an opacity-valued field this is the cull `OccGridEstimator.sampling` does
    with `sigma_fn`: call it on the march's output and keep the samples it marks."""
    a = ops._gpu_f32(alphas.detach(), "alphas")
    keep = ops.packed_visibility_alpha(a, _spans(a, packed_info, ray_indices, n_rays), early_stop_eps, alpha_thre)
    return keep.reshape(a.shape)


class _AccumulateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, values, spans):
        out = ops.accumulate_fwd(weights, values, spans)
        ctx.save_for_backward(weights, values)
        ctx.spans = spans
        return out

    @staticmethod
    def backward(ctx, g):
        weights, values = ctx.saved_tensors
        want_v = values is not None and ctx.needs_input_grad[1]
        d_w, d_v = ops.accumulate_bwd(g, weights, values, ctx.spans, ctx.needs_input_grad[0], want_v)
        return (None if d_w is None else d_w.reshape(weights.shape), None if d_v is None else d_v.reshape(values.shape),
                None)


def accumulate_along_rays(weights: Tensor, values: Optional[Tensor] = None, ray_indices: Optional[Tensor] = None,
                          n_rays: Optional[int] = None) -> Tensor:
    """out[r] = sum over the ray's samples of weights_i * values_i -> [n_rays, D]; `values` None: the sum of the weights,
    [n_rays, 1].  Flat: weights [N], values [N, D], sorted `ray_indices` [N].  Dense (`ray_indices` None): weights
    [n_rays, n_samples], values [n_rays, n_samples, D].  A ray without samples gives an exact 0 row.  Differentiable
    w.r.t. `weights` and `values`."""
    w = ops._gpu_f32(weights, "weights")
    v = None if values is None else ops._gpu_f32(values, "values")
    if v is not None and (v.dim() != w.dim() + 1 or v.shape[:-1] != w.shape):
        raise ValueError(f"values: expected shape {tuple(w.shape)} + (D,), got {tuple(v.shape)}")
    if ray_indices is None and w.dim() != 2:
        raise ValueError("accumulate_along_rays without ray_indices: weights must be [n_rays, n_samples]")
    return _AccumulateFn.apply(w, v, _spans(w, None, ray_indices, n_rays))
