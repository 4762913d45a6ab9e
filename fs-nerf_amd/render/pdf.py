"""nerfacc's `pdf` call surface on HIP kernels (csrc/propnet.hip): what a proposal-network sampler is built from.

  RayIntervals(vals, packed_info=None, is_left=None, is_right=None)      interval edges per ray, [n_rays, n_edges]
  RaySamples(vals, packed_info=None, ray_indices=None, is_valid=None)    sample centres per ray, [n_rays, n_samples]
  searchsorted(sorted_sequence, values) -> (ids_left, ids_right)
  importance_sampling(intervals, cdfs, n_intervals_per_ray, stratified=False) -> (RayIntervals, RaySamples)

Names, argument names and return orders are nerfacc 0.5.x's.  nerfacc's source is not part of the reference, so the
arithmetic is THIS PACKAGE'S definition of nerfacc's documented semantics ("Proposal-network estimator");
parity with nerfacc's own kernels is not pinned.

Only the batched (dense) form is supported: every tensor is [n_rays, .] float32 on the GPU, all rays with the same
number of edges.  nerfacc's packed (flattened) form - a holder with `packed_info`, or a per-ray tensor of interval
counts - is a NotImplementedError that names the dense form.  A CPU tensor is a RuntimeError: there is no CPU fallback."""
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import torch
from torch import Tensor

from .. import ops


@dataclass
class RayIntervals:
    """Interval edges along rays: `vals` [n_rays, n_edges].  The optional fields are nerfacc's packed-form fields; the
    kernels take the batched form only, where they stay None."""
    vals: Tensor
    packed_info: Optional[Tensor] = None
    is_left: Optional[Tensor] = None
    is_right: Optional[Tensor] = None

    @property
    def device(self) -> torch.device:
        return self.vals.device


@dataclass
class RaySamples:
    """Sample centres along rays: `vals` [n_rays, n_samples]; optional fields as RayIntervals'."""
    vals: Tensor
    packed_info: Optional[Tensor] = None
    ray_indices: Optional[Tensor] = None
    is_valid: Optional[Tensor] = None

    @property
    def device(self) -> torch.device:
        return self.vals.device


def _dense_vals(x: Union[RayIntervals, RaySamples, Tensor], what: str) -> Tensor:
    """The [n_rays, k] tensor of a holder (or a plain tensor) in the batched form."""
    if isinstance(x, (RayIntervals, RaySamples)):
        if x.packed_info is not None:
            raise NotImplementedError(f"{what}: the packed (flattened) form is not supported; pass the dense form, "
                                      "vals [n_rays, k] with packed_info=None")
        x = x.vals
    if x.dim() < 1:
        raise ValueError(f"{what}: expected the dense form [n_rays, k]")
    return x


def searchsorted(sorted_sequence: Union[RayIntervals, RaySamples, Tensor],
                 values: Union[RayIntervals, RaySamples, Tensor]) -> Tuple[Tensor, Tensor]:
    """-> (ids_left, ids_right), int64, shaped like `values`.  Per ray, with h the number of entries of the sorted
    sequence that are <= the value and K their count: ids_left = max(h - 1, 0), ids_right = min(h, K - 1) - inside the
    range sorted_sequence[ids_left] <= value < sorted_sequence[ids_right]; below the first entry both are 0, at or
    beyond the last both are K - 1."""
    keys, q = _dense_vals(sorted_sequence, "searchsorted"), _dense_vals(values, "searchsorted")
    if keys.shape[:-1] != q.shape[:-1]:
        raise ValueError(f"searchsorted: leading shapes differ, {tuple(keys.shape)} and {tuple(q.shape)}")
    il, ir = ops.searchsorted_dense(keys.detach().reshape(-1, keys.shape[-1]), q.detach().reshape(-1, q.shape[-1]))
    return il.reshape(q.shape), ir.reshape(q.shape)


@torch.no_grad()
def importance_sampling(intervals: RayIntervals, cdfs: Tensor, n_intervals_per_ray: int, stratified: bool = False, *,
                        u: Optional[Tensor] = None) -> Tuple[RayIntervals, RaySamples]:
    """`n_intervals_per_ray` new intervals per ray from the piecewise-linear inverse of `cdfs` [n_rays, n_edges]
    (non-decreasing, 0 at the first edge, 1 at the last) over `intervals.vals` -> (RayIntervals [n_rays, n + 1],
    RaySamples [n_rays, n]).  The centres are the inverse cdf at u_i = (i + b) / n, b = 0.5, or with `stratified` one
    uniform draw in [0, 1) per ray (`u` [n_rays]: that draw, given); the edges are the midpoints of neighbouring centres,
    the two ends mirrored about the first / last centre and kept inside the support.  No gradient flows through it."""
    vals = _dense_vals(intervals, "importance_sampling")
    if isinstance(n_intervals_per_ray, Tensor):
        raise NotImplementedError("importance_sampling: a per-ray tensor of interval counts belongs to the packed "
                                  "(flattened) form, which is not supported; pass the dense form and one int")
    if cdfs.shape != vals.shape:
        raise ValueError(f"importance_sampling: cdfs {tuple(cdfs.shape)} and intervals {tuple(vals.shape)} differ")
    n = int(n_intervals_per_ray)
    lead = vals.shape[:-1]
    v2, c2 = vals.reshape(-1, vals.shape[-1]), cdfs.reshape(-1, vals.shape[-1])
    ops._gpu_f32(v2, "intervals")
    if u is None and stratified:
        u = torch.rand(v2.shape[0], device=v2.device)
    s, x, _ = ops.importance_sample(v2, c2, n, u)
    return RayIntervals(vals=s.reshape(*lead, n + 1)), RaySamples(vals=x.reshape(*lead, n))
