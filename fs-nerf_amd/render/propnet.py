"""nerfacc's `PropNetEstimator` on HIP kernels (csrc/propnet.hip): a sampler that learns where to sample.

A chain of small proposal networks turns a uniform (or uniform-in-disparity) lattice into the final intervals: per level,
importance-sample the current histogram, evaluate the level's density on the new intervals, take the cdf of its
transmittance.  The proposals are trained by the interlevel loss, which asks each proposal histogram to bound the final
network's own weights from above - `update_every_n_steps(extras["trans"])` after the main step.

  PropNetEstimator(optimizer=None, scheduler=None, *, prop_models=(), prop_samples=(), num_samples=64, ...)
      .sampling(prop_sigma_fns, prop_samples, num_samples, n_rays, near_plane, far_plane, sampling_type="lindisp",
                stratified=False, requires_grad=False) -> (t_starts, t_ends), each [n_rays, num_samples]
      .compute_loss(trans, loss_scaler=1.0) / .update_every_n_steps(trans, requires_grad=False, loss_scaler=1.0)
  prop_sigma_fn(model, rays_o, rays_d)       a (t_starts, t_ends) -> sigmas closure for this package's NeRF

Names, argument names and return orders are nerfacc 0.5.x's; the arithmetic is this package's definition (render/pdf.py,
DESIGN.md "Proposal-network estimator"), parity with nerfacc's kernels is not pinned.  Everything is in the dense form:
[n_rays, .] float32 GPU tensors."""
from typing import Callable, List, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from .. import ops
from ..core.models import NeRF
from . import volrend
from .pdf import RayIntervals


def _transform_stot(transform_type: str, s_vals: Tensor, t_min, t_max) -> Tensor:
    """s in [0, 1] -> t in [t_min, t_max]: "uniform": t = s t_max + (1 - s) t_min; "lindisp" (uniform in disparity):
    t = 1 / (s / t_max + (1 - s) / t_min).  The sampler kernels apply the same operation sequence themselves; this is the
    torch form for a caller's own s-values."""
    if transform_type == "uniform":
        return s_vals * t_max + (1.0 - s_vals) * t_min
    if transform_type == "lindisp":
        return 1.0 / (s_vals * (1.0 / t_max) + (1.0 - s_vals) * (1.0 / t_min))
    raise ValueError(f"sampling_type: expected 'uniform' or 'lindisp', got {transform_type!r}")


class _PdfLossFn(torch.autograd.Function):
    """The interlevel loss per query interval, one launch each way (fsn_prop_loss_fwd / _bwd); the gradient goes to the
    proposal's cdfs only."""

    @staticmethod
    def forward(ctx, cdfs_key, segments_query, cdfs_query, segments_key):
        ctx.save_for_backward(segments_query, cdfs_query, segments_key, cdfs_key)
        return ops.prop_loss_fwd(segments_query, cdfs_query, segments_key, cdfs_key)

    @staticmethod
    def backward(ctx, g):
        q, cq, k, ck = ctx.saved_tensors
        return ops.prop_loss_bwd(q, cq, k, ck, g.contiguous()), None, None, None


def _pdf_loss(segments_query: RayIntervals, cdfs_query: Tensor, segments_key: RayIntervals, cdfs_key: Tensor) -> Tensor:
    """-> [n_rays, n_query_intervals]: how far each query interval's mass w = cdfs_query[i+1] - cdfs_query[i] exceeds the
    bound the key histogram gives it, wo = cdfs_key[ids_right(q[i+1])] - cdfs_key[ids_left(q[i])]:
    max(w - wo, 0)^2 / (w + 1e-7) where w > 0, else 0.  The query side is detached; differentiable w.r.t. `cdfs_key`."""
    q = segments_query.vals if isinstance(segments_query, RayIntervals) else segments_query
    k = segments_key.vals if isinstance(segments_key, RayIntervals) else segments_key
    return _PdfLossFn.apply(ops._gpu_f32(cdfs_key, "cdfs_key"), q.detach(), cdfs_query.detach(), k.detach())


def prop_sigma_fn(model: NeRF, rays_o: Tensor, rays_d: Tensor) -> Callable[[Tensor, Tensor], Tensor]:
    """-> `(t_starts, t_ends) -> sigmas`, each [n_rays, n_samples], of this package's NeRF at the interval midpoints on
    these rays (NeRF.forward_rays: gathers and midpoints inside the launch).  Without gradients it is the density-only
    pass; with them (grad enabled, the model training) the sigma column of the full training pair, because the
    density-only pass has no backward.  Sigma is clamped at 0 either way: that keeps the cdfs monotone (up to the rounding of the transmittance walk)."""
    rows = {}

    def fn(t_starts: Tensor, t_ends: Tensor) -> Tensor:
        R, S = t_starts.shape
        if (R, S) not in rows:
            rows[(R, S)] = torch.arange(R, device=rays_o.device).repeat_interleave(S)
        t0, t1 = t_starts.reshape(-1).contiguous(), t_ends.reshape(-1).contiguous()
        if torch.is_grad_enabled() and model._differentiable():
            sig = model.forward_rays(rays_o, rays_d, rows[(R, S)], t0, t1, full=True)[..., -1]
        else:
            with torch.no_grad():
                sig = model.forward_rays(rays_o, rays_d, rows[(R, S)], t0, t1, full=False).squeeze(-1)
        return sig.clamp_min(0.0).reshape(R, S)

    return fn


class PropNetEstimator(nn.Module):
    """Proposal-network transmittance estimator (module docstring).  `optimizer` / `scheduler` are the PROPOSAL
    networks' own; `prop_models`, `prop_samples`, `num_samples`, `near_plane`, `far_plane` and `sampling_type` are what
    `render_rays` calls `sampling` with when this estimator sits in its estimator slot (the "propnet" route).
    `proposal_requires_grad`: a plain bool the training loop may schedule - whether a training call through the route
    keeps the proposals' graph for `update_every_n_steps` (nerfacc's examples switch it on for a share of the steps)."""

    def __init__(self, optimizer: Optional[torch.optim.Optimizer] = None, scheduler=None, *,
                 prop_models: Sequence[nn.Module] = (), prop_samples: Sequence[int] = (), num_samples: int = 64,
                 near_plane: Optional[float] = None, far_plane: Optional[float] = None,
                 sampling_type: str = "lindisp") -> None:
        super().__init__()
        if len(prop_models) != len(prop_samples):
            raise ValueError("PropNetEstimator: prop_models and prop_samples must have the same length")
        if sampling_type not in ("uniform", "lindisp"):
            raise ValueError(f"sampling_type: expected 'uniform' or 'lindisp', got {sampling_type!r}")
        self.optimizer, self.scheduler = optimizer, scheduler
        self.prop_models = nn.ModuleList(prop_models)
        self.prop_samples, self.num_samples = tuple(int(n) for n in prop_samples), int(num_samples)
        self.near_plane, self.far_plane, self.sampling_type = near_plane, far_plane, sampling_type
        self.proposal_requires_grad = True
        self.prop_cache: List[Tuple[RayIntervals, Optional[Tensor]]] = []

    def sampling(self, prop_sigma_fns: Sequence[Callable], prop_samples: Sequence[int], num_samples: int, n_rays: int,
                 near_plane: float, far_plane: float, sampling_type: str = "lindisp", stratified: bool = False,
                 requires_grad: bool = False, *, u: Optional[Sequence[Tensor]] = None,
                 device: Optional[torch.device] = None) -> Tuple[Tensor, Tensor]:
        """-> (t_starts, t_ends), each [n_rays, num_samples].  From vals = cdfs = [0, 1], per level: importance-sample
        `prop_samples[l]` intervals, transform them to [near_plane, far_plane], sigmas = prop_sigma_fns[l](t_starts,
        t_ends) [n_rays, n], cdfs = 1 - cat(trans, 0); one more importance sample of `num_samples` intervals ends it.
        Without `requires_grad` every level after the first is one launch (fsn_prop_resample).  With it the cdfs come
        from the differentiable render_transmittance_from_density, the sampler runs on their detached values, and
        (intervals, cdfs) is pushed on `prop_cache` for `compute_loss`.  `stratified`: one uniform jitter per ray and
        level; `u`: those jitters, len(prop_samples) + 1 tensors [n_rays] (tests)."""
        if len(prop_sigma_fns) != len(prop_samples):
            raise ValueError("sampling: prop_sigma_fns and prop_samples must have the same length")
        if sampling_type not in ("uniform", "lindisp"):
            raise ValueError(f"sampling_type: expected 'uniform' or 'lindisp', got {sampling_type!r}")
        counts = [int(n) for n in prop_samples] + [int(num_samples)]
        if u is not None and len(u) != len(counts):
            raise ValueError(f"u: expected {len(counts)} per-level jitters [n_rays], got {len(u)}")
        R = int(n_rays)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("PropNetEstimator.sampling: expected a GPU device (the HIP path has no CPU fallback)")
        near, far = float(near_plane), float(far_plane)

        def jitter(level: int) -> Optional[Tensor]:
            if u is not None:
                return u[level]
            return torch.rand(R, device=dev) if stratified else None

        unit = torch.tensor([0.0, 1.0], device=dev).expand(R, 2).contiguous()
        with torch.no_grad():
            s, _, t = ops.importance_sample(unit, unit, counts[0], jitter(0), sampling_type, near, far, want_centres=False)
        for level, fn in enumerate(prop_sigma_fns):
            t_starts, t_ends = t[:, :-1], t[:, 1:]
            with torch.set_grad_enabled(bool(requires_grad)):
                sigmas = fn(t_starts, t_ends)
            assert sigmas.shape == t_starts.shape, "sigmas must have shape {}! Got {}".format(tuple(t_starts.shape), tuple(sigmas.shape))
            n_next, b = counts[level + 1], jitter(level + 1)
            if requires_grad:
                trans, _ = volrend.render_transmittance_from_density(t_starts, t_ends, sigmas)
                cdfs = 1.0 - torch.cat([trans, torch.zeros_like(trans[:, :1])], dim=-1)
                self.prop_cache.append((RayIntervals(vals=s), cdfs))
                with torch.no_grad():
                    s, _, t = ops.importance_sample(s, cdfs.detach(), n_next, b, sampling_type, near, far, want_centres=False)
            else:
                with torch.no_grad():  # (one launch: 0.018 ms against 0.087 ms for the composed primitives)
                    _, s, _, t = ops.prop_resample(s, t, sigmas.detach(), n_next, b, sampling_type, near, far)
        if requires_grad:
            self.prop_cache.append((RayIntervals(vals=s), None))
        return t[:, :-1], t[:, 1:]

    def compute_loss(self, trans: Tensor, loss_scaler: float = 1.0) -> Tensor:
        """The interlevel loss of the cached proposal levels against the final network's transmittance `trans`
        [n_rays, num_samples] (detached here): for every cached level the mean of `_pdf_loss`, summed, times
        `loss_scaler`.  Empties the cache.  An empty cache gives 0."""
        if len(self.prop_cache) == 0:
            return torch.zeros((), device=trans.device)
        intervals, _ = self.prop_cache.pop()
        trans = trans.detach().reshape(intervals.vals.shape[0], -1)
        cdfs = 1.0 - torch.cat([trans, torch.zeros_like(trans[:, :1])], dim=-1)
        loss = torch.zeros((), device=trans.device)
        while self.prop_cache:
            prop_intervals, prop_cdfs = self.prop_cache.pop()
            loss = loss + _pdf_loss(intervals, cdfs, prop_intervals, prop_cdfs).mean()
        return loss * loss_scaler

    def update_every_n_steps(self, trans: Tensor, requires_grad: bool = False, loss_scaler: float = 1.0) -> float:
        """After the main step: with `requires_grad` (the step's `sampling` ran with it) the proposals' own step -
        compute_loss, backward, optimizer.step(), scheduler.step() - and the loss as a float (one host read); without,
        only the scheduler steps and 0 is returned.  An empty cache returns 0 as well."""
        if requires_grad and len(self.prop_cache) > 0:
            assert self.optimizer is not None, "No optimizer is provided."
            loss = self.compute_loss(trans, loss_scaler)
            self.optimizer.zero_grad()
            if loss.requires_grad:  # (no proposal level, or proposals that carry no graph: nothing to step on)
                loss.backward()
                self.optimizer.step()
            if self.scheduler is not None:
                self.scheduler.step()
            return float(loss.detach())
        self.prop_cache.clear()
        if self.scheduler is not None:
            self.scheduler.step()
        return 0.0
