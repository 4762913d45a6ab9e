"""Occupancy-grid estimator for the `estimator` slot of render_rays: the duck-typed interface
the reference uses from nerfacc's OccGridEstimator — construction `OccGridEstimator(roi_aabb=, resolution=, levels=)`
(src/run-nerf.py:96-98), `.sampling(rays_o, rays_d, sigma_fn=, render_step_size=, stratified=, near_plane=,
far_plane=)` (src/render/rendering.py:66-74; nerfacc's `t_min=`, `t_max=`, `cone_angle=` and its `ray_aabb_intersect`
helper as well), `.update_every_n_steps(step=, occ_eval_fn=, occ_thre=)`
(src/run-nerf.py:293-295), nn.Module modes / `.to()`.  nerfacc itself is not part of the reference; the sampling
rule is this build's definition of that contract (see csrc/occgrid.hip), on HIP kernels."""
import math
from typing import Callable, Optional, Sequence

import torch
from torch import Tensor, nn

from .. import ops
from ..core.models import OccEvalFn


def ray_aabb_intersect(rays_o: Tensor, rays_d: Tensor, aabbs, near_plane: float = -math.inf, far_plane: float = math.inf,
                       miss_value: float = math.inf):
    """nerfacc's helper of the same name: rays [R,3] against boxes [M,6] {xmin, ymin, zmin, xmax, ymax, zmax} ->
    (t_mins [R,M], t_maxs [R,M], hits bool [R,M]), with the march's own slab test - so `t_min` / `t_max` taken from the
    grid's outermost box change nothing.  A miss holds `miss_value` twice."""
    return ops.ray_aabb_intersect(rays_o, rays_d, aabbs, near_plane, far_plane, miss_value)


class OccGridEstimator(nn.Module):
    def __init__(self, roi_aabb, resolution: int = 128, levels: int = 1) -> None:
        super().__init__()
        aabb = [float(v) for v in (roi_aabb.tolist() if isinstance(roi_aabb, Tensor) else roi_aabb)]
        if len(aabb) != 6:
            raise ValueError("roi_aabb must hold 6 values {xmin, ymin, zmin, xmax, ymax, zmax}")
        self.aabb, self.resolution, self.levels = aabb, int(resolution), int(levels)
        n_cells = self.levels * self.resolution ** 3
        if n_cells % 64:
            raise ValueError("levels * resolution^3 must be a multiple of 64")
        self.register_buffer("occs", torch.zeros(n_cells, dtype=torch.float32))
        self.register_buffer("bits", torch.zeros(n_cells // 32, dtype=torch.int32))
        self.generator: Optional[torch.Generator] = None
        self._updates = 0      # update_every_n_steps calls that ran (part of the draws' seed; in the state_dict)
        self._pending = None   # scratch of the duplicate-safe EMA / the selection's popcount prefix (device)
        self._prefix = None
        self._prefix_levels = None  # ... of all levels at once (the fused refresh)
        self._mask_scratch = None   # partial sums of the masked end of an update (a marked estimator only)

    # -- state ---------------------------------------------------------------------
    # The update count is part of the draws' seed (update_seed): the state_dict carries it, so that a resumed run continues
    # the sequence of draws instead of replaying the first ones.  A state_dict saved before it did loads with the count 0.
    def get_extra_state(self) -> Tensor:
        return torch.tensor(self._updates, dtype=torch.int64)

    def set_extra_state(self, state) -> None:
        self._updates = int(state)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        state_dict.setdefault(prefix + "_extra_state", 0)  # (load_state_dict hands each module its own copy)
        # the visibility mask exists from the first mark_invisible_* call on: a marked state registers it here, a
        # state without it (saved unmarked, or before the mask existed) loads as all-visible
        if prefix + "vis_bits" in state_dict:
            if not self.marked:
                self.register_buffer("vis_bits", torch.zeros_like(self.bits))
        elif self.marked:
            del self._buffers["vis_bits"]
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    # -- helpers -------------------------------------------------------------------
    @property
    def binaries(self) -> Tensor:
        """[levels, res, res, res] bool view of the bit field (nerfacc's attribute of the same name)."""
        shifts = torch.arange(32, device=self.bits.device, dtype=torch.int32)
        b = ((self.bits[:, None] >> shifts[None, :]) & 1).bool()
        return b.reshape(self.levels, self.resolution, self.resolution, self.resolution)

    def set_binaries(self, binaries: Tensor) -> None:
        """Load an explicit occupancy ([levels, res, res, res] bool); occs become 1 / 0 (on a marked estimator -1 at
        the invisible cells, which stay off)."""
        flat = binaries.reshape(-1).to(self.occs.device)
        self.occs.copy_(flat.float())
        if self.marked:
            self._finish_masked(0.5)
            return
        thr = torch.full((1,), 0.5, device=self.occs.device)
        ops.occgrid_update(self.occs, self.bits, None, None, 1.0, thr)

    # -- cells no training camera sees ---------------------------------------------
    @property
    def marked(self) -> bool:
        """mark_invisible_cells / mark_invisible_from_views has run (or a marked state_dict was loaded)."""
        return "vis_bits" in self._buffers

    @property
    def visible(self) -> Tensor:
        """[levels, res, res, res] bool view of the visibility mask, like `binaries`; all True when never marked."""
        shape = (self.levels, self.resolution, self.resolution, self.resolution)
        if not self.marked:
            return torch.ones(shape, dtype=torch.bool, device=self.bits.device)
        shifts = torch.arange(32, device=self.bits.device, dtype=torch.int32)
        return ((self.vis_bits[:, None] >> shifts[None, :]) & 1).bool().reshape(shape)

    def _finish_masked(self, occ_thre: float, revive: bool = False) -> None:
        """The end of an update on a marked estimator: occs = -1 at the invisible cells, bits = (occs > min(mean over the
        visible cells, occ_thre)) & visible - two launches, no host sync (fsn_occgrid_update_masked)."""
        if self._mask_scratch is None or self._mask_scratch.device != self.occs.device:
            self._mask_scratch = torch.empty(2048, dtype=torch.float64, device=self.occs.device)
        ops.occgrid_update_masked(self.occs, self.bits, self.vis_bits, occ_thre, self._mask_scratch, revive=revive)

    def _mark(self, w2c: Tensor, fx, fy, cx, cy, width: int, height: int, near_plane: float, min_views: int, ndc) -> None:
        """cameras (world -> camera [N,3,4] in the kernel's convention, float64, any device) -> the mask; replaces an
        earlier one."""
        dev = self.occs.device
        N = w2c.shape[0]
        intr = torch.stack([torch.as_tensor(v, dtype=torch.float64, device=w2c.device).expand(N) for v in (fx, fy, cx, cy)], 1)
        cams = torch.cat([w2c.reshape(N, 12), intr], 1).to(torch.float32).contiguous().to(dev)
        vis = torch.empty_like(self.bits)
        ops.occgrid_visibility(self.aabb, self.resolution, self.levels, cams, int(width), int(height), float(near_plane),
                               int(min_views), vis, ndc=ndc)
        if self.marked:
            self.vis_bits.copy_(vis)
        else:
            self.register_buffer("vis_bits", vis)
        self.bits &= self.vis_bits
        if self._mask_scratch is None or self._mask_scratch.device != dev:
            self._mask_scratch = torch.empty(2048, dtype=torch.float64, device=dev)
        ops.occgrid_update_masked(self.occs, None, self.vis_bits, 0.0, self._mask_scratch, revive=True)  # (occs only)

    def _check_mark(self, poses: Tensor, width: int, height: int, near_plane: float, min_views: int) -> None:
        """The argument checks of both mark_invisible_* calls: they run before any launch."""
        if self.occs.device.type != "cuda":
            raise RuntimeError("mark_invisible_cells: the estimator must be on the GPU (there is no CPU path)")
        if int(min_views) < 1:
            raise ValueError("min_views must be at least 1")
        if not float(near_plane) >= 0.0:
            raise ValueError("near_plane must not be negative")
        if int(width) <= 0 or int(height) <= 0:
            raise ValueError("the image size must be positive")
        if poses.dim() != 3 or poses.shape[0] < 1 or poses.shape[1] not in (3, 4) or poses.shape[2] != 4:
            raise ValueError("camera poses must be [N,3,4] or [N,4,4], N >= 1")

    @staticmethod
    def _world_to_camera(c2w: Tensor) -> Tensor:
        """[N,3,4] / [N,4,4] camera -> world (rigid) -> float64 world -> camera [N,3,4]: [R^T | -R^T t]."""
        c2w = c2w.detach().to(torch.float64)
        Rt, t = c2w[:, :3, :3].transpose(1, 2), c2w[:, :3, 3]
        # (written out, not a matmul: tests/occ_invisible_ref.py forms the same table with the same roundings)
        tt = -((Rt[:, :, 0] * t[:, None, 0] + Rt[:, :, 1] * t[:, None, 1]) + Rt[:, :, 2] * t[:, None, 2])
        return torch.cat([Rt, tt[:, :, None]], 2)

    @torch.no_grad()
    def mark_invisible_cells(self, K: Tensor, c2w: Tensor, width: int, height: int, near_plane: float = 0.0,
                             chunk: Optional[int] = None, *, min_views: int = 1) -> None:
        """nerfacc's call of the same name: take every cell that fewer than `min_views` of the cameras cover, or that is
        nearer than `near_plane` to one, out of the grid for good (occs = -1, nerfacc's convention; later updates keep
        it off).  K [3,3] or [N,3,3], c2w [N,3,4] or [N,4,4], OpenCV convention (x right, y down, z forward); a pixel
        is in the image iff 0 <= u < width, 0 <= v < height.  Unlike nerfacc's one-point test the rule is a conservative
        frustum / box test (include/fsnerf_hip.h at fsn_occgrid_visibility): no cell a frustum meets is removed.
        `near_plane` is a depth along the optical axis.  `chunk` is accepted and ignored; a second call replaces the
        mask.  No host synchronisation beyond moving the camera table to the device."""
        K, c2w = torch.as_tensor(K), torch.as_tensor(c2w)
        self._check_mark(c2w, width, height, near_plane, min_views)
        if K.dim() == 2:
            K = K[None].expand(c2w.shape[0], *K.shape)
        if K.dim() != 3 or K.shape[1:] != (3, 3) or K.shape[0] != c2w.shape[0]:
            raise ValueError("K must be [3,3] or [N,3,3] with one matrix per pose")
        w2c = self._world_to_camera(c2w)
        K = K.detach().to(device=w2c.device, dtype=torch.float64)
        self._mark(w2c, K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], width, height, near_plane, min_views, None)

    @torch.no_grad()
    def mark_invisible_from_views(self, poses: Tensor, hwf, near_plane: float = 0.0, *, ndc: bool = False,
                                  min_views: int = 1) -> None:
        """mark_invisible_cells for the reference's cameras: `get_rays` poses (x right, y up, looking down -z) and
        (H, W, focal), as RayDataset.poses / .hwf / .ndc hold them.  The ray of pixel i passes u = i, so its footprint
        is [i - 1/2, i + 1/2]: the principal point moves to W/2 + 1/2, H/2 + 1/2 and the frustum 0 <= u' < W is the union
        of the pixel footprints.  ndc: the grid lives in the NDC space of to_ndc with near = 1 (the LLFF path)."""
        H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
        poses = torch.as_tensor(poses)
        self._check_mark(poses, W, H, near_plane, min_views)
        if not focal > 0.0:
            raise ValueError("the focal length must be positive")
        flip = torch.tensor([1.0, -1.0, -1.0, 1.0], dtype=torch.float64, device=poses.device)
        w2c = self._world_to_camera(poses.detach().to(torch.float64)[:, :3, :] * flip)
        self._mark(w2c, focal, focal, W / 2.0 + 0.5, H / 2.0 + 0.5, W, H, near_plane, min_views,
                   (W / (2.0 * focal), H / (2.0 * focal), 1.0) if ndc else None)

    def level_aabb(self, lvl: int):
        c = [(self.aabb[a] + self.aabb[3 + a]) / 2.0 for a in range(3)]
        h = [(self.aabb[3 + a] - self.aabb[a]) / 2.0 * 2 ** lvl for a in range(3)]
        return [c[a] - h[a] for a in range(3)], [c[a] + h[a] for a in range(3)]

    def max_steps(self, render_step_size: float, cone_angle: float = 0.0, near_plane: float = 0.0) -> int:
        """Lattice points a ray can have inside the outermost box (its diagonal / step, + 2).  With a `cone_angle` the
        step grows with distance: the count is the block recurrence of the cone march (64 intervals of width
        max(t cone_angle, step) per block) run from `near_plane` over the diagonal - a ray that enters later only takes
        larger steps, so it needs no more blocks for the same length."""
        lo, hi = self.level_aabb(self.levels - 1)
        diag = math.sqrt(sum((hi[a] - lo[a]) ** 2 for a in range(3)))
        if cone_angle == 0.0:
            return int(min(16384, math.ceil(diag / render_step_size) + 2))
        t, n = float(near_plane), 0
        while t < near_plane + diag and n < 16384:
            t += 64.0 * max(t * cone_angle, render_step_size)
            n += 64
        return n

    # -- reference surface ---------------------------------------------------------
    @torch.no_grad()
    def sampling(self, rays_o: Tensor, rays_d: Tensor, sigma_fn: Optional[Callable] = None,
                 alpha_fn: Optional[Callable] = None, near_plane: float = 0.0, far_plane: float = 1e10,
                 t_min: Optional[Tensor] = None, t_max: Optional[Tensor] = None, render_step_size: float = 1e-3,
                 early_stop_eps: float = 1e-4, alpha_thre: float = 0.0, stratified: bool = False,
                 cone_angle: float = 0.0, u: Optional[Tensor] = None):
        """-> (ray_indices int64 [N], t_starts [N], t_ends [N]), packed and sorted by ray.
        `t_min` / `t_max` [n_rays] tighten each ray's range (e.g. from `ray_aabb_intersect`); `cone_angle` > 0 lets the
        step grow with distance, dt = max(t cone_angle, render_step_size) (needs near_plane >= 0; the definition is in
        include/fsnerf_hip.h at fsn_occgrid_march_ex).  `alpha_fn` is out of scope."""
        if alpha_fn is not None:
            raise NotImplementedError("alpha_fn is not supported: pass sigma_fn (DESIGN.md 9)")
        if cone_angle < 0.0 or (cone_angle > 0.0 and near_plane < 0.0):
            raise ValueError("cone_angle must not be negative, and a cone_angle > 0 needs near_plane >= 0")
        R = rays_o.shape[0]
        if u is None and stratified:
            u = torch.rand(R, device=rays_o.device, generator=self.generator)
        max_steps = self.max_steps(render_step_size, cone_angle, near_plane)
        ri, t0, t1, _ = ops.occgrid_march(rays_o, rays_d, self.aabb, self.resolution, self.levels, self.bits, near_plane,
                                          far_plane, render_step_size, u, max_steps, t_min=t_min, t_max=t_max,
                                          cone_angle=cone_angle)
        if sigma_fn is not None and (early_stop_eps > 0.0 or alpha_thre > 0.0) and ri.numel() > 0:
            sig = sigma_fn(t0, t1, ri)
            keep = ops.packed_visibility(sig.reshape(-1), t0, t1, ri, R, early_stop_eps, alpha_thre)
            ri, t0, t1 = ri[keep], t0[keep], t1[keep]
        return ri, t0, t1

    @torch.no_grad()
    def update_every_n_steps(self, step: int, occ_eval_fn: Callable, occ_thre: float = 1e-2, ema_decay: float = 0.95,
                             warmup_steps: int = 256, n: int = 16) -> None:
        """Every n-th training step (run-nerf.py:288-295): re-evaluate cells - all of them during warm-up, else per level
        res^3/4 drawn uniformly with replacement + res^3/4 from the occupied ones - at a random point inside each,
        occs = max(occs*decay, occ), binaries = occs > min(mean, thre).  The occupied half follows nerfacc's rule: a
        level with at most res^3/4 occupied cells re-evaluates each of them exactly once (its other draws are unused:
        cell -1, skipped by the EMA, though occ_eval_fn still sees a point for them, so its batch size is fixed); only a
        denser level draws res^3/4 of them with replacement.
        An `OccEvalFn` (`NeRF.occ_eval_fn(step, precision)`) in the slot is not called: selection, its density pass in
        that single-pass mode, `* step` and the maximum per cell run in ONE launch for all levels (`_refresh_fused`) -
        same draws, same schedule, same values as calling it level by level, bit for bit.
        Round 4: selection, jitter and the duplicate-safe EMA are kernels reading the bit field directly
        (fsn_occgrid_select / fsn_occgrid_update_multi); no host sync, no bool expansion of the grid.  Randomness is a
        counter-based hash of (seed, draw): seed = the estimator generator's (or torch's) initial seed and the number of
        updates made so far - `oracle.occgrid_select` restates it."""
        if not self.training or step % n != 0:
            return
        res, res3 = self.resolution, self.resolution ** 3
        if self._pending is None or self._pending.device != self.occs.device:
            self._pending = torch.zeros(self.occs.numel(), dtype=torch.int32, device=self.occs.device)
            self._prefix = torch.empty(res3 // 32 + 1, dtype=torch.int32, device=self.occs.device)
        warm = step < warmup_steps
        if isinstance(occ_eval_fn, OccEvalFn):
            self._refresh_fused(occ_eval_fn, warm, ema_decay)
        else:
            for lvl in range(self.levels):
                seed = self.update_seed(lvl)
                cells, x = ops.occgrid_select(self.bits, self.aabb, res, self.levels, lvl, warm, res3 // 4, res3 // 4, seed,
                                              self._prefix)
                occ = occ_eval_fn(x).reshape(-1).float()
                ops.occgrid_update_multi(self.occs, self._pending, cells, occ, ema_decay)
        self._updates += 1
        if self.marked:  # (the EMA wrote max(-0.95, occ) into the invisible cells: restored here)
            self._finish_masked(occ_thre)
            return
        thr = torch.clamp(self.occs.mean(), max=occ_thre).reshape(1)
        ops.occgrid_update(self.occs, self.bits, None, None, 1.0, thr)

    def _refresh_fused(self, fn: OccEvalFn, warm: bool, ema_decay: float) -> None:
        """The level loop of update_every_n_steps in one launch (fsn_occgrid_refresh) + one EMA pass.  fp16: the range
        word is read once (one host sync per refresh); a flagged refresh is undone (`pending` cleared - `occs` has not
        been touched yet) and repeated in bf16, and `fn` stays in bf16."""
        res, res3, dev = self.resolution, self.resolution ** 3, self.occs.device
        if self._prefix_levels is None or self._prefix_levels.device != dev:
            self._prefix_levels = torch.empty(self.levels * (res3 // 32 + 1), dtype=torch.int32, device=dev)
        seeds = [self.update_seed(lvl) for lvl in range(self.levels)]
        m = fn.model
        fn.guarded(dev, "OccGridEstimator.update_every_n_steps",
                   lambda pm: ops.occgrid_refresh(pm, self.bits, self.aabb, res, self.levels, warm, res3 // 4, res3 // 4, seeds,
                                                  fn.render_step_size, self._pending, self._prefix_levels,
                                                  m._mask(m.pos_mask, dev)),
                   undo=self._pending.zero_)
        ops.occgrid_apply_pending(self.occs, self._pending, ema_decay)

    def update_seed(self, lvl: int = 0) -> int:
        """64-bit seed of the NEXT update's draws at level `lvl` (see update_every_n_steps)."""
        base = self.generator.initial_seed() if self.generator is not None else torch.initial_seed()
        return (base * 0x9E3779B97F4A7C15 + self._updates * 0x100000001B3 + lvl * 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF
