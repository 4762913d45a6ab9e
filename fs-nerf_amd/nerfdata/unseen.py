"""Unseen views (this package's own, after RegNeRF's pose sampling): a distribution of camera poses
fitted to the training cameras, and a loader whose next() is ONE launch from a step counter to B patches of P x P rays
of freshly drawn poses - the rays that core.loss.PatchDepthSmoothnessLoss, RayEntropyLoss and DistortionLoss are put on
where no photograph was taken.  Everything served is a pure function of (distribution, seed, step): no host RNG, no
state on the device, bit for bit reproducible and resumable.  There is no CPU implementation."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import _lib as L
from .. import ops
from .raydata import _NDC_NEAR, _seed_or_default

_MODES = {"shell": L.FSN_UNSEEN_SHELL, "box": L.FSN_UNSEEN_BOX}
_Z_LIMIT = 0.999  # from_poses keeps the shell's heights inside (-1, 1): at |z| = 1 the camera looks along `up`


def _vec3(v, name: str) -> np.ndarray:
    a = np.asarray(v.detach().cpu() if isinstance(v, Tensor) else v, dtype=np.float64).reshape(-1)
    if a.shape != (3,) or not np.all(np.isfinite(a)):
        raise ValueError(f"UnseenViewSampler: {name} must be three finite numbers, got {v!r}")
    return a


def _unit(v: np.ndarray, name: str) -> np.ndarray:
    n = float(np.linalg.norm(v))
    if not n > 1e-12:
        raise ValueError(f"UnseenViewSampler: {name} has no direction")
    return v / n


def _frame(up: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(e1, e2) completing the unit vector `up` to a right-handed orthonormal frame (e1, e2, up): e1 is the world axis
    least aligned with `up`, made orthogonal to it."""
    axis = np.zeros(3)
    axis[int(np.argmin(np.abs(up)))] = 1.0
    e1 = _unit(axis - float(axis @ up) * up, "e1")
    return e1, np.cross(up, e1)


class UnseenViewSampler:
    """A distribution of camera poses (camera-to-world, looking down the camera's own -z with y up, as get_rays reads
    them); include/fsnerf_hip.h has the arithmetic of a draw, tests/unseen_ref.py restates it in NumPy.

    mode "shell" (360-degree captures): the origin lies on a spherical shell around `centre`, height z = sin(elevation)
    uniform in [z_lo, z_hi] (area-uniform), azimuth uniform, radius uniform in [r_lo, r_hi]; -1 < z_lo <= z_hi < 1.
    mode "box" (forward-facing captures): the origin is uniform in the box [lo, hi].
    Both: the camera looks at a target uniform in the cube focus +- jitter, with `up` up.

    The plain constructor takes the numbers; from_poses() fits them to training cameras.  poses() draws."""

    def __init__(self, mode: str, *, focus: Sequence[float], up: Sequence[float], jitter: float = 0.0,
                 centre: Optional[Sequence[float]] = None, r: Optional[Sequence[float]] = None,
                 z: Optional[Sequence[float]] = None, lo: Optional[Sequence[float]] = None,
                 hi: Optional[Sequence[float]] = None, device=torch.device("cuda")):
        if mode not in _MODES:
            raise ValueError(f"UnseenViewSampler: mode {mode!r} is not 'shell' or 'box'")
        if not (np.isfinite(jitter) and jitter >= 0.0):
            raise ValueError(f"UnseenViewSampler: jitter {jitter} must be finite and not negative")
        self.mode, self.device = mode, torch.device(device)
        d = L.UnseenDist()
        d.mode, d.jitter = _MODES[mode], float(jitter)
        up_ = _unit(_vec3(up, "up"), "up")
        e1, e2 = _frame(up_)
        fields = {"focus": _vec3(focus, "focus"), "up": up_, "e1": e1, "e2": e2}
        if mode == "shell":
            if r is None or z is None:
                raise ValueError("UnseenViewSampler: a shell needs r=(r_lo, r_hi) and z=(z_lo, z_hi)")
            fields["centre"] = fields["focus"] if centre is None else _vec3(centre, "centre")
            # the ranges as the kernel reads them: float32
            d.r_lo, d.r_hi, d.z_lo, d.z_hi = float(r[0]), float(r[1]), float(z[0]), float(z[1])
            if not 0.0 <= d.r_lo <= d.r_hi < float("inf"):
                raise ValueError(f"UnseenViewSampler: bad radius range {tuple(r)} (0 <= r_lo <= r_hi)")
            if not -1.0 < d.z_lo <= d.z_hi < 1.0:
                raise ValueError(f"UnseenViewSampler: bad height range {tuple(z)} (-1 < z_lo <= z_hi < 1: at |z| = 1 the "
                                 "camera looks along `up`)")
        else:
            if lo is None or hi is None:
                raise ValueError("UnseenViewSampler: a box needs lo and hi")
            fields["lo"], fields["hi"] = _vec3(lo, "lo"), _vec3(hi, "hi")
            if not np.all(fields["lo"] <= fields["hi"]):
                raise ValueError(f"UnseenViewSampler: bad box {lo} .. {hi} (lo <= hi)")
        for name, v in fields.items():
            for k in range(3):
                getattr(d, name)[k] = float(v[k])
        self.dist = d

    @classmethod
    def from_poses(cls, poses, mode: str, *, margin: float = 0.1, jitter: float = 0.1, focus: Optional[Sequence[float]] = None,
                   device=torch.device("cuda")) -> "UnseenViewSampler":
        """Fit the distribution to the training cameras `poses` [n, 3|4, 4] (host, float64, once):
          focus   the least-squares point closest to the optical axes (or the `focus` given: parallel axes have none);
          up      the normalised mean of the camera y axes;
          shell   centre = focus; [r_lo, r_hi] = the cameras' distances to it, [r_min (1 - margin), r_max (1 + margin)];
                  [z_lo, z_hi] = their heights (offset . up / distance) -+ margin, kept inside +-0.999;
          box     the bounding box of the camera centres, each side widened by margin x its extent;
          jitter  x the mean camera distance to the focus = the half side of the target cube."""
        P = np.asarray(poses.detach().cpu() if isinstance(poses, Tensor) else poses, dtype=np.float64)
        if P.ndim != 3 or P.shape[0] < 1 or P.shape[1] not in (3, 4) or P.shape[2] != 4:
            raise ValueError(f"UnseenViewSampler.from_poses: poses {P.shape} are not [n, 3 or 4, 4]")
        if mode not in _MODES:
            raise ValueError(f"UnseenViewSampler: mode {mode!r} is not 'shell' or 'box'")
        if not (margin >= 0.0 and jitter >= 0.0):
            raise ValueError("UnseenViewSampler.from_poses: margin and jitter must not be negative")
        c, axis = P[:, :3, 3], -P[:, :3, 2]
        axis = axis / np.linalg.norm(axis, axis=1, keepdims=True)
        if focus is None:
            # sum_i (I - a_i a_i^T) x = sum_i (I - a_i a_i^T) c_i
            M = np.eye(3)[None] - axis[:, :, None] * axis[:, None, :]
            A, b = M.sum(0), np.einsum("nij,nj->i", M, c)
            if np.linalg.cond(A) > 1e8:
                raise ValueError("UnseenViewSampler.from_poses: the optical axes are parallel (or there is one camera), no "
                                 "point is closest to them: pass focus=")
            f = np.linalg.solve(A, b)
        else:
            f = _vec3(focus, "focus")
        up = _unit(P[:, :3, 1].mean(0), "the mean of the camera y axes")
        off = c - f
        dist = np.linalg.norm(off, axis=1)
        kw = dict(focus=f, up=up, jitter=float(jitter) * float(dist.mean()), device=device)
        if mode == "shell":
            if not dist.min() > 0.0:
                raise ValueError("UnseenViewSampler.from_poses: a camera sits on the focus")
            z = (off @ up) / dist
            return cls("shell", r=(dist.min() * (1.0 - min(margin, 1.0)), dist.max() * (1.0 + margin)),
                       z=(max(z.min() - margin, -_Z_LIMIT), min(z.max() + margin, _Z_LIMIT)), **kw)
        ext = c.max(0) - c.min(0)
        return cls("box", lo=c.min(0) - margin * ext, hi=c.max(0) + margin * ext, **kw)

    def poses12(self, count: int, *, seed: int, first: int = 0) -> Tensor:
        """Pose draws [first, first + count) as [count,12] on the device (ONE launch, ops.unseen_poses)."""
        return ops.unseen_poses(self.dist, count, self.device, seed=seed, first=first)

    def poses(self, count: int, *, seed: int, first: int = 0) -> Tensor:
        """... as [count,4,4] on the device, for render_frame / render_path / mark_invisible_from_views."""
        p = self.poses12(count, seed=seed, first=first).view(-1, 3, 4)
        return torch.cat([p, p.new_tensor([0.0, 0.0, 0.0, 1.0]).expand(p.shape[0], 1, 4)], dim=1)


class UnseenPatchLoader:
    """An endless iterator (no epochs) over patches of unseen views: every next() is ONE launch (ops.unseen_patch_batch),
    no host synchronisation, returning (rays_o, rays_d) of [B * patch^2, 3] (+ poses12 [B,12] with `with_poses`) for
    B = patches_per_batch patches of patch x patch rays `dilation` pixels apart, patch after patch, row-major inside a
    patch, so depth.view(B, patch, patch) is the stack PatchDepthSmoothnessLoss takes.  `patches_per_pose` consecutive
    patches share one pose draw; B must be a multiple of it, so a pose never straddles two batches or ranks.

    Step s of rank r serves the global patches [(s * world + r) * B, +B): the ranks of a step are disjoint and together
    the batch of a world=1 loader of B * world patches.  state_dict() = (seed, step); after load_state_dict() the very
    same batches follow.  hwf = (H, W, focal); ndc: the rays are mapped to NDC with near = 1, as the datasets do."""

    def __init__(self, sampler: UnseenViewSampler, hwf: Tuple[int, int, float], patch: int, patches_per_batch: int,
                 dilation: int = 1, patches_per_pose: int = 1, ndc: bool = False, seed: Optional[int] = None, rank: int = 0,
                 world: int = 1, with_poses: bool = False):
        H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
        patch, dilation, B, per_pose = int(patch), int(dilation), int(patches_per_batch), int(patches_per_pose)
        if B <= 0 or world <= 0 or not 0 <= rank < world:
            raise ValueError(f"UnseenPatchLoader: bad patches_per_batch {B}, rank {rank} or world {world}")
        if patch < 1 or dilation < 1 or H < 1 or W < 1 or not focal > 0.0:
            raise ValueError(f"UnseenPatchLoader: bad patch {patch}, dilation {dilation} or hwf {hwf}")
        ext = (patch - 1) * dilation + 1
        if ext > H or ext > W:
            raise ValueError(f"UnseenPatchLoader: a patch of {patch} pixels at dilation {dilation} spans {ext} pixels and "
                             f"does not fit the {H} x {W} image")
        if per_pose < 1 or B % per_pose != 0:
            raise ValueError(f"UnseenPatchLoader: patches_per_batch {B} is not a multiple of patches_per_pose {per_pose} "
                             "(a pose would straddle two batches)")
        self.sampler, self.hwf, self.patch, self.dilation = sampler, (H, W, focal), patch, dilation
        self.batch_size, self.patches_per_pose, self.ndc = B, per_pose, bool(ndc)
        self.seed = _seed_or_default(seed)
        self.rank, self.world, self.with_poses = int(rank), int(world), bool(with_poses)
        self.step = 0  # batches served

    def __iter__(self) -> "UnseenPatchLoader":
        return self

    def __next__(self):
        H, W, focal = self.hwf
        o, d, poses, _ = ops.unseen_patch_batch(
            self.sampler.dist, H, W, focal, self.patch, self.dilation, device=self.sampler.device,
            first_patch=(self.step * self.world + self.rank) * self.batch_size, count=self.batch_size,
            patches_per_pose=self.patches_per_pose, seed=self.seed, ndc=self.ndc, near=_NDC_NEAR, want_poses=self.with_poses)
        self.step += 1
        return (o, d, poses) if self.with_poses else (o, d)

    next = __next__

    def state_dict(self) -> dict:
        return {"seed": self.seed, "step": self.step}

    def load_state_dict(self, state: dict) -> None:
        self.seed, self.step = int(state["seed"]), int(state["step"])
