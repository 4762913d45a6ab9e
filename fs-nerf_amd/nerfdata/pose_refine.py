"""Learnable camera poses behind the loaders (this package's own: the reference keeps its poses fixed).

View v carries a correction xi_v = (omega_v, tau_v) on top of its stored pose [R0_v | t0_v]:
R_v = exp([omega_v]x) R0_v (left-multiplied, world frame), t_v = t0_v + tau_v; |omega| < pi; xi = 0 is the stored pose
value for value.  The intrinsics are IntrinsicsRefiner's (intrinsics_refine.py).  CameraRefiner holds xi; RayLoader / PatchLoader(cameras=refiner) serve their
batches over its corrected poses (one fsn_pose_compose launch per change of xi) and hand rays_o / rays_d out of one
autograd Function whose backward is the single deterministic fsn_ray_pose_grad launch into xi.grad.  pose_error scores
refined poses against the truth up to the joint problem's gauge (a similarity transform)."""
from __future__ import annotations

import math
from typing import Tuple

import torch
from torch import Tensor, nn

from .. import ops
from .raydata import ParamCache, RayDataset


class CameraRefiner(nn.Module):
    """xi [n,6] = (omega, tau) per view, float32 on the device, zeros at the start, over the stored poses of a RayDataset
    (its device-resident poses12) or of `poses` ([n,3|4,4] or [n,12], moved to `device`).

    learn_rotation / learn_translation = False: that half of xi.grad is zeroed (it stays where it is).
    poses12(): the corrected [n,12] matrices the loaders launch over - recomputed, by one launch, only when xi changed.
    poses(): [n,4,4] on the device, detached, for render_frame / render_path / mark_invisible_from_views.
    In data-parallel runs xi.grad is an ordinary parameter gradient: the caller all-reduces it with the network's."""

    def __init__(self, dataset_or_poses, *, learn_rotation: bool = True, learn_translation: bool = True,
                 device=torch.device("cuda")):
        super().__init__()
        if isinstance(dataset_or_poses, RayDataset):
            p0 = dataset_or_poses.poses12.detach().clone()
        else:
            p = torch.as_tensor(dataset_or_poses).detach().to(torch.float32)
            if p.dim() == 3 and p.shape[1] in (3, 4) and p.shape[2] == 4:
                p = p[:, :3, :4].reshape(-1, 12)
            if p.dim() != 2 or p.shape[1] != 12:
                raise ValueError(f"CameraRefiner: poses {tuple(p.shape)} are not [n, 3 or 4, 4] or [n, 12]")
            p0 = p.contiguous().to(device).clone()
        if not p0.is_cuda:
            raise RuntimeError("CameraRefiner: the poses live on the GPU (the HIP path has no CPU fallback)")
        self.learn_rotation, self.learn_translation = bool(learn_rotation), bool(learn_translation)
        self.register_buffer("poses0", p0)
        self.xi = nn.Parameter(torch.zeros(p0.shape[0], 6, device=p0.device, dtype=torch.float32))
        self._composed = ParamCache()

    @property
    def n_views(self) -> int:
        return self.poses0.shape[0]

    def poses12(self) -> Tensor:
        return self._composed.get(self.xi, lambda: ops.pose_compose(self.poses0, self.xi))

    def poses(self) -> Tensor:
        m = self.poses12().view(-1, 3, 4)
        last = torch.tensor([0.0, 0.0, 0.0, 1.0], device=m.device).expand(m.shape[0], 1, 4)
        return torch.cat([m, last], dim=1)


def _poses44(p, name: str) -> Tensor:
    p = torch.as_tensor(p).detach().to("cpu", torch.float64)
    if p.dim() != 3 or p.shape[1] not in (3, 4) or p.shape[2] != 4:
        raise ValueError(f"pose_error: {name} {tuple(p.shape)} is not [n, 3 or 4, 4]")
    return p


def pose_error(refined, truth) -> Tuple[Tensor, Tensor]:
    """(rotation error in degrees [n], translation error [n]) of `refined` against `truth` ([n,3|4,4] camera-to-world)
    after the similarity (Procrustes / Umeyama) alignment of the refined camera centres onto the true ones: the joint
    problem fixes the cameras only up to such a transform.  Host, float64.  With centres that do not determine a part
    of the alignment (one camera, coincident centres) that part is left out: scale 1, no rotation."""
    P, Q = _poses44(refined, "refined"), _poses44(truth, "truth")
    if P.shape[0] != Q.shape[0]:
        raise ValueError(f"pose_error: {P.shape[0]} refined poses against {Q.shape[0]} true ones")
    n = P.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.float64)
    c, cs = P[:, :3, 3], Q[:, :3, 3]
    mu, mus = c.mean(0), cs.mean(0)
    x, y = c - mu, cs - mus
    var = (x * x).sum() / n
    cov = y.T @ x / n
    Rg, s = torch.eye(3, dtype=torch.float64), 1.0
    if float(var) > 0.0 and float(cov.abs().max()) > 0.0:
        U, D, Vh = torch.linalg.svd(cov)
        S = torch.ones(3, dtype=torch.float64)
        if float(torch.linalg.det(U) * torch.linalg.det(Vh)) < 0.0:
            S[2] = -1.0
        Rg = U @ torch.diag(S) @ Vh
        s = float((D * S).sum() / var)
    aligned = s * (c @ Rg.T) + (mus - s * (Rg @ mu))
    t_err = (aligned - cs).norm(dim=1)
    D = Q[:, :3, :3].transpose(1, 2) @ (Rg @ P[:, :3, :3])  # the residual rotation of each camera
    sin = 0.5 * torch.stack([D[:, 2, 1] - D[:, 1, 2], D[:, 0, 2] - D[:, 2, 0], D[:, 1, 0] - D[:, 0, 1]], -1).norm(dim=1)
    cos = 0.5 * (D.diagonal(dim1=1, dim2=2).sum(-1) - 1.0)
    return torch.atan2(sin, cos) * (180.0 / math.pi), t_err
