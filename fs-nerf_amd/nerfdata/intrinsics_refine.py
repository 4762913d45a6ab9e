"""Learnable intrinsics behind the loaders (this package's own): the other half of nerfdata.CameraRefiner.

A camera table K = (fx, fy, cx, cy), float32 on the device, [1,4] (shared by all views) or [n_views,4], is formed from
the parameter phi (zeros at the start) over the dataset's hwf = (H, W, f0):
    fx = f0 exp(phi_0),  fy = f0 exp(phi_1) (tie_focal: fy = fx),  cx = W/2 + W phi_2,  cy = H/2 + H phi_3
so that phi = 0 is the stored intrinsics value for value and one learning rate serves all four columns.  RayLoader /
PatchLoader(intrinsics=refiner), alone or with cameras=, serve their one-launch batches over K() and hand rays_o /
rays_d out of one autograd node (raydata._CameraRays) whose backward is fsn_ray_camera_grad + fsn_intrinsics_grad
into phi.grad (and xi.grad).  The NDC map keeps the constants of the stored focal: a fixed warp of space."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor, nn

from .. import ops
from ..utils import utilities as U
from .raydata import _NDC_NEAR, ParamCache, RayDataset


class IntrinsicsRefiner(nn.Module):
    """phi [m,4], float32 on the device, zeros at the start; m = 1, or n_views with per_view=True.  `dataset_or_hwf`: a
    RayDataset (its hwf, view count and device) or (H, W, focal) with `n_views` (needed for per_view; None for a shared
    table serves any number of views).

    tie_focal (the reference's single focal): fy = fx, phi[:,1] is unused and its gradient exactly 0.
    learn_focal / learn_principal_point = False: that half of phi.grad is zeroed.  The principal point is off by default:
    with learnable poses it is nearly degenerate with the rotation at usual fields of view.
    K(): the [m,4] table the loaders launch over - recomputed, by one launch, only when phi changed."""

    def __init__(self, dataset_or_hwf, n_views: Optional[int] = None, *, per_view: bool = False, tie_focal: bool = True,
                 learn_focal: bool = True, learn_principal_point: bool = False, device=torch.device("cuda")):
        super().__init__()
        if isinstance(dataset_or_hwf, RayDataset):
            ds = dataset_or_hwf
            if n_views is not None and int(n_views) != ds.n_views:
                raise ValueError(f"IntrinsicsRefiner: n_views {n_views} against the dataset's {ds.n_views}")
            hwf, n_views, device = ds.hwf, ds.n_views, ds.device
        else:
            hwf = tuple(dataset_or_hwf)
        if len(hwf) != 3 or int(hwf[0]) <= 0 or int(hwf[1]) <= 0 or not float(hwf[2]) > 0.0:
            raise ValueError(f"IntrinsicsRefiner: hwf {hwf} is not (H > 0, W > 0, focal > 0)")
        if per_view and (n_views is None or int(n_views) < 1):
            raise ValueError("IntrinsicsRefiner: per_view=True needs the number of views (a dataset, or n_views)")
        device = U._need_gpu(device, "IntrinsicsRefiner")
        self.hwf0 = (int(hwf[0]), int(hwf[1]), float(hwf[2]))
        self.n_views = None if n_views is None else int(n_views)
        self.per_view, self.tie_focal = bool(per_view), bool(tie_focal)
        self.learn_focal, self.learn_principal_point = bool(learn_focal), bool(learn_principal_point)
        self.phi = nn.Parameter(torch.zeros(self.n_views if self.per_view else 1, 4, device=device, dtype=torch.float32))
        self._table = ParamCache()

    @property
    def device(self) -> torch.device:
        return self.phi.device

    def K(self) -> Tensor:
        H, W, f0 = self.hwf0
        return self._table.get(self.phi, lambda: ops.intrinsics_compose(self.phi, H, W, f0, self.tie_focal))

    def grad_phi(self, grad_K_views: Tensor) -> Tensor:
        """dL/dphi from ops.ray_camera_grad's per-view dL/dK: one launch, then the learn_* flags."""
        H, W, f0 = self.hwf0
        g = ops.intrinsics_grad(self.phi, grad_K_views, H, W, f0, self.tie_focal)
        if not self.learn_focal:
            g[:, :2].zero_()
        if not self.learn_principal_point:
            g[:, 2:].zero_()
        return g

    def hwf(self) -> Tuple[int, int, float]:
        """(H, W, focal) as host numbers (one read-back) for render_frame / render_path, which know one focal and a
        centred principal point: a shared table with a tied focal and phi[:, 2:] = 0 only."""
        H, W, _ = self.hwf0
        if self.per_view or not self.tie_focal or bool(self.phi.detach()[:, 2:].any()):
            raise ValueError("IntrinsicsRefiner.hwf: per-view intrinsics, an untied focal or a moved principal point do "
                             "not fit an (H, W, focal) triple; render the frame's rays instead: "
                             "render_rays(*refiner.frame_rays(pose, view), ...)")
        return H, W, float(self.K()[0, 0])

    def frame_rays(self, pose, view: int = 0, ndc: bool = False) -> Tuple[Tensor, Tensor]:
        """(rays_o, rays_d) [H*W, 3] of the frame seen from `pose` ([3|4,4]) under view `view`'s row of K, row-major
        pixels, in ONE launch, for render_rays; ndc: mapped as the loaders map (near 1, the stored focal's constants)."""
        H, W, f0 = self.hwf0
        p = torch.as_tensor(pose).detach().to(self.device, torch.float32)
        if p.dim() != 2 or p.shape[0] not in (3, 4) or p.shape[1] != 4:
            raise ValueError(f"IntrinsicsRefiner.frame_rays: pose {tuple(p.shape)} is not [3 or 4, 4]")
        K = self.K()
        if self.per_view:
            if not 0 <= int(view) < K.shape[0]:
                raise ValueError(f"IntrinsicsRefiner.frame_rays: view {view} is outside [0, {K.shape[0]})")
            K = K[int(view):int(view) + 1]
        # (a frame is H * W patches of one pixel in identity order: the patch entry point serves rays without images)
        o, d, _, _ = ops.ray_patch_batch(p[:3, :4].reshape(1, 12).contiguous(), None, H, W, f0, 1, 1, ndc=ndc, near=_NDC_NEAR,
                                         order="identity", start=0, count=H * W, want_rgb=False, K=K)
        return o, d
