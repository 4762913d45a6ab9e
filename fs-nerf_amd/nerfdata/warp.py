"""Depth-warp sampling against the training views (this package's own; DESIGN section 6.1 "Depth-warp consistency"):
WarpSource holds what the operator ops.warp_sample reads of a RayDataset - the resident uint8 images, the poses and the
intrinsics, refined ones included - and chooses source views.  core.loss.WarpConsistencyLoss is the loss on top.
There is no CPU implementation."""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor

from .. import ops
from .raydata import RayDataset


class WarpSource:
    """The training photographs as sources of a reprojection term: `sample(rays_o, rays_d, depth, src_view)` takes each
    rendered ray and its depth to the colour that view `src_view` shows at that 3-D point (ops.warp_sample: one launch
    each way over the dataset's bytes - no float copy of the images is made).

    cameras: a CameraRefiner, intrinsics: an IntrinsicsRefiner - the current corrected poses and camera table are read,
    detached, on every use; without them the dataset's stored poses and (focal, focal, W/2, H/2).  The source cameras
    are constants of the operator: no gradient reaches the refiners through it.
    A dataset with ndc=True is refused: its rays live in normalised device coordinates, where the ray parameter that
    the renderer integrates to a "depth" is not a metric distance along a world ray, so o + depth d is not the 3-D
    point the photographs see."""

    def __init__(self, dataset: RayDataset, cameras=None, intrinsics=None):
        if dataset.ndc:
            raise ValueError("WarpSource: the dataset serves NDC rays (ndc=True); an NDC ray parameter is not a metric depth, "
                             "so a rendered depth cannot be reprojected into the photographs")
        self.dataset, self.cameras, self.intrinsics = dataset, cameras, intrinsics
        self.images, self.white_bkgd = dataset.imgs, dataset.white_bkgd
        H, W, focal = dataset.hwf
        # the stored intrinsics as the ray batch forms them (pinhole_consts: W * 0.5 and H * 0.5 rounded to float32)
        self._K0 = torch.tensor([[focal, focal, W * 0.5, H * 0.5]], dtype=torch.float32, device=dataset.device)
        self._others: Dict[int, Tensor] = {}

    @property
    def n_views(self) -> int:
        return self.images.shape[0]

    def poses12(self) -> Tensor:
        """The source poses [V,12] of this moment: the refiner's, detached, else the stored ones."""
        return self.dataset.poses12 if self.cameras is None else self.cameras.poses12().detach()

    def K(self) -> Tensor:
        """The camera table [1 or V, 4] of this moment: the IntrinsicsRefiner's, detached, else the stored [1,4]."""
        return self._K0 if self.intrinsics is None else self.intrinsics.K().detach()

    def other_views(self, k: int = 1) -> Tensor:
        """[V,k] int64 on the device: for each training view the `k` other views whose STORED camera centres are
        nearest, nearest first (computed on the host, once per k); -1 where there are fewer than k others (V == 1
        gives -1 throughout), which the operator reads as "no source view"."""
        k = int(k)
        if k < 1:
            raise ValueError(f"WarpSource.other_views: k = {k} (at least 1)")
        if k not in self._others:
            c = self.dataset.poses[:, :3, 3].to(torch.float64)
            V = c.shape[0]
            dist = torch.cdist(c, c)
            dist.fill_diagonal_(float("inf"))
            order = torch.argsort(dist, dim=1, stable=True)[:, :min(k, max(V - 1, 0))]
            out = torch.full((V, k), -1, dtype=torch.int64)
            out[:, :order.shape[1]] = order
            self._others[k] = out.to(self.dataset.device)
        return self._others[k]

    def nearest_views(self, poses12: Tensor) -> Tensor:
        """[B] int64: for each query pose [B,12] (UnseenPatchLoader's, with_poses=True) the training view whose current
        camera centre is nearest.  Torch ops on the device, no host synchronisation."""
        q = poses12.reshape(-1, 3, 4)[:, :, 3]
        c = self.poses12().view(-1, 3, 4)[:, :, 3]
        return torch.cdist(q.to(c.dtype), c).argmin(dim=1)

    def sample(self, rays_o: Tensor, rays_d: Tensor, depth: Tensor, src_view: Tensor, **kw):
        """ops.warp_sample over this source's images, poses and camera table -> (colour [n,3], valid [n] bool, uvz or
        None); keywords: z_min, border, want_uvz."""
        return ops.warp_sample(rays_o, rays_d, depth, src_view, self.poses12(), self.images, self.K(),
                               white_bkgd=self.white_bkgd, **kw)
