"""Device-resident ray dataset and loaders: the arithmetic of the reference's src/nerfdata/datasets/{blender,llff}.py and
the three loaders of src/nerfdata/splitter.py:123-132, behind the duck-typed surface its train() and evaluation()
consume (run-nerf.py:134-152, 236-240, 384-456).

The ray tables are pure functions of (pose, pixel), so only the uint8 images (3-4 bytes per pixel instead of 36 bytes
of float tables), the poses and the region of interest are kept on the GPU.  A batch is ONE launch (ops.ray_batch /
fsn_ray_batch): position in the epoch -> shuffled ray index -> (view, row, column) -> ray (+ NDC) -> ground-truth
colour, bit for bit what the reference's float tables hold.  There is no CPU implementation.

PatchLoader (this package's own: the reference trains on single rays) serves batches of P x P pixel patches the same
way (ops.ray_patch_batch / fsn_ray_patch_batch), for losses that need several rendered pixels at once.

Auxiliary planes (this package's own): per-pixel float targets other than colour - sparse or sensor depth, a mask, a
monocular depth prior - kept beside the images as `dataset.aux` [n,H,W,A] float32 and served by the batch's own launch
(`want_aux` / `with_aux`), bit for bit; NaN is the documented "nothing known here"."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import ops
from ..utils import utilities as U

_NDC_NEAR = 1.0  # the reference maps to NDC with near = 1 (llff.py:76), as U.build_rays does


class RayDataset:
    """imgs: uint8 [n,H,W,3|4] (numpy or tensor), poses [n,3|4,4], hwf = (H, W, focal).

    len() = n*H*W rays in the reference's order (view-major, then row-major pixels); dataset[i] and
    dataset[index_tensor] -> (ray_o, ray_d, rgb), rows `i` of the reference's tables.  Attributes the reference's loops
    read: near, far, ndc, hwf, aabb (device), poses ([n,4,4] float32 on the host, as the reference keeps them).
    aux: auxiliary planes (`set_aux`), None for a dataset without."""

    def __init__(self, imgs, poses, hwf: Tuple[int, int, float], *, near: float, far: float, ndc: bool = False,
                 white_bkgd: bool = False, device=torch.device("cuda"), aux=None):
        device = U._need_gpu(device, "RayDataset")
        imgs = torch.as_tensor(imgs)
        if imgs.dtype != torch.uint8:
            raise TypeError(f"RayDataset: images must be uint8 bytes, got {imgs.dtype}.  The colours served are bit for bit "
                            "the reference's byte / 255.0 (and its alpha composition); a float image has already been "
                            "rounded once and cannot give them back.  Pass the decoded bytes (R.to8b for renders).")
        H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
        if imgs.dim() != 4 or tuple(imgs.shape[1:3]) != (H, W) or imgs.shape[3] not in (3, 4):
            raise ValueError(f"RayDataset: images {tuple(imgs.shape)} are not [n, {H}, {W}, 3 or 4]")
        if white_bkgd and imgs.shape[3] != 4:
            raise ValueError("RayDataset: white_bkgd composes over the alpha channel and needs RGBA images")
        P = torch.as_tensor(np.asarray(poses) if not isinstance(poses, Tensor) else poses).detach().to("cpu", torch.float32)
        if P.dim() != 3 or P.shape[0] != imgs.shape[0] or P.shape[1] not in (3, 4) or P.shape[2] != 4:
            raise ValueError(f"RayDataset: poses {tuple(P.shape)} are not [{imgs.shape[0]}, 3 or 4, 4]")
        if P.shape[1] == 3:
            P = torch.cat([P, torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(P.shape[0], 1, 4)], dim=1)
        self.hwf = (H, W, focal)
        self.near, self.far, self.ndc, self.white_bkgd = near, far, bool(ndc), bool(white_bkgd)
        self.poses = P.contiguous()
        self.imgs = imgs.to(device).contiguous()
        self.poses12 = self.poses[:, :3, :4].reshape(-1, 12).contiguous().to(device)
        self.device = self.imgs.device
        self.aux: Optional[Tensor] = None
        if aux is not None:
            self.set_aux(aux)
        # the region of interest of the occupancy estimator (llff.py:77-86, blender.py:140)
        if self.ndc and len(self):
            _o, _d, self.aabb = U.build_rays(self.poses, self.hwf, self.device, ndc=True)  # the existing reduction;
            del _o, _d                                                                     # its tables are dropped
        else:
            self.aabb = torch.tensor([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], device=self.device)

    @classmethod
    def blender(cls, imgs_rgba, poses, hwf, white_bkgd: bool = False, device=torch.device("cuda")) -> "RayDataset":
        """BlenderDataset's constants (blender.py:104-106, 140): near 2, far 6, no NDC, region of interest +-1.5."""
        return cls(imgs_rgba, poses, hwf, near=2.0, far=6.0, ndc=False, white_bkgd=white_bkgd, device=device)

    @classmethod
    def llff(cls, imgs, poses, min_bound: float, max_bound: float, hwf, ndc: bool = True,
             device=torch.device("cuda")) -> "RayDataset":
        """LLFFDataset's bounds (llff.py:48-53) and region of interest (llff.py:77-86)."""
        near, far = (0.0, 1.0) if ndc else (min_bound * 0.9, max_bound * 1.0)
        return cls(imgs, poses, hwf, near=near, far=far, ndc=ndc, white_bkgd=False, device=device)

    def set_aux(self, planes) -> None:
        """Store auxiliary planes: float32 [n,H,W,A] or [n,H,W] (numpy or tensor), 1 <= A <= 4, kept contiguous on the
        dataset's device as `aux` [n,H,W,A] and served by batch(..., want_aux=True) and the loaders' with_aux.  Any bit
        pattern is kept as it is, NaN and Inf included; None drops the planes."""
        if planes is None:
            self.aux = None
            return
        planes = torch.as_tensor(planes)
        if planes.dtype != torch.float32:
            raise TypeError(f"RayDataset: aux planes must be float32, got {planes.dtype}")
        n, (H, W, _) = self.imgs.shape[0], self.hwf
        if planes.dim() == 3:
            planes = planes.unsqueeze(-1)
        if planes.dim() != 4 or tuple(planes.shape[:3]) != (n, H, W) or not 1 <= planes.shape[3] <= 4:
            raise ValueError(f"RayDataset: aux planes {tuple(planes.shape)} are not [{n}, {H}, {W}] or [{n}, {H}, {W}, 1 to 4]")
        self.aux = planes.detach().to(self.device).contiguous()

    def _want_aux(self, who: str) -> dict:
        """The keywords of a batch that wants its aux rows."""
        if self.aux is None:
            raise ValueError(f"RayDataset.{who}: want_aux on a dataset without aux planes (set_aux)")
        return dict(aux=self.aux, want_aux=True)

    # ------------------------------------------------------------------
    @property
    def n_views(self) -> int:
        return self.imgs.shape[0]

    def __len__(self) -> int:
        return self.imgs.shape[0] * self.imgs.shape[1] * self.imgs.shape[2]

    def batch(self, order: str, *, start: int = 0, count: Optional[int] = None, seed: int = 0, epoch: int = 0,
              indices: Optional[Tensor] = None, want_rays: bool = True, want_rgb: bool = True, want_index: bool = False,
              poses12: Optional[Tensor] = None, K: Optional[Tensor] = None, want_aux: bool = False):
        """ops.ray_batch on this dataset's tensors: (rays_o, rays_d, rgb, index), None where not wanted; with want_aux
        a 5-tuple whose last element is the rows of the aux planes [count, A].
        poses12: other [n,12] matrices than the stored ones (CameraRefiner.poses12()); K: a camera table [1 or n, 4] in
        place of the stored intrinsics (IntrinsicsRefiner.K())."""
        H, W, focal = self.hwf
        return ops.ray_batch(self.poses12 if poses12 is None else poses12, self.imgs, H, W, focal, ndc=self.ndc, near=_NDC_NEAR, white_bkgd=self.white_bkgd,
                             order=order, seed=seed, epoch=epoch, indices=indices, start=start, count=count,
                             want_rays=want_rays, want_rgb=want_rgb, want_index=want_index, K=K,
                             **(self._want_aux("batch") if want_aux else {}))

    def n_anchors(self, patch: int, dilation: int = 1) -> int:
        """The number of `patch` x `patch` patches at `dilation` that fit the images: n * (H - ext + 1) * (W - ext + 1)
        anchors (top-left pixels), ext = (patch - 1) * dilation + 1; ValueError for a patch that does not fit."""
        H, W, _ = self.hwf
        if patch < 1 or dilation < 1:
            raise ValueError(f"RayDataset: bad patch {patch} or dilation {dilation} (both at least 1)")
        ext = (patch - 1) * dilation + 1
        if ext > H or ext > W:
            raise ValueError(f"RayDataset: a patch of {patch} pixels at dilation {dilation} spans {ext} pixels and does "
                             f"not fit the {H} x {W} images")
        return self.imgs.shape[0] * (H - ext + 1) * (W - ext + 1)

    def patch_batch(self, order: str, patch: int, dilation: int = 1, *, start: int = 0, count: Optional[int] = None,
                    seed: int = 0, epoch: int = 0, anchors: Optional[Tensor] = None, want_rays: bool = True,
                    want_rgb: bool = True, want_index: bool = False, poses12: Optional[Tensor] = None,
                    K: Optional[Tensor] = None, want_aux: bool = False):
        """ops.ray_patch_batch on this dataset's tensors: `count` patches of `patch` x `patch` pixels from position
        `start` of `order` over the n_anchors(patch, dilation) anchors -> (rays_o, rays_d, rgb, index) of
        count * patch^2 rows, patch after patch, row-major inside a patch; None where not wanted.
        poses12, K, want_aux: as batch() (aux [count * patch^2, A])."""
        self.n_anchors(patch, dilation)
        H, W, focal = self.hwf
        return ops.ray_patch_batch(self.poses12 if poses12 is None else poses12, self.imgs, H, W, focal, patch, dilation, ndc=self.ndc, near=_NDC_NEAR,
                                   white_bkgd=self.white_bkgd, order=order, seed=seed, epoch=epoch, anchors=anchors,
                                   start=start, count=count, want_rays=want_rays, want_rgb=want_rgb, want_index=want_index,
                                   K=K, **(self._want_aux("patch_batch") if want_aux else {}))

    def __getitem__(self, idx):
        """Not the hot path (the loaders never come here): a tensor of indices costs one min / max read-back so that an
        index outside [0, len) raises IndexError BEFORE anything is launched."""
        n = len(self)
        if isinstance(idx, Tensor) and idx.dim() > 0:
            if idx.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
                raise TypeError(f"RayDataset: indices must be integers, got {idx.dtype}")
            if idx.numel():
                lo, hi = (int(v) for v in torch.stack([idx.min(), idx.max()]).tolist())
                if lo < 0 or hi >= n:
                    raise IndexError(f"RayDataset: index {lo if lo < 0 else hi} is outside [0, {n})")
            o, d, rgb, _ = self.batch("explicit", indices=idx.reshape(-1).to(self.device, torch.int64))
            return o, d, rgb
        i = int(idx)
        if i < 0 or i >= n:
            raise IndexError(f"RayDataset: index {i} is outside [0, {n})")
        o, d, rgb, _ = self.batch("identity", start=i, count=1)
        return o[0], d[0], rgb[0]


def _seed_or_default(seed: Optional[int]) -> int:
    return int(torch.initial_seed() if seed is None else seed) & 0xFFFFFFFFFFFFFFFF


class ParamCache:
    """What one launch forms from a parameter (CameraRefiner's corrected poses, IntrinsicsRefiner's camera table), formed
    again only when the parameter changed: an optimizer step or load_state_dict writes in place (a new _version), .to()
    replaces the tensor (a new data_ptr)."""

    def __init__(self):
        self._value, self._key = None, None

    def get(self, param: Tensor, compute) -> Tensor:
        key = (param._version, param.data_ptr())
        if self._value is None or key != self._key:
            self._value, self._key = compute(), key
        return self._value


def served_rays(poses0: Tensor, cameras, intrinsics, geometry, launch):
    """A loader's batch over learnable cameras: `cameras` (a CameraRefiner) and / or `intrinsics` (an
    IntrinsicsRefiner), `poses0` the stored [n,12] poses, geometry = (H, W, focal, ndc, near) of the dataset;
    `launch(poses12, K)` is the loader's one ray_batch / ray_patch_batch call (with the index) over the matrices and the
    camera table it is handed (None: the stored ones) -> (rays_o, rays_d, rgb, index), rays_o / rays_d attached to xi
    and phi through ONE autograd node.  A launch that serves aux rows as well returns them fifth, and so does this."""
    return _CameraRays.apply(None if cameras is None else cameras.xi, None if intrinsics is None else intrinsics.phi,
                             poses0, cameras, intrinsics, geometry, launch)


class _CameraRays(torch.autograd.Function):
    """forward: the loader's launch over cameras.poses12() and intrinsics.K(); backward, with poses alone: ONE
    fsn_ray_pose_grad launch -> dL/dxi; with intrinsics: ONE fsn_ray_camera_grad launch -> dL/dxi and the per-view
    dL/dK, then fsn_intrinsics_grad -> dL/dphi.  No host synchronisation on either side."""

    @staticmethod
    def forward(ctx, xi: Optional[Tensor], phi: Optional[Tensor], poses0: Tensor, cameras, intrinsics, geometry, launch):
        K = None if intrinsics is None else intrinsics.K()
        o, d, rgb, index, *aux = launch(None if cameras is None else cameras.poses12(), K)
        ctx.save_for_backward(index, *[t for t in (xi, phi) if t is not None])
        ctx.poses0, ctx.K = poses0, K  # (K: the table of THIS batch - a later step makes a new one)
        ctx.cameras, ctx.intrinsics, ctx.geometry = cameras, intrinsics, geometry
        ctx.mark_non_differentiable(*[t for t in (rgb, index, *aux) if t is not None])
        ctx.set_materialize_grads(False)
        return (o, d, rgb, index, *aux)

    @staticmethod
    def backward(ctx, grad_o, grad_d, _grad_rgb, _grad_index, *_grad_aux):
        index, *params = ctx.saved_tensors
        cam, intr = ctx.cameras, ctx.intrinsics
        xi = params[0] if cam is not None else None
        H, W, focal, ndc, near = ctx.geometry
        if intr is None:
            g = ops.ray_pose_grad(cam.poses0, xi, H, W, focal, index, grad_o, grad_d, ndc=ndc, near=near)
            g_phi = None
        else:
            g, g_K = ops.ray_camera_grad(ctx.poses0, xi, H, W, focal, ctx.K, index, grad_o, grad_d, ndc=ndc, near=near)
            g_phi = intr.grad_phi(g_K)
        if cam is not None:
            if not cam.learn_rotation:
                g[:, :3].zero_()
            if not cam.learn_translation:
                g[:, 3:].zero_()
        return g, g_phi, None, None, None, None, None


class RayLoader:
    """The train loader (splitter.py:123-126: DataLoader(train_set, batch_size, shuffle=True)): every next() is ONE
    launch returning device tensors (rays_o [B,3], rays_d [B,3], rgb [B,3]) (+ index [B] with `with_index`, then
    + aux [B,A], the rows of the dataset's aux planes, with `with_aux`: the last element), no host synchronisation.  Every iter() starts the next epoch under a new permutation (an abandoned iterator counts), an
    epoch serves every ray exactly once, the last batch is short, then StopIteration.

    world > 1 (ray-batch data parallelism, shard.py): all ranks walk the same permutation; global batch g is positions
    [g*B*world, (g+1)*B*world) and rank r takes its r-th slice of B; the tail shorter than B*world is dropped so that
    every rank makes the same number of steps.

    state_dict() = (seed, epoch, next position); after load_state_dict() the next iter() continues that epoch at that
    position with the very batches the original would have served.

    cameras (a CameraRefiner over this dataset's views; None: the stored poses, the code path above): the same one
    launch runs over cameras.poses12(), and rays_o / rays_d come out of one autograd Function whose backward is one
    fsn_ray_pose_grad launch into cameras.xi.grad (pose_refine.py); still no host synchronisation.  The dataset's
    region of interest (aabb) stays that of the stored poses.

    intrinsics (an IntrinsicsRefiner, alone or with cameras): the launch runs over intrinsics.K() as well, and the one
    autograd node's backward is fsn_ray_camera_grad (+ fsn_intrinsics_grad) into xi.grad and intrinsics.phi.grad
    (intrinsics_refine.py).  The NDC map and the aabb stay those of the stored focal."""

    def __init__(self, dataset: RayDataset, batch_size: int, shuffle: bool = True, seed: Optional[int] = None, rank: int = 0,
                 world: int = 1, with_index: bool = False, cameras=None, intrinsics=None, with_aux: bool = False):
        if batch_size <= 0 or world <= 0 or not 0 <= rank < world:
            raise ValueError(f"RayLoader: bad batch_size {batch_size}, rank {rank} or world {world}")
        if cameras is not None and (cameras.n_views != dataset.n_views or cameras.poses0.device != dataset.device):
            raise ValueError(f"RayLoader: cameras of {cameras.n_views} views on {cameras.poses0.device} do not match the "
                             f"dataset's {dataset.n_views} views on {dataset.device}")
        if intrinsics is not None and (intrinsics.n_views not in (None, dataset.n_views)
                                       or intrinsics.device != dataset.device
                                       or tuple(intrinsics.hwf0) != tuple(dataset.hwf)):
            raise ValueError(f"RayLoader: intrinsics of {intrinsics.n_views} views over hwf {intrinsics.hwf0} on "
                             f"{intrinsics.device} do not match the dataset's {dataset.n_views} views over "
                             f"{dataset.hwf} on {dataset.device}")
        if with_aux and dataset.aux is None:
            raise ValueError("RayLoader: with_aux on a dataset without aux planes (RayDataset.set_aux)")
        self.cameras, self.intrinsics, self.with_aux = cameras, intrinsics, bool(with_aux)
        self.dataset, self.batch_size, self.shuffle = dataset, int(batch_size), bool(shuffle)
        self.seed = _seed_or_default(seed)
        self.rank, self.world, self.with_index = int(rank), int(world), bool(with_index)
        self.epoch = -1       # epoch of the latest iterator (-1: none yet)
        self.position = 0     # global batches of that epoch already served
        self._resume = False  # load_state_dict(): the next iter() continues instead of advancing

    def _n_items(self) -> int:
        """What an epoch serves once each (PatchLoader: anchors instead of rays)."""
        return len(self.dataset)

    def _batch(self, order: str, **kw):
        """The dataset call of this loader (PatchLoader: patch_batch)."""
        return self.dataset.batch(order, **kw)

    def _serve(self, order: str, start: int, count: int, epoch: int):
        """The one launch of a next(): `count` items from position `start` of this epoch's order, over the stored
        cameras or, through the one autograd node, over the learnable ones (which always needs the index)."""
        kw = dict(start=start, count=count, seed=self.seed, epoch=epoch)
        if self.with_aux:  # (a loader without aux makes the very call it made before the planes existed)
            kw["want_aux"] = True
        if self.cameras is None and self.intrinsics is None:
            return self._batch(order, want_index=self.with_index, **kw)
        ds = self.dataset
        return served_rays(ds.poses12, self.cameras, self.intrinsics, (ds.hwf[0], ds.hwf[1], ds.hwf[2], ds.ndc, _NDC_NEAR),
                           lambda poses12, K: self._batch(order, want_index=True, poses12=poses12, K=K, **kw))

    def __len__(self) -> int:
        n, stride = self._n_items(), self.batch_size * self.world
        return -(-n // stride) if self.world == 1 else n // stride

    def __iter__(self) -> "_RayIterator":
        if self._resume:
            self._resume = False
        else:
            self.epoch += 1
            self.position = 0
        return _RayIterator(self, self.epoch, self.position)

    def state_dict(self) -> dict:
        return {"seed": self.seed, "epoch": self.epoch, "position": self.position}

    def load_state_dict(self, state: dict) -> None:
        self.seed, self.epoch, self.position = int(state["seed"]), int(state["epoch"]), int(state["position"])
        self._resume = self.epoch >= 0


class _RayIterator:
    def __init__(self, loader: RayLoader, epoch: int, position: int):
        self.loader, self.epoch, self.position = loader, epoch, position

    def __iter__(self):
        return self

    def __next__(self):
        ld = self.loader
        if self.position >= len(ld):
            raise StopIteration
        B, n = ld.batch_size, ld._n_items()
        start = (self.position * ld.world + ld.rank) * B
        served = ld._serve("permuted" if ld.shuffle else "identity", start, min(B, n - start), self.epoch)
        self.position += 1
        if ld.epoch == self.epoch:  # (an iterator abandoned for a newer one no longer moves the loader's state)
            ld.position = self.position
        if ld.with_aux:  # (o, d, rgb, index, aux)
            return tuple(served) if ld.with_index else (served[0], served[1], served[2], served[4])
        o, d, rgb, index = served
        return (o, d, rgb, index) if ld.with_index else (o, d, rgb)


class PatchLoader(RayLoader):
    """RayLoader over patches, for losses that need several rendered pixels at once (core/loss.py: SSIMLoss; patch
    regularisers on depth): every next() is ONE launch (RayDataset.patch_batch) returning (rays_o, rays_d, rgb) of
    [B * patch^2, 3] (+ index [B * patch^2] with `with_index`, + aux [B * patch^2, A] with `with_aux`) for B = patches_per_batch patches of patch x patch pixels
    `dilation` apart, patch after patch, so rgb.view(B, patch, patch, 3) is the patch stack.  RayLoader's contract holds
    over the ANCHORS (top-left pixels, dataset.n_anchors(patch, dilation) of them): a new permutation per iter(), every
    anchor exactly once per epoch, a short last batch, the world / rank slices, state_dict() / load_state_dict().
    ValueError for a patch that does not fit the images.  cameras, intrinsics: as RayLoader."""

    def __init__(self, dataset: RayDataset, patch: int, patches_per_batch: int, dilation: int = 1, shuffle: bool = True,
                 seed: Optional[int] = None, rank: int = 0, world: int = 1, with_index: bool = False, cameras=None,
                 intrinsics=None, with_aux: bool = False):
        super().__init__(dataset, patches_per_batch, shuffle, seed, rank, world, with_index, cameras, intrinsics, with_aux)
        self.patch, self.dilation = int(patch), int(dilation)
        self._anchors = dataset.n_anchors(self.patch, self.dilation)

    def _n_items(self) -> int:
        return self._anchors

    def _batch(self, order: str, **kw):
        return self.dataset.patch_batch(order, self.patch, self.dilation, **kw)


class FrameLoader:
    """The val / test loader evaluation() consumes (splitter.py:127-132, image mode, batch size 1): yields
    (rgb_gt [1,H,W,3] float32 on the device, pose [1,4,4]) per view, one launch per frame (identity order over that
    frame's pixels, no rays).  shuffle: the views in the epoch permutation of (seed, epoch), a new one per iter()."""

    def __init__(self, dataset: RayDataset, shuffle: bool = False, seed: Optional[int] = None):
        self.dataset, self.shuffle, self.seed = dataset, bool(shuffle), _seed_or_default(seed)
        self.epoch = -1

    def __len__(self) -> int:
        return self.dataset.n_views

    def __iter__(self):
        self.epoch += 1
        ds, n = self.dataset, self.dataset.n_views
        H, W, _ = ds.hwf
        order = ops.ray_perm_host(n, self.seed, self.epoch).tolist() if self.shuffle else range(n)
        for v in order:
            _, _, rgb, _ = ds.batch("identity", start=v * H * W, count=H * W, want_rays=False)
            yield rgb.reshape(1, H, W, 3), ds.poses[v:v + 1]
