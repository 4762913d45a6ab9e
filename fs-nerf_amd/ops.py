"""Tensor-level wrappers over the C-ABI (include/fsnerf_hip.h).  Every function here launches
HIP kernels on the current torch stream; inputs must live on the GPU (float32, contiguous).
No function in this module computes anything on the CPU.

A wrapper has one shape: convert the inputs, allocate the outputs, `_launch(symbol, device, *args)`.  `_launch` is the one
door to a C entry point that takes a stream, `_size` the door of the size queries, `_Held` the argument struct that owns
its tensors.  The door takes tensors where the header has device pointers and checks each against the declared pointee
(DESIGN.md section 1 has the rules they enforce)."""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib as L


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


# profiling hook (bench.py): a list -> every render_fused / render_occ_fused launch appends a pair of HIP events recorded
# on the launch stream right around the C-ABI call (the kernel's own duration, without the host path around it)
launch_timer: Optional[list] = None
# measurement hook (bench.py): a uint64 [2] device tensor -> every render_fused launch adds its (s_memtime, s_memrealtime)
# differences to it (fsn_render_args.clock_out): the clock the chip held during the launches
clock_buffer: Optional[Tensor] = None


# What a device pointer of the header points at, as torch holds it: width and kind.  Signedness is ignored (torch callers
# keep `status`, `bits` and `pending` as int32); void: any dtype.
_POINTEE_DTYPE = {"float": torch.float32, "double": torch.float64, "int64_t": torch.int64, "uint64_t": torch.int64,
                  "int32_t": torch.int32, "uint32_t": torch.int32, "uint8_t": torch.uint8, "void": None}


def _tensor_plan(params) -> tuple:
    """Where an entry point takes a tensor: (position, name, dtype, strided) of every device data pointer among its
    `params` (not the `*_host` ones, pointer arrays and structs).  strided: the header reads it through the element
    strides `<name>_strides_host`, so any view will do."""
    names = {p.name for p in params}
    return tuple((i, p.name, _POINTEE_DTYPE[p.pointee], p.name + "_strides_host" in names) for i, p in enumerate(params)
                 if p.pointee in _POINTEE_DTYPE and not p.name.endswith("_host"))


# built once, from the header (L.FUNCTIONS / L.STRUCTS): per symbol its argument count and tensor plan, per argument
# struct the dtype behind each pointer field
_PLANS = {name: (len(params), _tensor_plan(params)) for name, (_, params) in L.FUNCTIONS.items()}
_FIELDS = {s: {f.name: _POINTEE_DTYPE[f.pointee] for f in s.fields if f.pointee in _POINTEE_DTYPE}
           for s in L.STRUCTS.values()}


_NO_GUARD = contextlib.nullcontext()


def _index(dev) -> Optional[int]:
    """The index of the GPU `dev` names ("cuda" without one: the current device, as the guard reads it); None where
    there is no GPU to compare with (a size query without a device; a CPU device, which `_addr` then refuses)."""
    if dev is None:
        return None
    dev = dev if isinstance(dev, torch.device) else torch.device(dev)
    if dev.type != "cuda":
        return None
    return torch.cuda.current_device() if dev.index is None else dev.index


def _addr(t: Tensor, dtype, strided: bool, idx: Optional[int], what: str, param: str) -> int:
    """The door's rule for a tensor behind a device pointer -> its address: on the GPU (number `idx`, where one is given),
    of the pointee's dtype, contiguous unless read through strides.  It checks; it never casts or copies."""
    if not t.is_cuda:
        raise RuntimeError(f"{what}: {param}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{what}: {param}: expected {dtype} (include/fsnerf_hip.h), got {t.dtype}")
    if not (strided or t.is_contiguous()):
        raise ValueError(f"{what}: {param}: expected a contiguous tensor")
    if idx is not None and t.get_device() != idx:
        raise RuntimeError(f"{what}: {param}: the tensor is on {t.device}, the call on GPU {idx}")
    return t.data_ptr()


def _door(name: str, dev, args: tuple, n_more: int = 0) -> Tuple[list, Optional[int]]:
    """`args` as the C function takes them: a tensor where the header has a device data pointer becomes its address,
    checked by `_addr`; None stays NULL; ctypes arrays, byref(...) and pointer arrays pass through.  The caller's
    `args` keeps every tensor referenced until the call is enqueued.  -> (arguments, `_index(dev)`)."""
    n, plan = _PLANS[name]
    if len(args) + n_more != n:
        raise TypeError(f"{name}: takes {n - n_more} arguments (include/fsnerf_hip.h), got {len(args)}")
    args, idx = list(args), _index(dev)
    for i, param, dtype, strided in plan:
        t = args[i]
        if t is not None and isinstance(t, Tensor):
            # (the per-call path: `_addr`'s tests in one expression - a CPU tensor's get_device() is -1; it is called
            # where one fails, to say which, and where there is no device to compare with)
            if t.get_device() != idx or (dtype is not None and t.dtype != dtype) or not (strided or t.is_contiguous()):
                _addr(t, dtype, strided, idx, name, param)
            args[i] = t.data_ptr()
    return args, idx


def _launch(name: str, dev, *args, what: Optional[str] = None, timed: bool = False, counts: bool = False) -> int:
    """The one door to a C entry point that takes a stream: `name(*args, stream)` under the device guard of `dev` (the
    tensors' device), with the stream handle read INSIDE the guard - outside it the handle is the current device's, not
    theirs; where that device is the current one already the guard would change nothing and is not entered.  Tensors go
    in as they are (`_door`).  `what`: the error's text where it says more than the symbol.
    `timed`: the `launch_timer` bracket.  `counts`: the symbol returns a count (> 0) instead of a status code; -> that
    value."""
    fn = getattr(L.lib(), name)
    cargs, idx = _door(name, dev, args, 1)
    with _NO_GUARD if idx == torch.cuda.current_device() else torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        if timed and launch_timer is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*cargs, stream)
            e1.record()
            launch_timer.append((e0, e1))
        else:
            rc = fn(*cargs, stream)
    if counts:
        if rc <= 0:
            L.check(rc if rc < 0 else -3, what or name)
    elif rc != 0:
        L.check(rc, what or name)
    return rc


def _size(name: str, dev, *args) -> int:
    """The door of the size queries (workspace floats / doubles, blob bytes, compute units): -> the size; a negative
    value is an error code and raises.  `dev`: the device the answer is for (fsn_nerf_train_workspace_floats looks at
    its compute units), None where the arguments alone decide."""
    fn = getattr(L.lib(), name)
    cargs, _ = _door(name, dev, args)
    if dev is None:
        n = int(fn(*cargs))
    else:
        with torch.cuda.device(dev):
            n = int(fn(*cargs))
    if n < 0:
        L.check(n, name)
    return n


def _f32(t: Tensor, name: str) -> Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _opt_f32(t: Optional[Tensor], name: str) -> Optional[Tensor]:
    return None if t is None else _f32(t, name)


def _gpu_f32(t: Tensor, name: str) -> Tensor:
    """The packed primitives take GPU float32 as it is: nothing is cast (a cast would hide from autograd)."""
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    return t.contiguous()


def _flat(t: Optional[Tensor], name: str, n: int, cast: bool = False) -> Optional[Tensor]:
    """An optional tensor of `n` values, flat.  Two policies that stay apart: `_gpu_f32` (float32 or an error) and,
    with `cast`, `_f32` (any dtype, converted)."""
    if t is None:
        return None
    t = (_f32 if cast else _gpu_f32)(t, name).reshape(-1)
    if t.numel() != n:
        raise ValueError(f"{name}: expected {n} values, got {t.numel()}")
    return t


def _i64(t: Tensor, name: str) -> Tensor:
    """ray_indices as the kernels read them: int64 (the reference contract, rendering.py:66,92), on the GPU,
    contiguous.  nerfacc-style callers may hand int32 indices: they are widened here, never reinterpreted."""
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype not in (torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8):
        raise TypeError(f"{name}: expected an integer tensor, got {t.dtype}")
    return t.to(torch.int64).contiguous()


def _p(t: Optional[Tensor]):
    """The bare address of a tensor, for a direct C-ABI call that does not go through the door: the test-only binding
    of tests/ref_fp32 (a library without a header) and tests that call two entry points side by side.  No wrapper of
    this package uses it; handed to `_launch` it passes through unchecked, like any ctypes object."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _bk(bkgd) -> Optional[C.Array]:
    if bkgd is None:
        return None
    vals = [float(v) for v in (bkgd.detach().cpu().tolist() if isinstance(bkgd, Tensor) else bkgd)]
    return (C.c_float * 3)(*vals)


class _Held:
    """An argument struct `a` and the tensors its pointers name.  A tensor a conversion made (`_f32` of a float64 mask,
    a reshaped `u`) must stay referenced until the call is enqueued: the outputs are allocated after it, and the caching
    allocator hands a dropped temporary's block to the next torch.empty of its size class.  So a pointer enters the
    struct only through `set`, which checks the tensor against the field's declared pointee (`_addr`: the door's rule;
    the GPU's index once `_ray_source` knows it), and the wrapper keeps the holder until it returns."""

    def __init__(self, a: C.Structure):
        self.a, self.tensors, self.idx = a, [], None

    def set(self, field: str, t: Optional[Tensor]) -> None:
        if t is not None:
            self.tensors.append(t)
            kind = type(self.a)
            setattr(self.a, field, _addr(t, _FIELDS[kind][field], False, self.idx, kind.__name__, field))


def _ray_source(h: _Held, rays_o: Optional[Tensor], rays_d: Optional[Tensor], camera) -> Tuple[int, torch.device]:
    """Ray tensors, or `camera` = (pose [3or4,4], H, W, focal, row0, nrows, device): the rays of the image rows
    [row0, row0+nrows) are generated inside the launch.  Fills R and rays_o / rays_d or cam_* -> (R, device)."""
    a = h.a
    if camera is None:
        o, d = _f32(rays_o, "rays_o").reshape(-1, 3), _f32(rays_d, "rays_d").reshape(-1, 3)
        a.R, h.idx = o.shape[0], _index(o.device)
        h.set("rays_o", o)
        h.set("rays_d", d)
        return o.shape[0], o.device
    pose, cH, cW, cfocal, crow0, cnrows, dev = camera
    a.R, h.idx = int(cnrows) * int(cW), _index(dev)
    pm = pose.detach().to("cpu", torch.float32)[:3, :4].contiguous().reshape(-1).tolist()
    for i in range(12):
        a.cam_pose[i] = pm[i]
    a.cam_H, a.cam_W, a.cam_row0, a.cam_focal = int(cH), int(cW), int(crow0), float(cfocal)
    return a.R, torch.device(dev)


def _masks(h: _Held, pos_mask: Optional[Tensor], dir_mask: Optional[Tensor]) -> None:
    h.set("pos_mask", _opt_f32(pos_mask, "pos_mask"))
    h.set("dir_mask", _opt_f32(dir_mask, "dir_mask"))


# ------------------------------------------------------------------ rays
def get_rays(pose: Tensor, H: int, W: int, focal: float, device, row0: int = 0,
             nrows: Optional[int] = None, out: Optional[Tuple[Tensor, Tensor]] = None) -> Tuple[Tensor, Tensor]:
    """`out`: optional pre-allocated ([nrows*W,3], [nrows*W,3]) contiguous fp32 slices to write into."""
    nrows = H - row0 if nrows is None else nrows
    p = pose.detach().to("cpu", torch.float32)[:3, :4].contiguous()
    pose_host = (C.c_float * 12)(*p.reshape(-1).tolist())
    if out is None:
        o = torch.empty(nrows * W, 3, device=device, dtype=torch.float32)
        d = torch.empty_like(o)
    else:
        o, d = out
        assert o.is_contiguous() and d.is_contiguous() and o.shape == (nrows * W, 3) and d.shape == o.shape
    _launch("fsn_get_rays", o.device, pose_host, H, W, float(focal), row0, nrows, o, d)
    return o, d


def build_rays(poses: Tensor, H: int, W: int, focal: float, device, ndc: bool = False, near: float = 1.0,
               want_aabb: bool = False):
    """Rays of all `poses` ([n, 3or4, 4]) in ONE launch (fsn_build_rays) -> (rays_o [n*H*W,3], rays_d [n*H*W,3],
    aabb [6] or None): get_rays per pose, optional NDC mapping, and the min / max region of interest over {o, o + d}
    (/ 2^3, llff.py:77-84) reduced inside the launch."""
    P = torch.as_tensor(poses, dtype=torch.float32)[:, :3, :4].reshape(-1, 12).contiguous().to(device)
    n = P.shape[0]
    o = torch.empty(n * H * W, 3, device=P.device, dtype=torch.float32)
    d = torch.empty_like(o)
    aabb = torch.empty(6, device=P.device, dtype=torch.float32) if want_aabb else None
    keys = torch.empty(6, device=P.device, dtype=torch.int32) if want_aabb else None
    _launch("fsn_build_rays", P.device, P, n, int(H), int(W), float(focal), 1 if ndc else 0, float(near), o, d, aabb, keys)
    return o, d, aabb


_RAY_ORDERS = {"identity": L.FSN_RAY_ORDER_IDENTITY, "permuted": L.FSN_RAY_ORDER_PERMUTED, "explicit": L.FSN_RAY_ORDER_EXPLICIT}


def _row_outputs(rows: int, dev, want_rays: bool, want_rgb: bool, want_index: bool):
    """The (rays_o, rays_d, rgb, index) outputs of a batch of `rows` rows; None where not asked for."""
    o = torch.empty(rows, 3, device=dev, dtype=torch.float32) if want_rays else None
    d = torch.empty(rows, 3, device=dev, dtype=torch.float32) if want_rays else None
    rgb = torch.empty(rows, 3, device=dev, dtype=torch.float32) if want_rgb else None
    index = torch.empty(rows, device=dev, dtype=torch.int64) if want_index else None
    return o, d, rgb, index


def _aux_planes(aux: Optional[Tensor], n_views: int, H: int, W: int, rows: int, dev, who: str):
    """The auxiliary planes of a batch that wants them, as the C-ABI takes them -> (aux, channels, aux_out [rows,
    channels]).  aux: float32 [n, H, W, A] or [n, H, W] on the batch's GPU, contiguous, 1 <= A <= 4."""
    if aux is None:
        raise ValueError(f"{who}: want_aux needs the aux planes")
    if not aux.is_cuda:
        raise RuntimeError(f"{who}: expected GPU aux planes (the HIP path has no CPU fallback)")
    if aux.dtype != torch.float32:
        raise TypeError(f"{who}: aux planes are float32, got {aux.dtype}")
    if aux.dim() not in (3, 4) or tuple(aux.shape[:3]) != (n_views, H, W) or not aux.is_contiguous():
        raise ValueError(f"{who}: aux planes {tuple(aux.shape)} are not a contiguous [{n_views}, {H}, {W}(, A)]")
    channels = 1 if aux.dim() == 3 else aux.shape[3]
    if not 1 <= channels <= 4:
        raise ValueError(f"{who}: {channels} aux channels (1 to 4)")
    return aux, channels, torch.empty(rows, channels, device=dev, dtype=torch.float32)


def _launch_cam(name: str, who: str, dev, head: tuple, K: Optional[Tensor], n_views: int, tail: tuple, planes=None) -> None:
    """`name` over the stored intrinsics, or its camera-table form `name`_k with (K, its rows) between head and tail;
    with `planes` (`_aux_planes`) its aux form `name`_aux, which takes both (no table: NULL and 0 rows)."""
    if planes is not None:
        table = (None, 0) if K is None else _camera_table(K, n_views, who)
        _launch(name + "_aux", dev, *head, *table, *tail, *planes)
    elif K is None:
        _launch(name, dev, *head, *tail)
    else:
        _launch(name + "_k", dev, *head, *_camera_table(K, n_views, who), *tail)


def ray_batch(poses12: Tensor, images: Tensor, H: int, W: int, focal: float, *, ndc: bool = False, near: float = 1.0,
              white_bkgd: bool = False, order: str = "identity", seed: int = 0, epoch: int = 0,
              indices: Optional[Tensor] = None, start: int = 0, count: Optional[int] = None, want_rays: bool = True,
              want_rgb: bool = True, want_index: bool = False, K: Optional[Tensor] = None, aux: Optional[Tensor] = None,
              want_aux: bool = False):
    """One batch of the data layer in ONE launch (fsn_ray_batch), no host synchronisation: `count` rays from position
    `start` of `order` ("identity", "permuted" by (seed, epoch), or "explicit" = the device int64 list `indices`) over
    the rays of the resident dataset (poses12 [n,12] float32, images uint8 [n,H,W,3|4], both on the GPU) ->
    (rays_o [count,3], rays_d [count,3], rgb [count,3], index [count] int64); an output not asked for is None.
    K: a camera table (intrinsics_compose) [1 or n, 4] -> the same launch over it (fsn_ray_batch_k); `focal` then feeds
    the NDC constants only.
    aux, want_aux: auxiliary float planes [n,H,W,A] or [n,H,W] (1 <= A <= 4) of the dataset; with want_aux the same
    launch (fsn_ray_batch_aux) also copies their rows, bit for bit, and a 5-tuple (..., index, aux [count, A]) comes back."""
    if not (poses12.is_cuda and images.is_cuda):
        raise RuntimeError("ray_batch: expected GPU tensors (the HIP path has no CPU fallback)")
    if images.dtype != torch.uint8 or poses12.dtype != torch.float32 or images.dim() != 4:
        raise TypeError("ray_batch: images are uint8 [n,H,W,C] and poses float32 [n,12]")
    assert images.is_contiguous() and poses12.is_contiguous() and images.shape[:3] == (poses12.shape[0], H, W)
    if order == "explicit":
        indices = _i64(indices, "indices")
        count = indices.numel()
    elif count is None:
        raise ValueError("ray_batch: count is needed for the identity and permuted orders")
    dev = images.device
    o, d, rgb, index = _row_outputs(count, dev, want_rays, want_rgb, want_index)
    planes = _aux_planes(aux, poses12.shape[0], int(H), int(W), count, dev, "ray_batch") if want_aux else None
    head = (poses12, poses12.shape[0], images, int(H), int(W), images.shape[3], float(focal))
    tail = (1 if ndc else 0, float(near), 1 if white_bkgd else 0, _RAY_ORDERS[order], int(seed) & 0xFFFFFFFFFFFFFFFF,
            int(epoch), indices, int(start), int(count), o, d, rgb, index)
    _launch_cam("fsn_ray_batch", "ray_batch", dev, head, K, poses12.shape[0], tail, planes)
    return (o, d, rgb, index, planes[2]) if want_aux else (o, d, rgb, index)


def ray_patch_batch(poses12: Tensor, images: Optional[Tensor], H: int, W: int, focal: float, patch: int, dilation: int = 1, *,
                    ndc: bool = False, near: float = 1.0, white_bkgd: bool = False, order: str = "identity", seed: int = 0,
                    epoch: int = 0, anchors: Optional[Tensor] = None, start: int = 0, count: Optional[int] = None,
                    want_rays: bool = True, want_rgb: bool = True, want_index: bool = False, K: Optional[Tensor] = None,
                    aux: Optional[Tensor] = None, want_aux: bool = False):
    """A batch of `patch` x `patch` pixel patches in ONE launch (fsn_ray_patch_batch), no host synchronisation: `count`
    patches from position `start` of `order` over the ANCHORS (top-left pixels) of the dataset - n * (H - ext + 1) *
    (W - ext + 1) of them, ext = (patch - 1) * dilation + 1; "explicit" = the device int64 list `anchors` ->
    (rays_o, rays_d, rgb [count * patch^2, 3], index [count * patch^2] int64), patch b in rows [b * patch^2, +patch^2),
    row-major, so rgb.view(count, patch, patch, 3) is the patch stack; an output not asked for is None.
    images=None (with want_rgb=False): ray-only patches for any poses.  K: as ray_batch (fsn_ray_patch_batch_k).
    aux, want_aux: as ray_batch (fsn_ray_patch_batch_aux): a 5-tuple with aux [count * patch^2, A] last."""
    if not (poses12.is_cuda and (images is None or images.is_cuda)):
        raise RuntimeError("ray_patch_batch: expected GPU tensors (the HIP path has no CPU fallback)")
    if poses12.dtype != torch.float32 or poses12.dim() != 2 or poses12.shape[1] != 12 or not poses12.is_contiguous():
        raise TypeError("ray_patch_batch: poses are float32 [n,12], contiguous")
    if images is None:
        if want_rgb:
            raise ValueError("ray_patch_batch: colours (want_rgb) need images")
        channels = 3
    else:
        if images.dtype != torch.uint8 or images.dim() != 4:
            raise TypeError("ray_patch_batch: images are uint8 [n,H,W,C]")
        assert images.is_contiguous() and images.shape[:3] == (poses12.shape[0], H, W)
        channels = images.shape[3]
    if order == "explicit":
        anchors = _i64(anchors, "anchors")
        count = anchors.numel()
    elif count is None:
        raise ValueError("ray_patch_batch: count is needed for the identity and permuted orders")
    dev = poses12.device
    o, d, rgb, index = _row_outputs(count * int(patch) * int(patch), dev, want_rays, want_rgb, want_index)
    planes = None
    if want_aux:
        planes = _aux_planes(aux, poses12.shape[0], int(H), int(W), count * int(patch) * int(patch), dev, "ray_patch_batch")
    head = (poses12, poses12.shape[0], images, int(H), int(W), channels, float(focal))
    tail = (1 if ndc else 0, float(near), 1 if white_bkgd else 0, _RAY_ORDERS[order], int(seed) & 0xFFFFFFFFFFFFFFFF,
            int(epoch), anchors, int(start), int(count), int(patch), int(dilation), o, d, rgb, index)
    _launch_cam("fsn_ray_patch_batch", "ray_patch_batch", dev, head, K, poses12.shape[0], tail, planes)
    return (o, d, rgb, index, planes[2]) if want_aux else (o, d, rgb, index)


def ray_perm_host(n: int, seed: int, epoch: int, start: int = 0, count: Optional[int] = None) -> Tensor:
    """Positions [start, start + count) of the epoch permutation of [0, n) as a CPU int64 tensor (fsn_ray_perm_host: the
    kernel's own function compiled for the host; no device is touched, so it takes no stream and needs no door)."""
    count = n - start if count is None else count
    out = torch.empty(max(count, 0), dtype=torch.int64)
    L.check(L.lib().fsn_ray_perm_host(int(n), int(seed) & 0xFFFFFFFFFFFFFFFF, int(epoch), int(start), int(count),
                                      C.c_void_p(out.data_ptr())), "fsn_ray_perm_host")
    return out


def unseen_poses(dist: L.UnseenDist, count: int, device, *, seed: int = 0, first: int = 0) -> Tensor:
    """Pose draws [first, first + count) of the distribution `dist` (a filled fsn_unseen_dist; nerfdata.UnseenViewSampler
    builds it) in ONE launch (fsn_unseen_poses) -> poses12 [count,12] on `device`: a pure function of (dist, seed, draw)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("unseen_poses: expected a GPU device (the HIP path has no CPU fallback)")
    out = torch.empty(int(count), 12, device=dev, dtype=torch.float32)
    _launch("fsn_unseen_poses", dev, C.byref(dist), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first), int(count), out)
    return out


def unseen_patch_batch(dist: L.UnseenDist, H: int, W: int, focal: float, patch: int, dilation: int = 1, *, device,
                       first_patch: int = 0, count: int, patches_per_pose: int = 1, seed: int = 0, ndc: bool = False,
                       near: float = 1.0, want_rays: bool = True, want_poses: bool = False, want_anchors: bool = False):
    """`count` patches of `patch` x `patch` rays of freshly drawn poses in ONE launch (fsn_unseen_patch_batch), no host
    synchronisation: patch q = first_patch + b is seen from pose draw q // patches_per_pose of `dist` at an anchor uniform
    over the (H - ext + 1) x (W - ext + 1) lattice, ext = (patch - 1) * dilation + 1 -> (rays_o, rays_d [count * patch^2,
    3], poses12 [count,12], anchors [count] int64 = row0 * (W - ext + 1) + col0); an output not asked for is None.  The
    rows are those of ray_patch_batch over `poses12` with the explicit anchors b * (H - ext + 1) * (W - ext + 1) +
    anchors[b], bit for bit."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("unseen_patch_batch: expected a GPU device (the HIP path has no CPU fallback)")
    count, rows = int(count), int(count) * int(patch) * int(patch)
    o = torch.empty(rows, 3, device=dev, dtype=torch.float32) if want_rays else None
    d = torch.empty(rows, 3, device=dev, dtype=torch.float32) if want_rays else None
    poses = torch.empty(count, 12, device=dev, dtype=torch.float32) if want_poses else None
    anchors = torch.empty(count, device=dev, dtype=torch.int64) if want_anchors else None
    _launch("fsn_unseen_patch_batch", dev, C.byref(dist), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_patch), count,
            int(patches_per_pose), int(H), int(W), float(focal), int(patch), int(dilation), 1 if ndc else 0, float(near),
            o, d, poses, anchors)
    return o, d, poses, anchors


def _pose_pair(poses0: Tensor, xi: Tensor, who: str) -> None:
    """The stored poses [n,12] and their corrections [n,6] as the pose kernels read them: nothing is cast or copied
    (xi is a parameter: a conversion would hide it from the caller)."""
    if not (poses0.is_cuda and xi.is_cuda):
        raise RuntimeError(f"{who}: expected GPU tensors (the HIP path has no CPU fallback)")
    if poses0.dtype != torch.float32 or xi.dtype != torch.float32:
        raise TypeError(f"{who}: poses and xi are float32, got {poses0.dtype} and {xi.dtype}")
    if poses0.dim() != 2 or poses0.shape[1] != 12 or tuple(xi.shape) != (poses0.shape[0], 6):
        raise ValueError(f"{who}: poses are [n,12] and xi [n,6], got {tuple(poses0.shape)} and {tuple(xi.shape)}")
    if not (poses0.is_contiguous() and xi.is_contiguous()) or poses0.device != xi.device:
        raise ValueError(f"{who}: poses and xi are contiguous tensors of one device")


def _ray_grads(index: Tensor, grad_o: Optional[Tensor], grad_d: Optional[Tensor]):
    """A batch's flat ray indices and ray gradients as the gradient kernels read them -> (index [count] int64, grad_o,
    grad_d [3 count] float32 or None, count)."""
    index = _i64(index, "index").reshape(-1)
    count = index.numel()
    return index, _flat(grad_o, "grad_o", 3 * count), _flat(grad_d, "grad_d", 3 * count), count


def pose_compose(poses0: Tensor, xi: Tensor) -> Tensor:
    """The corrected poses [n,12] = [exp([omega]x) R0 | t0 + tau] of the stored poses0 [n,12] and xi = (omega, tau)
    [n,6] in ONE launch (fsn_pose_compose)."""
    _pose_pair(poses0, xi, "pose_compose")
    xi = xi.detach()
    out = torch.empty_like(poses0)
    _launch("fsn_pose_compose", poses0.device, poses0, xi, poses0.shape[0], out)
    return out


def ray_pose_grad(poses0: Tensor, xi: Tensor, H: int, W: int, focal: float, index: Tensor, grad_o: Optional[Tensor],
                  grad_d: Optional[Tensor], *, ndc: bool = False, near: float = 1.0, want_pose_grad: bool = False):
    """dL/dxi [n,6] from the gradients of a batch's rays in ONE deterministic launch (fsn_ray_pose_grad): `index`
    [count] int64 are the batch's flat ray indices (ray_batch's `index` output), grad_o / grad_d [count,3] = dL/drays_o,
    dL/drays_d (None = zeros) of the rays served over pose_compose(poses0, xi).  A view without a ray gets exactly 0.
    want_pose_grad: -> (grad_xi, dL/d(corrected poses) [n,12])."""
    _pose_pair(poses0, xi, "ray_pose_grad")
    xi = xi.detach()
    index, grad_o, grad_d, count = _ray_grads(index, grad_o, grad_d)
    dev = poses0.device
    grad_xi = torch.empty_like(xi)
    grad_poses = torch.empty_like(poses0) if want_pose_grad else None
    _launch("fsn_ray_pose_grad", dev, poses0, xi, poses0.shape[0], int(H), int(W), float(focal), 1 if ndc else 0, float(near),
            index, grad_o, grad_d, count, grad_xi, grad_poses)
    return (grad_xi, grad_poses) if want_pose_grad else grad_xi


def _camera_table(K: Tensor, n_views: int, who: str) -> Tuple[Tensor, int]:
    """A camera table K = (fx, fy, cx, cy) [1 or n_views, 4] as the kernels read it -> (K, its rows); nothing is cast."""
    if not K.is_cuda:
        raise RuntimeError(f"{who}: K: expected a GPU tensor (the HIP path has no CPU fallback)")
    if K.dtype != torch.float32:
        raise TypeError(f"{who}: the camera table K is float32, got {K.dtype}")
    if K.dim() != 2 or K.shape[1] != 4 or K.shape[0] not in (1, n_views) or not K.is_contiguous():
        raise ValueError(f"{who}: the camera table K is [1 or {n_views}, 4], contiguous, got {tuple(K.shape)}")
    return K.detach(), K.shape[0]


def _phi(phi: Tensor, who: str) -> Tensor:
    if not phi.is_cuda:
        raise RuntimeError(f"{who}: expected GPU tensors (the HIP path has no CPU fallback)")
    if phi.dtype != torch.float32:
        raise TypeError(f"{who}: phi is float32, got {phi.dtype}")
    if phi.dim() != 2 or phi.shape[1] != 4 or not phi.is_contiguous():
        raise ValueError(f"{who}: phi is [m, 4], contiguous, got {tuple(phi.shape)}")
    return phi.detach()


def intrinsics_compose(phi: Tensor, H: int, W: int, focal0: float, tie_focal: bool = True) -> Tensor:
    """The camera table K = (fx, fy, cx, cy) [m,4] of the parameter phi [m,4] over the stored (H, W, focal0) in ONE
    launch (fsn_intrinsics_compose): fx = f0 exp(phi_0), fy = f0 exp(phi_1) (tie_focal: fy = fx),
    cx = W/2 + W phi_2, cy = H/2 + H phi_3; phi = 0 gives the stored intrinsics value for value."""
    phi = _phi(phi, "intrinsics_compose")
    out = torch.empty_like(phi)
    _launch("fsn_intrinsics_compose", phi.device, phi, phi.shape[0], int(H), int(W), float(focal0), 1 if tie_focal else 0, out)
    return out


def ray_camera_grad(poses0: Tensor, xi: Optional[Tensor], H: int, W: int, focal0: float, K: Tensor, index: Tensor,
                    grad_o: Optional[Tensor], grad_d: Optional[Tensor], *, ndc: bool = False, near: float = 1.0,
                    want_xi_grad: Optional[bool] = None) -> Tuple[Optional[Tensor], Tensor]:
    """(dL/dxi [n,6] or None, dL/dK per view [n,4]) from the gradients of a batch's rays in ONE deterministic launch
    (fsn_ray_camera_grad): ray_pose_grad's arguments over the camera table K [1 or n, 4] the rays were served with.
    xi=None: no pose correction (the rays of poses0).  want_xi_grad: None = where xi is given.  Row v of the second
    output is view v's rays' share of dL/d(fx, fy, cx, cy) (intrinsics_grad chains it to phi); a view without a ray gets
    exactly 0 in both."""
    if xi is None:
        if not poses0.is_cuda:
            raise RuntimeError("ray_camera_grad: expected GPU tensors (the HIP path has no CPU fallback)")
        if poses0.dtype != torch.float32 or poses0.dim() != 2 or poses0.shape[1] != 12 or not poses0.is_contiguous():
            raise TypeError("ray_camera_grad: poses are float32 [n,12], contiguous")
    else:
        _pose_pair(poses0, xi, "ray_camera_grad")
        xi = xi.detach()
    n, dev = poses0.shape[0], poses0.device
    K, k_rows = _camera_table(K, n, "ray_camera_grad")
    index, grad_o, grad_d, count = _ray_grads(index, grad_o, grad_d)
    want_xi_grad = xi is not None if want_xi_grad is None else want_xi_grad
    grad_xi = torch.empty(n, 6, device=dev, dtype=torch.float32) if want_xi_grad else None
    grad_K = torch.empty(n, 4, device=dev, dtype=torch.float32)
    _launch("fsn_ray_camera_grad", dev, poses0, xi, n, int(H), int(W), float(focal0), K, k_rows, 1 if ndc else 0, float(near),
            index, grad_o, grad_d, count, grad_xi, grad_K)
    return grad_xi, grad_K


def intrinsics_grad(phi: Tensor, grad_K_views: Tensor, H: int, W: int, focal0: float, tie_focal: bool = True) -> Tensor:
    """dL/dphi [m,4] from ray_camera_grad's per-view dL/dK [n,4] in ONE launch (fsn_intrinsics_grad): the chain K -> phi
    and, for a shared row (m = 1), the sum over the views in float64 in a fixed order."""
    phi = _phi(phi, "intrinsics_grad")
    g = _gpu_f32(grad_K_views, "grad_K_views")
    if g.dim() != 2 or g.shape[1] != 4 or phi.shape[0] not in (1, g.shape[0]) or g.device != phi.device:
        raise ValueError(f"intrinsics_grad: grad_K_views is [n,4] and phi [1 or n,4] on one device, got {tuple(g.shape)} "
                         f"and {tuple(phi.shape)}")
    out = torch.empty_like(phi)
    _launch("fsn_intrinsics_grad", phi.device, phi, g, g.shape[0], phi.shape[0], int(H), int(W), float(focal0),
            1 if tie_focal else 0, out)
    return out


def to_ndc(rays_o: Tensor, rays_d: Tensor, H: int, W: int, focal: float, near: float) -> Tuple[Tensor, Tensor]:
    o, d = _f32(rays_o, "rays_o"), _f32(rays_d, "rays_d")
    n = o.numel() // 3
    no, nd = torch.empty_like(o), torch.empty_like(d)
    _launch("fsn_to_ndc", o.device, o, d, n, H, W, float(focal), float(near), no, nd)
    return no, nd


def posenc(x: Tensor, freqs: Sequence[float], mask: Optional[Tensor] = None) -> Tensor:
    x = _f32(x, "x")
    d_in = x.shape[-1]
    n = x.numel() // d_in
    nf = len(freqs)
    out = torch.empty(*x.shape[:-1], d_in * (1 + 2 * nf), device=x.device, dtype=torch.float32)
    fr = (C.c_float * max(nf, 1))(*[float(f) for f in freqs])
    m = _opt_f32(mask, "mask")
    _launch("fsn_posenc_fwd", x.device, x, n, d_in, nf, fr, m, out)
    return out


# ------------------------------------------------------------------ sampling
def _u_mode(u: Optional[Tensor], R: int, S: int) -> Tuple[int, Optional[Tensor]]:
    if u is None:
        return 0, None
    u = _f32(u, "u")
    if u.numel() == R:
        return 1, u
    if tuple(u.shape) == (R, S + 1):
        return 2, u
    raise ValueError(f"jitter u must have {R} or {R}x{S + 1} elements, got {tuple(u.shape)}")


def stratified_edges(near: float, far: float, S: int, R: int, u: Optional[Tensor], device) -> Tensor:
    mode, u = _u_mode(u, R, S)
    edges = torch.empty(R, S + 1, device=device, dtype=torch.float32)
    _launch("fsn_stratified_edges", edges.device, float(near), float(far), S, R, u, mode, edges)
    return edges


def edges_to_packed(edges: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    edges = _f32(edges, "edges")
    R, S = edges.shape[0], edges.shape[1] - 1
    ri = torch.empty(R * S, device=edges.device, dtype=torch.int64)
    t0 = torch.empty(R * S, device=edges.device, dtype=torch.float32)
    t1 = torch.empty_like(t0)
    _launch("fsn_edges_to_packed", edges.device, edges, R, S, ri, t0, t1)
    return ri, t0, t1


def sample_pdf_merge(edges: Tensor, weights: Tensor, n_imp: int, u: Optional[Tensor] = None) -> Tensor:
    edges, weights = _f32(edges, "edges"), _f32(weights, "weights")
    R, S = weights.shape
    assert edges.shape == (R, S + 1)
    u = _opt_f32(u, "u")
    out = torch.empty(R, S + 1 + n_imp, device=edges.device, dtype=torch.float32)
    _launch("fsn_sample_pdf_merge", edges.device, edges, weights, R, S, n_imp, u, out)
    return out


# ------------------------------------------------------------------ compositing
def composite(sigmas: Tensor, rgbs: Tensor, t_starts: Tensor, t_ends: Tensor, bkgd=None, extras: bool = True):
    """Dense [R,S] volume integration.  Returns colors [R,3], opacity [R,1], depth [R,1], extras."""
    sig, rgb = _f32(sigmas, "sigmas"), _f32(rgbs, "rgbs")
    t0, t1 = _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends")
    R, S = sig.shape
    dev = sig.device
    colors = torch.empty(R, 3, device=dev)
    opacity = torch.empty(R, 1, device=dev)
    depth = torch.empty(R, 1, device=dev)
    w = torch.empty(R, S, device=dev) if extras else None
    a = torch.empty(R, S, device=dev) if extras else None
    tr = torch.empty(R, S, device=dev) if extras else None
    _launch("fsn_composite_fwd", dev, sig, rgb, t0, t1, R, S, _bk(bkgd), colors, opacity, depth, w, a, tr)
    ex = {"weights": w, "alphas": a, "trans": tr, "sigmas": sig, "rgbs": rgb} if extras else {}
    return colors, opacity, depth, ex


def composite_packed(sigmas: Tensor, rgbs: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor,
                     n_rays: int, bkgd=None):
    sig, rgb = _f32(sigmas, "sigmas"), _f32(rgbs, "rgbs")
    t0, t1 = _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends")
    ri = _i64(ray_indices, "ray_indices")
    N = sig.numel()
    dev = t0.device
    colors = torch.empty(n_rays, 3, device=dev)
    opacity = torch.empty(n_rays, 1, device=dev)
    depth = torch.empty(n_rays, 1, device=dev)
    w, a, tr = (torch.empty(N, device=dev) for _ in range(3))
    _launch("fsn_composite_packed_fwd", dev, sig, rgb, t0, t1, ri, N, n_rays, _bk(bkgd), colors, opacity, depth, w, a, tr)
    return colors, opacity, depth, {"weights": w, "alphas": a, "trans": tr, "sigmas": sig, "rgbs": rgb}


# ------------------------------------------------------------------ MLP
SD_ORDER_TAIL = ("sigma", "connection", "branch", "rgb")


def _device_word(cache: Dict[torch.device, Tensor], device) -> Tensor:
    """One zero-initialised int32 word per GPU in `cache`, made on first use."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    w = cache.get(device)
    if w is None:
        w = cache[device] = torch.zeros(1, dtype=torch.int32, device=device)
    return w


# Range guard of the fp16 modes (include/fsnerf_hip.h, FSN_STATUS_FP16_RANGE): one sticky device word per GPU that
# every MLP launch of this process reports into.
_status_words: Dict[torch.device, Tensor] = {}
_step_flags: Dict[torch.device, Tensor] = {}


def status_word(device) -> Tensor:
    return _device_word(_status_words, device)


def step_flag(device) -> Tensor:
    """Per-device word of the current training step for parameters that NO gradient bucket owns (plain torch
    optimizers): a NeRF backward ORs its per-call range word into it (device op).  Parameters in a `shard.FlatGrads`
    bucket (`FusedAdam`) report into the bucket's own `step_flag` instead, which that optimizer hands to its
    Adam launch (bit 0 / bit 2 set: the update is skipped on the device) and clears.  Never read by the host."""
    return _device_word(_step_flags, device)


def range_flags(device) -> int:
    """FSN_STATUS_* bits reported by the launches since the last call (0 = all inside the fp16 modes' envelope); the
    word is cleared.  Reads 4 bytes back: one host sync."""
    w = status_word(device)
    bits = int(w.item()) & (L.FSN_STATUS_FP16_RANGE | L.FSN_STATUS_FP16_SMALL)
    if bits:
        w.zero_()
    return bits


# Deferred look at the range word (`NeRF.range_check = "deferred"`): batch rendering in small launches must not wait for
# the GPU after every call.  range_post(): asynchronous copy of the word into pinned host memory + an event, on the
# launch stream.  range_poll(): bits seen by the most recent post (waits for its event - normally long complete when the
# NEXT call polls), clearing the device word when it was raised.
_range_pending: Dict[torch.device, Tuple[Tensor, "torch.cuda.Event"]] = {}


def range_post(device) -> None:
    w = status_word(device)
    ent = _range_pending.get(w.device)
    host = ent[0] if ent is not None else torch.zeros(1, dtype=torch.int32).pin_memory()
    host.copy_(w, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    _range_pending[w.device] = (host, ev, True)


def range_poll(device) -> int:
    w = status_word(device)
    ent = _range_pending.get(w.device)
    if ent is None or not ent[2]:
        return 0
    host, ev, _ = ent
    ev.synchronize()
    _range_pending[w.device] = (host, ev, False)
    bits = int(host[0]) & (L.FSN_STATUS_FP16_RANGE | L.FSN_STATUS_FP16_SMALL)
    if bits:
        w.zero_()
    return bits


def range_ok(device) -> bool:
    """False when a launch since the last call reported values outside the fp16 modes' envelope (either end)."""
    return range_flags(device) == 0


def describe_flags(bits: int) -> str:
    what = []
    if bits & L.FSN_STATUS_FP16_RANGE:
        what.append("values reached the top of the fp16 range (|v| >= 65504)")
    if bits & L.FSN_STATUS_FP16_SMALL:
        what.append("a layer's activations were all below 2^-14 (below the split's float32-grade envelope; scaled "
                    "inference: a wavefront's layer maximum below 2^-4)")
    return " and ".join(what) if what else "inside the envelope"



def make_desc(n_layers: int, d_hidden: int, skip: Sequence[int], freqs_pos: Sequence[float],
              freqs_dir: Sequence[float]) -> L.MlpDesc:
    d = L.MlpDesc()
    d.n_layers, d.d_hidden = n_layers, d_hidden
    mask = 0
    for i in skip:
        if 0 <= i < n_layers - 1:
            mask |= 1 << i
        elif i == n_layers - 1:
            raise ValueError(f"skip index {i} == n_layers-1: the reference model cannot run this either "
                             "(sigma expects d_hidden inputs, src/core/models.py:107,123)")
    d.skip_mask = mask
    d.n_freqs_pos, d.n_freqs_dir = len(freqs_pos), len(freqs_dir)
    if len(freqs_pos) > 16 or len(freqs_dir) > 16:
        raise ValueError("too many frequency bands")
    for i, f in enumerate(freqs_pos):
        d.freqs_pos[i] = float(f)
    for i, f in enumerate(freqs_dir):
        d.freqs_dir[i] = float(f)
    return d


def sd_tensor_lists(sd: Dict[str, Tensor], n_layers: int) -> Tuple[List[Tensor], List[Tensor]]:
    names = [f"layers.{i}" for i in range(n_layers)] + list(SD_ORDER_TAIL)
    return [sd[n + ".weight"] for n in names], [sd[n + ".bias"] for n in names]


class PackedMLP:
    """A reference-format state_dict packed for the MFMA kernels (device blob + descriptor)."""

    def __init__(self, desc: L.MlpDesc, prec: int, device):
        self.desc, self.prec = desc, prec
        self.blob = torch.empty(_size("fsn_mlp_blob_bytes", None, C.byref(desc), prec), dtype=torch.uint8, device=device)

    def pack(self, weights: Sequence[Tensor], biases: Sequence[Tensor], exps: Optional[Sequence[int]] = None) -> "PackedMLP":
        """`exps`: n_layers + 2 per-GEMM activation exponents (fsn_mlp_pack_scaled: the blob then holds the network whose
        GEMM g produces 2^exps[g] times the reference's activations, heads unscaled accordingly), or None."""
        n = self.desc.n_layers + 4
        assert len(weights) == n and len(biases) == n
        ws = [_f32(w.detach(), "weight") for w in weights]
        bs = [_f32(b.detach(), "bias") for b in biases]
        ex = None
        if exps is not None:
            assert len(exps) == self.desc.n_layers + 2
            ex = (C.c_int32 * len(exps))(*[int(e) for e in exps])
        self.exps = None if exps is None else tuple(int(e) for e in exps)
        _launch("fsn_mlp_pack_scaled", self.blob.device, C.byref(self.desc), self.prec, _ptr_array(ws), _ptr_array(bs), ex,
                self.blob)
        self._keep = (ws, bs)  # alive until the stream work is queued behind later launches
        return self


def mlp_layer_maxima(pm: PackedMLP, x: Tensor, dirs: Tensor, pos_mask: Optional[Tensor] = None,
                     dir_mask: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """Per-GEMM largest |activation| of NeRF.forward(x, dirs) over the probe samples (fsn_mlp_layer_maxima) ->
    float32 [n_layers + 2] on the device, in the scale of the blob `pm`.  `out`: accumulate into an earlier result."""
    x, d = _f32(x, "x").reshape(-1, 3), _f32(dirs, "dirs").reshape(-1, 3)
    assert x.shape == d.shape
    pmk, dmk = _opt_f32(pos_mask, "pos_mask"), _opt_f32(dir_mask, "dir_mask")
    if out is None:
        out = torch.zeros(pm.desc.n_layers + 2, device=x.device, dtype=torch.float32)
    _launch("fsn_mlp_layer_maxima", x.device, C.byref(pm.desc), pm.prec, pm.blob, x, d, pmk, dmk, x.shape[0], out)
    return out


def mlp_fwd(pm: PackedMLP, x: Tensor, dirs: Optional[Tensor] = None, pos_mask: Optional[Tensor] = None,
            dir_mask: Optional[Tensor] = None) -> Tensor:
    x = _f32(x, "x")
    lead = x.shape[:-1]
    n = x.numel() // 3
    d = _opt_f32(dirs, "dirs")
    pmk, dmk = _opt_f32(pos_mask, "pos_mask"), _opt_f32(dir_mask, "dir_mask")
    out = torch.empty(*lead, 4 if d is not None else 1, device=x.device, dtype=torch.float32)
    _launch("fsn_mlp_fwd", x.device, C.byref(pm.desc), pm.prec, pm.blob, x, d, pmk, dmk, n, out, status_word(x.device))
    return out


def mlp_fwd_rays(pm: PackedMLP, rays_o: Tensor, rays_d: Tensor, ray_indices: Tensor, t_starts: Tensor, t_ends: Tensor,
                 full: bool, pos_mask: Optional[Tensor] = None, dir_mask: Optional[Tensor] = None) -> Tensor:
    """NeRF.forward on the midpoints of packed intervals (the reference's sigma_fn / rgb_sigma_fn, rendering.py:58-64,
    76-84) without materialising the gathered [N,3] positions / directions: -> [N,4] (full) or [N,1]."""
    o, d = _f32(rays_o, "rays_o"), _f32(rays_d, "rays_d")
    ri, t0, t1 = _i64(ray_indices, "ray_indices"), _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends")
    n = ri.numel()
    pmk, dmk = _opt_f32(pos_mask, "pos_mask"), _opt_f32(dir_mask, "dir_mask")
    out = torch.empty(n, 4 if full else 1, device=o.device, dtype=torch.float32)
    _launch("fsn_mlp_fwd_rays", o.device, C.byref(pm.desc), pm.prec, pm.blob, o, d, ri, t0, t1, 1 if full else 0, pmk, dmk, n,
            out, status_word(o.device))
    return out


_edges_ws: Dict[Tuple[torch.device, int], Tensor] = {}


def _edges_workspace(dev, n: int) -> Tensor:
    """Hand-over buffer of the two-phase frame mode when the caller does not ask for the edges: one cached tensor per
    device (grown on demand), so that a path of frames does not re-allocate 0.5 GB per frame."""
    dev = torch.device(dev)
    w = _edges_ws.get((dev, 0))
    if w is None or w.numel() < n:
        w = _edges_ws[(dev, 0)] = torch.empty(n, device=dev, dtype=torch.float32)
    return w


def _render_args(rays_o: Optional[Tensor], rays_d: Optional[Tensor], camera, near: float, far: float, S: int, NI: int,
                 u: Optional[Tensor], u_fine: Optional[Tensor], pos_mask: Optional[Tensor],
                 dir_mask: Optional[Tensor]) -> Tuple[_Held, int, torch.device]:
    """The inputs of fsn_render_rays_fused (rays or camera, range, jitter, masks) -> (held RenderArgs, R, device)."""
    h = _Held(L.RenderArgs())
    a = h.a
    R, dev = _ray_source(h, rays_o, rays_d, camera)
    mode, u = _u_mode(u, R, S)
    a.near, a.far, a.S, a.n_imp, a.u_mode = float(near), float(far), S, NI, mode
    h.set("u", u)
    if u_fine is not None:
        u_fine = _f32(u_fine, "u_fine")
        assert tuple(u_fine.shape) == (R, NI)
        h.set("u_fine", u_fine)
    _masks(h, pos_mask, dir_mask)
    return h, R, dev


def render_fused(pm_coarse: Optional[PackedMLP], pm_fine: PackedMLP, rays_o: Optional[Tensor], rays_d: Optional[Tensor], *,
                 near: float, far: float, n_samples: int, n_importance: int = 0, u: Optional[Tensor] = None,
                 u_fine: Optional[Tensor] = None, bkgd=(0.0, 0.0, 0.0), pos_mask: Optional[Tensor] = None,
                 dir_mask: Optional[Tensor] = None, want_extras: bool = True, camera=None,
                 two_phase: Optional[bool] = None):
    """One launch for the whole path (fsn_render_rays_fused).  Returns colors [R,3], opacity [R,1],
    depth [R,1], extras {weights, alphas, trans, sigmas [R,S'], rgbs [R,S',3], edges [R,S'+1],
    weights_coarse [R,S] (hierarchical only)}.
    `camera` = (pose [3or4,4], H, W, focal, row0, nrows, device) instead of ray tensors: the rays of the image rows
    [row0, row0+nrows) are generated inside the launch (the arithmetic of get_rays), R = nrows*W.
    `two_phase` (default: hierarchical launches of >= 65,536 rays): all coarse passes of a workgroup before its fine
    passes, the resampled edges handed over through HBM (its own kernel instantiation: two simple loops instead of
    one long one, half the register spills); same results, 3 % faster on the 800x800 frame (A/B on one device)."""
    S, NI = n_samples, n_importance
    So = S + NI
    h, R, dev = _render_args(rays_o, rays_d, camera, near, far, S, NI, u, u_fine, pos_mask, dir_mask)
    a = h.a
    for i in range(3):
        a.bkgd[i] = float(bkgd[i])
    colors = torch.empty(R, 3, device=dev)
    opacity = torch.empty(R, 1, device=dev)
    depth = torch.empty(R, 1, device=dev)
    ex: Dict[str, Tensor] = {}
    if want_extras:
        for k, shape in (("weights", (R, So)), ("alphas", (R, So)), ("trans", (R, So)), ("sigmas", (R, So)),
                         ("rgbs", (R, So, 3))):
            ex[k] = torch.empty(*shape, device=dev)
        ex["edges"] = torch.empty(R, So + 1, device=dev)
        if NI > 0:
            ex["weights_coarse"] = torch.empty(R, S, device=dev)
    for k, t in (("colors", colors), ("opacity", opacity), ("depth", depth), *ex.items()):
        h.set("edges_out" if k == "edges" else k, t)
    if two_phase is None:
        two_phase = NI > 0 and R >= 65536
    if two_phase and NI > 0:
        if "edges" not in ex:
            h.set("edges_out", _edges_workspace(dev, R * (So + 1)))
        a.two_phase = 1
    if NI > 0 and pm_coarse is None:
        pm_coarse = pm_fine
    if pm_coarse is not None and pm_coarse.prec != pm_fine.prec:
        raise ValueError("render_fused: the coarse and the fine network must be packed in the same precision mode")
    h.set("status", status_word(dev))
    h.set("clock_out", clock_buffer)
    _launch("fsn_render_rays_fused", dev, C.byref(pm_fine.desc), pm_fine.prec,
            pm_coarse.blob if pm_coarse is not None else None, pm_fine.blob, C.byref(a), timed=True)
    return colors, opacity, depth, ex


def bench_bare_stream(pm: PackedMLP, layers: int) -> Tuple[int, Tensor]:
    """Measurement aid (fsn_bench_bare_stream): `layers` 256 -> 256 hidden layers back to back per workgroup through the
    render kernels' own GEMM code, the weight stream walking the hidden phases of `pm`'s blob.  -> (workgroups launched,
    uint64 [workgroups * 8, 2] per-wave (s_memtime, s_memrealtime) differences around the loop)."""
    dev = pm.blob.device
    clk = torch.zeros(max(_size("fsn_device_cus", dev), 1) * 8, 2, dtype=torch.int64, device=dev)
    n = _launch("fsn_bench_bare_stream", dev, C.byref(pm.desc), pm.prec, pm.blob, int(layers), clk, counts=True)
    return n, clk


def sample_fused(pm_coarse: PackedMLP, rays_o: Tensor, rays_d: Tensor, *, near: float, far: float, n_samples: int,
                 n_importance: int, u: Optional[Tensor] = None, u_fine: Optional[Tensor] = None,
                 pos_mask: Optional[Tensor] = None, dir_mask: Optional[Tensor] = None,
                 want_weights: bool = False, status: Optional[Tensor] = None):
    """The hierarchical sampler as ONE launch (fsn_render_rays_fused with two_phase = 2): stratified edges -> density
    pass of `pm_coarse` -> weights -> inverse-CDF resampling -> sorted union.  -> edges [R, S+NI+1] (and the coarse
    weights [R,S] when asked for): what StratifiedEstimator.sampling builds from five launches around a sigma_fn."""
    S, NI = n_samples, n_importance
    if NI <= 0:
        raise ValueError("sample_fused: hierarchical sampling only (n_importance > 0)")
    h, R, dev = _render_args(rays_o, rays_d, None, near, far, S, NI, u, u_fine, pos_mask, dir_mask)
    a = h.a
    edges = torch.empty(R, S + NI + 1, device=dev)
    wc = torch.empty(R, S, device=dev) if want_weights else None
    h.set("edges_out", edges)
    h.set("weights_coarse", wc)
    a.two_phase = 2
    h.set("status", status_word(dev) if status is None else status)  # `status`: a per-call word (training steps)
    if R > 0:
        _launch("fsn_render_rays_fused", dev, C.byref(pm_coarse.desc), pm_coarse.prec, pm_coarse.blob, None, C.byref(a))
    return (edges, wc) if want_weights else edges


# ------------------------------------------------------------------ "next" rows
class _OcclusionRegFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sig, t, ri, n_rays, a, b, func):
        N = sig.numel()
        sums = torch.empty(max(n_rays, 1), device=sig.device, dtype=torch.float32)
        out = torch.empty(1, device=sig.device, dtype=torch.float32)
        _launch("fsn_occlusion_reg_fwd", sig.device, sig, t, ri, N, n_rays, float(a), float(b), func, sums, out)
        ctx.save_for_backward(t, sums)
        ctx.cfg = (N, n_rays, float(a), float(b), func)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        t, sums = ctx.saved_tensors
        N, n_rays, a, b, func = ctx.cfg
        d_sig = torch.zeros(N, device=t.device, dtype=torch.float32)
        cnt = torch.empty(1, device=t.device, dtype=torch.int32)
        g = _f32(g, "grad").reshape(1)
        _launch("fsn_occlusion_reg_bwd", t.device, t, N, sums, n_rays, a, b, func, g, cnt, d_sig)
        return d_sig, None, None, None, None, None, None


def occlusion_reg(sigmas: Tensor, t_vals: Tensor, ray_idxs: Tensor, a: float, b: float, func: str = "linear",
                  n_rays: Optional[int] = None) -> Tensor:
    """OcclusionRegularizer (src/core/loss.py:26-60) -> 0-dim tensor; differentiable w.r.t. sigmas."""
    sig, t = _f32(sigmas, "sigmas").reshape(-1), _f32(t_vals.detach(), "t_vals").reshape(-1)
    ri = ray_idxs.contiguous()
    if ri.dtype != torch.int64:
        ri = ri.long()
    N = sig.numel()
    if n_rays is None:
        n_rays = int(ri[-1].item()) + 1 if N > 0 else 0
    if func not in ("linear", "exp"):
        raise ValueError(f"Unknown occlusion regularizer type: {func}")
    return _OcclusionRegFn.apply(sig, t, ri, n_rays, a, b, 0 if func == "linear" else 1)


def to8b(x: Tensor) -> Tensor:
    """(255 * clip(x, 0, 1)).astype(uint8) on the device (src/render/rendering.py:21)."""
    x = _f32(x, "x")
    out = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
    _launch("fsn_to8b", x.device, x, x.numel(), out)
    return out


_lut_cache: Dict[Tuple[str, torch.device], Tensor] = {}


def video_tensors(frames: Tensor, d_frames: Tensor, cmap: str = "plasma") -> Tuple[Tensor, Tensor]:
    """render_video (src/render/rendering.py:240-266) on the device: frames [N,H,W,3], d_frames [N,H,W] ->
    (uint8 [N,3,H,W], uint8 [N,3,H,W]): to8b + NHWC->NCHW for the colour frames; global min / max normalisation,
    colormap lookup and to8b for the depth frames."""
    from .render.cmaps import TABLES
    if cmap not in TABLES:
        raise ValueError(f"render_video: colormap {cmap!r} is not in the shipped tables {sorted(TABLES)}")
    fr, dp = _f32(frames, "frames"), _f32(d_frames, "d_frames")
    N, H, W = dp.shape
    assert fr.shape == (N, H, W, 3)
    dev = fr.device
    key = (cmap, dev)
    if key not in _lut_cache:
        _lut_cache[key] = torch.frombuffer(bytearray(TABLES[cmap]), dtype=torch.uint8).to(dev)
    out_f = torch.empty(N, 3, H, W, device=dev, dtype=torch.uint8)
    out_d = torch.empty(N, 3, H, W, device=dev, dtype=torch.uint8)
    if N * H * W == 0:
        return out_f, out_d
    vmm = torch.stack(torch.aminmax(dp)).to(torch.float32).contiguous()  # np.amin / np.amax over ALL frames
    _launch("fsn_to8b_nchw", dev, fr, N, H * W, out_f)
    _launch("fsn_depth_colormap", dev, dp, N, H * W, vmm, _lut_cache[key], out_d)
    return out_f, out_d


# ------------------------------------------------------------------ training step
def _ptr_array(ts: Sequence[Tensor]):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _nerf_train_fwd(name: str, desc: L.MlpDesc, prec: int, weights, biases, inputs: Sequence[Tensor], n: int, pos_mask,
                    dir_mask, status):
    """Both forms of the training forward: `inputs` are the converted sample arguments of `name`, in its order."""
    dev = inputs[0].device
    ws_ = [_f32(w.detach(), "weight") for w in weights]
    bs_ = [_f32(b.detach(), "bias") for b in biases]
    pm, dm = _opt_f32(pos_mask, "pos_mask"), _opt_f32(dir_mask, "dir_mask")
    out = torch.empty(n, 4, device=dev, dtype=torch.float32)
    nfl = _size("fsn_nerf_train_workspace_floats", dev, C.byref(desc), prec, n)
    work = torch.empty(max(nfl, 1), device=dev, dtype=torch.float32)
    _launch(name, dev, C.byref(desc), prec, _ptr_array(ws_), _ptr_array(bs_), *inputs, pm, dm, n, work, out, status)
    return out, work


def nerf_train_fwd_rays(desc: L.MlpDesc, prec: int, weights: Sequence[Tensor], biases: Sequence[Tensor], rays_o: Tensor,
                        rays_d: Tensor, ray_indices: Tensor, t_starts: Tensor, t_ends: Tensor, pos_mask: Optional[Tensor],
                        dir_mask: Optional[Tensor], status: Optional[Tensor] = None):
    """nerf_train_fwd with the samples in ray form (midpoints of packed intervals): -> (out [n,4], workspace)."""
    o, d = _f32(rays_o, "rays_o"), _f32(rays_d, "rays_d")
    ri, t0, t1 = _i64(ray_indices, "ray_indices"), _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends")
    return _nerf_train_fwd("fsn_nerf_train_fwd_rays", desc, prec, weights, biases, (o, d, ri, t0, t1), ri.numel(), pos_mask,
                           dir_mask, status)


def nerf_train_fwd(desc: L.MlpDesc, prec: int, weights: Sequence[Tensor], biases: Sequence[Tensor], x: Tensor,
                   dirs: Tensor, pos_mask: Optional[Tensor], dir_mask: Optional[Tensor], status: Optional[Tensor] = None):
    """NeRF.forward keeping what the backward needs: -> (out [n,4], workspace).  prec: L.FSN_PREC_*.  `status`: this
    call's range-guard word (int32[1], zeroed by the caller; the same tensor goes to nerf_train_bwd)."""
    x, d = _f32(x, "x").reshape(-1, 3), _f32(dirs, "dirs").reshape(-1, 3)
    return _nerf_train_fwd("fsn_nerf_train_fwd", desc, prec, weights, biases, (x, d), x.shape[0], pos_mask, dir_mask, status)


def grad_scale_for(d_out: Tensor) -> Tensor:
    """Power of two that brings max|d_out| to ~2^10 (device scalar, no host sync): the fp16 MFMA modes of the
    backward multiply d_out by it on entry and divide the gradients by it at the end.  One launch (fsn_grad_scale):
    2^clamp(floor(log2(1024 / max|d_out|)), -40, 60), 1 when the maximum is 0 / inf / NaN."""
    d = _f32(d_out.detach(), "d_out").reshape(-1)
    buf = torch.zeros(4, dtype=torch.float32, device=d.device)
    _launch("fsn_grad_scale", d.device, d, d.numel(), buf)
    return buf[:1]


def _check_into(into, ws_):
    """`into` = (weight .grad buffers, bias .grad buffers) of nerf_train_bwd -> (d_weights, flat d_biases), validated."""
    for g in list(into[0]) + list(into[1]):
        if not (g.is_cuda and g.dtype == torch.float32 and g.is_contiguous()):
            raise ValueError("nerf_train_bwd: `into` buffers must be contiguous float32 GPU tensors (they are written in place)")
    dW, db = list(into[0]), [g.view(-1) for g in into[1]]
    if len(dW) != len(ws_) or len(db) != len(ws_) or any(g.shape != w.shape for g, w in zip(dW, ws_)) or \
            any(g.numel() != w.shape[0] for g, w in zip(db, ws_)):
        raise ValueError("nerf_train_bwd: `into` must hold one gradient buffer per weight / bias, of its shape")
    return dW, db


def _grad_buffers(ws_, n: int, into, prec: int, d_out: Tensor, param_grads: bool = True):
    """-> (d_weights, d_biases, scale) of a training backward over n samples: `into` validated, else fresh buffers (zeros
    at n == 0, where nothing is launched; both None without `param_grads`), and the fp16 modes' loss scale."""
    if not param_grads:
        if into is not None:
            raise ValueError("nerf_train_bwd_inputs: `into` needs param_grads")
        dW = db = None
    elif into is not None:
        dW, db = _check_into(into, ws_)
    elif n == 0:  # e.g. the all-background first batch of an empty occupancy grid (run-nerf.py:243 precedes :293)
        dW, db = [torch.zeros_like(w) for w in ws_], [torch.zeros(w.shape[0], device=w.device) for w in ws_]
    else:
        dW = [torch.empty_like(w) for w in ws_]
        db = [torch.empty(w.shape[0], device=w.device, dtype=torch.float32) for w in ws_]
    scale = grad_scale_for(d_out) if n > 0 and prec in (L.FSN_PREC_FP16X3, L.FSN_PREC_FP16) else None
    return dW, db, scale


def nerf_train_bwd(desc: L.MlpDesc, prec: int, weights: Sequence[Tensor], work: Tensor, out: Tensor, d_out: Tensor,
                   status: Optional[Tensor] = None, into: Optional[Tuple[Sequence[Tensor], Sequence[Tensor]]] = None,
                   stage_state: Optional[Tuple[Tensor, Tensor]] = None):
    """-> (d_weights, d_biases) lists in state_dict order.  `status`: the word given to nerf_train_fwd.
    `into` = (weight .grad buffers, bias .grad buffers): the gradients are ADDED to them on the device (what autograd's
    AccumulateGrad does with returned tensors, without the temporaries and one add launch per parameter); -> into.
    `stage_state` = (scales float32 [n_layers + 2], maxima int32 [n_layers + 2]), fp16 modes: the backward chain's delayed
    per-stage power-of-two factors (include/fsnerf_hip.h); the call uses the scales and updates them for the next one."""
    ws_ = [_f32(w.detach(), "weight") for w in weights]
    d_out = _f32(d_out, "d_out").reshape(-1, 4)
    n = d_out.shape[0]
    dW, db, scale = _grad_buffers(ws_, n, into, prec, d_out)
    if n == 0:
        return dW, db
    _launch("fsn_nerf_train_bwd", work.device, C.byref(desc), prec, _ptr_array(ws_), n, work, out, d_out, scale,
            _ptr_array(dW), _ptr_array(db), 0 if into is None else 1, stage_state[0] if stage_state else None,
            stage_state[1] if stage_state else None, status)
    return dW, db


def nerf_train_bwd_inputs(desc: L.MlpDesc, prec: int, weights: Sequence[Tensor], work: Tensor, out: Tensor, d_out: Tensor, *,
                          x: Optional[Tensor] = None, dirs: Optional[Tensor] = None,
                          rays: Optional[Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]] = None,
                          pos_mask: Optional[Tensor] = None, dir_mask: Optional[Tensor] = None, want_x: bool = True,
                          want_dirs: bool = True, param_grads: bool = True, status: Optional[Tensor] = None,
                          into: Optional[Tuple[Sequence[Tensor], Sequence[Tensor]]] = None,
                          stage_state: Optional[Tuple[Tensor, Tensor]] = None):
    """nerf_train_bwd plus the gradients of the network's inputs (fsn_nerf_train_bwd_inputs) -> (d_weights, d_biases,
    d_x, d_dirs).  The forward's inputs are handed in again: `x` and `dirs`, or `rays` = (rays_o, rays_d, ray_indices,
    t_starts, t_ends), with its `pos_mask` / `dir_mask`.  d_x / d_dirs: per-SAMPLE float32 [n,3] gradients of the
    positions / directions (None where not wanted; the ray form's per-ray sums are `ray_grad_reduce`).
    `param_grads=False`: a frozen network - the dgrad chain and the input gradient only, no weight-gradient launches,
    d_weights = d_biases = None (with neither `want_x` nor `want_dirs`: the chain alone, which still moves `stage_state`).
    `status`, `into`, `stage_state` as in nerf_train_bwd; the parameter gradients are those of nerf_train_bwd bit for bit."""
    if (rays is None) == (x is None) or (rays is None and dirs is None):
        raise ValueError("nerf_train_bwd_inputs: give x and dirs, or rays")
    ws_ = [_f32(w.detach(), "weight") for w in weights]
    d_out = _f32(d_out, "d_out").reshape(-1, 4)
    n = d_out.shape[0]
    dev = d_out.device
    if rays is not None:
        o, d, ri, t0, t1 = rays
        src = (None, None, _f32(o.detach(), "rays_o"), _f32(d.detach(), "rays_d"), _i64(ri, "ray_indices"),
               _f32(t0, "t_starts"), _f32(t1, "t_ends"))
        n_in = src[4].numel()
    else:
        src = (_f32(x.detach(), "x").reshape(-1, 3), _f32(dirs.detach(), "dirs").reshape(-1, 3), None, None, None, None, None)
        n_in = src[0].shape[0] if src[0].shape[0] == src[1].shape[0] else -1
    if n_in != n:
        raise ValueError("nerf_train_bwd_inputs: the inputs are not the forward's samples")
    # (the kernel writes every row of a call with samples; a call without samples launches nothing)
    d_x = torch.empty(n, 3, device=dev, dtype=torch.float32) if want_x else None
    d_dirs = torch.empty(n, 3, device=dev, dtype=torch.float32) if want_dirs else None
    dW, db, scale = _grad_buffers(ws_, n, into, prec, d_out, param_grads)
    if n == 0:
        return dW, db, d_x, d_dirs
    pm, dm = _opt_f32(pos_mask, "pos_mask"), _opt_f32(dir_mask, "dir_mask")
    _launch("fsn_nerf_train_bwd_inputs", work.device, C.byref(desc), prec, _ptr_array(ws_), n, work, out, d_out, scale,
            _ptr_array(dW) if param_grads else None, _ptr_array(db) if param_grads else None, 0 if into is None else 1,
            stage_state[0] if stage_state else None, stage_state[1] if stage_state else None, status, *src, pm, dm, d_x,
            d_dirs)
    return dW, db, d_x, d_dirs


def ray_grad_reduce(d_x: Optional[Tensor], d_dirs: Optional[Tensor], ray_indices: Tensor, t_starts: Tensor, t_ends: Tensor,
                    n_rays: int, want_o: bool = True, want_d: bool = True) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """The ray form's reduction of per-sample input gradients (fsn_ray_grad_reduce): d_rays_o[r] = sum d_x, d_rays_d[r] =
    sum ((t0 + t1) / 2 d_x + d_dirs) over ray r's samples -> ([n_rays,3] or None, [n_rays,3] or None).  One wave per ray,
    fixed order: deterministic; rays without samples get zeros."""
    ri, t0, t1 = _i64(ray_indices, "ray_indices"), _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends")
    n = ri.numel()
    dev = ri.device
    d_x, d_dirs = _opt_f32(d_x, "d_x"), _opt_f32(d_dirs, "d_dirs")
    for g in (d_x, d_dirs):
        if g is not None and tuple(g.shape) != (n, 3):
            raise ValueError("ray_grad_reduce: d_x / d_dirs must be [n_samples, 3]")
    d_o = torch.empty(n_rays, 3, device=dev, dtype=torch.float32) if want_o else None
    d_d = torch.empty(n_rays, 3, device=dev, dtype=torch.float32) if want_d else None
    _launch("fsn_ray_grad_reduce", dev, d_x, d_dirs, ri, t0, t1, n, n_rays, d_o, d_d)
    return d_o, d_d


def _composite_bwd(lean, sigmas, rgbs, t_starts, t_ends, ray_indices, n_rays, bkgd, d_colors, d_opacity, opacity=None,
                   depth=None, d_depth=None, d_weights=None, d_alphas=None, d_trans=None):
    """Both forms of the compositor's backward: `lean` calls fsn_composite_packed_bwd, which takes the first two
    cotangents only; the kernel behind the two entry points is the same one."""
    sig, rgb = _f32(sigmas, "sigmas"), _f32(rgbs, "rgbs")
    t0, t1 = _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends")
    ri = _i64(ray_indices, "ray_indices")
    N = sig.numel()
    dc = _flat(d_colors, "d_colors", 3 * n_rays, cast=True)
    dop, op, dep, dd = (_flat(t, name, n_rays, cast=True) for t, name in ((d_opacity, "d_opacity"), (opacity, "opacity"),
                                                                          (depth, "depth"), (d_depth, "d_depth")))
    dw, da, dt = (_flat(t, name, N, cast=True) for t, name in ((d_weights, "d_weights"), (d_alphas, "d_alphas"),
                                                               (d_trans, "d_trans")))
    if t0.numel() != N or t1.numel() != N or ri.numel() != N or rgb.numel() != 3 * N:
        raise ValueError(f"composite_packed_bwd{'' if lean else '_full'}: sigmas, rgbs, t_starts, t_ends and ray_indices "
                         "disagree in length")
    ds, dr = torch.empty_like(sig), torch.empty_like(rgb)
    head, tail = (sig, rgb, t0, t1, ri, N, n_rays, _bk(bkgd), dc, dop), (ds, dr)
    if lean:
        _launch("fsn_composite_packed_bwd", sig.device, *head, *tail)
    else:
        _launch("fsn_composite_packed_bwd_full", sig.device, *head, op, dep, dd, dw, da, dt, *tail)
    return ds, dr


def composite_packed_bwd(sigmas, rgbs, t_starts, t_ends, ray_indices, n_rays, bkgd, d_colors, d_opacity):
    """The backward of `composite_packed` for the cotangents of colours (required) and opacity: the training step's."""
    return _composite_bwd(True, sigmas, rgbs, t_starts, t_ends, ray_indices, n_rays, bkgd, _f32(d_colors, "d_colors"),
                          d_opacity)


def composite_packed_bwd_full(sigmas, rgbs, t_starts, t_ends, ray_indices, n_rays, bkgd, d_colors, d_opacity, opacity=None,
                              depth=None, d_depth=None, d_weights=None, d_alphas=None, d_trans=None):
    """The full backward of `composite_packed` (fsn_composite_packed_bwd_full): -> (d_sigmas [N], d_rgbs [N,3]) from the
    cotangents of all six outputs.  Every cotangent may be None: it reaches the kernel as a NULL pointer and its term is
    absent.  `opacity` / `depth` are the forward's outputs, needed when `d_depth` is given."""
    return _composite_bwd(False, sigmas, rgbs, t_starts, t_ends, ray_indices, n_rays, bkgd, d_colors, d_opacity, opacity,
                          depth, d_depth, d_weights, d_alphas, d_trans)


class _DistortionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, t0, t1, ri, n_rays):
        N = w.numel()
        out = torch.empty(n_rays, device=w.device, dtype=torch.float32)
        _launch("fsn_distortion_fwd", w.device, w, t0, t1, ri, N, n_rays, out)
        ctx.save_for_backward(w, t0, t1, ri)
        ctx.n_rays = n_rays
        return out.reshape(n_rays, 1)

    @staticmethod
    def backward(ctx, g):
        w, t0, t1, ri = ctx.saved_tensors
        g = _f32(g, "grad").reshape(-1)
        d_w = torch.empty_like(w)
        _launch("fsn_distortion_bwd", w.device, w, t0, t1, ri, w.numel(), ctx.n_rays, g, d_w)
        return d_w, None, None, None, None


def distortion(weights: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, n_rays: int) -> Tensor:
    """Per-ray distortion of the compositor's weights -> [n_rays, 1] (fsn_distortion_fwd / _bwd; core.loss.DistortionLoss
    has the definition).  Differentiable w.r.t. `weights` only; a ray without samples gives 0."""
    w = _f32(weights, "weights").reshape(-1)
    t0, t1 = _f32(t_starts.detach(), "t_starts").reshape(-1), _f32(t_ends.detach(), "t_ends").reshape(-1)
    ri = _i64(ray_indices, "ray_indices").reshape(-1)
    if not (t0.numel() == t1.numel() == ri.numel() == w.numel()):
        raise ValueError("distortion: weights, t_starts, t_ends and ray_indices disagree in length")
    return _DistortionFn.apply(w, t0, t1, ri, int(n_rays))


# ------------------------------------------------------------------ few-shot geometry losses (csrc/ray_losses.hip)
class _RayEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, ri, n_rays, c, eps, scale):
        out = torch.empty(n_rays, device=v.device, dtype=torch.float32)
        _launch("fsn_ray_entropy_fwd", v.device, v, ri, v.numel(), n_rays, c, eps, scale, out)
        ctx.save_for_backward(v, ri, c)
        ctx.n_rays, ctx.eps, ctx.scale = n_rays, eps, scale
        return out.reshape(n_rays, 1)

    @staticmethod
    def backward(ctx, g):
        v, ri, c = ctx.saved_tensors
        g = _f32(g, "grad").reshape(-1)
        d_v = torch.empty_like(v)
        _launch("fsn_ray_entropy_bwd", v.device, v, ri, v.numel(), ctx.n_rays, c, ctx.eps, ctx.scale, g, d_v)
        return d_v, None, None, None, None, None


def ray_entropy(values: Tensor, ray_indices: Tensor, n_rays: int, ray_weight: Optional[Tensor] = None, eps: float = 1e-10,
                log2: bool = True) -> Tensor:
    """Per-ray entropy of the termination distribution -> [n_rays, 1] (fsn_ray_entropy_fwd / _bwd;
    core.loss.RayEntropyLoss has the definition): p = max(values, 0) / (sum + eps) over the ray, -sum p log(p + eps), in
    bits (`log2`) or nats.  `values`: the compositor's alphas (InfoNeRF) or weights.  `ray_weight` [n_rays] scales each
    ray and is not differentiated; a ray whose weight is 0 is skipped (value 0, gradient exactly 0), as is a ray without
    samples.  Differentiable w.r.t. `values` only."""
    if ray_indices.numel() != values.numel():
        raise ValueError("ray_entropy: values and ray_indices disagree in length")
    if ray_weight is not None and ray_weight.numel() != int(n_rays):
        raise ValueError(f"ray_entropy: ray_weight has {ray_weight.numel()} entries for {int(n_rays)} rays")
    v = _f32(values, "values").reshape(-1)
    ri = _i64(ray_indices, "ray_indices").reshape(-1)
    c = None if ray_weight is None else _f32(ray_weight.detach(), "ray_weight").reshape(-1)
    return _RayEntropyFn.apply(v, ri, int(n_rays), c, float(eps), 1.0 / math.log(2.0) if log2 else 1.0)


class _DepthKLFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, t0, t1, ri, n_rays, depth, var, eps):
        out = torch.empty(n_rays, device=w.device, dtype=torch.float32)
        _launch("fsn_depth_kl_fwd", w.device, w, t0, t1, ri, w.numel(), n_rays, depth, var, eps, out)
        ctx.save_for_backward(w, t0, t1, ri, depth, var)
        ctx.n_rays, ctx.eps = n_rays, eps
        return out.reshape(n_rays, 1)

    @staticmethod
    def backward(ctx, g):
        w, t0, t1, ri, depth, var = ctx.saved_tensors
        g = _f32(g, "grad").reshape(-1)
        d_w = torch.empty_like(w)
        _launch("fsn_depth_kl_bwd", w.device, w, t0, t1, ri, w.numel(), ctx.n_rays, depth, var, ctx.eps, g, d_w)
        return d_w, None, None, None, None, None, None, None


def depth_kl(weights: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, n_rays: int, depth: Tensor, var,
             eps: float = 1e-5) -> Tensor:
    """Per-ray depth KL term on the compositor's weights -> [n_rays, 1] (fsn_depth_kl_fwd / _bwd; core.loss.DepthKLLoss
    has the definition): sum_i -log(max(w_i, 0) + eps) exp(-(m_i - depth_r)^2 / (2 var_r)) dt_i.  `depth` [n_rays] and
    `var` [n_rays] (or a Python float, expanded on the device) are per ray; a ray whose depth or variance is not finite
    and positive is unsupervised: value 0, gradient exactly 0.  Differentiable w.r.t. `weights` only."""
    n_rays = int(n_rays)
    if not (t_starts.numel() == t_ends.numel() == ray_indices.numel() == weights.numel()):
        raise ValueError("depth_kl: weights, t_starts, t_ends and ray_indices disagree in length")
    if depth.numel() != n_rays or (isinstance(var, Tensor) and var.numel() != n_rays):
        raise ValueError(f"depth_kl: depth and var must have one entry for each of the {n_rays} rays")
    w = _f32(weights, "weights").reshape(-1)
    t0, t1 = _f32(t_starts.detach(), "t_starts").reshape(-1), _f32(t_ends.detach(), "t_ends").reshape(-1)
    ri = _i64(ray_indices, "ray_indices").reshape(-1)
    d = _f32(depth.detach(), "depth").reshape(-1)
    if isinstance(var, Tensor):
        v = _f32(var.detach(), "var").reshape(-1)
    else:
        v = torch.full((n_rays,), float(var), device=w.device, dtype=torch.float32)
    return _DepthKLFn.apply(w, t0, t1, ri, n_rays, d, v, float(eps))


class _PatchTVFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d):
        B, P, Q = d.shape
        out = torch.empty(B, device=d.device, dtype=torch.float32)
        _launch("fsn_patch_tv_fwd", d.device, d, B, P, Q, out)
        ctx.save_for_backward(d)
        return out

    @staticmethod
    def backward(ctx, g):
        d, = ctx.saved_tensors
        B, P, Q = d.shape
        g = _f32(g, "grad").reshape(-1)
        d_d = torch.empty_like(d)
        _launch("fsn_patch_tv_bwd", d.device, d, B, P, Q, g, d_d)
        return d_d


def patch_depth_smoothness(depth: Tensor) -> Tensor:
    """Per-patch l2 total variation of rendered depth patches [B, P, Q] -> [B] (fsn_patch_tv_fwd / _bwd;
    core.loss.PatchDepthSmoothnessLoss has the definition): the sum over the anchors i < P-1, j < Q-1 of
    (d[i,j] - d[i,j+1])^2 + (d[i,j] - d[i+1,j])^2; 0 when P or Q is 1.  Any strides (a copy is made when needed)."""
    if depth.dim() != 3 or depth.shape[1] < 1 or depth.shape[2] < 1:
        raise ValueError(f"patch_depth_smoothness: expected depth of shape [B, P, Q] with P, Q >= 1, got {tuple(depth.shape)}")
    return _PatchTVFn.apply(_f32(depth, "depth"))


# ------------------------------------------------------------------ monocular depth priors (csrc/depth_prior.hip)
def _prior_patches(who: str, depth: Tensor, prior: Tensor, weight: Optional[Tensor]):
    """depth, prior and the optional weight of the two prior losses as the kernels read them: [B, P, Q] float32,
    contiguous; prior and weight detached (gradients go to depth only)."""
    if depth.dim() != 3 or depth.shape[1] < 1 or depth.shape[2] < 1:
        raise ValueError(f"{who}: expected depth of shape [B, P, Q] with P, Q >= 1, got {tuple(depth.shape)}")
    for t, name in ((prior, "prior"), (weight, "weight")):
        if t is not None and tuple(t.shape) != tuple(depth.shape):
            raise ValueError(f"{who}: {name} has shape {tuple(t.shape)} for depth {tuple(depth.shape)}")
    return (_f32(depth, "depth"), _f32(prior.detach(), "prior"),
            None if weight is None else _f32(weight.detach(), "weight"))


class _SsiDepthFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d, p, w, inverse, z_min, rel_eps):
        B, P, Q = d.shape
        out = torch.empty(B, device=d.device, dtype=torch.float32)
        fit = torch.empty(B, 4, device=d.device, dtype=torch.float32)
        fit64 = torch.empty(B, 4, device=d.device, dtype=torch.float64)  # (unrounded, for the backward's residual)
        _launch("fsn_ssi_depth_fwd", d.device, d, p, w, B, P, Q, inverse, z_min, rel_eps, out, fit, fit64)
        ctx.save_for_backward(d, p, w, fit64)
        ctx.args = (inverse, z_min)
        ctx.mark_non_differentiable(fit)
        return out, fit

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_fit):
        d, p, w, fit64 = ctx.saved_tensors
        B, P, Q = d.shape
        d_d = torch.empty_like(d)
        _launch("fsn_ssi_depth_bwd", d.device, d, p, w, fit64, B, P, Q, *ctx.args, _f32(g, "grad").reshape(-1), d_d)
        return d_d, None, None, None, None, None


def ssi_depth(depth: Tensor, prior: Tensor, weight: Optional[Tensor] = None, *, inverse: bool = False, z_min: float = 1e-3,
              rel_eps: float = 1e-10) -> Tuple[Tensor, Tensor]:
    """Scale-and-shift-invariant fit of rendered depth patches to a prior: depth, prior, weight [B, P, Q] ->
    (out [B], fit [B, 4]) (fsn_ssi_depth_fwd / _bwd, one launch each way; core.loss.ScaleShiftDepthLoss has the
    definition).  Per patch x = depth or, with `inverse`, 1 / max(depth, z_min); over the VALID pixels (prior and depth
    finite, weight > 0; no weight: 1), in float64: the weighted least-squares (s, t) of s x + t against the prior and
    out = sum w (s x + t - p)^2 / sum w.  fit = (s, t, sum w, degenerate): a patch with fewer than two valid pixels,
    sum w <= 0 or var(x) <= rel_eps mean(x)^2 is degenerate - value 0, gradient exactly 0, flag 1.  P * Q <= 4096.
    Differentiable w.r.t. depth only (not again); an invalid pixel gets a gradient of exactly 0.  Any strides (a copy is
    made when needed).  Bitwise reproducible."""
    d, p, w = _prior_patches("ssi_depth", depth, prior, weight)
    if inverse and not z_min > 0.0:
        raise ValueError(f"ssi_depth: z_min must be positive in disparity space, got {z_min}")
    if not rel_eps >= 0.0:
        raise ValueError(f"ssi_depth: rel_eps must not be negative, got {rel_eps}")
    return _SsiDepthFn.apply(d, p, w, 1 if inverse else 0, float(z_min), float(rel_eps))


class _DepthRankFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d, p, w, margin, gap, disparity):
        B, P, Q = d.shape
        out = torch.empty(B, device=d.device, dtype=torch.float32)
        pairs = torch.empty(B, device=d.device, dtype=torch.int64)
        _launch("fsn_depth_rank_fwd", d.device, d, p, w, B, P, Q, margin, gap, disparity, out, pairs)
        ctx.save_for_backward(d, p, w)
        ctx.args = (margin, gap, disparity)
        ctx.mark_non_differentiable(pairs)
        return out, pairs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_pairs):
        d, p, w = ctx.saved_tensors
        B, P, Q = d.shape
        d_d = torch.empty_like(d)
        _launch("fsn_depth_rank_bwd", d.device, d, p, w, B, P, Q, *ctx.args, _f32(g, "grad").reshape(-1), d_d)
        return d_d, None, None, None, None, None


def depth_rank(depth: Tensor, prior: Tensor, weight: Optional[Tensor] = None, *, margin: float = 1e-4, prior_gap: float = 0.0,
               prior_is_disparity: bool = False) -> Tuple[Tensor, Tensor]:
    """Ordinal ranking of rendered depth patches against a prior over ALL pairs of a patch: depth, prior, weight
    [B, P, Q] -> (out [B], pairs [B] int64) (fsn_depth_rank_fwd / _bwd, one launch each way;
    core.loss.DepthRankingLoss has the definition).  An ordered pair (i, j) of VALID pixels (prior and depth finite,
    weight > 0: the weight is a mask here) counts iff the prior puts i nearer - p_i < p_j - prior_gap, or
    p_i > p_j + prior_gap with `prior_is_disparity` - and adds max(0, d_i - d_j + margin) to out.  P * Q <= 4096.
    Differentiable w.r.t. depth only (not again): +1 / -1 per active pair, 0 at a hinge of exactly 0 and for an invalid
    pixel.  Any strides (a copy is made when needed).  Bitwise reproducible."""
    d, p, w = _prior_patches("depth_rank", depth, prior, weight)
    if not prior_gap >= 0.0:
        raise ValueError(f"depth_rank: prior_gap must not be negative, got {prior_gap}")
    return _DepthRankFn.apply(d, p, w, float(margin), float(prior_gap), 1 if prior_is_disparity else 0)


# ------------------------------------------------------------------ neighbouring-ray KL (csrc/ray_hist.hip)
def _hist_axis(who: str, bins, t_min, t_max) -> Tuple[int, float, float]:
    """The histogram's axis as the C-ABI takes it; what it refuses is refused here first, with a ValueError."""
    bins, t_min, t_max = int(bins), float(t_min), float(t_max)
    if not 1 <= bins <= 4096:
        raise ValueError(f"{who}: 1 <= bins <= 4096, got {bins}")
    if not (math.isfinite(t_min) and math.isfinite(t_max) and t_min < t_max):
        raise ValueError(f"{who}: t_min < t_max, both finite, got {t_min} and {t_max}")
    return bins, t_min, t_max


def ray_histogram_edges(bins: int = 64, *, t_min: float, t_max: float) -> Tensor:
    """The bins + 1 float32 edges of `ray_histogram`'s axis, as the kernels form them (fsn_ray_hist_edges: host
    arithmetic, no GPU): h = (t_max - t_min) / bins, e_b = t_min + b h, every step rounded to float32 -> CPU tensor."""
    bins, t_min, t_max = _hist_axis("ray_histogram_edges", bins, t_min, t_max)
    edges = (C.c_float * (bins + 1))()
    L.check(L.lib().fsn_ray_hist_edges(bins, t_min, t_max, edges), "fsn_ray_hist_edges")
    return torch.tensor(list(edges), dtype=torch.float32)


class _RayHistFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, t0, t1, ri, n_rays, first, count, bins, t_min, t_max, normalize, eps):
        out = torch.empty(count, bins, device=v.device, dtype=torch.float32)
        _launch("fsn_ray_hist_fwd", v.device, v, t0, t1, ri, v.numel(), n_rays, first, count, bins, t_min, t_max, normalize,
                eps, out)
        ctx.save_for_backward(v, t0, t1, ri, out)
        ctx.args = (n_rays, first, count, bins, t_min, t_max, normalize, eps)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        v, t0, t1, ri, out = ctx.saved_tensors
        d_v = torch.empty_like(v)
        _launch("fsn_ray_hist_bwd", v.device, v, t0, t1, ri, v.numel(), *ctx.args, out, _f32(g, "grad"), d_v)
        return (d_v,) + (None,) * 11


def ray_histogram(values: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, n_rays: int, *, bins: int = 64,
                  t_min: float, t_max: float, normalize: bool = True, eps: float = 1e-10,
                  rays: Optional[Tuple[int, int]] = None) -> Tensor:
    """Each ray's termination histogram over `bins` fixed bins of [t_min, t_max] -> [count, bins] (fsn_ray_hist_fwd /
    _bwd, one launch each way; this package's own definition, DESIGN 6.1 "Neighbouring-ray KL"): a ray's distribution
    on a depth axis that all rays share, whatever their sample counts.  Float32, in this order: h = (t_max - t_min) /
    bins, edges e_b = t_min + b h (`ray_histogram_edges`); sample i with a = t_starts_i, c = t_ends_i counts iff both
    are finite and c - a > 0, with u_i = max(values_i, 0) (0 where it does not count);
        H_rb = sum_i u_i max(min(c, e_{b+1}) - max(a, e_b), 0) / (c - a)    (ascending sample order, from +0)
    and the output is P_rb = H_rb / (sum_i u_i + eps) (`normalize`) or H.  Mass outside [t_min, t_max] is dropped, so a
    row sums to at most 1; a ray without samples gives a row of zeros.  `rays` = (first, count) computes the rows of the
    rays first ... first + count - 1 only (the patch rays behind a ray batch); the samples of every other ray get a
    gradient of exactly 0.  `values`: the compositor's alphas or weights.  Differentiable w.r.t. `values` only (not
    again): negative entries get no gradient (torch.clamp's rule, passing at 0); there is NO gradient to t_starts,
    t_ends or the edges.  Bitwise reproducible."""
    bins, t_min, t_max = _hist_axis("ray_histogram", bins, t_min, t_max)
    n_rays = int(n_rays)
    first, count = (0, n_rays) if rays is None else (int(rays[0]), int(rays[1]))
    if n_rays < 0 or first < 0 or count < 0 or first + count > n_rays:
        raise ValueError(f"ray_histogram: rays = ({first}, {count}) are not rows of the {n_rays} rays")
    if not eps > 0.0:
        raise ValueError(f"ray_histogram: eps must be positive, got {eps}")
    if not (t_starts.numel() == t_ends.numel() == ray_indices.numel() == values.numel()):
        raise ValueError("ray_histogram: values, t_starts, t_ends and ray_indices disagree in length")
    v = _f32(values, "values").reshape(-1)
    t0, t1 = _f32(t_starts.detach(), "t_starts").reshape(-1), _f32(t_ends.detach(), "t_ends").reshape(-1)
    ri = _i64(ray_indices, "ray_indices").reshape(-1)
    return _RayHistFn.apply(v, t0, t1, ri, n_rays, first, count, bins, t_min, t_max, 1 if normalize else 0, float(eps))


class _PatchNklFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, c, eps):
        B, Ph, Pw, bins = P.shape
        out = torch.empty(B, Ph, Pw, device=P.device, dtype=torch.float32)
        _launch("fsn_patch_nkl_fwd", P.device, P, c, B, Ph, Pw, bins, eps, out)
        ctx.save_for_backward(P, c)
        ctx.eps = eps
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        P, c = ctx.saved_tensors
        B, Ph, Pw, bins = P.shape
        d_P = torch.empty_like(P)
        _launch("fsn_patch_nkl_bwd", P.device, P, c, B, Ph, Pw, bins, ctx.eps, _f32(g, "grad"), d_P)
        return d_P, None, None


def patch_neighbor_kl(P: Tensor, pair_weight: Optional[Tensor] = None, eps: float = 1e-5) -> Tensor:
    """KL divergence between the histograms of neighbouring pixels of rendered patches: P [B, Ph, Pw, bins] ->
    [B, Ph, Pw] (fsn_patch_nkl_fwd / _bwd, one launch each way; core.loss.NeighborRayKLLoss has the definition): with
    D(p, q) = sum_b p_b (log(p_b + eps) - log(q_b + eps)), out[i,j] = D(P_ij, P_i,j+1) + D(P_ij, P_i+1,j), each term
    where that neighbour exists - every adjacent pair once, owned by its left or upper pixel.  `pair_weight`
    [B, Ph, Pw] is a 0/1 mask, not differentiated (default: all ones): a pair with a masked pixel is skipped, value 0
    and gradient exactly 0.  Any strides (a copy is made when needed).  Differentiable w.r.t. P (not again)."""
    if P.dim() != 4 or min(P.shape[1:]) < 1 or P.shape[3] > 4096:
        raise ValueError(f"patch_neighbor_kl: expected P of shape [B, Ph, Pw, bins] with Ph, Pw >= 1 and 1 <= bins <= 4096, "
                         f"got {tuple(P.shape)}")
    if pair_weight is not None and tuple(pair_weight.shape) != tuple(P.shape[:3]):
        raise ValueError(f"patch_neighbor_kl: pair_weight has shape {tuple(pair_weight.shape)} for patches {tuple(P.shape[:3])}")
    if not eps > 0.0:
        raise ValueError(f"patch_neighbor_kl: eps must be positive, got {eps}")
    c = None if pair_weight is None else _f32(pair_weight.detach(), "pair_weight")
    return _PatchNklFn.apply(_f32(P, "P"), c, float(eps))


def patch_neighbor_pairs(B: int, Ph: int, Pw: int) -> int:
    """The number of adjacent pairs of B patches of Ph x Pw pixels: what an unmasked `patch_neighbor_kl` counts."""
    return _size("fsn_patch_nkl_pairs", None, int(B), int(Ph), int(Pw))


# ------------------------------------------------------------------ depth-warp sampling (csrc/warp.hip)
class _WarpSampleFn(torch.autograd.Function):
    """colour / valid / uvz of fsn_warp_sample_fwd in one node; the backward is one fsn_warp_sample_bwd launch that
    recomputes the projection and the taps, with NULL where an input needs no gradient."""

    @staticmethod
    def forward(ctx, o, d, t, sv, poses12, images, K, white_bkgd, z_min, border, want_uvz):
        n, dev = t.numel(), t.device
        colour = torch.empty(n, 3, device=dev, dtype=torch.float32)
        valid = torch.empty(n, device=dev, dtype=torch.uint8)
        uvz = torch.empty(n, 3, device=dev, dtype=torch.float32) if want_uvz else None
        ctx.flags = (white_bkgd, z_min, border)
        if n:
            _launch("fsn_warp_sample_fwd", dev, o, d, t, sv, n, poses12, poses12.shape[0], images, images.shape[1],
                    images.shape[2], images.shape[3], white_bkgd, K, K.shape[0], z_min, border, colour, valid, uvz)
        ctx.save_for_backward(o, d, t, sv, poses12, images, K)
        valid = valid.view(torch.bool)
        ctx.mark_non_differentiable(*((valid,) if uvz is None else (valid, uvz)))
        return colour, valid, uvz

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_valid, _g_uvz):
        o, d, t, sv, poses12, images, K = ctx.saved_tensors
        white_bkgd, z_min, border = ctx.flags
        want_o, want_d, want_t = ctx.needs_input_grad[:3]
        d_o = torch.empty_like(o) if want_o else None
        d_d = torch.empty_like(d) if want_d else None
        d_t = torch.empty_like(t) if want_t else None
        if t.numel() and (want_o or want_d or want_t):
            _launch("fsn_warp_sample_bwd", t.device, o, d, t, sv, t.numel(), poses12, poses12.shape[0], images,
                    images.shape[1], images.shape[2], images.shape[3], white_bkgd, K, K.shape[0], z_min, border,
                    _f32(g, "grad"), d_t, d_o, d_d)
        return (d_o, d_d, d_t) + (None,) * 8


def warp_sample(rays_o: Tensor, rays_d: Tensor, depth: Tensor, src_view: Tensor, poses12: Tensor, images: Tensor, K: Tensor,
                *, white_bkgd: bool = False, z_min: float = 1e-3, border: float = 0.0, want_uvz: bool = False):
    """Depth-warp sampling in ONE launch each way (fsn_warp_sample_fwd / _bwd; DESIGN 6.1 and include/fsnerf_hip.h have
    the definition): row r's point rays_o_r + depth_r rays_d_r is projected into source view src_view_r (poses12 [V,12]
    float32, K = (fx, fy, cx, cy) [1 or V, 4] float32) and the resident bytes `images` uint8 [V,H,W,3|4] are sampled
    bilinearly there, each tap converted as the ray batch converts its pixel (`white_bkgd` composes over alpha) ->
    (colour [n,3] float32, valid [n] bool, uvz [n,3] or None with want_uvz=False).
    A row is valid iff 0 <= src_view < V (-1 is the documented "no source view"), depth is finite and > 0, the point lies
    at least `z_min` in front of the source camera and its pixel coordinates at least `border` pixels inside the image;
    an invalid row gets colour 0 and every gradient exactly 0.  uvz = (u, v, z), the pixel coordinates and the depth in
    the source camera, for every row whose view is in range (for an occlusion mask against source depths).
    rays_o, rays_d [n,3] and depth [n] or [n,1] are float32 GPU tensors taken as they are (nothing is cast); gradients
    go to whichever of them require one, and the cell of the four taps is a constant of the backward (as for
    grid_sample).  `valid` and `uvz` are not differentiable, and there is NO gradient to the images, to poses12 or to
    K: the source cameras are constants here."""
    o, d = _gpu_f32(rays_o, "warp_sample: rays_o"), _gpu_f32(rays_d, "warp_sample: rays_d")
    t = _gpu_f32(depth, "warp_sample: depth").reshape(-1)
    n = t.numel()
    if o.dim() != 2 or tuple(o.shape) != (n, 3) or tuple(d.shape) != (n, 3):
        raise ValueError(f"warp_sample: rays_o and rays_d are [n,3] for a depth of n = {n} entries, got {tuple(o.shape)} "
                         f"and {tuple(d.shape)}")
    if src_view.numel() != n:
        raise ValueError(f"warp_sample: src_view has {src_view.numel()} entries for {n} rows")
    sv = _i64(src_view, "warp_sample: src_view").reshape(-1)
    if not (poses12.is_cuda and images.is_cuda):
        raise RuntimeError("warp_sample: poses12 and images: expected GPU tensors (the HIP path has no CPU fallback)")
    if poses12.dtype != torch.float32 or poses12.dim() != 2 or poses12.shape[1] != 12 or not poses12.is_contiguous():
        raise TypeError("warp_sample: poses12 is float32 [V,12], contiguous")
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[0] != poses12.shape[0] or not images.is_contiguous():
        raise TypeError(f"warp_sample: images are uint8 [{poses12.shape[0]},H,W,3|4], contiguous, got {images.dtype} "
                        f"{tuple(images.shape)}")
    K, _ = _camera_table(K, poses12.shape[0], "warp_sample")
    return _WarpSampleFn.apply(o, d, t, sv, poses12.detach(), images, K, 1 if white_bkgd else 0, float(z_min),
                               float(border), bool(want_uvz))


# ------------------------------------------------------------------ packed volume-rendering primitives (csrc/packed_scan.hip)
class RaySpans:
    """Where each ray's samples are among N flat samples - the "span" arguments of include/fsnerf_hip.h: exactly one of
    sorted `ray_indices` [N], `packed_info` [n_rays, 2] = (start, count), dense rows of `dense_S` samples."""

    def __init__(self, N: int, n_rays: int, ray_indices: Optional[Tensor] = None, packed_info: Optional[Tensor] = None,
                 dense_S: int = 0):
        if (ray_indices is not None) + (packed_info is not None) + (dense_S > 0) != 1 and N > 0 and n_rays > 0:
            raise ValueError("RaySpans: exactly one of ray_indices, packed_info and dense_S")
        self.N, self.R, self.S = int(N), int(n_rays), int(dense_S)
        self.ri = None if ray_indices is None else _i64(ray_indices, "ray_indices").reshape(-1)
        self.pi = None if packed_info is None else _i64(packed_info, "packed_info")
        if self.ri is not None and self.ri.numel() != self.N:
            raise ValueError(f"ray_indices: expected {self.N} values, got {self.ri.numel()}")
        if self.pi is not None and tuple(self.pi.shape) != (self.R, 2):
            raise ValueError(f"packed_info: expected shape ({self.R}, 2), got {tuple(self.pi.shape)}")
        if self.S > 0 and self.N != self.R * self.S:
            raise ValueError(f"dense rows: {self.N} values are not {self.R} rows of {self.S}")

    def args(self):
        return self.ri, self.pi, self.N, self.R, self.S


def pack_info(ray_indices: Tensor, n_rays: int) -> Tensor:
    """(start, count) int64 [n_rays, 2] of every ray in the sorted `ray_indices` (fsn_pack_info)."""
    ri = _i64(ray_indices, "ray_indices").reshape(-1)
    info = torch.empty(int(n_rays), 2, dtype=torch.int64, device=ri.device)
    _launch("fsn_pack_info", ri.device, ri, ri.numel(), int(n_rays), info)
    return info


def _zeroed_by_call(shape, spans: RaySpans, dev, dtype=torch.float32) -> Tensor:
    """An output the entry point zeroes itself before its launch (gradients, keep flags): zeros here only when it
    returns without one."""
    make = torch.empty if spans.N > 0 and spans.R > 0 else torch.zeros
    return make(shape, dtype=dtype, device=dev)


def _out(like: Tensor, spans: RaySpans, dtype=torch.float32) -> Tensor:
    """An output the kernel fills per ray: zeroed where no launch (or no ray) would write it."""
    if spans.R == 0 or spans.pi is not None:
        return torch.zeros(like.shape, dtype=dtype, device=like.device)
    return torch.empty(like.shape, dtype=dtype, device=like.device)


def packed_scan_fwd(x: Tensor, spans: RaySpans, prod: bool, exclusive: bool) -> Tensor:
    x = _flat(x, "inputs", spans.N)
    out = _out(x, spans)
    _launch("fsn_packed_scan_fwd", x.device, x, *spans.args(), L.FSN_SCAN_PROD if prod else L.FSN_SCAN_SUM, int(exclusive),
            out)
    return out


def packed_scan_bwd(x: Optional[Tensor], d_out: Tensor, spans: RaySpans, prod: bool, exclusive: bool) -> Tensor:
    g = _flat(d_out, "d_out", spans.N)
    x = _flat(x, "inputs", spans.N)
    d_x = _zeroed_by_call(g.shape, spans, g.device)
    _launch("fsn_packed_scan_bwd", g.device, x, g, *spans.args(), L.FSN_SCAN_PROD if prod else L.FSN_SCAN_SUM, int(exclusive),
            d_x)
    return d_x


def packed_weights_fwd(v: Tensor, t_starts: Optional[Tensor], t_ends: Optional[Tensor], spans: RaySpans, from_alpha: bool,
                       prefix_trans: Optional[Tensor] = None, want=(True, True, True)):
    """-> (weights, trans, alphas), each [N] or None where `want` says so (fsn_packed_weights_fwd)."""
    n = spans.N
    v = _flat(v, "alphas" if from_alpha else "sigmas", n)
    t0, t1 = _flat(t_starts, "t_starts", n), _flat(t_ends, "t_ends", n)
    p = _flat(prefix_trans, "prefix_trans", n)
    if not from_alpha and (t0 is None or t1 is None):
        raise ValueError("packed_weights_fwd: the density form needs t_starts and t_ends")
    outs = [_out(v, spans) if k else None for k in want]
    _launch("fsn_packed_weights_fwd", v.device, v, t0, t1, *spans.args(), int(from_alpha), p, *(o for o in outs))
    return tuple(outs)


def packed_weights_bwd(v: Tensor, t_starts: Optional[Tensor], t_ends: Optional[Tensor], spans: RaySpans, from_alpha: bool,
                       prefix_trans: Optional[Tensor], d_weights: Optional[Tensor], d_trans: Optional[Tensor],
                       d_alphas: Optional[Tensor]) -> Tensor:
    """-> d_sigmas (or d_alphas) [N]; a cotangent that is None reaches the kernel as NULL (fsn_packed_weights_bwd)."""
    n = spans.N
    v = _flat(v, "alphas" if from_alpha else "sigmas", n)
    t0, t1 = _flat(t_starts, "t_starts", n), _flat(t_ends, "t_ends", n)
    p = _flat(prefix_trans, "prefix_trans", n)
    dw, dtr, dal = _flat(d_weights, "d_weights", n), _flat(d_trans, "d_trans", n), _flat(d_alphas, "d_alphas", n)
    d_v = _zeroed_by_call(v.shape, spans, v.device)
    _launch("fsn_packed_weights_bwd", v.device, v, t0, t1, *spans.args(), int(from_alpha), p, dw, dtr, dal, d_v)
    return d_v


def packed_visibility_alpha(alphas: Tensor, spans: RaySpans, early_stop_eps: float, alpha_thre: float) -> Tensor:
    a = _flat(alphas, "alphas", spans.N)
    keep = _zeroed_by_call((spans.N,), spans, a.device, torch.uint8)
    _launch("fsn_packed_visibility_alpha", a.device, a, *spans.args(), float(early_stop_eps), float(alpha_thre), keep)
    return keep.bool()


def accumulate_fwd(weights: Tensor, values: Optional[Tensor], spans: RaySpans) -> Tensor:
    """-> [n_rays, C] (C = 1 without values) (fsn_accumulate_fwd)"""
    w = _flat(weights, "weights", spans.N)
    C = 1
    if values is not None:
        C = int(values.shape[-1])
        if C < 1:
            raise ValueError("accumulate: values need at least one channel")
        values = _flat(values, "values", spans.N * C)
    out = torch.empty(spans.R, C, device=w.device, dtype=torch.float32)  # (every row is written; N == 0: zeroed by the call)
    _launch("fsn_accumulate_fwd", w.device, w, values, C, *spans.args(), out)
    return out


def accumulate_bwd(d_out: Tensor, weights: Tensor, values: Optional[Tensor], spans: RaySpans, want_weights: bool,
                   want_values: bool):
    """-> (d_weights [N] or None, d_values [N, C] or None) (fsn_accumulate_bwd)"""
    w = _flat(weights, "weights", spans.N)
    C = 1 if values is None else int(values.shape[-1])
    g = _flat(d_out, "d_out", spans.R * C)
    v = _flat(values, "values", spans.N * C)
    d_w = _zeroed_by_call(w.shape, spans, w.device) if want_weights else None
    d_v = _zeroed_by_call((spans.N, C), spans, w.device) if want_values and v is not None else None
    if d_w is not None or d_v is not None:
        _launch("fsn_accumulate_bwd", w.device, g, w, v, C, *spans.args(), d_w, d_v)
    return d_w, d_v


# ------------------------------------------------------------------ proposal-network sampler (csrc/propnet.hip)
_STOT = {None: L.FSN_STOT_NONE, "uniform": L.FSN_STOT_UNIFORM, "lindisp": L.FSN_STOT_LINDISP}


def _rows(t: Tensor, name: str, R: int, cols: int) -> Tensor:
    """A required [R, cols] tensor (`_gpu_f32` policy): the dense rows keep their shape, unlike `_flat`."""
    t = _gpu_f32(t, name)
    if tuple(t.shape) != (R, cols):
        raise ValueError(f"{name}: expected shape ({R}, {cols}), got {tuple(t.shape)}")
    return t


def _stot_args(transform: Optional[str], near: float, far: float):
    if transform not in _STOT:
        raise ValueError(f"transform: expected None, 'uniform' or 'lindisp', got {transform!r}")
    return _STOT[transform], float(near), float(far)


def _jitter(b: Optional[Tensor], R: int) -> Optional[Tensor]:
    return None if b is None else _rows(b.reshape(-1, 1), "b", R, 1)


def importance_sample(vals: Tensor, cdfs: Tensor, n: int, b: Optional[Tensor] = None, transform: Optional[str] = None,
                      near: float = 0.0, far: float = 0.0, want_centres: bool = True):
    """vals / cdfs [R, S+1] -> (s_edges [R, n+1], centres [R, n] or None, t_edges [R, n+1] or None (no transform));
    b: one jitter per ray [R], None: 0.5 (fsn_importance_sample)."""
    vals = _gpu_f32(vals, "vals")
    R, S, n = int(vals.shape[0]), int(vals.shape[1]) - 1, int(n)
    vals, cdfs, b = _rows(vals, "vals", R, S + 1), _rows(cdfs, "cdfs", R, S + 1), _jitter(b, R)
    tf, near, far = _stot_args(transform, near, far)
    dev = vals.device
    s = torch.empty(R, max(n, 0) + 1, device=dev)
    x = torch.empty(R, max(n, 0), device=dev) if want_centres else None
    t = torch.empty_like(s) if transform is not None else None
    _launch("fsn_importance_sample", dev, vals, cdfs, R, S, n, b, tf, near, far, s, x, t)
    return s, x, t


def prop_resample(s_edges: Tensor, t_edges: Tensor, sigmas: Tensor, n: int, b: Optional[Tensor] = None,
                  transform: Optional[str] = None, near: float = 0.0, far: float = 0.0, want_centres: bool = False):
    """s_edges / t_edges [R, S+1], sigmas [R, S] -> (cdfs [R, S+1], s_out [R, n+1], centres or None, t_out or None):
    the proposal's cdfs and the next level's intervals in one launch (fsn_prop_resample)."""
    sigmas = _gpu_f32(sigmas, "sigmas")
    R, S, n = int(sigmas.shape[0]), int(sigmas.shape[1]), int(n)
    s_edges, t_edges, b = _rows(s_edges, "s_edges", R, S + 1), _rows(t_edges, "t_edges", R, S + 1), _jitter(b, R)
    tf, near, far = _stot_args(transform, near, far)
    dev = sigmas.device
    cdfs = torch.empty(R, S + 1, device=dev)
    s = torch.empty(R, max(n, 0) + 1, device=dev)
    x = torch.empty(R, max(n, 0), device=dev) if want_centres else None
    t = torch.empty_like(s) if transform is not None else None
    _launch("fsn_prop_resample", dev, s_edges, t_edges, sigmas, R, S, n, b, tf, near, far, cdfs, s, x, t)
    return cdfs, s, x, t


def searchsorted_dense(keys: Tensor, values: Tensor) -> Tuple[Tensor, Tensor]:
    """keys [R, K] sorted per row, values [R, Q] -> (ids_left, ids_right) int64 [R, Q] (fsn_searchsorted_dense)."""
    keys, values = _gpu_f32(keys, "sorted_sequence"), _gpu_f32(values, "values")
    if keys.dim() != 2 or values.dim() != 2 or keys.shape[0] != values.shape[0]:
        raise ValueError(f"searchsorted: expected [R, K] and [R, Q], got {tuple(keys.shape)} and {tuple(values.shape)}")
    R, K, Q = int(keys.shape[0]), int(keys.shape[1]), int(values.shape[1])
    il = torch.empty(R, Q, dtype=torch.int64, device=keys.device)
    ir = torch.empty_like(il)
    _launch("fsn_searchsorted_dense", keys.device, keys, values, R, K, Q, il, ir)
    return il, ir


def _prop_loss_rows(q_edges, q_cdfs, k_edges, k_cdfs):
    q_edges = _gpu_f32(q_edges, "segments_query")
    k_edges = _gpu_f32(k_edges, "segments_key")
    R, n, S = int(q_edges.shape[0]), int(q_edges.shape[1]) - 1, int(k_edges.shape[1]) - 1
    return (_rows(q_edges, "segments_query", R, n + 1), _rows(q_cdfs, "cdfs_query", R, n + 1),
            _rows(k_edges, "segments_key", R, S + 1), _rows(k_cdfs, "cdfs_key", R, S + 1)), R, n, S


def prop_loss_fwd(q_edges: Tensor, q_cdfs: Tensor, k_edges: Tensor, k_cdfs: Tensor) -> Tensor:
    """-> the interlevel loss per query interval [R, n] (fsn_prop_loss_fwd)"""
    rows, R, n, S = _prop_loss_rows(q_edges, q_cdfs, k_edges, k_cdfs)
    loss = torch.empty(R, max(n, 0), device=rows[0].device)
    _launch("fsn_prop_loss_fwd", loss.device, *rows, R, n, S, loss)
    return loss


def prop_loss_bwd(q_edges: Tensor, q_cdfs: Tensor, k_edges: Tensor, k_cdfs: Tensor, d_loss: Tensor) -> Tensor:
    """-> d_cdfs_key [R, S+1] (fsn_prop_loss_bwd)"""
    rows, R, n, S = _prop_loss_rows(q_edges, q_cdfs, k_edges, k_cdfs)
    g = _rows(d_loss, "d_loss", R, n)
    d_ck = torch.empty(R, S + 1, device=g.device)
    _launch("fsn_prop_loss_bwd", g.device, *rows, g, R, n, S, d_ck)
    return d_ck


# ------------------------------------------------------------------ occupancy-grid sampler
def occgrid_march(rays_o: Tensor, rays_d: Tensor, aabb: Sequence[float], res: int, levels: int, bits: Tensor,
                  near_plane: float, far_plane: float, step: float, u: Optional[Tensor], max_steps: int,
                  t_min: Optional[Tensor] = None, t_max: Optional[Tensor] = None, cone_angle: float = 0.0):
    """Lattice march through the occupancy grid -> (ray_indices int64 [N], t_starts [N], t_ends [N], counts [R]).
    Two launches around an exclusive scan of the per-ray counts; one host sync for N (as nerfacc's does).
    Optional per-ray bounds `t_min` / `t_max` [R] and a `cone_angle` > 0 (the step grows with distance): every call
    goes through fsn_occgrid_march_ex (include/fsnerf_hip.h has the definition), of which fsn_occgrid_march is the form
    without bounds and with cone_angle 0 - one kernel serves both."""
    o, d = _f32(rays_o, "rays_o").reshape(-1, 3), _f32(rays_d, "rays_d").reshape(-1, 3)
    R, dev = o.shape[0], o.device
    ab = (C.c_float * 6)(*[float(v) for v in aabb])
    u_ = None if u is None else _f32(u, "u").reshape(-1)
    if u_ is not None and u_.numel() != R:
        raise ValueError("u must hold one value per ray")
    bounds = [None if t is None else _f32(t, k).reshape(-1) for t, k in ((t_min, "t_min"), (t_max, "t_max"))]
    if any(t is not None and t.numel() != R for t in bounds):
        raise ValueError("t_min / t_max must hold one value per ray")
    args = (o, d, R, ab, int(res), int(levels), bits, float(near_plane), float(far_plane), float(step), u_,
            int(max_steps), bounds[0], bounds[1], float(cone_angle))
    counts = torch.zeros(R, device=dev, dtype=torch.int64)
    _launch("fsn_occgrid_march_ex", dev, *args, counts, None, None, None, None)
    ends = torch.cumsum(counts, 0)
    offsets = (ends - counts).contiguous()
    N = int(ends[-1].item()) if R > 0 else 0  # the one host read: the sample count sizes the outputs
    ri = torch.empty(N, device=dev, dtype=torch.int64)
    t0 = torch.empty(N, device=dev, dtype=torch.float32)
    t1 = torch.empty(N, device=dev, dtype=torch.float32)
    if N > 0:
        _launch("fsn_occgrid_march_ex", dev, *args, None, offsets, ri, t0, t1)
    return ri, t0, t1, counts


def ray_aabb_intersect(rays_o: Tensor, rays_d: Tensor, aabbs: Tensor, near_plane: float = -math.inf,
                       far_plane: float = math.inf, miss_value: float = math.inf):
    """Rays [R,3] against boxes [M,6] -> (t_mins [R,M], t_maxs [R,M], hits bool [R,M]) (fsn_ray_aabb_intersect: the
    march's slab test; a hit holds the range clipped to [near_plane, far_plane], a miss `miss_value` twice)."""
    o, d = _f32(rays_o, "rays_o").reshape(-1, 3), _f32(rays_d, "rays_d").reshape(-1, 3)
    boxes = _f32(torch.as_tensor(aabbs, dtype=torch.float32).to(o.device), "aabbs").reshape(-1, 6)
    R, M = o.shape[0], boxes.shape[0]
    t0 = torch.empty(R, M, device=o.device, dtype=torch.float32)
    t1 = torch.empty(R, M, device=o.device, dtype=torch.float32)
    hits = torch.empty(R, M, device=o.device, dtype=torch.uint8)
    _launch("fsn_ray_aabb_intersect", o.device, o, d, R, boxes, M, float(near_plane), float(far_plane), float(miss_value), t0,
            t1, hits)
    return t0, t1, hits.bool()


def _occ_march_options(R: int, cone_angle: float, t_min: Optional[Tensor], t_max: Optional[Tensor], camera, h: _Held):
    """The extended arguments of fsn_render_rays_occgrid_ex (cone_angle, t_min, t_max), checked: per-ray bounds hold one
    value per ray and need ray tensors.  `h` holds the converted bounds."""
    if t_min is not None or t_max is not None:
        if camera is not None:
            raise TypeError("per-ray t_min / t_max need ray tensors, not a camera")
    if any(t is not None and t.numel() != R for t in (t_min, t_max)):
        raise ValueError("t_min / t_max must hold one value per ray")
    bounds = _flat(t_min, "t_min", R, cast=True), _flat(t_max, "t_max", R, cast=True)
    h.tensors += bounds
    return (float(cone_angle), *bounds)


def _occ_args(rays_o: Optional[Tensor], rays_d: Optional[Tensor], camera, aabb: Sequence[float], res: int, levels: int,
              bits: Tensor, near_plane: float, far_plane: float, step: float, max_steps: int, u: Optional[Tensor],
              early_stop_eps: float, alpha_thre: float, pos_mask: Optional[Tensor], dir_mask: Optional[Tensor],
              cone_angle: float, t_min: Optional[Tensor], t_max: Optional[Tensor]):
    """The inputs of fsn_render_rays_occgrid_ex (rays or camera, bounds, grid, march, jitter, thresholds, masks) ->
    (held OccRenderArgs, R, device, march = the extended arguments (cone_angle, t_min, t_max))."""
    h = _Held(L.OccRenderArgs())
    a = h.a
    R, dev = _ray_source(h, rays_o, rays_d, camera)
    march = _occ_march_options(R, cone_angle, t_min, t_max, camera, h)
    for i in range(6):
        a.aabb[i] = float(aabb[i])
    a.res, a.levels = int(res), int(levels)
    h.set("bits", bits)
    a.near_plane, a.far_plane, a.step, a.max_steps = float(near_plane), float(far_plane), float(step), int(max_steps)
    if u is not None:
        u = _f32(u, "u").reshape(-1)
        if u.numel() != R:
            raise ValueError("u must hold one value per ray")
        h.set("u", u)
    a.early_stop_eps, a.alpha_thre = float(early_stop_eps), float(alpha_thre)
    _masks(h, pos_mask, dir_mask)
    return h, R, dev, march


def _occ_launch(pm: "PackedMLP", h: _Held, march, ends: Optional[Tensor], dev, status: Optional[Tensor] = None,
                launch: bool = True, **door) -> None:
    """The end of both occupancy wrappers: the work counter, the status word and the launch itself."""
    # (one queue counter PER CALL - ADVICE r3: a per-device buffer let two launches on different streams race on it; the
    # launch zeroes it itself)
    h.set("work_counter", torch.empty(1, dtype=torch.int64, device=dev))
    h.set("status", status_word(dev) if status is None else status)
    if launch:
        _launch("fsn_render_rays_occgrid_ex", dev, C.byref(pm.desc), pm.prec, pm.blob, C.byref(h.a), *march, ends, **door)


def _occ_gather(n_kept: Tensor, t0_slots: Tensor, t1_slots: Optional[Tensor], cap: int, R: int, step: float,
                slots: Optional[Dict[str, Tensor]] = None):
    """The tail of both occupancy wrappers: exclusive scan of the kept counts, ONE host read, the packed outputs and
    fsn_occ_gather_ex -> (ray_indices int64 [N], t_starts [N], t_ends [N], extras).  `slots`: the extras' slot rows
    (weights, alphas, trans, sigmas, rgbs), gathered into `extras`; None: interval starts and ends only."""
    dev = n_kept.device
    order = ("weights", "alphas", "trans", "sigmas", "rgbs") if slots is not None else ()
    incl = torch.cumsum(n_kept, 0, dtype=torch.int64)
    N = int(incl[-1].item()) if R > 0 else 0  # the one host read: the sample count sizes the outputs
    ri = torch.empty(N, dtype=torch.int64, device=dev)
    ts, te = torch.empty(N, device=dev), torch.empty(N, device=dev)
    ex = {k: torch.empty(N, 3, device=dev) if k == "rgbs" else torch.empty(N, device=dev) for k in order}
    if N > 0:
        sp = _ptr_array([slots[k] for k in order]) if order else None
        op = _ptr_array([ex[k] for k in order]) if order else None
        _launch("fsn_occ_gather_ex", dev, n_kept, incl - n_kept, t0_slots, t1_slots, cap, R, float(step), ri, ts, te, sp, op)
    return ri, ts, te, ex


def occ_sample_fused(pm: PackedMLP, rays_o: Tensor, rays_d: Tensor, *, aabb: Sequence[float], res: int, levels: int, bits: Tensor,
                     near_plane: float, far_plane: float, step: float, max_steps: int, u: Optional[Tensor] = None,
                     early_stop_eps: float = 1e-4, alpha_thre: float = 0.0, pos_mask: Optional[Tensor] = None,
                     dir_mask: Optional[Tensor] = None, status: Optional[Tensor] = None, cone_angle: float = 0.0,
                     t_min: Optional[Tensor] = None, t_max: Optional[Tensor] = None):
    """OccGridEstimator.sampling(..., sigma_fn = the model's density) of a training step as ONE launch + one gather:
    grid march -> density pass -> visibility cull inside persistent workgroups (the sampler mode of
    fsn_render_rays_occgrid), the kept samples of every ray in a slot of its own, then an exclusive scan of the counts,
    ONE host read (the sample count sizes the outputs) and fsn_occ_gather_samples.  -> (ray_indices int64 [N], t_starts
    [N], t_ends [N]): what occgrid_march (two launches + a read) -> density pass -> packed_visibility -> compaction
    (a second read) give, bit for bit.  `cone_angle` / `t_min` / `t_max`: occgrid_march's (fsn_render_rays_occgrid_ex);
    with a cone angle the launch also leaves the kept samples' interval ends in slot rows, which the gather copies."""
    h, Rn, dev, march = _occ_args(rays_o, rays_d, None, aabb, res, levels, bits, near_plane, far_plane, step, max_steps, u,
                                  early_stop_eps, alpha_thre, pos_mask, dir_mask, cone_angle, t_min, t_max)
    a, cap = h.a, int(max_steps)
    n_kept = torch.zeros(Rn, dtype=torch.int32, device=dev)
    slots = torch.empty(max(Rn, 1), cap, dtype=torch.float32, device=dev)
    ends = torch.empty_like(slots) if cone_angle > 0.0 else None  # (uniform regime: t_end = t_start + step)
    a.sample_cap = cap
    h.set("n_kept", n_kept)
    h.set("sample_t0", slots)
    _occ_launch(pm, h, march, ends, dev, status, launch=Rn > 0, what="fsn_render_rays_occgrid_ex (sampler mode)")
    return _occ_gather(n_kept, slots, ends, cap, Rn, step)[:3]


def render_occ_fused(pm: PackedMLP, rays_o: Optional[Tensor], rays_d: Optional[Tensor], *, aabb: Sequence[float], res: int,
                     levels: int, bits: Tensor, near_plane: float, far_plane: float, step: float, max_steps: int,
                     u: Optional[Tensor] = None, early_stop_eps: float = 1e-4, alpha_thre: float = 0.0,
                     bkgd=(0.0, 0.0, 0.0), pos_mask: Optional[Tensor] = None, dir_mask: Optional[Tensor] = None,
                     camera=None, want_counts: bool = False, want_extras: bool = False, cone_angle: float = 0.0,
                     t_min: Optional[Tensor] = None, t_max: Optional[Tensor] = None):
    """render_rays with the occupancy estimator in ONE launch (fsn_render_rays_occgrid): grid march -> density pass ->
    visibility cull -> full pass -> packed integration, no host sync.  -> colors [R,3], opacity [R,1], depth [R,1],
    counts {"n_cand", "n_kept"} (int32 [R]) when asked for.  `camera` as in render_fused.
    `want_extras` (EXTRAS mode): the launch also leaves the kept samples' weights / alphas / trans / sigmas / rgbs and
    interval starts in per-ray slot rows; behind an exclusive scan of the kept counts and ONE host read (the sample count
    sizes the outputs) fsn_occ_gather_extras packs them: -> colors, opacity, depth, counts, (ray_indices int64 [N],
    t_starts [N], t_ends [N], extras {weights, alphas, trans, sigmas [N], rgbs [N,3]}) - render_rays' full return
    contract (rendering.py:88-107) from one launch + one gather.
    `cone_angle` / `t_min` / `t_max`: occgrid_march's (fsn_render_rays_occgrid_ex; the bounds need ray tensors); with a
    cone angle the extras mode holds a ninth slot row per sample, the interval ends."""
    h, R, dev, march = _occ_args(rays_o, rays_d, camera, aabb, res, levels, bits, near_plane, far_plane, step, max_steps, u,
                                 early_stop_eps, alpha_thre, pos_mask, dir_mask, cone_angle, t_min, t_max)
    a, cap = h.a, int(max_steps)
    for i in range(3):
        a.bkgd[i] = float(bkgd[i])
    colors = torch.empty(R, 3, device=dev)
    opacity = torch.empty(R, 1, device=dev)
    depth = torch.empty(R, 1, device=dev)
    counts = {}
    if want_counts or want_extras:
        counts = {"n_cand": torch.zeros(R, dtype=torch.int32, device=dev), "n_kept": torch.zeros(R, dtype=torch.int32, device=dev)}
    slots = {}
    if want_extras:
        slots = {k: torch.empty(max(R, 1), cap, device=dev) for k in ("t0", "weights", "alphas", "trans", "sigmas")}
        slots["rgbs"] = torch.empty(max(R, 1), cap, 3, device=dev)
        if cone_angle > 0.0:  # (uniform regime: t_end = t_start + step)
            slots["t1"] = torch.empty(max(R, 1), cap, device=dev)
        a.sample_cap = cap
    for k, t in (("colors", colors), ("opacity", opacity), ("depth", depth), *counts.items()):
        h.set(k, t)
    for k, t in slots.items():  # (the interval ends, "t1", are an argument of the launch, not a field)
        if k != "t1":
            h.set("sample_t0" if k == "t0" else "ex_" + k, t)
    _occ_launch(pm, h, march, slots.get("t1"), dev, timed=True)
    if want_extras:
        return colors, opacity, depth, counts, _occ_gather(counts["n_kept"], slots["t0"], slots.get("t1"), cap, R, step, slots)
    return colors, opacity, depth, counts


def packed_visibility(sigmas: Tensor, t_starts: Tensor, t_ends: Tensor, ray_indices: Tensor, n_rays: int,
                      early_stop_eps: float, alpha_thre: float) -> Tensor:
    sig, t0, t1 = _f32(sigmas, "sigmas").reshape(-1), _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends")
    N = sig.numel()
    keep = torch.zeros(N, device=sig.device, dtype=torch.uint8)
    ri = _i64(ray_indices, "ray_indices")
    _launch("fsn_packed_visibility", sig.device, sig, t0, t1, ri, N, int(n_rays), float(early_stop_eps), float(alpha_thre),
            keep)
    return keep.bool()


def occgrid_update(occs: Tensor, bits: Tensor, cells: Optional[Tensor], vals: Optional[Tensor], decay: float,
                   threshold: Optional[Tensor]) -> None:
    """occs[cells] = max(occs[cells]*decay, vals) (unique cells), then bits = occs > threshold (device scalar)."""
    n = 0 if cells is None else cells.numel()
    thr = None if threshold is None else _f32(threshold, "threshold").reshape(1)
    vals = _opt_f32(vals, "vals")
    _launch("fsn_occgrid_update", occs.device, occs, occs.numel(), cells, vals, n, float(decay), thr, bits)


def occgrid_select(bits: Tensor, aabb: Sequence[float], res: int, levels: int, lvl: int, all_cells: bool, n_uniform: int,
                   n_occupied: int, seed: int, scratch: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Cells of level `lvl` an update re-evaluates and a random point inside each (fsn_occgrid_select) ->
    (cells int64 [n] global indices, x [n,3]); n = res^3 (all_cells) or n_uniform + n_occupied.  No host sync.
    n_uniform draws are uniform over the level, with replacement.  The n_occupied draws follow nerfacc's rule: with
    m <= n_occupied occupied cells they are those cells in index order, each once, then the sentinel cell -1 (its x is
    still a point inside the level's box; occgrid_update / occgrid_update_multi skip it); with m > n_occupied they are
    uniform over the occupied cells, with replacement."""
    res3 = res ** 3
    n = res3 if all_cells else int(n_uniform) + int(n_occupied)
    dev = bits.device
    cells = torch.empty(n, dtype=torch.int64, device=dev)
    x = torch.empty(n, 3, dtype=torch.float32, device=dev)
    if scratch is None and not all_cells and n_occupied > 0:
        scratch = torch.empty(res3 // 32 + 1, dtype=torch.int32, device=dev)
    ab = (C.c_float * 6)(*[float(v) for v in aabb])
    _launch("fsn_occgrid_select", dev, bits, int(res), int(levels), int(lvl), ab, 1 if all_cells else 0, int(n_uniform),
            int(n_occupied), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), scratch, cells, x)
    return cells, x


def occgrid_update_multi(occs: Tensor, pending: Tensor, cells: Tensor, vals: Tensor, decay: float) -> None:
    """occs[c] = max(occs[c]*decay, max of the vals drawn for c); `cells` may repeat (fsn_occgrid_update_multi)."""
    n = cells.numel()
    vals = _f32(vals, "vals").reshape(-1)
    _launch("fsn_occgrid_update_multi", occs.device, occs, occs.numel(), pending, cells, vals, n, float(decay))


def occgrid_refresh(pm: PackedMLP, bits: Tensor, aabb: Sequence[float], res: int, levels: int, all_cells: bool,
                    n_uniform: int, n_occupied: int, seeds: Sequence[int], step: float, pending: Tensor,
                    prefix: Optional[Tensor] = None, pos_mask: Optional[Tensor] = None) -> None:
    """The draws of ALL levels of an update, their densities in the single-pass mode of `pm` (FSN_PREC_FP16 / _BF16) and
    pending[cell] = max(key(sigma * step)) in one launch (fsn_occgrid_refresh): what occgrid_select -> mlp_fwd -> `* step`
    -> the first half of occgrid_update_multi do per level, same draws (seeds[l]: level l's seed) and same values bit
    for bit, without the points, cells and densities in memory.  occgrid_apply_pending makes it the grid's.  prefix:
    int32 [levels * (res^3/32 + 1)] scratch of the occupied draws.  Reports into the device's range word."""
    res3 = int(res) ** 3
    dev = bits.device
    if prefix is None and not all_cells and n_occupied > 0:
        prefix = torch.empty(int(levels) * (res3 // 32 + 1), dtype=torch.int32, device=dev)
    if len(seeds) != int(levels):
        raise ValueError("occgrid_refresh: one seed per level")
    ab = (C.c_float * 6)(*[float(v) for v in aabb])
    sd = (C.c_uint64 * int(levels))(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in seeds])
    pmk = _opt_f32(pos_mask, "pos_mask")
    _launch("fsn_occgrid_refresh", dev, C.byref(pm.desc), pm.prec, pm.blob, pmk, bits, int(res), int(levels), ab,
            1 if all_cells else 0, int(n_uniform), int(n_occupied), sd, float(step), prefix, pending, status_word(dev))


def occgrid_apply_pending(occs: Tensor, pending: Tensor, decay: float) -> None:
    """occs[c] = max(occs[c] * decay, pending[c]) for the cells a refresh touched; `pending` is cleared
    (fsn_occgrid_apply_pending: the second half of occgrid_update_multi)."""
    _launch("fsn_occgrid_apply_pending", occs.device, occs, occs.numel(), pending, float(decay))


def occgrid_visibility(aabb: Sequence[float], res: int, levels: int, cams: Tensor, width: int, height: int,
                       near_plane: float, min_views: int, visible: Tensor, ndc: Optional[Tuple[float, float, float]] = None) -> None:
    """visible (int32 [levels res^3 / 32], layout of `bits`) = the cells at least `min_views` of the cameras cover and
    none is too near to (fsn_occgrid_visibility; the rule is in include/fsnerf_hip.h).  cams: device float32 [N,16], the
    world -> camera map [3,4] then fx, fy, cx, cy.  ndc: (W / 2f, H / 2f, near) of a grid in NDC space."""
    if not cams.is_cuda or not visible.is_cuda:
        raise RuntimeError("occgrid_visibility: needs device tensors (there is no CPU path)")
    if cams.dtype != torch.float32 or cams.dim() != 2 or cams.shape[1] != 16 or not cams.is_contiguous():
        raise ValueError("occgrid_visibility: cams must be a contiguous float32 [N,16]")
    if visible.dtype != torch.int32 or visible.numel() != int(levels) * int(res) ** 3 // 32:
        raise ValueError("occgrid_visibility: visible must be int32 [levels res^3 / 32]")
    ab = (C.c_float * 6)(*[float(v) for v in aabb])
    wf, hf, nr = (0.0, 0.0, 0.0) if ndc is None else (float(v) for v in ndc)
    _launch("fsn_occgrid_visibility", visible.device, ab, int(res), int(levels), cams, cams.shape[0], int(width), int(height),
            float(near_plane), int(min_views), 0 if ndc is None else 1, wf, hf, nr, visible)


def occgrid_update_masked(occs: Tensor, bits: Optional[Tensor], visible: Tensor, occ_thre: float, scratch: Tensor,
                          revive: bool = False) -> None:
    """The end of an update on a marked grid (fsn_occgrid_update_masked): occs = -1 at the invisible cells, bits =
    (occs > min(mean of occs over the visible cells, occ_thre)) & visible (bits None: occs only; revive: a visible cell
    holding -1 becomes 0).  scratch: float64 [2048].  No host sync."""
    if scratch.dtype != torch.float64 or scratch.numel() < 2048:
        raise ValueError("occgrid_update_masked: scratch must be float64 [2048]")
    _launch("fsn_occgrid_update_masked", occs.device, occs, occs.numel(), visible, float(occ_thre), 1 if revive else 0,
            scratch, bits)


# ------------------------------------------------------------------ evaluation metrics (run-nerf.py:108-191)
def _f32_view(t: Tensor, name: str) -> Tensor:
    """_f32 without the copy to a contiguous tensor: the metric kernels take any element strides."""
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    return t if t.dtype == torch.float32 else t.float()


def _gpu_f32_view(t: Tensor, name: str) -> Tensor:
    """_gpu_f32 without the copy: float32 or an error (a cast would hide the tensor a gradient belongs to)."""
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    return t


def _nchw_strides(t: Tensor):
    assert t.dim() == 4
    return (C.c_int64 * 4)(*t.stride())


def ssim_nchw(x: Tensor, y: Tensor, window: int, use_sample_covariance: bool, data_range: float, K1: float, K2: float,
              smap: Optional[Tensor] = None) -> Tensor:
    """fsn_ssim on two (N, C, H, W) views of any strides -> float64 [N + 1]: each image's SSIM, then their mean.
    smap (optional): a float32 (N, C, H, W) view of any strides that receives the uncropped S map."""
    x, y = _f32_view(x, "im1"), _f32_view(y, "im2")
    N, Ch, H, W = x.shape
    assert y.shape == x.shape and y.device == x.device
    dev = x.device
    out = torch.empty(N + 1, dtype=torch.float64, device=dev)
    ws = torch.empty(max(_size("fsn_ssim_workspace_doubles", None, N, Ch, H, W), 1), dtype=torch.float64, device=dev)
    _launch("fsn_ssim", dev, x, y, N, Ch, H, W, _nchw_strides(x), _nchw_strides(y), int(window),
            1 if use_sample_covariance else 0, float(data_range), float(K1), float(K2), ws, out, smap,
            None if smap is None else _nchw_strides(smap))
    return out


def ssim_grad_nchw(x: Tensor, y: Tensor, window: int, use_sample_covariance: bool, data_range: float, K1: float, K2: float,
                   upstream: Tensor, *, want_dx: bool = True, want_dy: bool = True, dx: Optional[Tensor] = None,
                   dy: Optional[Tensor] = None) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """fsn_ssim_grad on two float32 (N, C, H, W) views of any strides: the gradient of sum_n upstream[n] * ssim_n
    (ssim_n = ssim_nchw(...)[n]) -> (dx, dy), float32 (N, C, H, W); a gradient not wanted is None (not both).
    upstream: N values (float64 on the device as the kernel reads them; anything else is converted).  `dx` / `dy`:
    optional float32 (N, C, H, W) views of any strides to write into instead of new contiguous tensors."""
    x, y = _gpu_f32_view(x, "im1"), _gpu_f32_view(y, "im2")
    N, Ch, H, W = x.shape
    assert y.shape == x.shape and y.device == x.device
    if not (want_dx or want_dy):
        raise ValueError("ssim_grad_nchw: neither dx nor dy is wanted")
    dev = x.device
    if not upstream.is_cuda:
        raise RuntimeError("upstream: expected a GPU tensor (the HIP path has no CPU fallback)")
    up = upstream.detach().to(torch.float64).reshape(-1).contiguous()
    if up.numel() != N:
        raise ValueError(f"upstream: expected {N} values (one per image), got {up.numel()}")
    outs = []
    for want, t, name in ((want_dx, dx, "dx"), (want_dy, dy, "dy")):
        if not want:
            t = None
        elif t is None:
            t = torch.empty(x.shape, dtype=torch.float32, device=dev)
        elif t.dtype != torch.float32 or t.shape != x.shape or t.device != dev:
            raise ValueError(f"{name}: expected a float32 {tuple(x.shape)} view on {dev}")
        outs.append(t)
    ws = torch.empty(max(_size("fsn_ssim_grad_workspace_doubles", None, N, Ch, H, W), 1), dtype=torch.float64, device=dev)
    _launch("fsn_ssim_grad", dev, x, y, N, Ch, H, W, _nchw_strides(x), _nchw_strides(y), int(window),
            1 if use_sample_covariance else 0, float(data_range), float(K1), float(K2), up, ws, outs[0],
            None if outs[0] is None else _nchw_strides(outs[0]), outs[1], None if outs[1] is None else _nchw_strides(outs[1]))
    return outs[0], outs[1]


def psnr_nchw(x: Tensor, y: Tensor) -> Tensor:
    """fsn_psnr on two (N, C, H, W) views of any strides -> float32 [N + 1]: each image's -10 log10(MSE), then the
    stack's (one MSE over every element)."""
    x, y = _f32_view(x, "pred"), _f32_view(y, "gt")
    N, Ch, H, W = x.shape
    assert y.shape == x.shape and y.device == x.device
    dev = x.device
    out = torch.empty(N + 1, dtype=torch.float32, device=dev)
    ws = torch.empty(max(_size("fsn_psnr_workspace_doubles", None, N, Ch, H, W), 1), dtype=torch.float64, device=dev)
    _launch("fsn_psnr", dev, x, y, N, Ch, H, W, _nchw_strides(x), _nchw_strides(y), ws, out)
    return out


# ------------------------------------------------------------------ LPIPS-VGG (csrc/lpips.hip)
def lpips_pack(conv_w: Sequence[Tensor], conv_b: Sequence[Tensor], lin_w: Sequence[Tensor], shift: Tensor,
               scale: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """fsn_lpips_pack: the 13 VGG16 convolutions ([Cout, Cin, 3, 3], [Cout]), the 5 lin heads ([1, C, 1, 1]) and the
    scaling layer's shift / scale (3 values each) -> the kernels' uint8 blob on their device (re-uses `out`)."""
    dev = conv_w[0].device
    keep = [t.detach().to(dev, torch.float32).contiguous() for t in list(conv_w) + list(conv_b) + list(lin_w)]
    keep += [shift.detach().to(dev, torch.float32).reshape(-1).contiguous(),
             scale.detach().to(dev, torch.float32).reshape(-1).contiguous()]
    if not all(t.is_cuda for t in keep):
        raise RuntimeError("lpips_pack: expected GPU tensors (the HIP path has no CPU fallback)")
    nbytes = _size("fsn_lpips_pack_bytes", None)
    if out is None or out.numel() != nbytes or out.device != dev:
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _launch("fsn_lpips_pack", dev, _ptr_array(keep[:13]), _ptr_array(keep[13:26]), _ptr_array(keep[26:31]), keep[31], keep[32],
            out)
    return out


def lpips_vgg(packed: Tensor, x: Tensor, y: Tensor, normalize: bool) -> Tuple[Tensor, Tensor]:
    """fsn_lpips_vgg on two (N, 3, H, W) views of any strides -> (float32 [N], float32 [5, N]): each pair's LPIPS and
    its five per-tap values.  The workspace depends on H and W only."""
    x, y = _f32_view(x, "in0"), _f32_view(y, "in1")
    N, Ch, H, W = x.shape
    assert Ch == 3 and y.shape == x.shape and y.device == x.device
    dev = x.device
    out = torch.empty(N, dtype=torch.float32, device=dev)
    per = torch.empty(5, N, dtype=torch.float32, device=dev)
    ws = torch.empty(_size("fsn_lpips_workspace_floats", None, H, W), dtype=torch.float32, device=dev)
    _launch("fsn_lpips_vgg", dev, packed, x, y, N, H, W, _nchw_strides(x), _nchw_strides(y), 1 if normalize else 0, out, per,
            ws)
    return out, per


def lpips_grad_pack(conv_w: Sequence[Tensor], out: Optional[Tensor] = None) -> Tensor:
    """fsn_lpips_grad_pack: the 13 VGG16 convolution weights -> the data-gradient kernels' uint8 blob ([Cin][9 Cout]
    per layer, taps flipped) on their device (re-uses `out`)."""
    dev = conv_w[0].device
    keep = [t.detach().to(dev, torch.float32).contiguous() for t in conv_w]
    if len(keep) != 13 or not all(t.is_cuda for t in keep):
        raise RuntimeError("lpips_grad_pack: expected 13 GPU tensors (the HIP path has no CPU fallback)")
    nbytes = _size("fsn_lpips_grad_pack_bytes", None)
    if out is None or out.numel() != nbytes or out.device != dev:
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _launch("fsn_lpips_grad_pack", dev, _ptr_array(keep), out)
    return out


def lpips_vgg_fwd_save(packed: Tensor, x: Tensor, y: Tensor, normalize: bool, *, want_dx: bool = True,
                       want_dy: bool = True) -> Tuple[Tensor, Tensor, Tensor]:
    """fsn_lpips_vgg_fwd_save on two float32 (B, 3, H, W) views of any strides, all B pairs in one pass ->
    (float32 [B], float32 [5, B], workspace): lpips_vgg's values bit for bit, and the workspace lpips_vgg_bwd reads
    (the activations of the images that need a gradient)."""
    x, y = _gpu_f32_view(x, "in0"), _gpu_f32_view(y, "in1")
    B, Ch, H, W = x.shape
    assert Ch == 3 and y.shape == x.shape and y.device == x.device
    if not (want_dx or want_dy):
        raise ValueError("lpips_vgg_fwd_save: neither dx nor dy is wanted")
    dev = x.device
    out = torch.empty(B, dtype=torch.float32, device=dev)
    per = torch.empty(5, B, dtype=torch.float32, device=dev)
    ws = torch.empty(_size("fsn_lpips_train_workspace_floats", None, B, H, W, int(want_dx), int(want_dy)),
                     dtype=torch.float32, device=dev)
    _launch("fsn_lpips_vgg_fwd_save", dev, packed, x, y, B, H, W, _nchw_strides(x), _nchw_strides(y), 1 if normalize else 0,
            int(want_dx), int(want_dy), out, per, ws)
    return out, per, ws


def lpips_vgg_bwd(packed: Tensor, packed_grad: Tensor, workspace: Tensor, shape: Sequence[int], normalize: bool,
                  upstream: Tensor, *, want_dx: bool = True, want_dy: bool = True, dx: Optional[Tensor] = None,
                  dy: Optional[Tensor] = None) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """fsn_lpips_vgg_bwd on the workspace lpips_vgg_fwd_save returned for (B, 3, H, W) = `shape` and the same
    normalize / want_dx / want_dy: the gradient of sum_b upstream[b] * lpips_b -> (dx, dy), float32 (B, 3, H, W); a
    gradient not wanted is None.  upstream: B values on the device (converted to float64).  `dx` / `dy`: optional
    float32 (B, 3, H, W) views of any strides to write into instead of new contiguous tensors."""
    B, Ch, H, W = (int(v) for v in shape)
    assert Ch == 3
    if not (want_dx or want_dy):
        raise ValueError("lpips_vgg_bwd: neither dx nor dy is wanted")
    dev = workspace.device
    need = _size("fsn_lpips_train_workspace_floats", None, B, H, W, int(want_dx), int(want_dy))
    if workspace.dtype != torch.float32 or workspace.numel() != need or not workspace.is_contiguous():
        raise ValueError(f"lpips_vgg_bwd: workspace of {workspace.numel()} values, lpips_vgg_fwd_save's has {need}")
    if not upstream.is_cuda:
        raise RuntimeError("upstream: expected a GPU tensor (the HIP path has no CPU fallback)")
    up = upstream.detach().to(torch.float64).reshape(-1).contiguous()
    if up.numel() != B:
        raise ValueError(f"upstream: expected {B} values (one per pair), got {up.numel()}")
    outs = []
    for want, t, name in ((want_dx, dx, "dx"), (want_dy, dy, "dy")):
        if not want:
            t = None
        elif t is None:
            t = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        elif t.dtype != torch.float32 or tuple(t.shape) != (B, 3, H, W) or t.device != dev:
            raise ValueError(f"{name}: expected a float32 {(B, 3, H, W)} view on {dev}")
        outs.append(t)
    _launch("fsn_lpips_vgg_bwd", dev, packed, packed_grad, B, H, W, 1 if normalize else 0, int(want_dx), int(want_dy), up,
            workspace, outs[0], None if outs[0] is None else _nchw_strides(outs[0]), outs[1],
            None if outs[1] is None else _nchw_strides(outs[1]))
    return outs[0], outs[1]
