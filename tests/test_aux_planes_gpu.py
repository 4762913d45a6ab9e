"""GPU: auxiliary float planes behind the data layer (csrc/raydata.hip: fsn_ray_batch_aux / fsn_ray_patch_batch_aux;
nerfdata/raydata.py; DESIGN 7 "Data layer").  Images 5 x 7, 3 views, planes of distinct bit patterns (NaN payloads, Inf):
the aux rows are compared as uint32 words against the NumPy gather of tests/depth_prior_ref.py, and every other output
bit for bit against the entry point without aux."""
import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import ops
from fs_nerf_amd.nerfdata import CameraRefiner, IntrinsicsRefiner, PatchLoader, RayDataset, RayLoader

import depth_prior_ref as DR
import intrinsics_ref as IR
import pose_refine_ref as PR
import test_pose_refine_gpu as TP

pytestmark = pytest.mark.gpu

N_VIEWS, H, W, FOCAL = 3, TP.H, TP.W, TP.FOCAL  # 5 x 7 images at focal 10: 105 rays
N_RAYS = N_VIEWS * H * W
SENTINEL = 0x7FC12345  # a NaN payload that is none of the planes' words


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def words(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.dtype == torch.float32:
        return a.shape == b.shape and np.array_equal(words(a), words(b))
    return torch.equal(a, b)


def dataset(dev, A, ndc=False, seed=0):
    ds = TP.dataset(dev, N_VIEWS, H, W, FOCAL, ndc, seed=seed)
    planes = DR.bit_planes(N_VIEWS, H, W, A, seed=A)
    ds.set_aux(planes if A > 1 else planes[..., 0])  # (one plane goes in as [n, H, W])
    assert ds.aux.shape == (N_VIEWS, H, W, A) and ds.aux.dtype == torch.float32 and ds.aux.device == ds.device
    assert ds.aux.is_contiguous() and np.array_equal(words(ds.aux), planes.view(np.uint32))
    return ds, planes


def cameras_of(ds, dev):
    """A random camera table and CameraRefiner poses for the dataset"""
    intr = IntrinsicsRefiner(ds, per_view=True, tie_focal=False)
    cam = CameraRefiner(ds)
    with torch.no_grad():
        intr.phi.copy_(IR.random_phi(N_VIEWS, np.random.default_rng(4)))
        cam.xi.copy_(PR.random_xi(N_VIEWS, 0.05, np.random.default_rng(1), tau=0.02))
    return cam, intr


def check_rows(planes, with_aux, without):
    o, d, rgb, index, aux = with_aux
    assert all(same_bits(x, y) for x, y in zip((o, d, rgb, index), without))
    A = planes.shape[3]
    assert aux.shape == (index.numel(), A) and aux.dtype == torch.float32 and not aux.requires_grad
    assert np.array_equal(words(aux), DR.aux_rows(planes, index.cpu().numpy()))


@pytest.mark.parametrize("A", [1, 4])
@pytest.mark.parametrize("ndc", [False, True])
def test_ray_batches_serve_the_aux_rows_bit_for_bit(dev, A, ndc):
    ds, planes = dataset(dev, A, ndc)
    cam, intr = cameras_of(ds, dev)
    rng = np.random.default_rng(7)
    for count in (1, 64, 65, N_RAYS):
        explicit = torch.from_numpy(rng.integers(0, N_RAYS, size=count)).to(dev)
        for order, kw in (("identity", dict(start=N_RAYS - count, count=count)),
                          ("permuted", dict(start=(N_RAYS - count) // 2, count=count, seed=11, epoch=2)),
                          ("explicit", dict(indices=explicit))):
            for cams in (dict(), dict(K=intr.K(), poses12=cam.poses12())):
                got = ds.batch(order, want_index=True, want_aux=True, **kw, **cams)
                assert len(got) == 5
                check_rows(planes, got, ds.batch(order, want_index=True, **kw, **cams))
    # every output is optional beside aux: aux alone, and aux without the index
    alone = ds.batch("permuted", start=3, count=70, seed=5, want_rays=False, want_rgb=False, want_aux=True)
    assert alone[:4] == (None, None, None, None)
    index = ds.batch("permuted", start=3, count=70, seed=5, want_rays=False, want_rgb=False, want_index=True)[3]
    assert np.array_equal(words(alone[4]), DR.aux_rows(planes, index.cpu().numpy()))
    # the default call is the 4-tuple it was
    assert len(ds.batch("identity", start=0, count=4)) == 4


@pytest.mark.parametrize("A", [1, 4])
@pytest.mark.parametrize("P", [1, 2, 3])
@pytest.mark.parametrize("dilation", [1, 2])
def test_patch_batches_serve_the_aux_rows_bit_for_bit(dev, A, P, dilation):
    ds, planes = dataset(dev, A)
    cam, intr = cameras_of(ds, dev)
    n_anchors = ds.n_anchors(P, dilation)
    rng = np.random.default_rng(P * 10 + dilation)
    for count in sorted({1, min(29, n_anchors), n_anchors}):  # 29 patches of 3 x 3 pixels: 261 rows, more than one block
        explicit = torch.from_numpy(rng.integers(0, n_anchors, size=count)).to(dev)
        for order, kw in (("identity", dict(start=n_anchors - count, count=count)),
                          ("permuted", dict(start=0, count=count, seed=3, epoch=1)),
                          ("explicit", dict(anchors=explicit))):
            for cams in (dict(), dict(K=intr.K(), poses12=cam.poses12())):
                got = ds.patch_batch(order, P, dilation, want_index=True, want_aux=True, **kw, **cams)
                assert got[4].shape == (count * P * P, A)
                check_rows(planes, got, ds.patch_batch(order, P, dilation, want_index=True, **kw, **cams))
    # ray-only patches (no images) still serve aux
    o, d, rgb, index, aux = ops.ray_patch_batch(ds.poses12, None, H, W, FOCAL, P, dilation, order="identity", start=0,
                                                count=2, want_rgb=False, want_index=True, aux=ds.aux, want_aux=True)
    assert rgb is None and np.array_equal(words(aux), DR.aux_rows(planes, index.cpu().numpy()))


@pytest.mark.parametrize("A", [1, 4])
def test_an_index_outside_the_range_leaves_its_aux_row_untouched(dev, A):
    """The outputs are pre-filled through the C-ABI (the wrappers allocate their own), so the call is made directly."""
    from fs_nerf_amd import _lib as L
    ds, planes = dataset(dev, A)
    assert not (planes.view(np.uint32) == SENTINEL).any()
    for patch in (0, 2):
        n_items = ds.n_anchors(patch, 1) if patch else N_RAYS
        items = torch.tensor([5, -1, n_items, 0, n_items - 1, 2 ** 40], dtype=torch.int64, device=dev)
        rows = items.numel() * max(patch * patch, 1)
        aux_out = torch.full((rows, A), 0.0, device=dev).view(torch.int32).fill_(SENTINEL).view(torch.float32)
        index = torch.full((rows,), -7, dtype=torch.int64, device=dev)
        rgb = torch.full((rows, 3), -7.0, device=dev)
        head = (ds.poses12, N_VIEWS, ds.imgs, H, W, 3, FOCAL, None, 0, 0, 1.0, 0, L.FSN_RAY_ORDER_EXPLICIT, 0, 0, items, 0,
                items.numel())
        tail = (None, None, rgb, index, ds.aux, A, aux_out)
        if patch:
            ops._launch("fsn_ray_patch_batch_aux", dev, *head, patch, 1, *tail)
        else:
            ops._launch("fsn_ray_batch_aux", dev, *head, *tail)
        torch.cuda.synchronize()
        pp = max(patch * patch, 1)
        bad = torch.tensor([False, True, True, False, False, True]).repeat_interleave(pp)
        got = words(aux_out)
        assert (got[bad.numpy()] == SENTINEL).all() and (index.cpu()[bad] == -7).all() and (rgb.cpu()[bad] == -7).all()
        good = ~bad
        assert (index.cpu()[good] >= 0).all()
        assert np.array_equal(got[good.numpy()], DR.aux_rows(planes, index.cpu()[good].numpy()))


def loader_rows(loader):
    return [tuple(t.detach() for t in batch) for batch in loader]


@pytest.mark.parametrize("A", [1, 4])
def test_loaders_with_aux(dev, A):
    ds, planes = dataset(dev, A)
    flat = planes.view(np.uint32).reshape(-1, A)
    # with and without the index: aux is the last element and the others are what they were
    for cls, args in ((RayLoader, (ds, 40)), (PatchLoader, (ds, 2, 7))):
        plain = loader_rows(cls(*args, shuffle=True, seed=3, with_index=True))
        both = loader_rows(cls(*args, shuffle=True, seed=3, with_index=True, with_aux=True))
        only = loader_rows(cls(*args, shuffle=True, seed=3, with_aux=True))
        assert len(plain) == len(both) == len(only) > 1
        for a, b, c in zip(plain, both, only):
            assert len(a) == 4 and len(b) == 5 and len(c) == 4
            assert all(same_bits(x, y) for x, y in zip(a, b[:4])) and all(same_bits(x, y) for x, y in zip(a[:3], c[:3]))
            assert same_bits(b[4], c[3]) and np.array_equal(words(b[4]), flat[a[3].cpu().numpy()])
            assert b[4].shape == (a[3].numel(), A)
        assert len(next(iter(cls(*args, seed=3)))) == 3
    # one epoch serves every pixel's aux exactly once
    served = np.concatenate([words(b[3]) for b in loader_rows(RayLoader(ds, 40, shuffle=True, seed=9, with_aux=True))])
    assert served.shape == (N_RAYS, A)
    assert sorted(map(tuple, served.tolist())) == sorted(map(tuple, flat.tolist()))
    # ... and patches of one pixel are the pixels
    served = np.concatenate([words(b[3]) for b in loader_rows(PatchLoader(ds, 1, 16, shuffle=True, seed=9, with_aux=True))])
    assert sorted(map(tuple, served.tolist())) == sorted(map(tuple, flat.tolist()))
    # resume: the batches after a state_dict() are the ones the original goes on to serve
    first = RayLoader(ds, 25, shuffle=True, seed=4, with_index=True, with_aux=True)
    it = iter(first)
    next(it), next(it)
    state = first.state_dict()
    rest = [tuple(t.detach() for t in b) for b in it]
    second = RayLoader(ds, 25, shuffle=True, seed=0, with_index=True, with_aux=True)
    second.load_state_dict(state)
    resumed = loader_rows(second)
    assert len(rest) == len(resumed) == 3 and all(same_bits(x, y) for a, b in zip(rest, resumed) for x, y in zip(a, b))
    # world = 3: rank r's batch g is slice r of the world = 1 loader's rows [g * 3 B, (g + 1) * 3 B)
    B = 10
    whole = loader_rows(RayLoader(ds, B * 3, shuffle=True, seed=6, with_index=True, with_aux=True))
    for rank in range(3):
        part = loader_rows(RayLoader(ds, B, shuffle=True, seed=6, rank=rank, world=3, with_index=True, with_aux=True))
        assert len(part) == N_RAYS // (3 * B) == 3
        for g, b in enumerate(part):
            assert all(same_bits(x, y[rank * B:(rank + 1) * B]) for x, y in zip(b, whole[g]))
    whole = loader_rows(PatchLoader(ds, 2, 6, shuffle=True, seed=6, with_index=True, with_aux=True))
    for rank in range(3):
        part = loader_rows(PatchLoader(ds, 2, 2, shuffle=True, seed=6, rank=rank, world=3, with_index=True, with_aux=True))
        assert len(part) == ds.n_anchors(2) // 6
        for g, b in enumerate(part):
            assert all(same_bits(x, y[rank * 8:(rank + 1) * 8]) for x, y in zip(b, whole[g]))
    # a dataset without planes
    bare = TP.dataset(dev, N_VIEWS, H, W, FOCAL, False)
    assert bare.aux is None
    for make in (lambda: RayLoader(bare, 10, with_aux=True), lambda: PatchLoader(bare, 2, 2, with_aux=True),
                 lambda: bare.batch("identity", start=0, count=1, want_aux=True),
                 lambda: bare.patch_batch("identity", 2, start=0, count=1, want_aux=True)):
        with pytest.raises(ValueError):
            make()
    for bad in (np.zeros((N_VIEWS, H, W, 5), np.float32), np.zeros((N_VIEWS, H, W + 1), np.float32),
                np.zeros((N_VIEWS, H, W, 0), np.float32)):
        with pytest.raises(ValueError):
            bare.set_aux(bad)
    with pytest.raises(TypeError):
        bare.set_aux(np.zeros((N_VIEWS, H, W), np.float64))
    made = RayDataset.blender(bare.imgs.cpu(), bare.poses, (H, W, FOCAL), False, dev)
    assert made.aux is None
    made = RayDataset(bare.imgs.cpu(), bare.poses, (H, W, FOCAL), near=2.0, far=6.0, device=dev, aux=planes)
    assert np.array_equal(words(made.aux), planes.view(np.uint32))


@pytest.mark.parametrize("patches", [False, True])
def test_learnable_cameras_with_aux_keep_their_gradient_bits(dev, patches):
    ds, planes = dataset(dev, 4)
    flat = planes.view(np.uint32).reshape(-1, 4)
    grads = []
    for with_aux in (False, True):
        cam, intr = cameras_of(ds, dev)
        if patches:
            loader = PatchLoader(ds, 2, 9, shuffle=True, seed=8, with_index=True, cameras=cam, intrinsics=intr, with_aux=with_aux)
        else:
            loader = RayLoader(ds, 50, shuffle=True, seed=8, with_index=True, cameras=cam, intrinsics=intr, with_aux=with_aux)
        batch = next(iter(loader))
        assert len(batch) == 4 + with_aux
        o, d, rgb, index = batch[:4]
        assert o.requires_grad and d.requires_grad and not rgb.requires_grad
        if with_aux:
            aux = batch[4]
            assert not aux.requires_grad
            assert np.array_equal(words(aux), flat[index.cpu().numpy()])
        g = torch.Generator().manual_seed(0)
        go, gd = torch.randn(o.shape, generator=g).to(dev), torch.randn(d.shape, generator=g).to(dev)
        ((o * go).sum() + (d * gd).sum()).backward()
        assert bool(cam.xi.grad.any()) and bool(intr.phi.grad.any())
        grads.append((o.detach(), d.detach(), cam.xi.grad.clone(), intr.phi.grad.clone()))
    assert all(same_bits(x, y) for x, y in zip(*grads))
