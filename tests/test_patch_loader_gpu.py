"""-m gpu: patch batches (fsn_ray_patch_batch through RayDataset.patch_batch and PatchLoader): every batch is bit for bit
`dataset.batch("explicit", indices=expected)` with `expected` from the Python restatement of tests/patch_ref.py over
the NumPy permutation of tests/raydata_ref.py."""
import math

import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import ops
from fs_nerf_amd.nerfdata import PatchLoader, RayDataset

import patch_ref as PR
import raydata_ref as RR

pytestmark = pytest.mark.gpu

N_VIEWS, H, W = 3, 9, 13
HWF = (H, W, 0.9 * W)
GEOMETRIES = [(P, dil) for P in (1, 2, 4) for dil in (1, 2)]
CASES = [(3, False, True), (4, True, False), (4, True, True), (3, False, False)]  # (C, white_bkgd, ndc)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def forward_poses(n, seed=0):
    """[n,4,4] forward-facing cameras a few degrees off identity (NDC rays stay far from d_z = 0)."""
    rng = np.random.default_rng(seed)
    out = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    for k in range(n):
        ax, ay = np.radians(rng.uniform(-5, 5, size=2))
        Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
        Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
        out[k, :3, :3] = (Ry @ Rx).astype(np.float32)
        out[k, :3, 3] = rng.uniform(-0.15, 0.15, size=3)
    return out


def dataset(dev, C, white, ndc):
    imgs = np.random.default_rng(C).integers(0, 256, size=(N_VIEWS, H, W, C), dtype=np.uint8)
    return RayDataset(imgs, forward_poses(N_VIEWS), HWF, near=0.0, far=1.0, ndc=ndc, white_bkgd=white, device=dev)


def same(got, want):
    return all(torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("P,dil", GEOMETRIES)
@pytest.mark.parametrize("C,white,ndc", CASES)
def test_every_batch_of_an_epoch_is_the_explicit_route(dev, C, white, ndc, P, dil):
    ds = dataset(dev, C, white, ndc)
    A, B, seed = PR.n_anchors(N_VIEWS, H, W, P, dil), 50, 21
    assert ds.n_anchors(P, dil) == A
    ld = PatchLoader(ds, P, B, dilation=dil, seed=seed, with_index=True)
    for epoch in (0, 1):
        order = RR.perm(A, seed, epoch)
        batches = list(ld)
        assert len(batches) == len(ld) == -(-A // B) and A % B != 0
        for k, (o, d, rgb, index) in enumerate(batches):
            anchors = order[k * B:(k + 1) * B]  # the last one is short
            expected = torch.from_numpy(PR.patch_indices(anchors, H, W, P, dil)).to(dev)
            assert o.shape == d.shape == rgb.shape == (len(anchors) * P * P, 3)
            assert torch.equal(index, expected)
            assert same((o, d, rgb), ds.batch("explicit", indices=expected)[:3])
    # the patch stack: rgb.view(B, P, P, 3)[b, i, j] is pixel (r0 + i dil, c0 + j dil) of the anchor's view
    o, d, rgb, index = ds.patch_batch("identity", P, dil, start=A - 2, count=2, want_index=True)
    full = ds.batch("identity", start=0, count=len(ds))[2].view(N_VIEWS, H, W, 3)
    ext = (P - 1) * dil + 1
    assert torch.equal(rgb.view(2, P, P, 3)[1], full[-1, H - ext::dil, W - ext::dil])
    # no shuffle: identity order; three-tuples without with_index
    first = next(iter(PatchLoader(ds, P, 4, dilation=dil, shuffle=False)))
    assert len(first) == 3 and same(first, ds.batch("explicit", indices=torch.from_numpy(
        PR.patch_indices(np.arange(4), H, W, P, dil)).to(dev))[:3])


def test_ray_only_patches_without_images(dev):
    ds = dataset(dev, 4, True, True)
    P, dil = 4, 2
    A = PR.n_anchors(N_VIEWS, H, W, P, dil)
    kw = dict(ndc=True, near=1.0, order="permuted", seed=3, epoch=2, start=5, count=A - 5)
    o, d, rgb, index = ops.ray_patch_batch(ds.poses12, None, H, W, HWF[2], P, dil, want_rgb=False, want_index=True, **kw)
    wo, wd, wrgb, windex = ops.ray_patch_batch(ds.poses12, ds.imgs, H, W, HWF[2], P, dil, white_bkgd=True, want_index=True, **kw)
    assert rgb is None and wrgb is not None
    assert torch.equal(o, wo) and torch.equal(d, wd) and torch.equal(index, windex)
    with pytest.raises(ValueError):
        ops.ray_patch_batch(ds.poses12, None, H, W, HWF[2], P, dil, **kw)
    # outputs not asked for are not made
    assert ds.patch_batch("identity", P, dil, count=2, want_rays=False)[:2] == (None, None)


def test_explicit_anchors_and_out_of_range_rows_stay_untouched(dev):
    ds = dataset(dev, 3, False, False)
    P, dil = 2, 2
    A = PR.n_anchors(N_VIEWS, H, W, P, dil)
    anchors = torch.tensor([0, A, 17, -1, A - 1, 2 ** 40], device=dev)
    good = torch.tensor([True, False, True, False, True, False])
    o, d, rgb, index = ds.patch_batch("explicit", P, dil, anchors=anchors.to(torch.int32)[:5], want_index=True)  # int32 is widened
    assert index.shape == (5 * P * P,)
    # pre-filled outputs through the C entry point: the rows of the bad anchors keep the sentinel
    rows = anchors.numel() * P * P
    so, sd, sc = (torch.full((rows, 3), -9.0, device=dev) for _ in range(3))
    si = torch.full((rows,), -9, device=dev, dtype=torch.int64)
    ops._launch("fsn_ray_patch_batch", dev, ops._p(ds.poses12), N_VIEWS, ops._p(ds.imgs), H, W, 3, float(HWF[2]), 0, 1.0, 0,
                ops._RAY_ORDERS["explicit"], 0, 0, ops._p(anchors), 0, anchors.numel(), P, dil, ops._p(so), ops._p(sd),
                ops._p(sc), ops._p(si))
    keep = good.repeat_interleave(P * P).to(dev)
    expected = torch.from_numpy(PR.patch_indices(anchors[good.to(dev)].cpu().numpy(), H, W, P, dil)).to(dev)
    assert torch.equal(si[keep], expected) and torch.all(si[~keep] == -9)
    wo, wd, wc, _ = ds.batch("explicit", indices=expected)
    assert torch.equal(so[keep], wo) and torch.equal(sd[keep], wd) and torch.equal(sc[keep], wc)
    assert torch.all(so[~keep] == -9.0) and torch.all(sd[~keep] == -9.0) and torch.all(sc[~keep] == -9.0)
    with pytest.raises(ValueError):
        ds.patch_batch("identity", 4, 3, count=1)  # 4 pixels 3 apart span 10 > H
    with pytest.raises(RuntimeError, match="start \\+ count > A"):
        ds.patch_batch("permuted", P, dil, start=A - 1, count=2)
