"""CPU: patch batches without a device - the anchor -> flat-index restatement (tests/patch_ref.py), epochs of anchors
over the library's host permutation, PatchLoader's bookkeeping with the launch replaced by a recorder, and argument
validation of fsn_ray_patch_batch / fsn_ssim_grad / SSIMLoss / PatchLoader."""
import ctypes as C

import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L
from fs_nerf_amd import ops
from fs_nerf_amd.core.loss import SSIMLoss
from fs_nerf_amd.nerfdata import PatchLoader, RayDataset

import patch_ref as PR

N_VIEWS, H, W = 3, 9, 13
GEOMETRIES = [(P, dil) for P in (1, 2, 4) for dil in (1, 2)]


def test_patch_indices_restatement():
    # P = 1: the anchors are the pixels themselves
    assert PR.n_anchors(N_VIEWS, H, W, 1, 1) == PR.n_anchors(N_VIEWS, H, W, 1, 2) == N_VIEWS * H * W
    assert np.array_equal(PR.patch_indices(np.arange(N_VIEWS * H * W), H, W, 1, 2), np.arange(N_VIEWS * H * W))
    # a 2 x 2 patch at dilation 2 spans 3 pixels: 7 x 11 anchors per view
    assert PR.n_anchors(N_VIEWS, H, W, 2, 2) == 3 * 7 * 11
    first_of_view_1, last = 7 * 11, 3 * 7 * 11 - 1
    assert PR.patch_indices([first_of_view_1], H, W, 2, 2).tolist() == [H * W, H * W + 2, H * W + 2 * W, H * W + 2 * W + 2]
    # the last anchor's patch ends at the last pixel of the last view
    assert PR.patch_indices([last], H, W, 2, 2)[-1] == N_VIEWS * H * W - 1
    assert PR.patch_indices([PR.n_anchors(N_VIEWS, H, W, 4, 2) - 1], H, W, 4, 2)[-1] == N_VIEWS * H * W - 1


@pytest.mark.parametrize("P,dil", GEOMETRIES)
def test_an_epoch_of_anchors_covers_every_anchor_once(P, dil):
    A = PR.n_anchors(N_VIEWS, H, W, P, dil)
    for epoch in (0, 1):
        order = ops.ray_perm_host(A, 7, epoch).numpy()
        assert np.array_equal(np.sort(order), np.arange(A))
        idx = PR.patch_indices(order, H, W, P, dil)
        assert idx.shape == (A * P * P,) and idx.min() >= 0 and idx.max() < N_VIEWS * H * W
        # every patch stays inside one view and is a dilated P x P grid
        grid = idx.reshape(A, P, P)
        assert np.all(grid // (H * W) == grid[:, :1, :1] // (H * W))
        assert np.all(np.diff(grid, axis=2) == dil) and np.all(np.diff(grid, axis=1) == dil * W)
        assert len(np.unique(grid[:, 0, 0])) == A  # distinct top-left pixels


# ---------------------------------------------------------------- loader bookkeeping
@pytest.fixture
def launches(monkeypatch):
    """ops.ray_patch_batch replaced by a recorder: every call is one launch; it returns (start, count, a colour tensor
    of count * P^2 rows, (seed, epoch)) in the four output slots."""
    calls = []

    def ray_patch_batch(poses12, images, H_, W_, focal, patch, dilation=1, **kw):
        assert images.dtype == torch.uint8 and tuple(images.shape[1:3]) == (H_, W_) and poses12.shape == (images.shape[0], 12)
        calls.append(dict(kw, patch=patch, dilation=dilation))
        return kw["start"], kw["count"], torch.zeros(kw["count"] * patch * patch, 3), (kw["seed"], kw["epoch"])
    monkeypatch.setattr(ops, "ray_patch_batch", ray_patch_batch)
    return calls


def _dataset():
    """A RayDataset around host tensors (its constructor needs a GPU; the recorder never looks at the data)."""
    ds = RayDataset.__new__(RayDataset)
    ds.imgs, ds.poses = torch.zeros(N_VIEWS, H, W, 3, dtype=torch.uint8), torch.eye(4).repeat(N_VIEWS, 1, 1)
    ds.poses12, ds.hwf = ds.poses[:, :3, :4].reshape(N_VIEWS, 12), (H, W, 10.0)
    ds.near, ds.far, ds.ndc, ds.white_bkgd, ds.device = 2.0, 6.0, False, False, torch.device("cpu")
    return ds


@pytest.mark.parametrize("P,dil", GEOMETRIES)
def test_patch_loader_batches_epochs_and_stop(launches, P, dil):
    A, B = PR.n_anchors(N_VIEWS, H, W, P, dil), 17
    ld = PatchLoader(_dataset(), P, B, dilation=dil, seed=5, with_index=True)
    assert len(ld) == -(-A // B) and ld.dataset.n_anchors(P, dil) == A
    got = list(iter(ld))
    assert [(g[0], g[1]) for g in got] == [(s, min(B, A - s)) for s in range(0, A, B)]  # a short last batch
    assert A % B != 0 and got[-1][2].shape == ((A % B) * P * P, 3)
    assert len(launches) == len(ld)  # one launch per next
    assert all(c["order"] == "permuted" and c["want_index"] and (c["patch"], c["dilation"]) == (P, dil) for c in launches)
    assert all(g[3] == (5, 0) for g in got)
    assert next(iter(ld))[3] == (5, 1)  # a new permutation per iter()
    # every anchor exactly once per epoch: the positions served are [0, A) and the permutation is a bijection of it
    assert sorted(p for g in got for p in range(g[0], g[0] + g[1])) == list(range(A))
    plain = PatchLoader(_dataset(), P, B, dilation=dil, shuffle=False)
    assert all(len(b) == 3 for b in plain) and launches[-1]["order"] == "identity" and not launches[-1]["want_index"]


def test_patch_loader_resume_and_rank_slices(launches):
    P, dil, B = 2, 2, 8
    A = PR.n_anchors(N_VIEWS, H, W, P, dil)
    ld = PatchLoader(_dataset(), P, B, dilation=dil, seed=9, with_index=True)
    for _ in iter(ld):
        pass
    it = iter(ld)
    head = [next(it) for _ in range(3)]
    state = ld.state_dict()
    assert state == {"seed": 9, "epoch": 1, "position": 3}
    rest = [(b[0], b[1], b[3]) for b in it]
    other = PatchLoader(_dataset(), P, B, dilation=dil, seed=77, with_index=True)
    other.load_state_dict(state)
    assert [(b[0], b[1], b[3]) for b in iter(other)] == rest and len(head) + len(rest) == len(ld)
    assert next(iter(other))[3] == (9, 2)
    # world / rank: the same permutation, disjoint slices of B anchors, the tail shorter than B * world dropped
    world = 4
    loaders = [PatchLoader(_dataset(), P, B, dilation=dil, seed=3, rank=r, world=world, with_index=True) for r in range(world)]
    steps = A // (B * world)
    assert all(len(x) == steps for x in loaders) and steps > 0 and A % (B * world) != 0
    per_rank = [list(iter(x)) for x in loaders]
    covered = []
    for g in range(steps):
        slices = [per_rank[r][g] for r in range(world)]
        assert all(s[1] == B and s[3] == (3, 0) for s in slices)
        covered += sorted(p for s in slices for p in range(s[0], s[0] + s[1]))
    assert covered == list(range(steps * B * world))


def test_patch_loader_refuses_patches_that_do_not_fit_and_cpu_tensors():
    ds = _dataset()
    for P, dil in ((10, 1), (4, 3), (0, 1), (2, 0)):  # 4 pixels 3 apart span 10 > H = 9
        with pytest.raises(ValueError):
            PatchLoader(ds, P, 4, dilation=dil)
    with pytest.raises(ValueError):
        PatchLoader(ds, 2, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        next(iter(PatchLoader(ds, 2, 4)))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ray_patch_batch(ds.poses12, None, H, W, 10.0, 2, count=1, want_rgb=False)


# ---------------------------------------------------------------- validation of the two entry points
def test_ray_patch_batch_argument_validation_without_gpu():
    lib = L.lib()
    one = C.c_void_p(1)  # never dereferenced: every call below fails its checks before a launch

    def call(images=one, C_=3, white=0, order=0, start=0, count=4, poses=one, n=2, H_=9, W_=13, P=2, dil=2, rgb=one,
             anchors=None):
        return lib.fsn_ray_patch_batch(poses, n, images, H_, W_, C_, 5.0, 0, 1.0, white, order, 0, 0, anchors, start, count,
                                       P, dil, one, one, rgb, None, None)
    A = PR.n_anchors(2, 9, 13, 2, 2)
    assert call(P=0) == -1 and b"bad patch" in lib.fsn_last_error()
    assert call(dil=0) == -1 and b"bad patch" in lib.fsn_last_error()
    assert call(P=4, dil=3) == -1 and b"does not fit" in lib.fsn_last_error()  # ext = 10 > H
    assert call(P=14, dil=1, H_=20) == -1 and b"does not fit" in lib.fsn_last_error()  # ext = 14 > W
    assert call(start=A - 3, count=4) == -1 and b"start + count > A" in lib.fsn_last_error()
    assert call(order=1, start=0, count=A + 1) == -1 and b"start + count > A" in lib.fsn_last_error()
    assert call(C_=5) == -1 and b"channels" in lib.fsn_last_error()
    assert call(C_=3, white=1) == -1 and b"white_bkgd" in lib.fsn_last_error()
    assert call(order=7) == -1 and b"order" in lib.fsn_last_error()
    assert call(H_=0) == -1 and b"geometry" in lib.fsn_last_error()
    assert call(poses=None) == -1 and b"null poses" in lib.fsn_last_error()
    assert call(images=None) == -1 and b"null images" in lib.fsn_last_error()  # colours asked for
    assert call(order=2, count=4) == -1 and b"null anchor list" in lib.fsn_last_error()
    assert call(order=2, start=1, count=4, anchors=one) == -1 and b"start = 0" in lib.fsn_last_error()
    assert call(count=0) == 0 and call(images=None, rgb=None, count=0) == 0  # an empty batch is not an error


def test_ssim_grad_argument_validation_without_gpu():
    lib = L.lib()
    one = C.c_void_p(1)
    st = (C.c_int64 * 4)(3 * 11 * 11, 11 * 11, 11, 1)

    def call(N=1, Cn=3, H_=11, W_=11, window=0, x=one, up=one, ws=one, dx=one, dy=one, xs=st, dxs=st, dys=st):
        return lib.fsn_ssim_grad(x, one, N, Cn, H_, W_, xs, st, window, 1, 1.0, 0.01, 0.03, up, ws, dx, dxs, dy, dys, None)
    assert call(Cn=0) == -1 and b"fsn_ssim_grad: bad shape" in lib.fsn_last_error()
    assert call(window=5) == -2 and b"window code" in lib.fsn_last_error()
    assert call(H_=10) == -1 and b"smaller than the 11x11 window" in lib.fsn_last_error()
    assert call(window=1, W_=6) == -1 and b"smaller than the 7x7 window" in lib.fsn_last_error()
    assert call(x=None) == -1 and b"null pointer" in lib.fsn_last_error()
    assert call(up=None) == -1 and b"null pointer" in lib.fsn_last_error()
    assert call(ws=None) == -1 and b"null pointer" in lib.fsn_last_error()
    assert call(dx=None, dy=None) == -1 and b"both gradients" in lib.fsn_last_error()
    assert call(xs=None) == -1 and b"null stride array" in lib.fsn_last_error()
    assert call(dy=None, dxs=None) == -1 and b"null stride array" in lib.fsn_last_error()
    assert call(N=0, x=None, up=None, ws=None, dx=None, dy=None) == 0  # N = 0 is a no-op
    assert lib.fsn_ssim_grad_workspace_doubles(2, 3, 12, 17) == 2 * 3 * 4 * 12 * 17
    assert lib.fsn_ssim_grad_workspace_doubles(2, 0, 12, 17) == -1
    buf = (C.c_uint32 * 4)()
    assert lib.fsn_debug_report(b"ssim_grad", buf) == -2 and b"not a debug build" in lib.fsn_last_error()


def test_ssim_loss_refuses_cpu_tensors_and_bad_arguments():
    x = torch.rand(2, 12, 12, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        SSIMLoss()(x, x.clone())
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ssim_grad_nchw(x.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2), L.FSN_SSIM_GAUSSIAN, True, 1.0, 0.01, 0.03,
                           torch.ones(2, dtype=torch.float64))
    with pytest.raises(ValueError, match="same shape"):
        SSIMLoss()(x, x[:1])
    with pytest.raises(ValueError, match="win_size"):
        SSIMLoss()(x[:, :10], x[:, :10])
    with pytest.raises(ValueError, match="reduction"):
        SSIMLoss(reduction="sum")
    with pytest.raises(ValueError):
        SSIMLoss(channel_axis=2)(x, x)
    SSIMLoss(gaussian_weights=False, channel_axis=1, reduction="none")  # the keywords of the issue are accepted
