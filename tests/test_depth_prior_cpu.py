"""CPU: the mathematics behind the monocular-depth-prior losses (tests/depth_prior_ref.py restates them) and
the presence of the feature's interface.  No GPU is touched."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L
from fs_nerf_amd import ops
from fs_nerf_amd.core import loss as loss_mod

import depth_prior_ref as DR

SYMBOLS = ("fsn_ray_batch_aux", "fsn_ray_patch_batch_aux", "fsn_ssi_depth_fwd", "fsn_ssi_depth_bwd",
           "fsn_depth_rank_fwd", "fsn_depth_rank_bwd")


def patches(B, P, Q, seed, nan_every=0, weights=False):
    """depth in [2, 6], a prior that is an affine map of another noisy depth, optional NaN priors and weights"""
    g = torch.Generator().manual_seed(seed)
    depth = 2.0 + 4.0 * torch.rand(B, P, Q, generator=g, dtype=torch.float64)
    prior = 0.7 * (depth + 0.5 * torch.rand(B, P, Q, generator=g, dtype=torch.float64)) - 1.3
    if nan_every:
        flat = prior.reshape(-1)
        flat[torch.arange(0, flat.numel(), nan_every)] = float("nan")
    weight = None
    if weights:
        weight = torch.rand(B, P, Q, generator=g, dtype=torch.float64) - 0.2  # a fifth of them masked (<= 0)
    return depth, prior, weight


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("weights", [False, True])
def test_envelope_autograd_through_the_fit_equals_the_partial_derivative(inverse, weights):
    depth, prior, weight = patches(4, 5, 13, seed=1, nan_every=7, weights=weights)
    depth.requires_grad_(True)
    L_b = DR.ssi_loss(depth, prior, weight, inverse=inverse)
    assert L_b.dtype == torch.float64 and bool((L_b > 0).all())
    up = torch.tensor([1.0, 0.5, 2.0, 1.5], dtype=torch.float64)
    (L_b * up).sum().backward()
    want = DR.ssi_partial_grad(depth.detach(), prior, weight, inverse=inverse) * up[:, None, None]
    err = DR.rel_error(depth.grad, want)
    print(f"envelope inverse={inverse} weights={weights}: relative difference {err:.3e}")
    assert err <= 1e-12
    bad = ~DR.valid_mask(depth.detach(), prior, weight)
    assert bool(bad.any()) and not bool(depth.grad[bad].any())


def test_invariance_under_affine_maps_of_depth_and_scaling_with_the_prior():
    depth, prior, weight = patches(3, 4, 6, seed=2, nan_every=5, weights=True)
    base = DR.ssi_loss(depth, prior, weight)
    for a, b in ((3.0, 1.0), (-0.5, 2.0), (1e-2, -4.0)):
        moved = DR.ssi_loss(a * depth + b, prior, weight)
        assert DR.rel_error(moved, base) <= 1e-9, (a, b)
        scaled = DR.ssi_loss(depth, a * prior + b, weight)
        assert DR.rel_error(scaled, a * a * base) <= 1e-9, (a, b)


def test_degenerate_patches_give_zero_and_no_gradient():
    depth, prior, _ = patches(4, 3, 5, seed=3)
    weight = torch.ones_like(depth)
    depth[0] = 3.0          # a constant patch fixes no scale
    weight[1] = 0.0
    weight[1, 1, 2] = 1.0   # one valid pixel
    weight[2] = 0.0         # all masked
    for inverse in (False, True):
        d = depth.clone().requires_grad_(True)
        L_b, s, t, M, deg, _ = DR.ssi_fit(d, prior, weight, inverse=inverse)
        assert deg.tolist() == [True, True, True, False]
        assert L_b[:3].tolist() == [0.0, 0.0, 0.0] and float(L_b[3].detach()) > 0
        L_b.sum().backward()
        assert not bool(d.grad[:3].any()) and bool(d.grad[3].any()) and bool(torch.isfinite(d.grad).all())
        assert not bool(DR.ssi_partial_grad(depth, prior, weight, inverse=inverse)[:3].any())
        assert float(DR.ssi_mean(depth, prior, weight, inverse=inverse)) == float(L_b[3].detach())


def test_ranking_pair_count_on_a_hand_example():
    # 2 x 2: priors 0 < 1 < 2 and one NaN; the ranked ordered pairs are (0,1), (0,2), (1,2) - indices in row-major order
    prior = torch.tensor([[[0.0, 1.0], [2.0, float("nan")]]], dtype=torch.float64)
    depth = torch.tensor([[[3.0, 2.0], [4.0, 1.0]]], dtype=torch.float64)
    out, pairs = DR.rank_loss(depth, prior, margin=0.25)
    assert pairs.tolist() == [3]
    # hinges: (0,1): 3 - 2 + .25 = 1.25;  (0,2): 3 - 4 + .25 < 0;  (1,2): 2 - 4 + .25 < 0
    assert out.tolist() == [1.25]
    assert DR.rank_counts(depth, prior, margin=0.25).tolist() == [[[1, -1], [0, 0]]]
    # a gap of 1 keeps only (0,2); as disparities the order flips: (1,0), (2,0), (2,1)
    assert DR.rank_loss(depth, prior, margin=0.25, prior_gap=1.0)[1].tolist() == [1]
    out, pairs = DR.rank_loss(depth, prior, margin=0.25, prior_is_disparity=True)
    assert pairs.tolist() == [3] and out.tolist() == [0.0 + 1.25 + 2.25]  # 2 - 3 + .25 < 0;  4 - 3 + .25;  4 - 2 + .25
    # a mask takes pixel 0 out: only (1,2) is left
    weight = torch.tensor([[[0.0, 1.0], [1.0, 1.0]]], dtype=torch.float64)
    assert DR.rank_loss(depth, prior, weight, margin=0.25)[1].tolist() == [1]
    # autograd through the restatement gives the integer counts
    d = depth.clone().requires_grad_(True)
    DR.rank_loss(d, prior, margin=0.25)[0].sum().backward()
    assert torch.equal(d.grad, DR.rank_counts(depth, prior, margin=0.25).double())


def test_the_interface_exists_in_the_package_the_header_and_the_library():
    for name in SYMBOLS:
        assert name in L.FUNCTIONS, f"{name} is not declared in include/fsnerf_hip.h"
        assert hasattr(L.lib(), name), f"{name} is not exported by the library"
        assert L.FUNCTIONS[name][1][-1].name == "stream"
    names = [p.name for p in L.FUNCTIONS["fsn_ray_batch_aux"][1]]
    assert names[:-4] == [p.name for p in L.FUNCTIONS["fsn_ray_batch_k"][1]][:-1]
    assert names[-4:] == ["aux", "aux_channels", "aux_out", "stream"]
    names = [p.name for p in L.FUNCTIONS["fsn_ray_patch_batch_aux"][1]]
    assert names[:-4] == [p.name for p in L.FUNCTIONS["fsn_ray_patch_batch_k"][1]][:-1]
    assert names[-4:] == ["aux", "aux_channels", "aux_out", "stream"]
    assert callable(ops.ssi_depth) and callable(ops.depth_rank)
    for fn in (ops.ray_batch, ops.ray_patch_batch):
        sig = inspect.signature(fn).parameters
        assert sig["aux"].default is None and sig["want_aux"].default is False
    sig = inspect.signature(loss_mod.ScaleShiftDepthLoss.__init__).parameters
    assert [sig[k].default for k in ("space", "z_min", "threshold", "rel_eps")] == ["depth", 1e-3, None, 1e-10]
    sig = inspect.signature(loss_mod.DepthRankingLoss.__init__).parameters
    assert [sig[k].default for k in ("margin", "prior_gap", "prior_is_disparity", "threshold")] == [1e-4, 0.0, False, None]
    with pytest.raises(ValueError):
        loss_mod.ScaleShiftDepthLoss(space="log")
    from fs_nerf_amd.nerfdata import PatchLoader, RayDataset, RayLoader
    assert "aux" in inspect.signature(RayDataset.__init__).parameters and callable(RayDataset.set_aux)
    for cls in (RayLoader, PatchLoader):
        assert inspect.signature(cls.__init__).parameters["with_aux"].default is False
    for name in ("batch", "patch_batch"):
        assert inspect.signature(getattr(RayDataset, name)).parameters["want_aux"].default is False


def test_argument_errors_are_raised_before_any_device_work():
    lib = L.lib()
    one = C.c_void_p(64)  # never dereferenced: every call below is refused on its arguments
    unsupported = lib.fsn_ssi_depth_fwd(one, one, None, 1, 64, 65, 0, 1e-3, 1e-10, one, one, one, None)
    assert unsupported == L.FSN_E_UNSUPPORTED and b"64 x 65" in lib.fsn_last_error()
    assert lib.fsn_depth_rank_fwd(one, one, None, 1, 64, 65, 1e-4, 0.0, 0, one, one, None) == L.FSN_E_UNSUPPORTED
    assert lib.fsn_ssi_depth_bwd(one, one, None, one, 1, 4097, 1, 0, 1e-3, one, one, None) == L.FSN_E_UNSUPPORTED
    assert lib.fsn_depth_rank_bwd(one, one, None, 1, 1, 4097, 1e-4, 0.0, 0, one, one, None) == L.FSN_E_UNSUPPORTED
    # B == 0: nothing to do, whatever the pointers
    assert lib.fsn_ssi_depth_fwd(None, None, None, 0, 8, 8, 0, 1e-3, 1e-10, None, None, None, None) == L.FSN_OK
    assert lib.fsn_ssi_depth_bwd(None, None, None, None, 0, 8, 8, 0, 1e-3, None, None, None) == L.FSN_OK
    assert lib.fsn_depth_rank_fwd(None, None, None, 0, 8, 8, 1e-4, 0.0, 0, None, None, None) == L.FSN_OK
    assert lib.fsn_depth_rank_bwd(None, None, None, 0, 8, 8, 1e-4, 0.0, 0, None, None, None) == L.FSN_OK
    assert lib.fsn_ssi_depth_fwd(None, one, None, 1, 8, 8, 0, 1e-3, 1e-10, one, one, one, None) == L.FSN_E_INVALID
    assert lib.fsn_ssi_depth_fwd(one, one, None, 1, 0, 8, 0, 1e-3, 1e-10, one, one, one, None) == L.FSN_E_INVALID
    assert lib.fsn_ssi_depth_fwd(one, one, None, 1, 8, 8, 1, 0.0, 1e-10, one, one, one, None) == L.FSN_E_INVALID
    assert lib.fsn_depth_rank_fwd(one, one, None, 1, 8, 8, 1e-4, -1.0, 0, one, one, None) == L.FSN_E_INVALID
    # the aux entry points: aux_out without aux, channels outside 1..4, a table of the wrong size
    head = (one, 3, one, 5, 7, 3, 10.0)
    mid = (0, 1.0, 0, L.FSN_RAY_ORDER_IDENTITY, 0, 0, None, 0, 4)
    outs = (one, one, one, one)
    assert lib.fsn_ray_batch_aux(*head, None, 0, *mid, *outs, None, 1, one, None) == L.FSN_E_INVALID
    assert b"aux_out without aux" in lib.fsn_last_error()
    for channels in (0, 5):
        assert lib.fsn_ray_batch_aux(*head, None, 0, *mid, *outs, one, channels, one, None) == L.FSN_E_INVALID
        assert lib.fsn_ray_patch_batch_aux(*head, None, 0, *mid, 2, 1, *outs, one, channels, one, None) == L.FSN_E_INVALID
    assert lib.fsn_ray_batch_aux(*head, one, 2, *mid, *outs, one, 1, one, None) == L.FSN_E_INVALID  # k_rows not 1 or n
    assert lib.fsn_ray_batch_aux(*head, None, 1, *mid, *outs, one, 1, one, None) == L.FSN_E_INVALID  # rows without a table
    assert lib.fsn_ray_patch_batch_aux(*head, None, 0, *mid, 6, 1, *outs, one, 1, one, None) == L.FSN_E_INVALID  # no fit
    assert lib.fsn_ray_batch_aux(*head, None, 0, 0, 1.0, 0, L.FSN_RAY_ORDER_IDENTITY, 0, 0, None, 100, 10, *outs, one, 1, one,
                                 None) == L.FSN_E_INVALID  # start + count > N
    # count == 0 is a call with nothing to do
    assert lib.fsn_ray_batch_aux(*head, None, 0, 0, 1.0, 0, L.FSN_RAY_ORDER_IDENTITY, 0, 0, None, 0, 0, *outs, one, 1, one,
                                 None) == L.FSN_OK


def test_aux_gather_restatement():
    planes = DR.bit_planes(3, 5, 7, 4, seed=0)
    index = np.array([0, 104, 35, 3])
    rows = DR.aux_rows(planes, index)
    assert rows.dtype == np.uint32 and rows.shape == (4, 4)
    assert rows[2].tolist() == planes.view(np.uint32)[1, 0, 0].tolist()
    assert rows[1].tolist() == planes.view(np.uint32)[2, 4, 6].tolist()
    assert np.isnan(planes).any() and np.isinf(planes).any()
    assert DR.aux_rows(planes[..., 0], index).shape == (4, 1)
