"""-m "not gpu": the CPU restatement of the LPIPS loss's gradient (tests/lpips_grad_ref.py) against torch autograd and
central differences, its all-zero-pixel definition, the margins of the committed GPU cases, LPIPSLoss's argument checks
and the new size queries."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_grad_ref as GR  # noqa: E402
import lpips_ref as LR  # noqa: E402

import fs_nerf_amd  # noqa: E402,F401
from fs_nerf_amd import _lib as L  # noqa: E402
from fs_nerf_amd.core import metrics  # noqa: E402
from fs_nerf_amd.core.loss import LPIPSLoss  # noqa: E402


@pytest.fixture(scope="module")
def sd():
    return LR.random_state_dict(seed=GR.SD_SEED)


@pytest.mark.parametrize("H,W,normalize", [(16, 16, False), (19, 23, True)])
def test_restatement_is_torch_autograd(sd, H, W, normalize):
    x, y = GR.make_pair(3, 2, H, W)
    up = torch.tensor([0.7, -1.3], dtype=torch.float64)
    v, per, dx, dy = GR.value_and_grad(sd, x, y, up, normalize)
    v0, per0 = LR.lpips(sd, x, y, normalize)
    assert torch.allclose(v, v0, rtol=1e-13, atol=0) and torch.allclose(per, per0, rtol=1e-13, atol=0)
    va, ax, ay = GR.autograd_value_and_grad(sd, x, y, up, normalize)
    assert torch.allclose(v, va, rtol=1e-13, atol=0)
    for mine, auto in ((dx, ax), (dy, ay)):
        assert float((mine - auto).abs().max()) <= 1e-10 * float(auto.abs().max())


def test_restatement_agrees_with_central_differences(sd):
    x, y = GR.make_pair(12, 1, 16, 16)
    x, y = x.double(), y.double()
    _, _, dx, dy = GR.value_and_grad(sd, x, y, None, True)
    g = torch.Generator().manual_seed(0)
    h = 1e-6
    for which, grad in ((0, dx), (1, dy)):
        for _ in range(3):  # directional derivatives along random directions
            d = torch.randn(x.shape, generator=g, dtype=torch.float64)
            lo = [x, y]
            hi = [x, y]
            lo[which] = lo[which] - h * d
            hi[which] = hi[which] + h * d
            fd = (LR.lpips(sd, hi[0], hi[1], True)[0] - LR.lpips(sd, lo[0], lo[1], True)[0]).sum() / (2 * h)
            an = (grad * d).sum()
            assert abs(float(fd - an)) <= 1e-7 * float(grad.abs().sum()), (float(fd), float(an))


def test_all_zero_tap_pixels_give_a_finite_gradient_with_no_share_of_that_tap(sd):
    dead = dict(sd)
    dead["net.slice1.2.bias"] = torch.full((64,), -10.0)  # relu1_2 is zero everywhere
    x, y = GR.make_pair(1, 1, 16, 16)
    _, a = GR.forward(dead, x)
    assert float(a[1].abs().max()) == 0.0
    v, per, dx, dy = GR.value_and_grad(dead, x, y)
    assert float(per[0]) == 0.0
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dy).all())
    # (nothing passes relu1_2's mask, so here the whole gradient is zero, not only tap 0's share)
    assert float(dx.abs().max()) == 0.0 and float(dy.abs().max()) == 0.0
    _, _, sx, sy = GR.value_and_grad(dead, x, y, taps=(0,))
    assert float(sx.abs().max()) == 0.0 and float(sy.abs().max()) == 0.0
    # autograd has NaN behind relu1_2 there (0 * inf from sqrt); its ReLU backward selects, so the images see 0 too
    _, ax, ay = GR.autograd_value_and_grad(dead, x, y)
    assert float(ax.abs().max()) == 0.0 and float(ay.abs().max()) == 0.0
    # a network with live pixels next to dead ones: only the dead tap's share vanishes
    _, _, t4x, _ = GR.value_and_grad(sd, x, y, taps=(4,))
    assert float(t4x.abs().max()) > 0.0


def test_first_maximum_takes_the_pooled_gradient():
    v = torch.tensor([[1.0, 3.0, 3.0, 2.0], [2.0, 2.0, 2.0, 2.0]]).t().reshape(4, 2)
    win = GR._first_max(v)
    assert win[:, 0].tolist() == [False, True, False, False] and win[:, 1].tolist() == [True, False, False, False]


@pytest.mark.parametrize("name", sorted(GR.CASES))
def test_committed_cases_cannot_flip_a_unit_or_a_pool_winner(sd, name):
    x, y, normalize = GR.case_inputs(name)
    rows = GR.margins(sd, x, y, normalize)
    factor = GR.CASES[name][4]
    assert len(rows) == 13 and factor in (GR.SAFETY, GR.SAFETY_LARGE)
    if x.shape[2] * x.shape[3] <= 256:
        assert factor == GR.SAFETY
    for l, (small, gap, diff) in enumerate(rows):
        assert min(small, gap) >= factor * diff, f"{name} layer {l}: |pre| {small:.3e}, gap {gap:.3e}, f32 {diff:.3e}"
    _, acts = GR.forward(sd, torch.cat([x, y]), normalize)
    for l, t in enumerate(GR.TAP_OF):  # no all-zero tap pixel
        if t >= 0:
            assert float((acts[l] ** 2).sum(dim=1).min()) > 0.0


# ---------------------------------------------------------------- LPIPSLoss's checks (no GPU needed to refuse)
def _net(sd):
    m = metrics.LPIPS()
    m.load_state_dict(sd)
    return m


def test_lpips_loss_refuses_what_it_cannot_run(sd):
    x = torch.rand(2, 16, 16, 3)
    with pytest.raises(RuntimeError, match="no weights loaded"):
        LPIPSLoss(metrics.LPIPS())(x, x)
    loss = LPIPSLoss(_net(sd))
    with pytest.raises(RuntimeError, match="not a GPU tensor"):
        loss(x, x)
    with pytest.raises(TypeError, match="must be float32"):
        loss(x.double(), x.double())
    with pytest.raises(TypeError, match="must be float32"):
        loss(x, x.half())
    with pytest.raises(ValueError, match="same shape"):
        loss(x, x[:1])
    with pytest.raises(ValueError, match="at least 16 x 16"):
        loss(x[:, :15], x[:, :15])
    with pytest.raises(ValueError, match="3 channels"):
        loss(torch.rand(2, 16, 16, 4), torch.rand(2, 16, 16, 4))
    with pytest.raises(ValueError):
        loss(x[0], x[0])
    with pytest.raises(ValueError, match="3 channels"):
        LPIPSLoss(_net(sd), channel_axis=1)(x, x)  # (N, H, W, 3) read as (N, 3, H, W)
    with pytest.raises(ValueError):
        LPIPSLoss(_net(sd), reduction="sum")
    with pytest.raises(ValueError):
        LPIPSLoss(_net(sd), channel_axis=2)
    with pytest.raises(TypeError):
        LPIPSLoss(object())
    assert loss.max_workspace_bytes == metrics.TRAIN_WORKSPACE_BYTES and loss.pairs_per_pass is None


def test_size_queries_validate_without_a_gpu():
    lib = L.lib()
    one = lib.fsn_lpips_train_workspace_floats(1, 32, 32, 1, 0)
    both = lib.fsn_lpips_train_workspace_floats(1, 32, 32, 1, 1)
    assert 0 < one < both
    # about 270 H W floats of activations and 128 H W of gradients per back-propagated image
    assert 2 * (270 + 128) * 1024 <= both <= 2 * (270 + 128 + 16) * 1024
    assert lib.fsn_lpips_train_workspace_floats(1, 32, 32, 0, 1) == one
    assert lib.fsn_lpips_train_workspace_floats(4, 32, 32, 1, 1) == 4 * both  # linear in the pairs
    assert lib.fsn_lpips_train_workspace_floats(1, 37, 53, 1, 1) > 0
    for bad in ((1, 15, 32, 1, 1), (1, 32, 15, 1, 1), (1, 16385, 32, 1, 1), (1, 32, 32, 0, 0), (0, 32, 32, 1, 1),
                (40000, 32, 32, 1, 1)):
        assert lib.fsn_lpips_train_workspace_floats(*bad) < 0, bad
    grad_bytes = lib.fsn_lpips_grad_pack_bytes()
    convs = sum(cin * cout * 9 for _, _, cin, cout in LR.CONVS)
    assert grad_bytes == 4 * convs
    assert metrics.lpips_pairs_per_pass(32, 32, True, True, 4 * both * 5 + 3) == 5
    assert metrics.lpips_pairs_per_pass(32, 32, True, True, 1) == 1
