"""GPU: the two monocular-depth-prior patch losses (csrc/depth_prior.hip, ops.ssi_depth / ops.depth_rank,
core.loss.ScaleShiftDepthLoss / DepthRankingLoss) against the restatements of tests/depth_prior_ref.py.
Accuracy is measured as in tests/test_intrinsics_gpu.py, with its bar unchanged:
    E = max |a - g64| relative to the largest |g64|,   E_kernel <= 4 E_f32 + 16 * 2^-24
with g64 the float64 restatement (autograd through the closed-form fit) and E_f32 the same restatement in float32 on the
CPU.  Every pair goes to profiles/depth_prior_accuracy.json (FSN_DEPTH_PRIOR_ACCURACY_OUT names another file)."""
import json
import os

import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import ops
from fs_nerf_amd.core.loss import DepthRankingLoss, ScaleShiftDepthLoss

import depth_prior_ref as DR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLACK = DR.SLACK
# 8 x 8 is exactly one wave, 5 x 13 one pixel over, 64 x 64 the cap; five patches are one over a four-wave workgroup
SHAPES = [(1, 1), (1, 2), (2, 2), (3, 5), (8, 8), (5, 13), (64, 64)]
_ACCURACY = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _write_accuracy():
    out = os.environ.get("FSN_DEPTH_PRIOR_ACCURACY_OUT", os.path.join(ROOT, "profiles", "depth_prior_accuracy.json"))
    try:
        with open(out, "w") as f:
            json.dump({"measure": "E = max |a - g64| relative to the largest |g64|; bar E_kernel <= 4 E_f32 + 16 * 2^-24; "
                                  "g64: the float64 restatement of tests/depth_prior_ref.py, E_f32: the same in float32",
                       "cases": _ACCURACY}, f, indent=1)
    except OSError:  # (a read-only checkout: the figures stay in the test's output)
        pass


def record(tag, what, e_kernel, e_f32):
    _ACCURACY.setdefault(tag, {})[what] = {"E_kernel": e_kernel, "E_f32": e_f32}
    print(f"{tag} {what}: E_kernel {e_kernel:.3e}  E_f32 {e_f32:.3e}")
    _write_accuracy()


def fit_inputs(B, P, Q, seed, weights, nans):
    """float32 patches: depth in [2, 6], a prior that is an affine map of a noisy copy (residuals of the signal's own
    size), optional weights (a fifth <= 0) and NaN priors scattered"""
    g = torch.Generator().manual_seed(seed)
    depth = 2.0 + 4.0 * torch.rand(B, P, Q, generator=g)
    prior = 0.7 * (depth + 2.0 * torch.rand(B, P, Q, generator=g)) - 1.3
    if nans and B * P * Q > 3:
        flat = prior.reshape(-1)
        flat[torch.arange(1, flat.numel(), 7)] = float("nan")
    weight = (torch.rand(B, P, Q, generator=g) - 0.2) if weights else None
    up = 0.5 + torch.rand(B, generator=g)
    return depth, prior, weight, up


def restated_fit(depth, prior, weight, up, inverse, dtype):
    d = depth.detach().clone().to(dtype).requires_grad_(True)  # (a copy: .to() of the same dtype is the tensor itself)
    L_b = DR.ssi_loss(d, prior.to(dtype), None if weight is None else weight.to(dtype), inverse=inverse)
    (L_b * up.to(dtype)).sum().backward()
    return L_b.detach(), d.grad


# ---------------------------------------------------------------- the scale-and-shift-invariant fit
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("inverse", [False, True], ids=["depth", "disparity"])
@pytest.mark.parametrize("weights", [False, True], ids=["plain", "weighted"])
def test_fit_accuracy(dev, shape, inverse, weights):
    P, Q = shape
    B = 5
    depth, prior, weight, up = fit_inputs(B, P, Q, seed=P * 100 + Q, weights=weights, nans=True)
    want_L, want_g = restated_fit(depth, prior, weight, up, inverse, torch.float64)
    f32_L, f32_g = restated_fit(depth, prior, weight, up, inverse, torch.float32)
    d = depth.to(dev).requires_grad_(True)
    out, fit = ops.ssi_depth(d, prior.to(dev), None if weight is None else weight.to(dev), inverse=inverse)
    assert out.shape == (B,) and fit.shape == (B, 4) and not fit.requires_grad
    (out * up.to(dev)).sum().backward()
    tag = f"fit {P}x{Q} {'disparity' if inverse else 'depth'} {'weighted' if weights else 'plain'}"
    e_L, f_L = DR.rel_error(out.cpu(), want_L), DR.rel_error(f32_L, want_L)
    e_g, f_g = DR.rel_error(d.grad.cpu(), want_g), DR.rel_error(f32_g, want_g)
    record(tag, "loss", e_L, f_L)
    record(tag, "gradient", e_g, f_g)
    assert e_L <= 4 * f_L + SLACK and e_g <= 4 * f_g + SLACK
    # the saved fit is the restatement's, and an invalid pixel has a gradient of exactly 0
    _, s, t, M, deg, _ = DR.ssi_fit(depth.double(), prior.double(), None if weight is None else weight.double(), inverse)
    assert torch.equal(fit[:, 3].cpu() != 0, deg)
    assert torch.allclose(fit[:, :3].cpu().double(), torch.stack([s, t, M], 1), rtol=1e-5, atol=1e-6)
    bad = ~DR.valid_mask(depth, prior, weight)
    assert not bool(d.grad.cpu()[bad].any()) and bool(torch.isfinite(d.grad).all())
    if P * Q == 1:
        assert bool(deg.all()) and not bool(out.any()) and not bool(d.grad.any())


@pytest.mark.parametrize("B", [0, 1, 4, 5])
def test_batch_sizes(dev, B):
    P, Q = 3, 5
    depth, prior, weight, up = fit_inputs(B, P, Q, seed=B, weights=True, nans=True)
    want_L, want_g = restated_fit(depth, prior, weight, up, False, torch.float64)
    f32_L, f32_g = restated_fit(depth, prior, weight, up, False, torch.float32)
    d = depth.to(dev).requires_grad_(True)
    out, fit = ops.ssi_depth(d, prior.to(dev), weight.to(dev))
    assert out.shape == (B,) and fit.shape == (B, 4)
    (out * up.to(dev)).sum().backward()
    assert d.grad.shape == (B, P, Q)
    assert DR.rel_error(out.cpu(), want_L) <= 4 * DR.rel_error(f32_L, want_L) + SLACK
    assert DR.rel_error(d.grad.cpu(), want_g) <= 4 * DR.rel_error(f32_g, want_g) + SLACK
    rd, rp = rank_inputs(B, P, Q, seed=B)
    d = rd.to(dev).requires_grad_(True)
    out, pairs = ops.depth_rank(d, rp.to(dev), margin=MARGIN, prior_gap=GAP)
    assert out.shape == (B,) and pairs.shape == (B,) and pairs.dtype == torch.int64
    out.sum().backward()
    assert torch.equal(pairs.cpu(), DR.rank_loss(rd.double(), rp.double(), margin=MARGIN, prior_gap=GAP)[1])
    assert torch.equal(d.grad.cpu().to(torch.int64), DR.rank_counts(rd.double(), rp.double(), margin=MARGIN, prior_gap=GAP))
    # the classes' reductions are defined for an empty batch too
    assert float(ScaleShiftDepthLoss()(depth.to(dev), prior.to(dev))) >= 0.0
    assert float(DepthRankingLoss(MARGIN, GAP)(rd.to(dev), rp.to(dev))) >= 0.0


def test_a_patch_over_the_cap_is_refused(dev):
    depth = torch.ones(1, 64, 65, device=dev)
    for call in (lambda: ops.ssi_depth(depth, depth), lambda: ops.depth_rank(depth, depth)):
        with pytest.raises(RuntimeError, match=r"code -2"):
            call()
    with pytest.raises(ValueError):
        ops.ssi_depth(depth, depth[:, :, :64])
    with pytest.raises(ValueError):
        ops.depth_rank(depth[0], depth[0])


def test_degenerate_patches(dev):
    depth, prior, _, _ = fit_inputs(5, 3, 5, seed=3, weights=False, nans=False)
    weight = torch.ones_like(depth)
    depth[0] = 3.0           # a constant patch fixes no scale
    weight[1] = 0.0
    weight[1, 1, 2] = 1.0    # one valid pixel
    weight[2] = 0.0          # all masked
    prior[3] = float("nan")  # nothing known
    for inverse in (False, True):
        d = depth.to(dev).requires_grad_(True)
        out, fit = ops.ssi_depth(d, prior.to(dev), weight.to(dev), inverse=inverse)
        out.sum().backward()
        assert fit[:, 3].tolist() == [1.0, 1.0, 1.0, 1.0, 0.0]
        assert out[:4].tolist() == [0.0] * 4 and float(out[4].detach()) > 0
        assert not bool(d.grad[:4].any()) and bool(d.grad[4].any())
        # the class divides by the number of fitted patches: one
        loss, fit2 = ScaleShiftDepthLoss("disparity" if inverse else "depth")(depth.to(dev), prior.to(dev), weight.to(dev),
                                                                             return_fit=True)
        assert float(loss) == float(out[4].detach()) and torch.equal(fit, fit2)
    # a patch of all-degenerate input gives 0 (the count is clamped at 1), and the opacity mask is a weight of 0
    assert float(ScaleShiftDepthLoss()(depth[:1].to(dev), prior[:1].to(dev))) == 0.0
    opacity = torch.ones_like(depth)
    opacity[4] = 0.05
    masked = ScaleShiftDepthLoss(threshold=0.1)
    assert float(masked(depth.to(dev), prior.to(dev), weight.to(dev), opacity=opacity.to(dev))) == 0.0
    with pytest.raises(ValueError):
        masked(depth.to(dev), prior.to(dev))


def test_anticorrelated_patch_reports_a_negative_scale(dev):
    depth, _, _, _ = fit_inputs(2, 4, 4, seed=8, weights=False, nans=False)
    prior = -2.0 * depth + 5.0
    out, fit = ops.ssi_depth(depth.to(dev), prior.to(dev))
    assert bool((fit[:, 0] < -1.9).all()) and bool((out < 1e-10).all())


# ---------------------------------------------------------------- the ranking term
MARGIN, GAP = 1.0 / 64, 0.5


def rank_inputs(B, P, Q, seed):
    """No kinks: depths are multiples of 1/32 in [2, 6] and the margin is 1/64, so d_i - d_j + margin is an odd multiple
    of 1/64 and never 0; priors are integers in [0, 15] and the gap is 0.5 - float32 and float64 agree on every pair."""
    g = torch.Generator().manual_seed(1000 + seed)
    depth = 2.0 + torch.randint(0, 129, (B, P, Q), generator=g).float() / 32
    prior = torch.randint(0, 16, (B, P, Q), generator=g).float()
    return depth, prior


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("disparity", [False, True], ids=["depth", "disparity"])
def test_ranking_counts_are_exact(dev, shape, disparity):
    P, Q = shape
    B = 2 if P * Q == 4096 else 5  # (the restatement builds an [N, N] table per patch)
    depth, prior = rank_inputs(B, P, Q, seed=P * 100 + Q)
    weight = None
    if P * Q > 2:  # a mask and a few NaN priors
        g = torch.Generator().manual_seed(5)
        weight = (torch.rand(B, P, Q, generator=g) > 0.2).float()
        prior.reshape(-1)[torch.arange(2, prior.numel(), 11)] = float("nan")
    kw = dict(margin=MARGIN, prior_gap=GAP, prior_is_disparity=disparity)
    w64 = None if weight is None else weight.double()
    want_out, want_pairs = DR.rank_loss(depth.double(), prior.double(), w64, **kw)
    f32_out, f32_pairs = DR.rank_loss(depth, prior, weight, **kw)
    want_counts = DR.rank_counts(depth.double(), prior.double(), w64, **kw)
    assert torch.equal(f32_pairs, want_pairs) and torch.equal(DR.rank_counts(depth, prior, weight, **kw), want_counts)
    up = torch.tensor([0.5, 2.0, 1.0, 4.0, 0.25])[:B]  # powers of two: the division below is exact
    d = depth.to(dev).requires_grad_(True)
    out, pairs = ops.depth_rank(d, prior.to(dev), None if weight is None else weight.to(dev), **kw)
    (out * up.to(dev)).sum().backward()
    assert pairs.dtype == torch.int64 and torch.equal(pairs.cpu(), want_pairs)
    assert torch.equal((d.grad.cpu() / up[:, None, None]).double(), want_counts.double())
    tag = f"rank {P}x{Q} {'disparity' if disparity else 'depth'}"
    e, f = DR.rel_error(out.cpu(), want_out), DR.rel_error(f32_out, want_out)
    record(tag, "loss", e, f)
    assert e <= 4 * f + SLACK
    if P * Q > 4:
        assert int(want_pairs.sum()) > 0 and bool(want_counts.any())
    # the class: sum of the hinges over the number of pairs
    got = DepthRankingLoss(MARGIN, GAP, disparity)(depth.to(dev), prior.to(dev), None if weight is None else weight.to(dev))
    want = float(want_out.sum()) / max(int(want_pairs.sum()), 1)
    assert abs(float(got) - want) <= (4 * f + SLACK) * max(abs(want), 1e-30) + 1e-30


def test_ranking_opacity_mask(dev):
    depth, prior = rank_inputs(3, 4, 4, seed=1)
    opacity = torch.rand(3, 4, 4, generator=torch.Generator().manual_seed(2))
    loss = DepthRankingLoss(MARGIN, GAP, threshold=0.3)
    d = depth.to(dev).requires_grad_(True)
    loss(d, prior.to(dev), opacity=opacity.to(dev)).backward()
    keep = (opacity > 0.3).double()
    want = DR.rank_mean(depth.double(), prior.double(), keep, margin=MARGIN, prior_gap=GAP)
    got = float(loss(depth.to(dev), prior.to(dev), opacity=opacity.to(dev)))
    assert abs(got - float(want)) <= SLACK * float(want)
    assert not bool(d.grad.cpu()[keep == 0].any()) and bool(d.grad.any())


# ---------------------------------------------------------------- determinism
def test_two_runs_give_identical_bits(dev):
    depth, prior, weight, up = fit_inputs(5, 5, 13, seed=21, weights=True, nans=True)
    rd, rp = rank_inputs(5, 5, 13, seed=21)
    runs = []
    for _ in range(2):
        got = []
        for inverse in (False, True):
            d = depth.to(dev).requires_grad_(True)
            out, fit = ops.ssi_depth(d, prior.to(dev), weight.to(dev), inverse=inverse)
            (out * up.to(dev)).sum().backward()
            got += [out.detach(), fit, d.grad]
        d = rd.to(dev).requires_grad_(True)
        out, pairs = ops.depth_rank(d, rp.to(dev), margin=MARGIN, prior_gap=GAP)
        (out * up.to(dev)).sum().backward()
        got += [out.detach(), pairs, d.grad]
        runs.append([t.cpu() for t in got])
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                  b.view(torch.int32) if b.dtype == torch.float32 else b)


# ---------------------------------------------------------------- a short recovery
def adam_recovery(loss_of, start, steps=300, lr=0.02):
    """Adam on a depth patch from `start`, driven by loss_of(depth); -> the final loss."""
    depth = start.clone().requires_grad_(True)
    opt = torch.optim.Adam([depth], lr=lr)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss_of(depth).backward()
        opt.step()
    with torch.no_grad():
        return float(loss_of(depth))


def test_adam_recovery_against_a_scaled_and_shifted_prior(dev):
    """A 16 x 16 depth patch initialised 10 % off - every pixel by its own factor in [0.9, 1.1]: one common factor is
    an affine map, which the loss does not see - is driven against prior = 3 truth + 1.  The float64 restatement under
    the same recipe sets the target: the device run ends within 10 x of it or below 1e-6, whichever is larger."""
    g = torch.Generator().manual_seed(4)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 16), torch.linspace(0, 1, 16), indexing="ij")
    truth = (3.0 + yy + 0.5 * torch.sin(6.0 * xx)).reshape(1, 16, 16)
    start = truth * (1.0 + 0.1 * (2.0 * torch.rand(1, 16, 16, generator=g) - 1.0))
    prior = 3.0 * truth + 1.0
    want = adam_recovery(lambda d: DR.ssi_mean(d, prior.double()), start.double())
    loss = ScaleShiftDepthLoss()
    prior_dev = prior.to(dev)
    with torch.no_grad():
        first = float(loss(start.to(dev), prior_dev))
    got = adam_recovery(lambda d: loss(d, prior_dev), start.to(dev))
    _ACCURACY["adam recovery 16x16 (prior = 3 truth + 1, 300 steps, lr 0.02)"] = {"start": first, "final_kernel": got,
                                                                                "final_f64_restatement": want}
    _write_accuracy()
    print(f"recovery: start {first:.3e}  device {got:.3e}  float64 restatement {want:.3e}")
    assert first > 0.1  # (the start is far from a fit)
    assert got <= max(10.0 * want, 1e-6)
