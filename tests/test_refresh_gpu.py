"""The single-pass occupancy refresh on the GPU: `NeRF.occ_eval_fn` in the slot of
`OccGridEstimator.update_every_n_steps` (one fused launch for all levels), `NeRF.autocast_precision` (the reference's own
closure under its autocast line), their range guard and frequency masks, and their accuracy against the reference's
refresh arithmetic under autocast (tests/golden/g7_refresh_autocast.npz).

Equalities are exact: the fused launch draws the same points with the same device function as fsn_occgrid_select, a
sample's density depends on its own MFMA rows only, `sigma * step` is the same float32 product torch forms, and a
maximum does not depend on the order of its arguments.  The accuracy bounds come from the golden: twice the reference's
own deviation from float64 under autocast, the project's standing margin for "the reference's grade"."""
import copy
import warnings

import numpy as np
import pytest
import torch

from oracle import fsnerf_oracle as O
from test_parity_fp64 import hidden_max, scaled_sd
from test_refresh_cpu import BAND_CAP, golden_refresh

pytestmark = pytest.mark.gpu

AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
STEP = 5e-3
MODES = ["fp16", "bf16"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def make_model(sd, L, D, dev, precision="fp16x3"):
    from fs_nerf_amd.core.models import NeRF
    m = NeRF(3, 3, L, D, (4,), precision=precision, pos_fn={"n_freqs": 10, "log_space": True},
             dir_fn={"n_freqs": 4, "log_space": True})
    m.load_state_dict(sd)
    return m.to(dev).train()  # (the refresh runs inside the training loop)


def grid_sd(L, D, seed):
    """A network whose occ = sigma * STEP straddles zero and the refresh threshold inside the box: the sigma head
    scaled by 256 and its bias shifted so that the median density over the box (float64 oracle) is 1."""
    sd = O.init_nerf_state_dict(L, D, [4], 10, 4, seed=seed)
    sd["sigma.weight"] = sd["sigma.weight"] * 256.0
    x = torch.rand(4096, 3, generator=torch.Generator().manual_seed(seed)).double() * 3 - 1.5
    sig = O.nerf_forward({k: v.double() for k, v in sd.items()}, x, None, n_layers=L, skip=[4], n_freqs=10, n_freqs_dir=4)
    sd["sigma.bias"] = sd["sigma.bias"] + (1.0 - float(sig.median()))
    return sd


def make_est(dev, res, levels, seed=5):
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    est = OccGridEstimator(AABB, res, levels).to(dev).train()
    est.generator = torch.Generator().manual_seed(seed)
    return est


def random_binaries(levels, res, fill, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(levels, res, res, res, generator=g) < fill


def assert_same_grid(a, b, what):
    assert torch.equal(a.occs, b.occs), (what, int((a.occs != b.occs).sum()), float((a.occs - b.occs).abs().max()))
    assert torch.equal(a.bits, b.bits), (what, int((a.bits != b.bits).sum()))
    assert a._updates == b._updates and a.update_seed(0) == b.update_seed(0)
    assert int(b._pending.count_nonzero()) == 0, what


# ---------------------------------------------------------------- 1. same draws, same arithmetic, fewer launches
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("levels,res,L,D,fill", [(1, 128, 8, 256, 0.1), (4, 16, 8, 256, 0.1), (4, 16, 8, 256, 0.5),
                                                 (1, 16, 8, 256, 0.5), (4, 4, 8, 256, 0.1), (4, 8, 4, 128, 0.5)])
def test_fused_refresh_equals_the_level_loop_bit_for_bit(dev, mode, levels, res, L, D, fill):
    """A: today's path, a plain closure over a copy of the model whose `precision` is the single-pass mode.  B: the
    `OccEvalFn` (fused launch).  C: the reference's closure under torch.autocast("cuda") with `autocast_precision`.
    Steps 0, 16 (warm-up: every cell) and 256, 272 (uniform + occupied draws), the latter on a grid loaded with `fill`
    occupied cells: 0.1 takes every occupied cell once and leaves sentinel draws, 0.5 draws them with replacement.
    (4, 4): 64 / 32 draws per level, so one tile holds all four levels; 4x128: one sample group per wave.)"""
    model = make_model(grid_sd(L, D, 11), L, D, dev)
    model_a = copy.deepcopy(model)
    model_a.precision = mode
    model_c = copy.deepcopy(model)
    model_c.autocast_precision = mode
    fn_a = lambda x: model_a(x) * STEP
    fn_b = model.occ_eval_fn(STEP, mode)
    fn_c = lambda x: model_c(x) * STEP
    ests = [make_est(dev, res, levels) for _ in range(3)]
    for step in (0, 16, 256, 272):
        if step == 256:
            seen = ests[0].binaries
            assert 0 < int(seen.sum()) < seen.numel(), "the warm-up left a grid with both kinds of cell"
            for e in ests:
                e.set_binaries(random_binaries(levels, res, fill, 3).to(dev))
        ests[0].update_every_n_steps(step, fn_a, occ_thre=1e-2)
        ests[1].update_every_n_steps(step, fn_b, occ_thre=1e-2)
        with torch.autocast("cuda"):
            ests[2].update_every_n_steps(step, fn_c, occ_thre=1e-2)
        assert_same_grid(ests[0], ests[1], ("fused", step))
        assert_same_grid(ests[0], ests[2], ("autocast closure", step))
        ests[1].update_every_n_steps(step + 1, fn_b)  # off the schedule: nothing happens
        assert_same_grid(ests[0], ests[1], ("off-schedule", step))
    assert fn_b.precision == mode and model_a.precision == mode and model_c.autocast_precision == mode
    assert model.precision == "fp16x3", "the model's own mode is not touched"
    # ... and the object is an ordinary occ_eval_fn too: model(x) * step in that mode
    x = (torch.rand(1000, 3, generator=torch.Generator().manual_seed(1)) * 3 - 1.5).to(dev)
    with torch.no_grad():
        assert torch.equal(fn_b(x), fn_a(x))


# ---------------------------------------------------------------- 2. nothing moves by default
def test_autocast_is_ignored_by_default_and_outside_no_grad(dev):
    model = make_model(grid_sd(8, 256, 12), 8, 256, dev).eval()
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(3000, 3, generator=g) * 3 - 1.5).to(dev)
    d = torch.nn.functional.normalize(torch.randn(3000, 3, generator=g), dim=-1).to(dev)
    assert model.autocast_precision is None
    with torch.no_grad():
        y1, y4 = model(x), model(x, d)
        with torch.autocast("cuda"):
            z1, z4 = model(x), model(x, d)
        assert torch.equal(y1, z1) and torch.equal(y4, z4) and z1.dtype == torch.float32
        model.autocast_precision = "fp16"
        assert torch.equal(model(x), y1), "no autocast region: the model's own mode"
        with torch.autocast("cuda", enabled=False):
            assert torch.equal(model(x), y1)
        with torch.autocast("cuda"):
            h1, h4 = model(x), model(x, d)
        single = copy.deepcopy(model)
        single.autocast_precision, single.precision = None, "fp16"
        assert torch.equal(h1, single(x)) and torch.equal(h4, single(x, d)) and h1.dtype == torch.float32
        assert not torch.equal(h1, y1)
    # a training forward never looks at the attribute
    model.train()
    with torch.autocast("cuda"):
        t = model(x[:256], d[:256])
    model.autocast_precision = None
    assert torch.equal(t.detach(), model(x[:256], d[:256]).detach())


# ---------------------------------------------------------------- 3. / 4. against the reference's arithmetic under autocast
@pytest.mark.parametrize("mode", MODES)
def test_refresh_arithmetic_has_the_references_grade(dev, mode):
    """The OccEvalFn on the golden's points against the reference's float64 column.  3: largest deviation at most
    2 x dev_ref, the reference's own largest deviation under autocast.  4: the threshold decisions occ > thre differ
    from float64's only within 2 x dev_ref of the threshold, and that band holds at most 1 % (fp16) / 10 % (bf16) of
    the points.  Measured on the MI355X: fp16 2.73e-4 (dev_ref 4.68e-4), bf16 2.16e-3 (dev_ref 3.07e-3); DESIGN.md §7."""
    g, sd = golden_refresh()
    model = make_model(sd, 8, 256, dev)
    fn = model.occ_eval_fn(float(g["step"]), mode)
    occ = fn(torch.from_numpy(g["x"]).to(dev)).reshape(-1).cpu().numpy()
    occ64, thre, dev_ref = g["occ_f64"], float(g["thre"]), float(g["dev_ref_" + mode])
    assert occ.dtype == np.float32 and np.isfinite(occ).all() and fn.precision == mode
    dev_max = float(np.abs(occ.astype(np.float64) - occ64).max())
    flips = (occ > thre) != (occ64 > thre)
    band = np.abs(occ64 - thre) <= 2.0 * dev_ref
    print(f"{mode}: max |occ - occ64| {dev_max:.3e} (dev_ref {dev_ref:.3e}), {int(flips.sum())} flipped decisions, "
          f"{int((flips & ~band).sum())} outside the band, {100 * band.mean():.2f} % of the points inside it")
    assert dev_max <= 2.0 * dev_ref
    assert float(band.mean()) <= BAND_CAP[mode]
    assert not bool((flips & ~band).any())


# ---------------------------------------------------------------- 5. range guard
def test_flagged_fp16_refresh_leaves_no_trace_and_continues_in_bf16(dev):
    from fs_nerf_amd import ops
    L, D, res, levels = 8, 256, 16, 2
    sd = scaled_sd(L, D, 43, 4e5)
    pts = torch.rand(4096, 3, generator=torch.Generator().manual_seed(4)) * 3 - 1.5
    assert hidden_max(sd, pts, L) > 2 * 65504.0
    model = make_model(sd, L, D, dev)
    fn = model.occ_eval_fn(STEP, "fp16")
    est, fresh = make_est(dev, res, levels), make_est(dev, res, levels)
    assert ops.range_ok(dev)  # clean slate
    events = model.range_events
    with pytest.warns(RuntimeWarning, match="fp16 range") as rec:
        est.update_every_n_steps(0, fn)
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 1
    assert fn.precision == "bf16" and model.range_events == events + 1 and model.precision == "fp16x3"
    fresh.update_every_n_steps(0, model.occ_eval_fn(STEP, "bf16"))
    assert_same_grid(fresh, est, "bf16 re-run")
    assert bool(torch.isfinite(est.occs).all()) and ops.range_ok(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # ... and stays there: no second warning, no second look
        est.update_every_n_steps(16, fn)
        fresh.update_every_n_steps(16, model.occ_eval_fn(STEP, "bf16"))
    assert_same_grid(fresh, est, "second refresh")
    # the attribute has the same guard
    model.autocast_precision = "fp16"
    x = pts.to(dev)
    with torch.no_grad(), torch.autocast("cuda"):
        with pytest.warns(RuntimeWarning, match="fp16 range"):
            y = model(x)
        assert model.autocast_precision == "bf16" and bool(torch.isfinite(y).all())
        assert torch.equal(y * STEP, model.occ_eval_fn(STEP, "bf16")(x))


# ---------------------------------------------------------------- 6. frequency masks
@pytest.mark.parametrize("mode", MODES)
def test_frequency_mask_reaches_the_fused_refresh(dev, mode):
    model = make_model(grid_sd(8, 256, 13), 8, 256, dev)
    plain = make_est(dev, 16, 2)
    plain.update_every_n_steps(0, model.occ_eval_fn(STEP, mode))
    model.set_freq_mask(O.freq_mask(3, 10, 0.4).to(dev))
    model_a = copy.deepcopy(model)
    model_a.precision = mode
    a, b = make_est(dev, 16, 2), make_est(dev, 16, 2)
    for step in (0, 256):
        a.update_every_n_steps(step, lambda x: model_a(x) * STEP)
        b.update_every_n_steps(step, model.occ_eval_fn(STEP, mode))
        assert_same_grid(a, b, ("masked", step))
        if step == 0:
            assert not torch.equal(b.occs, plain.occs), "the mask changes the densities"
