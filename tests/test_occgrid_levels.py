"""The occupancy grid as the reference trains and renders with it (run-nerf.py:91-98): resolution 128, one level for
synthetic scenes and four for LLFF (whose box is the NDC rays' own extent / 2^3, llff.py:75-85), step 5e-3.  What only
these configurations reach: the 64-words-per-thread popcount prefix and the 65,536-word rank search of the selection,
the level offsets into the bit field and `occs`, the level boxes rebuilt in float on the device, the finest-level
lookup, rays that start on the outer box's faces, and render_rays' route switch at max_steps > 2048.
The selection's occupied half follows nerfacc's rule (each occupied cell once when there are at most res^3/4 of them);
the CPU tests pin that rule in the oracle, the GPU tests hold the kernels to the oracle bit for bit."""
import math

import numpy as np
import pytest
import torch

from oracle import fsnerf_oracle as O
from test_occgrid import _orbit_rays, _relu_margin_rel

AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
STEP = 5e-3


def _box(lo, hi):
    return ([float(v) for v in lo], [float(v) for v in hi])


# ---------------------------------------------------------------- the oracle's selection rule (CPU)
def _sel(b, n_uniform, n_occupied, seed=0x1234ABCD9876, res=8):
    return O.occgrid_select(b, _box([-1] * 3, [1] * 3), res, False, n_uniform, n_occupied, seed)


@pytest.mark.parametrize("m", [0, 1, 37, 128])
def test_oracle_selection_takes_each_occupied_cell_once_when_m_le_n(m):
    """m <= n (n = 128 = 8^3/4): draw n_uniform + q is the q-th occupied cell in ascending order for q < m, the
    sentinel -1 for q >= m; m == n gives every occupied cell exactly once (nerfacc draws with replacement only for n < m);
    the uniform half and the jitter are those of the hashed draws."""
    res, n = 8, 128
    g = torch.Generator().manual_seed(m)
    b = torch.zeros(res ** 3, dtype=torch.bool)
    occ = torch.randperm(res ** 3, generator=g)[:m]
    b[occ] = True
    b = b.reshape(res, res, res)
    cells, x = _sel(b, n, n)
    assert cells.shape == (2 * n,) and x.shape == (2 * n, 3) and x.dtype == torch.float32
    assert torch.equal(cells[n:n + m], torch.sort(occ).values)
    assert bool((cells[n + m:] == -1).all())
    # uniform half: r(i, 0) % res^3, as with the old rule
    r = O.occ_rand(np.arange(n, dtype=np.uint64), 0, 0x1234ABCD9876)
    assert torch.equal(cells[:n], torch.from_numpy((r % np.uint64(res ** 3)).astype(np.int64)))
    # every point lies inside its cell (a sentinel draw: inside the cell of its uniform hash) within the level's box
    r_all = O.occ_rand(np.arange(2 * n, dtype=np.uint64), 0, 0x1234ABCD9876) % np.uint64(res ** 3)
    pos = torch.where(cells >= 0, cells, torch.from_numpy(r_all.astype(np.int64)))
    q = torch.floor((x.double() + 1.0) / 2.0 * res).long().clamp(0, res - 1)
    assert torch.equal((q[:, 0] * res + q[:, 1]) * res + q[:, 2], pos)
    assert float(x.abs().max()) <= 1.0


def test_oracle_selection_draws_with_replacement_when_m_gt_n():
    res, n = 8, 128
    b = torch.zeros(res ** 3, dtype=torch.bool)
    occ = torch.randperm(res ** 3, generator=torch.Generator().manual_seed(3))[:n + 1]
    b[occ] = True
    cells, _ = _sel(b.reshape(res, res, res), n, n)
    seed = 0x1234ABCD9876
    r = O.occ_rand(np.arange(n, 2 * n, dtype=np.uint64), 0, seed)
    want = torch.sort(occ).values[torch.from_numpy((r % np.uint64(n + 1)).astype(np.int64))]
    assert torch.equal(cells[n:], want)
    assert bool(b[cells[n:]].all()) and int(torch.unique(cells[n:]).numel()) < n, "with replacement: repeats"


def test_oracle_selection_empty_level_and_other_levels():
    """An empty level: every occupied draw is the sentinel, the points are still inside the level's box; a level other
    than 0: same indices inside the level, points in that level's box; warm-up: every cell once."""
    res, n = 8, 128
    cells, x = _sel(torch.zeros(res, res, res, dtype=torch.bool), n, n)
    assert bool((cells[n:] == -1).all()) and bool((cells[:n] >= 0).all()) and float(x.abs().max()) <= 1.0
    b = torch.zeros(res ** 3, dtype=torch.bool)
    b[[5, 100, 511]] = True
    b = b.reshape(res, res, res)
    box2 = _box([-4.0] * 3, [4.0] * 3)  # level 2 of the [-1, 1] box
    c2, x2 = O.occgrid_select(b, box2, res, False, n, n, 77)
    c0, x0 = O.occgrid_select(b, _box([-1] * 3, [1] * 3), res, False, n, n, 77)
    assert torch.equal(c2, c0) and c2[n:n + 3].tolist() == [5, 100, 511] and bool((c2[n + 3:] == -1).all())
    assert float(x2.abs().max()) <= 4.0 and float(x2.abs().max()) > 1.0
    assert torch.allclose(x2, x0 * 4.0, rtol=1e-6, atol=1e-6)
    cw, _ = O.occgrid_select(b, box2, res, True, 0, 0, 77)
    assert torch.equal(cw, torch.arange(res ** 3))
    # n_occupied = 0: every draw uniform
    cu, _ = O.occgrid_select(b, box2, res, False, 2 * n, 0, 77)
    assert bool((cu >= 0).all()) and torch.equal(cu[:n], c2[:n])


def test_oracle_update_rule():
    """occs = max(occs*decay, max over a cell's draws) once per touched cell in float32; sentinels and NaN skipped;
    threshold = min(mean, occ_thre); binaries = occs > threshold."""
    occs = torch.tensor([0.5, 0.2, 0.0, 1.0, 0.3, 0.0, 0.0, 0.04], dtype=torch.float32)
    cells = torch.tensor([1, 1, -1, 3, 2, 7, 6, -1, 4])
    vals = torch.tensor([0.1, 0.15, 9.0, 0.5, 0.02, 0.01, float("nan"), 5.0, 0.25])
    new, touched, thr, bins = O.occgrid_update(occs, cells, vals, 0.95, 0.2)
    f = np.float32
    want = occs.clone()
    want[1] = float(max(f(0.2) * f(0.95), f(0.15)))
    want[3] = float(f(1.0) * f(0.95))
    want[2] = 0.02
    want[7] = float(max(f(0.04) * f(0.95), f(0.01)))
    want[4] = float(max(f(0.3) * f(0.95), f(0.25)))
    assert torch.equal(new, want)
    assert touched.tolist() == [False, True, True, True, True, False, False, True]
    assert thr == pytest.approx(min(float(want.double().mean()), 0.2), rel=1e-15)
    assert torch.equal(bins, want > thr)
    _, _, thr2, _ = O.occgrid_update(occs, cells, vals, 0.95, 1e-2)
    assert thr2 == 1e-2


# ---------------------------------------------------------------- calibration probe and persisted update count (CPU)
def test_probe_spans_every_level_box_and_survives_zero_rays():
    from fs_nerf_amd.render import rendering as Rm
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    est = OccGridEstimator(AABB, 16, 4)
    d = torch.nn.functional.normalize(torch.randn(300, 3, generator=torch.Generator().manual_seed(0)), dim=-1)
    x, dd = Rm._probe_in_box(torch.zeros(300, 3), d, None, est)
    assert x.shape == (16384, 3) and dd.shape == (16384, 3)
    lo, hi = est.level_aabb(3)
    assert bool((x >= torch.tensor(lo)).all()) and bool((x <= torch.tensor(hi)).all())
    for lvl in range(4):  # an equal share per level, uniform in that level's box
        xs = x[lvl * 4096:(lvl + 1) * 4096]
        lo, hi = est.level_aabb(lvl)
        assert bool((xs >= torch.tensor(lo)).all()) and bool((xs <= torch.tensor(hi)).all())
        assert float(xs.abs().max()) > 0.9 * hi[0]
    assert float(x.abs().max()) > 0.9 * 12.0
    assert bool((torch.isin(dd, d)).all())
    # zero rays: default (random unit) directions instead of indexing an empty tensor
    x0, d0 = Rm._probe_in_box(torch.zeros(0, 3), torch.zeros(0, 3), None, est)
    assert x0.shape == (16384, 3) and d0.shape == (16384, 3)
    assert torch.allclose(d0.norm(dim=-1), torch.ones(16384), atol=1e-5)
    # one level: the level-0 box, as before
    x1, _ = Rm._probe_in_box(torch.zeros(300, 3), d, None, OccGridEstimator(AABB, 16, 1))
    assert float(x1.abs().max()) <= 1.5 and float(x1.abs().max()) > 1.4


def test_update_count_is_in_the_state_dict():
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    est = OccGridEstimator(AABB, 16, 4)
    est.generator = torch.Generator().manual_seed(11)
    est._updates = 7
    sd = est.state_dict()
    other = OccGridEstimator(AABB, 16, 4)
    other.generator = torch.Generator().manual_seed(11)
    assert other.update_seed(2) != est.update_seed(2)
    other.load_state_dict(sd, strict=True)
    assert other._updates == 7 and all(other.update_seed(lvl) == est.update_seed(lvl) for lvl in range(4))
    # a state_dict saved without the count loads strictly, with the count at 0
    old = {k: v for k, v in sd.items() if k in ("occs", "bits")}
    assert set(sd) - set(old)
    other.load_state_dict(old, strict=True)
    assert other._updates == 0
    assert set(old) == {"occs", "bits"}, "the caller's dict is left as it was"
    # inside a parent module (the prefix path)
    parent = torch.nn.ModuleDict({"est": est})
    psd = parent.state_dict()
    fresh = torch.nn.ModuleDict({"est": OccGridEstimator(AABB, 16, 4)})
    fresh.load_state_dict(psd, strict=True)
    assert fresh["est"]._updates == 7
    fresh.load_state_dict({k: v for k, v in psd.items() if k in ("est.occs", "est.bits")}, strict=True)
    assert fresh["est"]._updates == 0


# ---------------------------------------------------------------- GPU fixtures
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import fs_nerf_amd  # noqa: F401
    return torch.device("cuda:0")


def _net(dev, L=4, D=128, skip=(), seed=4, gain=64.0, shift=3.0, train=False):
    from fs_nerf_amd.core.models import NeRF
    sd = O.init_nerf_state_dict(L, D, list(skip), 10, 4, seed=seed)
    sd["sigma.weight"] *= gain
    sd["sigma.bias"] += shift
    m = NeRF(3, 3, L, D, skip, pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
    m.load_state_dict(sd)
    m = m.to(dev)
    return (m.train() if train else m.eval()), sd


def _level_balls(est, radius=0.7):
    """occupied = cell centre within `radius` of the box centre, in each level's own normalised coordinates [-1, 1]^3"""
    r = est.resolution
    c = (torch.arange(r, dtype=torch.float64) + 0.5) / r * 2 - 1
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    ball = (x * x + y * y + z * z).sqrt() < radius
    return ball[None].expand(est.levels, r, r, r).clone()


def _random_bits(levels, res, p, seed):
    return torch.rand(levels, res, res, res, generator=torch.Generator().manual_seed(seed)) < p


def _llff(dev, n_poses=3, hwf=(24, 32, 28.0)):
    """A few forward-facing poses through the dataset recipe (build_rays, NDC, near 1): rays and llff.py's box."""
    from fs_nerf_amd.utils import utilities as U
    poses = []
    for i in range(n_poses):
        a = math.radians(4.0 * (i - 1))
        p = torch.tensor([[math.cos(a), 0.0, math.sin(a), 0.15 * (i - 1)],
                          [0.0, 1.0, 0.0, -0.1 * i],
                          [-math.sin(a), 0.0, math.cos(a), 0.2 * i]], dtype=torch.float32)
        poses.append(p)
    ro, rd, aabb = U.build_rays(poses, hwf, dev, ndc=True)
    return ro.cpu(), rd.cpu(), [float(v) for v in aabb.cpu().tolist()]


def _subset(o, d, n, seed):
    idx = torch.randperm(o.shape[0], generator=torch.Generator().manual_seed(seed))[:n]
    return o[idx].contiguous(), d[idx].contiguous()


def _estimator(dev, aabb, res, levels, bins=None):
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    est = OccGridEstimator(roi_aabb=torch.tensor(aabb), resolution=res, levels=levels).to(dev)
    if bins is not None:
        est.set_binaries(bins)
        assert torch.equal(est.binaries.cpu(), bins)
    return est


# ---------------------------------------------------------------- selection, exact
def _states(levels, res):
    """name -> (binaries [levels,res,res,res], warm-up).  Every level differs from the others (level offsets)."""
    res3, n = res ** 3, res ** 3 // 4
    g = torch.Generator().manual_seed(res * 10 + levels)
    s = {"empty": (torch.zeros(levels, res, res, res, dtype=torch.bool), False),
         "full": (torch.ones(levels, res, res, res, dtype=torch.bool), False)}
    last = torch.zeros(levels, res3, dtype=torch.bool)
    for lvl in range(levels):
        last[lvl, res3 - 32 + 3 + 7 * lvl] = True  # one cell in the level's last bit-field word
    s["last-word"] = (last.reshape(levels, res, res, res), False)
    for name, count in (("sparse", lambda lvl: n // 7 + 131 * lvl), ("m==n", lambda lvl: n)):
        b = torch.zeros(levels, res3, dtype=torch.bool)
        for lvl in range(levels):
            b[lvl, torch.randperm(res3, generator=g)[:count(lvl)]] = True
        s[name] = (b.reshape(levels, res, res, res), False)
    s["dense"] = (torch.rand(levels, res, res, res, generator=g) < 0.45 + 0.1 * torch.arange(levels)[:, None, None, None]
                  / max(levels, 1), False)
    s["warm-up"] = (torch.rand(levels, res, res, res, generator=g) < 0.3, True)
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("res,levels", [(128, 1), (64, 4), (128, 4)])
def test_selection_matches_oracle(dev, res, levels):
    from fs_nerf_amd import ops
    res3, n = res ** 3, res ** 3 // 4
    est = _estimator(dev, AABB, res, levels)
    for k, (name, (bins, warm)) in enumerate(_states(levels, res).items()):
        est.set_binaries(bins)
        for lvl in range(levels):
            seed = (0x9E3779B97F4A7C15 * (lvl + 1) + 0x51ED * res + 977 * k) & 0xFFFFFFFFFFFFFFFF
            cells_h, x_h = ops.occgrid_select(est.bits, est.aabb, res, levels, lvl, warm, n, n, seed)
            cells_o, x_o = O.occgrid_select(bins[lvl], est.level_aabb(lvl), res, warm, n, n, seed)
            want = torch.where(cells_o >= 0, cells_o + lvl * res3, cells_o)
            assert torch.equal(cells_h.cpu(), want), (name, lvl)
            assert torch.equal(x_h.cpu(), x_o), (name, lvl)
            m = int(bins[lvl].sum())
            if not warm:
                unused = int((cells_o[n:] < 0).sum())
                assert unused == max(n - m, 0), (name, lvl)
                if m <= n:
                    assert torch.equal(cells_o[n:n + m], torch.nonzero(bins[lvl].reshape(-1)).reshape(-1)), (name, lvl)


# ---------------------------------------------------------------- update_every_n_steps replay
@pytest.mark.gpu
@pytest.mark.parametrize("levels,radius", [(1, 0.9), (4, 1.4)])
def test_update_every_n_steps_replays_the_oracle(dev, levels, radius):
    """Warm-up then post-warm-up update at 128^3 with an analytic density (a ball of `radius`: at one level 11 % of the
    cells are occupied, m < n; at four, level 0 is 58 % full, m > n, and the outer levels are sparse).  occ_eval_fn is
    evaluated once; the oracle gets the same values."""
    res, res3, n, thre = 128, 128 ** 3, 128 ** 3 // 4, 1e-2
    est = _estimator(dev, AABB, res, levels).train()
    est.generator = torch.Generator(device=dev).manual_seed(2024)
    calls = []

    def occ_eval_fn(x):
        v = 40.0 * STEP * torch.relu(radius - x.norm(dim=-1)) * (1.0 + 0.5 * torch.sin(7.0 * x[:, 0]))
        calls.append((x.cpu(), v.cpu()))
        return v

    bins_prev = torch.zeros(levels, res, res, res, dtype=torch.bool)
    for step in (0, 512):  # warm-up (every cell), then past it (uniform + occupied draws, EMA decay)
        warm = step < 256
        before = est.occs.cpu()
        seeds = [est.update_seed(lvl) for lvl in range(levels)]
        calls.clear()
        est.update_every_n_steps(step=step, occ_eval_fn=occ_eval_fn, occ_thre=thre)
        assert len(calls) == levels
        cells_all, vals_all = [], []
        for lvl in range(levels):
            c, x = O.occgrid_select(bins_prev[lvl], est.level_aabb(lvl), res, warm, n, n, seeds[lvl])
            assert torch.equal(calls[lvl][0], x), (step, lvl)
            cells_all.append(torch.where(c >= 0, c + lvl * res3, c))
            vals_all.append(calls[lvl][1])
            if not warm:
                assert int((c[n:] < 0).sum()) == max(n - int(bins_prev[lvl].sum()), 0)
        occs_o, touched, thr_o, _ = O.occgrid_update(before, torch.cat(cells_all), torch.cat(vals_all), 0.95, thre)
        occs_h = est.occs.cpu()
        assert torch.equal(occs_h, occs_o), (step, int((occs_h != occs_o).sum()))
        assert torch.equal(occs_h[~touched], before[~touched]), "cells not drawn stay unchanged"
        thr_h = torch.clamp(est.occs.mean(), max=thre)
        assert abs(float(thr_h) - thr_o) <= 1e-6 * thr_o, (float(thr_h), thr_o)
        assert torch.equal(est.binaries.reshape(-1).cpu(), (est.occs > thr_h).cpu())
        bins_prev = est.binaries.cpu()
        if step == 0:
            frac = [float(bins_prev[lvl].float().mean()) for lvl in range(levels)]
            assert any(f < 0.25 for f in frac), frac  # the m <= n rule is exercised
            if levels == 4:
                assert frac[0] > 0.25, frac  # ... and the with-replacement one


# ---------------------------------------------------------------- march, exact
def _hand_made_rays():
    """axis-parallel, along box faces (level 0 / 1 / outer of the 4-level synthetic box), origin inside level 0,
    missing every box"""
    o = torch.tensor([[0.2, -0.3, 4.0], [-20.0, 0.1, 0.3], [0.4, -20.0, -0.7],
                      [-20.0, 1.5, 0.3], [-20.0, 3.0, -3.0], [-20.0, 12.0, 0.3], [12.0, -20.0, 12.0],
                      [0.1, 0.2, -0.3], [0.0, 0.0, 0.0],
                      [20.0, 20.0, 20.0], [20.0, 20.0, 20.0], [-20.0, 13.0, 0.0]])
    d = torch.tensor([[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0],
                      [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0],
                      [0.3, -0.5, 0.8], [-0.6, 0.0, 0.8],
                      [1.0, 0.0, 0.0], [0.6, 0.8, 0.0], [1.0, 0.0, 0.01]])
    return o, d


def _march_both(est, bins, o, d, step, u, near=0.0, far=1e10):
    ms = est.max_steps(step)
    dev = est.bits.device
    ri, t0, t1 = est.sampling(o.to(dev), d.to(dev), render_step_size=step, stratified=u is not None,
                              u=None if u is None else u.to(dev), near_plane=near, far_plane=far)
    wri, wt0, wt1 = O.occgrid_march(o, d, est.aabb, est.resolution, est.levels, bins, near, far, step, u, ms)
    assert torch.equal(ri.cpu(), wri)
    assert torch.equal(t0.cpu(), wt0) and torch.equal(t1.cpu(), wt1)
    return wri, wt0


@pytest.mark.gpu
@pytest.mark.parametrize("strat", [False, True])
def test_march_four_levels_matches_oracle(dev, strat):
    """levels 4, res 128, step 5e-3, bit for bit: orbit rays + hand-made ones on the synthetic box; NDC rays of
    forward-facing poses on llff.py's box (their origins lie on the outer box's z face)."""
    bins = _random_bits(4, 128, 0.5, 1)
    est = _estimator(dev, AABB, 128, 4, bins)
    o, d = _orbit_rays(500, 3)
    ho, hd = _hand_made_rays()
    o, d = torch.cat([o, ho]), torch.cat([d, hd])
    u = torch.rand(o.shape[0], generator=torch.Generator().manual_seed(1)) if strat else None
    ri, _ = _march_both(est, bins, o, d, STEP, u)
    R0 = 500
    cnt = torch.bincount(ri, minlength=o.shape[0])
    assert int(cnt[:R0].min()) > 0
    assert bool((cnt[R0:R0 + 9] > 0).all()) and bool((cnt[R0 + 9:] == 0).all()), cnt[R0:].tolist()
    assert int(cnt.max()) > 2048  # longer than the fused kernel's slot rows
    # clipped by near and far
    rc, tc = _march_both(est, bins, o, d, STEP, u, near=2.0, far=9.0)
    assert 0 < rc.numel() < ri.numel() and float(tc.min()) >= 2.0 and float(tc.max()) < 9.0
    # the LLFF fixture
    lo_, ld_, box = _llff(dev)
    lo_, ld_ = _subset(lo_, ld_, 512, 2)
    lbins = _random_bits(4, 128, 0.5, 2)
    lest = _estimator(dev, box, 128, 4, lbins)
    lo3, hi3 = lest.level_aabb(3)
    assert abs(lo3[2] - float(lo_[:, 2].min())) < 1e-6, (lo3, float(lo_[:, 2].min()))  # the outer box's z face
    u2 = torch.rand(512, generator=torch.Generator().manual_seed(3)) if strat else None
    lri, _ = _march_both(lest, lbins, lo_, ld_, STEP, u2)
    assert int(torch.bincount(lri, minlength=512).min()) > 0


# ---------------------------------------------------------------- render_rays on 4-level grids
def _oracle_render(sd, o, d, ri, tv, R, step, L=4, skip=()):
    t0, t1 = (tv - step / 2).double(), (tv + step / 2).double()
    oo, dd = o.double(), d.double()
    sdd = {k: v.double() for k, v in sd.items()}

    def fn(a, b, c):
        out = O.nerf_forward(sdd, oo[c] + dd[c] * ((a + b) / 2)[:, None], dd[c], n_layers=L, skip=list(skip), n_freqs=10,
                             n_freqs_dir=4)
        return out[:, :3], out[:, 3]

    wc, wo, wd, _ = O.rendering_packed(t0, t1, ri, R, fn, torch.ones(3, dtype=torch.float64))
    return wc, wo, wd


def _check_against_oracle(rgb, opacity, depth, sd, o, d, ri, tv, step):
    R = o.shape[0]
    wc, wo, wd = _oracle_render(sd, o, d, ri.cpu(), tv.cpu(), R, step)
    assert float((rgb.cpu().double() - wc).abs().max()) < 2e-4
    assert float((opacity.cpu().double() - wo).abs().max()) < 2e-4
    # depth = sum(w t) / opacity: the same 2e-4 on sum(w t), in units of the farthest sample
    dd = (depth.cpu().double() - wd).abs() * wo.clamp(min=1e-2)
    assert float(dd.max()) < 2e-4 * max(1.0, float(tv.abs().max()))


@pytest.mark.gpu
def test_render_rays_llff_four_levels(dev):
    """llff.py's box at four levels takes the fused routes (max_steps <= 2048); fused = unfused bit for bit; both = the
    float64 oracle on the same samples."""
    from fs_nerf_amd.render import rendering as Rm
    from test_occ_fused import unfused
    o, d, box = _llff(dev)
    o, d = _subset(o, d, 512, 5)
    est = _estimator(dev, box, 128, 4, _level_balls(_estimator(dev, box, 128, 4), 0.7)).eval()
    m, sd = _net(dev, gain=16.0, shift=1.0)
    R = o.shape[0]
    assert est.max_steps(STEP) <= Rm.FUSED_OCC_MAX_STEPS
    assert Rm._rays_route(est, m, None, False, True, R, STEP) == "occ-extras"
    assert Rm._rays_route(est, m, None, False, False, R, STEP) == "occ-frame"
    with torch.no_grad():
        (rgb_u, op_u, dep_u, ex_u), ri, tv = unfused(lambda: Rm.render_rays(o, d, est, m, white_bkgd=True,
                                                                           render_step_size=STEP, device=dev))
        (rgb_e, op_e, dep_e, ex_e), ri_e, tv_e = Rm.render_rays(o, d, est, m, white_bkgd=True, render_step_size=STEP,
                                                               device=dev)
        (rgb_f, op_f, dep_f, _), ri_f, _ = Rm.render_rays(o, d, est, m, white_bkgd=True, render_step_size=STEP, device=dev,
                                                         want_extras=False)
    assert ri_f is None and ri.numel() > 10 * R
    for a, b in ((rgb_f, rgb_u), (op_f, op_u), (dep_f, dep_u), (rgb_e, rgb_u), (op_e, op_u), (dep_e, dep_u)):
        assert torch.equal(a, b), float((a - b).abs().max())
    assert torch.equal(ri_e, ri) and torch.equal(tv_e, tv) and torch.equal(ex_e["weights"], ex_u["weights"])
    _check_against_oracle(rgb_u, op_u, dep_u, sd, o, d, ri, tv, STEP)


@pytest.mark.gpu
def test_render_rays_synthetic_four_levels_takes_estimator_sampling(dev):
    from fs_nerf_amd.render import rendering as Rm
    bins = _level_balls(_estimator(dev, AABB, 128, 4), 0.6)
    est = _estimator(dev, AABB, 128, 4, bins).eval()
    m, sd = _net(dev)
    o, d = _orbit_rays(256, 9)
    assert est.max_steps(STEP) > Rm.FUSED_OCC_MAX_STEPS
    for grad, extras in ((False, True), (False, False), (True, True)):
        assert Rm._rays_route(est, m, None, grad, extras, 256, STEP) == "estimator-sampling"
    assert Rm._rays_route(est, m, None, True, True, 8192, STEP) == "estimator-sampling"
    with torch.no_grad():
        (rgb, op, dep, _), ri, tv = Rm.render_rays(o, d, est, m, white_bkgd=True, render_step_size=STEP, device=dev)
    assert ri.numel() > 10 * 256
    _check_against_oracle(rgb, op, dep, sd, o, d, ri, tv, STEP)


# ---------------------------------------------------------------- training gradients at four levels
@pytest.mark.gpu
def test_training_step_gradients_four_levels_llff(dev):
    """test_occgrid.test_training_step_gradients_through_the_occupancy_path on llff.py's box at four levels: parameter
    gradients within 2e-4 of each tensor's largest entry against float64 autograd on the same samples, rays with a ReLU
    unit within 4e-6 (relative) of zero weighted out of both losses."""
    from fs_nerf_amd.core.optim import FusedAdam
    from fs_nerf_amd.render import rendering as Rm
    L, skip = 4, ()
    m, sd = _net(dev, gain=16.0, shift=1.0, seed=6, train=True)
    opt = FusedAdam(m.parameters(), lr=1e-3)
    o, d, box = _llff(dev)
    R = 800
    o, d = _subset(o, d, R, 7)
    est = _estimator(dev, box, 128, 4, _level_balls(_estimator(dev, box, 128, 4), 0.7))
    est.train()
    est.generator = torch.Generator(device=dev).manual_seed(2)
    with torch.no_grad():
        _, ri0, tv0 = Rm.render_rays(o, d, est, m, train=True, white_bkgd=True, render_step_size=STEP, device=dev)
    ri0, tv0 = ri0.cpu(), tv0.cpu()
    risky = _relu_margin_rel(sd, o[ri0] + d[ri0] * tv0[:, None], d[ri0], L, skip) < 4e-6
    ray_ok = torch.ones(R, dtype=torch.bool)
    ray_ok[ri0[risky]] = False
    assert int(ray_ok.sum()) >= 40, int(ray_ok.sum())
    c = torch.randn(R, 3, generator=torch.Generator().manual_seed(4)) * ray_ok[:, None]
    est.generator = torch.Generator(device=dev).manual_seed(2)
    opt.zero_grad()
    (rgb, _, _, _), ri, tv = Rm.render_rays(o, d, est, m, train=True, white_bkgd=True, render_step_size=STEP, device=dev)
    assert torch.equal(ri.cpu(), ri0) and torch.equal(tv.cpu(), tv0) and ri.numel() > 2000 and rgb.requires_grad
    (rgb * c.to(dev)).sum().backward()
    cfg = dict(n_layers=L, skip=list(skip), n_freqs=10, n_freqs_dir=4)
    sdr = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    oo, dd = o.double(), d.double()
    t0, t1 = (tv0 - STEP / 2).double(), (tv0 + STEP / 2).double()

    def fn(a, b, cc):
        y = O.nerf_forward(sdr, oo[cc] + dd[cc] * ((a + b) / 2)[:, None], dd[cc], **cfg)
        return y[:, :3], y[:, 3]

    col = O.rendering_packed(t0, t1, ri0, R, fn, torch.ones(3, dtype=torch.float64))[0]
    (col * c.double()).sum().backward()
    for name, p in m.named_parameters():
        t = sdr[name].grad
        err = float((p.grad.cpu().double() - t).abs().max() / t.abs().max().clamp(min=1e-30))
        assert err < 2e-4, (name, err)


# ---------------------------------------------------------------- the three defects on the GPU
@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 4])
def test_zero_rays_with_a_fresh_fp16x3_model(dev, levels):
    """render_rays with no rays on an occupancy estimator and a model that has not calibrated its fp16x3 scales yet:
    the calibration probe must not index the empty ray batch."""
    from fs_nerf_amd.render import rendering as Rm
    est = _estimator(dev, AABB, 32, levels, _level_balls(_estimator(dev, AABB, 32, levels), 0.7)).eval()
    step = 2.5e-2  # max_steps <= 2048 at four levels too: the fused routes, which calibrate on the estimator's probe
    for extras in (True, False):
        m, _ = _net(dev)
        assert m.precision == "fp16x3" and m.act_state.exps is None
        assert Rm._rays_route(est, m, None, False, extras, 0, step) == ("occ-extras" if extras else "occ-frame")
        z = torch.zeros(0, 3)
        with torch.no_grad():
            (rgb, op, dep, _), ri, _ = Rm.render_rays(z, z, est, m, white_bkgd=True, render_step_size=step, device=dev,
                                                      want_extras=extras)
        assert rgb.shape == (0, 3) and op.shape == (0, 1) and dep.shape == (0, 1)
        assert ri is None or ri.numel() == 0
        assert m.act_state.exps is not None  # calibrated on the probe of the level boxes


@pytest.mark.gpu
def test_state_dict_round_trip_gives_the_same_next_update(dev):
    est = _estimator(dev, AABB, 64, 2).train()
    est.generator = torch.Generator(device=dev).manual_seed(9)

    def occ_eval_fn(x):
        return STEP * 40.0 * torch.relu(1.0 - x.norm(dim=-1))

    for step in (0, 256, 272):
        est.update_every_n_steps(step=step, occ_eval_fn=occ_eval_fn)
    sd = {k: v.clone() for k, v in est.state_dict().items()}
    resumed = _estimator(dev, AABB, 64, 2).train()
    resumed.generator = torch.Generator(device=dev).manual_seed(9)
    resumed.load_state_dict(sd, strict=True)
    assert resumed._updates == 3 and resumed.update_seed(1) == est.update_seed(1)
    est.update_every_n_steps(step=288, occ_eval_fn=occ_eval_fn)
    resumed.update_every_n_steps(step=288, occ_eval_fn=occ_eval_fn)
    assert torch.equal(resumed.occs, est.occs) and torch.equal(resumed.bits, est.bits)
