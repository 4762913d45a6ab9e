"""CPU: the occupancy march with per-ray bounds and cone-angle steps (fsn_occgrid_march_ex), as restated by
tests/occ_cone_ref.py: it is the oracle's march when nothing new is asked for; the properties of the cone lattice
(blocks of 64 intervals of one width, dt = max(t cone_angle, step)); the lattice-point counts the cone angle buys in
the reference's LLFF configuration, from OccGridEstimator.max_steps itself; the routes `sampling_kwargs` selects; and
the new entry points' argument validation without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L
from fs_nerf_amd.core.models import NeRF
from fs_nerf_amd.render import rendering as Rm
from fs_nerf_amd.render.occgrid import OccGridEstimator
from oracle import fsnerf_oracle as O

import occ_cone_ref as CR
from test_occgrid import AABB, _orbit_rays, _sphere_binaries

RES, LEVELS, STEP = 16, 2, 0.02


@pytest.mark.parametrize("with_u", [False, True])
def test_restatement_is_the_oracle_without_cone_and_bounds(with_u):
    bins = _sphere_binaries(RES, LEVELS)
    o, d = _orbit_rays(50, 1)
    u = torch.rand(50, generator=torch.Generator().manual_seed(0)) if with_u else None
    want = O.occgrid_march(o, d, AABB, RES, LEVELS, bins, 0.0, 1e10, 0.05, u)
    got = CR.march(o, d, AABB, RES, LEVELS, bins, 0.0, 1e10, 0.05, u)
    assert want[0].numel() > 100
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g, w)
    # infinite bounds tighten nothing
    inf = torch.full((50,), float("inf"))
    got = CR.march(o, d, AABB, RES, LEVELS, bins, 0.0, 1e10, 0.05, u, t_min=-inf, t_max=inf)
    assert all(torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("cone", [0.01, 0.05])
@pytest.mark.parametrize("near", [0.0, 0.7])
def test_cone_lattice_properties(cone, near):
    o, d = _orbit_rays(50, 1)
    u = torch.rand(50, generator=torch.Generator().manual_seed(0))
    full = torch.ones(LEVELS, RES, RES, RES, dtype=torch.bool)
    est = OccGridEstimator(AABB, RES, LEVELS)
    bound = est.max_steps(STEP, cone, near)
    for bins, uu in ((full, None), (full, u), (_sphere_binaries(RES, LEVELS), u)):
        ri, t0, t1 = CR.march(o, d, AABB, RES, LEVELS, bins, near, 1e10, STEP, uu, cone_angle=cone)
        assert ri.numel() > 100 and bool((ri[1:] >= ri[:-1]).all()), "sorted by ray"
        same = ri[1:] == ri[:-1]
        assert bool((t0[1:][same] > t0[:-1][same]).all()), "sorted by t inside a ray"
        if bins is full:
            assert torch.equal(t1[:-1][same], t0[1:][same]), "a full grid's samples are contiguous, bitwise"
        # step <= dt <= max(step, t_start cone_angle) (1 + 1e-6) for the block width dt; t_ends - t_starts is that width
        # seen through two float32 endpoints t_b + j dt, each rounded twice (the product, the sum) by at most half a
        # unit in the last place of t_ends: 2 ulp in all
        dt, ulp = (t1.double() - t0.double()), 2 * torch.from_numpy(np.spacing(t1.numpy())).double()
        assert bool((dt >= np.float32(STEP) - ulp).all())
        assert bool((dt <= torch.clamp(t0.double() * cone, min=float(np.float32(STEP))) * (1 + 1e-6) + ulp).all())
        assert float(t0.min()) >= float(np.float32(near))
        p = o[ri] + d[ri] * ((t0 + t1) / 2)[:, None]
        assert float(p.abs().max()) <= 1.5 * 2 ** (LEVELS - 1) + 1e-5, "midpoints inside the outermost box"
        assert int(torch.bincount(ri, minlength=50).max()) <= bound
    # the step really grows: far samples are wider than near ones
    assert float((t1 - t0).max()) > 1.5 * STEP
    # an empty grid gives nothing
    z = CR.march(o, d, AABB, RES, LEVELS, torch.zeros_like(full), near, 1e10, STEP, u, cone_angle=cone)
    assert z[0].numel() == 0
    # max_steps = 100 truncates inside the second block: the first 100 intervals of the untruncated march
    ri, t0, t1 = CR.march(o, d, AABB, RES, LEVELS, full, near, 1e10, STEP, u, cone_angle=cone)
    ri_c, t0_c, t1_c = CR.march(o, d, AABB, RES, LEVELS, full, near, 1e10, STEP, u, max_steps=100, cone_angle=cone)
    n, n_c = torch.bincount(ri, minlength=50), torch.bincount(ri_c, minlength=50)
    assert int(n.max()) > 100 and torch.equal(n_c, n.clamp(max=100))
    first = torch.cat([torch.arange(int(k)) < 100 for k in n])
    assert torch.equal(t0_c, t0[first]) and torch.equal(t1_c, t1[first])


def test_lattice_point_counts_of_the_llff_configuration():
    """run-nerf.py:92-98: the +-1.5 region of interest at step 5e-3, one level and four."""
    one, four = OccGridEstimator(AABB, 4, 1), OccGridEstimator(AABB, 4, 4)
    assert one.max_steps(5e-3) == 1042 and four.max_steps(5e-3) == 8316
    assert one.max_steps(5e-3, 0.0, 0.0) == 1042
    assert 64 <= one.max_steps(5e-3, 0.004) <= 704 + 64
    assert 64 <= four.max_steps(5e-3, 0.004) <= 1280 + 64
    assert four.max_steps(5e-3, 0.01) <= 704 + 64
    assert four.max_steps(5e-3, 0.004) <= Rm.FUSED_OCC_MAX_STEPS < four.max_steps(5e-3)
    assert four.max_steps(1e-6, 1e-9) == 16384, "capped"
    assert four.max_steps(5e-3, 0.004, near_plane=2.0) <= four.max_steps(5e-3, 0.004)


def _nerf():
    return NeRF(3, 3, 2, 16, (), precision="fp16x3", pos_fn={"n_freqs": 2, "log_space": True},
                dir_fn={"n_freqs": 1, "log_space": True}).eval()


def test_routes_with_sampling_options():
    est, m = OccGridEstimator(AABB, resolution=16), _nerf()
    scalars = dict(near_plane=3.0, far_plane=5.0, early_stop_eps=1e-3, alpha_thre=1e-3)
    bounds = torch.zeros(64)
    for grad, extras, n_rays in ((False, False, 64), (False, True, 64), (True, True, 64), (True, True, 4096)):
        base = Rm._rays_route(est, m, None, grad, extras, n_rays, 5e-3)
        assert base in ("occ-frame", "occ-extras", "occ-sampler", "estimator-sampling")
        assert Rm._rays_route(est, m, None, grad, extras, n_rays, 5e-3, None) == base
        assert Rm._rays_route(est, m, None, grad, extras, n_rays, 5e-3, {}) == base
        assert Rm._rays_route(est, m, None, grad, extras, n_rays, 5e-3, scalars) == base
        assert Rm._rays_route(est, m, None, grad, extras, n_rays, 5e-3, dict(cone_angle=0.0)) == base
        for opts in (dict(cone_angle=0.004), dict(t_min=bounds), dict(t_max=bounds), dict(scalars, cone_angle=0.01)):
            assert Rm._rays_route(est, m, None, grad, extras, n_rays, 5e-3, opts) == "estimator-sampling"
    assert Rm._frame_route(est, m, None, False, False, 5e-3) == "camera-occupancy"
    assert Rm._frame_route(est, m, None, False, False, 5e-3, scalars) == "camera-occupancy"
    assert Rm._frame_route(est, m, None, False, False, 5e-3, dict(cone_angle=0.004)) == "chunked"
    strat = Rm.StratifiedEstimator(2.0, 6.0, 8, 16)
    assert Rm._frame_route(strat, m, None, False, False, 5e-3, dict(near_plane=3.0)) == "camera-stratified"


def test_sampling_kwargs_are_checked():
    est, m = OccGridEstimator(AABB, resolution=16), _nerf()
    o, d = torch.zeros(8, 3), torch.ones(8, 3)
    with pytest.raises(TypeError, match="bogus"):
        Rm.render_rays(o, d, est, m, device="cpu", sampling_kwargs={"bogus": 1})
    with pytest.raises(TypeError, match="bogus"):
        Rm.render_frame((4, 4, 5.0), 2.0, 6.0, torch.eye(4), 64, est, m, device="cpu", sampling_kwargs={"bogus": 1})
    with pytest.raises(TypeError, match="t_min"):  # frames take no per-ray bounds
        Rm.render_frame((4, 4, 5.0), 2.0, 6.0, torch.eye(4), 64, est, m, device="cpu",
                        sampling_kwargs={"t_min": torch.zeros(16)})
    with pytest.raises(TypeError, match="bogus"):
        Rm.render_path(torch.eye(4)[None], (4, 4, 5.0), 2.0, 6.0, 64, m, est, device="cpu", sampling_kwargs={"bogus": 1})
    strat = Rm.StratifiedEstimator(2.0, 6.0, 8, 0)
    for kw in (dict(cone_angle=0.01), dict(t_min=torch.zeros(8)), dict(t_max=torch.zeros(8))):
        with pytest.raises(ValueError):
            strat.sampling(o, d, **kw)
    with pytest.raises(NotImplementedError):
        est.sampling(o, d, alpha_fn=lambda *a: None)
    with pytest.raises(ValueError):
        est.sampling(o, d, cone_angle=-0.1)
    with pytest.raises(ValueError):
        est.sampling(o, d, cone_angle=0.1, near_plane=-1.0)


def test_new_entry_points_validate_without_gpu():
    lib = L.lib()
    aabb = (C.c_float * 6)(0, 0, 0, 1, 1, 1)
    march = lambda R=5, res=16, near=0.0, step=0.1, cone=0.0: lib.fsn_occgrid_march_ex(
        None, None, R, aabb, res, 1, None, near, 1.0, step, None, 8, None, None, cone, None, None, None, None, None, None)
    assert march(R=0) == 0  # no rays: nothing to do
    assert march(res=0) != 0 and b"resolution" in lib.fsn_last_error()
    assert march(step=0.0) != 0 and b"fsn_occgrid_march_ex" in lib.fsn_last_error()
    assert march(cone=-0.01) != 0 and b"cone_angle" in lib.fsn_last_error()
    assert march(cone=0.01, near=-1.0) != 0 and b"near_plane" in lib.fsn_last_error()
    assert march(cone=0.01) != 0 and b"null pointer" in lib.fsn_last_error()
    assert march() != 0 and b"null pointer" in lib.fsn_last_error()
    inf = float("inf")
    assert lib.fsn_ray_aabb_intersect(None, None, 0, None, 3, -inf, inf, inf, None, None, None, None) == 0
    assert lib.fsn_ray_aabb_intersect(None, None, 5, None, 3, -inf, inf, inf, None, None, None, None) != 0
    assert b"fsn_ray_aabb_intersect: null pointer" in lib.fsn_last_error()
    assert lib.fsn_ray_aabb_intersect(None, None, -1, None, 3, -inf, inf, inf, None, None, None, None) != 0


def test_ray_aabb_restatement():
    """The restatement against hand-worked cases: an axis-parallel ray, a miss, an origin inside, finite planes."""
    o = torch.tensor([[0.0, 0.0, -3.0], [0.0, 2.0, -3.0], [0.2, 0.1, 0.0], [0.0, 0.0, -3.0]])
    d = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]])
    box = torch.tensor([[-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]])
    t0, t1, hit = CR.ray_aabb_intersect(o, d, box)
    assert hit.reshape(-1).tolist() == [True, False, True, True]  # (no near plane: the box behind the last ray counts)
    assert float(t0[0, 0]) == 2.0 and float(t1[0, 0]) == 4.0 and float(t0[3, 0]) == -4.0 and float(t1[3, 0]) == -2.0
    assert abs(float(t0[2, 0]) + 1.1) < 1e-6 and abs(float(t1[2, 0]) - 0.9) < 1e-6
    assert float(t0[1, 0]) == np.inf and float(t1[1, 0]) == np.inf
    t0, t1, hit = CR.ray_aabb_intersect(o, d, box, near_plane=0.0, far_plane=3.0, miss_value=-1.0)
    assert hit.reshape(-1).tolist() == [True, False, True, False]
    assert float(t0[0, 0]) == 2.0 and float(t1[0, 0]) == 3.0 and float(t0[2, 0]) == 0.0
    assert float(t0[1, 0]) == -1.0 and float(t1[3, 0]) == -1.0
