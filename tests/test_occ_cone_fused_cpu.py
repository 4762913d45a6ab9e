"""CPU: cone-angle steps and per-ray bounds in the one-launch occupancy kernel (fsn_render_rays_occgrid_ex,
fsn_occ_gather_ex): the new entry points' argument validation without a device (every check runs before any device
work, so the pointers handed over here are never followed), and the routes `sampling_kwargs` selects with the
FUSED_OCC_CONE switch off (today's) and on."""
import ctypes as C

import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L
from fs_nerf_amd import ops
from fs_nerf_amd.core.models import NeRF
from fs_nerf_amd.render import rendering as Rm
from fs_nerf_amd.render.occgrid import OccGridEstimator

from test_occgrid import AABB

INVALID, UNSUPPORTED = -1, -2


def _args(R=5, near=0.0, max_steps=8, rays=True, sampler=False, host=None):
    """Launch arguments that pass every check of the plain entry point up to the device work; `host`: a host buffer
    whose address stands for the device pointers (validation only)."""
    a = L.OccRenderArgs()
    p = C.addressof(host)
    a.R, a.step, a.max_steps, a.near_plane, a.far_plane = R, 0.1, max_steps, near, 1e10
    for i, v in enumerate((0, 0, 0, 1, 1, 1)):
        a.aabb[i] = v
    a.res, a.levels, a.bits, a.work_counter = 16, 1, p, p
    a.colors, a.opacity, a.depth = p, p, p
    if rays:
        a.rays_o, a.rays_d = p, p
    else:
        a.cam_H, a.cam_W, a.cam_focal = 4, 4, 5.0
    if sampler:
        a.sample_t0, a.sample_cap, a.n_kept = p, max_steps, p
    return a


def test_extended_render_entry_validates_without_gpu():
    lib = L.lib()
    d = ops.make_desc(8, 256, (4,), [2.0 ** i for i in range(10)], [2.0 ** i for i in range(4)])
    host = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(host))

    def call(a, cone=0.0, t_min=None, t_max=None, t1=None, prec=L.FSN_PREC_FP16X3):
        return lib.fsn_render_rays_occgrid_ex(C.byref(d), prec, p, C.byref(a), cone, t_min, t_max, t1, None)

    assert call(_args(R=0, host=host)) == 0  # no rays: nothing to do
    assert call(_args(R=0, host=host), cone=0.01, t1=None) == 0
    assert call(_args(host=host), cone=-0.01) == INVALID
    assert b"fsn_render_rays_occgrid_ex" in lib.fsn_last_error() and b"cone_angle" in lib.fsn_last_error()
    assert call(_args(R=0, host=host), cone=-0.01) == INVALID, "the scalar checks come first"
    assert call(_args(near=-1.0, host=host), cone=0.01) == INVALID and b"near_plane" in lib.fsn_last_error()
    for kw in (dict(t_min=p), dict(t_max=p), dict(t_min=p, t_max=p)):
        assert call(_args(rays=False, host=host), **kw) == INVALID and b"camera" in lib.fsn_last_error(), kw
    assert call(_args(sampler=True, host=host), cone=0.01) == INVALID and b"sample_t1" in lib.fsn_last_error()
    # max_steps above one ray group's LDS list: unsupported, with and without a cone angle
    assert call(_args(max_steps=2049, host=host)) == UNSUPPORTED and b"max_steps 2049" in lib.fsn_last_error()
    assert call(_args(max_steps=2049, sampler=True, host=host), cone=0.01, t1=p) == UNSUPPORTED
    assert b"max_steps 2049" in lib.fsn_last_error()
    # the plain entry point reports under its own name
    assert lib.fsn_render_rays_occgrid(C.byref(d), L.FSN_PREC_FP16X3, p, C.byref(_args(max_steps=2049, host=host)), None) == UNSUPPORTED
    assert b"fsn_render_rays_occgrid: max_steps 2049" in lib.fsn_last_error()
    assert call(_args(host=host), prec=L.FSN_PREC_FP16X2) == UNSUPPORTED and b"precision mode 6" in lib.fsn_last_error()


def test_extended_gather_entry_validates_without_gpu():
    lib = L.lib()
    host = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(host))
    five = (C.c_void_p * 5)(*[C.addressof(host)] * 5)
    assert lib.fsn_occ_gather_ex(None, None, None, None, 8, 0, 0.1, None, None, None, None, None, None) == 0
    assert lib.fsn_occ_gather_ex(None, None, None, None, 8, 5, 0.1, None, None, None, None, None, None) == INVALID
    assert b"fsn_occ_gather_ex: null pointer" in lib.fsn_last_error()
    assert lib.fsn_occ_gather_ex(p, p, p, p, 0, 5, 0.1, p, p, p, None, None, None) == INVALID and b"bad sizes" in lib.fsn_last_error()
    assert lib.fsn_occ_gather_ex(p, p, p, p, 8, 5, 0.1, p, p, p, five, None, None) == INVALID
    assert b"come together" in lib.fsn_last_error()
    holes = (C.c_void_p * 5)(C.addressof(host), None, None, None, None)
    assert lib.fsn_occ_gather_ex(p, p, p, None, 8, 5, 0.1, p, p, p, holes, five, None) == INVALID
    assert b"array 1" in lib.fsn_last_error()


def _nerf():
    return NeRF(3, 3, 2, 16, (), precision="fp16x3", pos_fn={"n_freqs": 2, "log_space": True},
                dir_fn={"n_freqs": 1, "log_space": True}).eval()


GRID = ((False, False, 64), (False, True, 64), (True, True, 64), (True, True, 4096))
SCALARS = dict(near_plane=3.0, far_plane=5.0, early_stop_eps=1e-3, alpha_thre=1e-3)


def _option_sets():
    bounds = torch.zeros(64)
    return (dict(cone_angle=0.004), dict(t_min=bounds), dict(t_max=bounds), dict(SCALARS, cone_angle=0.01))


def test_switch_is_off_by_default_and_routes_are_todays():
    assert Rm.FUSED_OCC_CONE is False
    est, m = OccGridEstimator(AABB, resolution=16), _nerf()
    for grad, extras, n_rays in GRID:
        for opts in _option_sets():
            assert Rm._rays_route(est, m, None, grad, extras, n_rays, 5e-3, opts) == "estimator-sampling"
    assert Rm._frame_route(est, m, None, False, False, 5e-3, dict(cone_angle=0.004)) == "chunked"
    assert Rm._frame_route(est, m, None, False, False, 5e-3) == "camera-occupancy"


def test_switch_on_gives_the_route_of_the_call_without_options(monkeypatch):
    monkeypatch.setattr(Rm, "FUSED_OCC_CONE", True)
    est, m = OccGridEstimator(AABB, resolution=16), _nerf()
    seen = set()
    for grad, extras, n_rays in GRID:
        base = Rm._rays_route(est, m, None, grad, extras, n_rays, 5e-3)
        seen.add(base)
        for opts in _option_sets():
            assert Rm._rays_route(est, m, None, grad, extras, n_rays, 5e-3, opts) == base, (grad, extras, n_rays, opts)
    assert seen == {"occ-frame", "occ-extras", "occ-sampler", "estimator-sampling"}
    assert Rm._frame_route(est, m, None, False, False, 5e-3, dict(cone_angle=0.004)) == "camera-occupancy"
    assert Rm._frame_route(est, m, None, True, False, 5e-3, dict(cone_angle=0.004)) == "chunked"  # (training frames: as before)
    with pytest.raises(TypeError, match="t_min"):  # frames still take no per-ray bounds
        Rm.render_frame((4, 4, 5.0), 2.0, 6.0, torch.eye(4), 64, est, m, device="cpu", sampling_kwargs={"t_min": torch.zeros(16)})
    # the opt-in bf16 cull keeps its sampler route
    m.cull_precision = "bf16"
    for opts in (None,) + _option_sets():
        assert Rm._rays_route(est, m, None, False, True, 64, 5e-3, opts) == "occ-sampler"
        assert Rm._rays_route(est, m, None, False, False, 64, 5e-3, opts) == "occ-sampler"
    assert Rm._frame_route(est, m, None, False, False, 5e-3, dict(cone_angle=0.004)) == "chunked"


def test_four_level_grid_fits_one_launch_only_with_the_cone_angle(monkeypatch):
    """run-nerf.py:92-98: four levels at 128^3, step 5e-3: 8316 lattice points per ray without a cone angle, at most 1344
    intervals with cone_angle 0.004 (tests/test_occ_cone_cpu.py), against the 2048 one ray group holds."""
    est, m = OccGridEstimator(AABB, resolution=128, levels=4), _nerf()
    cone, thin = dict(cone_angle=0.004), dict(cone_angle=1e-4)
    assert est.max_steps(5e-3, 0.004) <= Rm.FUSED_OCC_MAX_STEPS < est.max_steps(5e-3, 1e-4)
    for on in (False, True):
        monkeypatch.setattr(Rm, "FUSED_OCC_CONE", on)
        assert Rm._rays_route(est, m, None, False, False, 64, 5e-3) == "estimator-sampling"
        assert Rm._rays_route(est, m, None, False, True, 64, 5e-3) == "estimator-sampling"
        assert Rm._frame_route(est, m, None, False, False, 5e-3) == "chunked"
        for opts in (thin, dict(thin, near_plane=0.5)):
            assert Rm._rays_route(est, m, None, False, False, 64, 5e-3, opts) == "estimator-sampling"
            assert Rm._rays_route(est, m, None, False, True, 64, 5e-3, opts) == "estimator-sampling"
            assert Rm._rays_route(est, m, None, True, True, 4096, 5e-3, opts) == "estimator-sampling"
            assert Rm._frame_route(est, m, None, False, False, 5e-3, opts) == "chunked"
    assert Rm.FUSED_OCC_CONE is True
    assert Rm._rays_route(est, m, None, False, False, 64, 5e-3, cone) == "occ-frame"
    assert Rm._rays_route(est, m, None, False, True, 64, 5e-3, cone) == "occ-extras"
    assert Rm._rays_route(est, m, None, True, True, 4096, 5e-3, cone) == "occ-sampler"
    assert Rm._rays_route(est, m, None, True, True, 64, 5e-3, cone) == "estimator-sampling"  # below the sampler's floor
    assert Rm._frame_route(est, m, None, False, False, 5e-3, cone) == "camera-occupancy"
    # the extras mode's slot rows: nine arrays per slot in the cone regime against eight
    ms = est.max_steps(5e-3, 0.004)
    n8, n9 = Rm.FUSED_OCC_EXTRAS_MAX_SLOTS // ms, Rm.FUSED_OCC_EXTRAS_MAX_SLOTS * 8 // (9 * ms)
    assert n9 < n8
    assert Rm._rays_route(est, m, None, False, True, n9, 5e-3, cone) == "occ-extras"
    assert n9 + 1 >= Rm.FUSED_OCC_SAMPLER_MIN_RAYS  # (past the bound: the sampler launch + the full pass)
    assert Rm._rays_route(est, m, None, False, True, n9 + 1, 5e-3, cone) == "occ-sampler"
    one = OccGridEstimator(AABB, resolution=16)
    ms1 = one.max_steps(5e-3)
    bounds = dict(t_min=torch.zeros(4))  # (the uniform regime with bounds: eight arrays, as without)
    assert Rm._rays_route(one, m, None, False, True, Rm.FUSED_OCC_EXTRAS_MAX_SLOTS // ms1, 5e-3, bounds) == "occ-extras"
    assert Rm._rays_route(one, m, None, False, True, Rm.FUSED_OCC_EXTRAS_MAX_SLOTS // ms1 + 1, 5e-3, bounds) == "occ-sampler"


def test_ops_keywords_are_checked_before_the_launch():
    """ops.render_occ_fused / occ_sample_fused: the bounds hold one value per ray and need ray tensors."""
    import inspect
    for fn in (ops.render_occ_fused, ops.occ_sample_fused):
        sig = inspect.signature(fn).parameters
        assert sig["cone_angle"].default == 0.0 and sig["t_min"].default is None and sig["t_max"].default is None
    keep = ops._Held(None)
    with pytest.raises(TypeError, match="camera"):
        ops._occ_march_options(16, 0.0, torch.zeros(16), None, object(), keep)
    assert ops._occ_march_options(16, 0.5, None, None, object(), keep) == (0.5, None, None)
    for kw in (dict(t_min=torch.zeros(15)), dict(t_max=torch.zeros(17)), dict(t_min=torch.zeros(16), t_max=torch.zeros(4, 5))):
        with pytest.raises(ValueError, match="one value per ray"):
            ops._occ_march_options(16, 0.0, kw.get("t_min"), kw.get("t_max"), None, keep)
    with pytest.raises(RuntimeError, match="t_max: expected a GPU tensor"):  # (no CPU fallback)
        ops._occ_march_options(16, 0.0, None, torch.zeros(16), None, keep)
