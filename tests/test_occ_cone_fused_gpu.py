"""GPU: cone-angle steps and per-ray bounds in the one-launch occupancy kernel (k_render_occ through
fsn_render_rays_occgrid_ex, csrc/render_occ.hip).  The yardstick throughout is bit-for-bit equality with the multi-launch
sequence, which has handled these options since the standalone march got them: occgrid_march -> density pass ->
packed_visibility -> compaction -> full pass -> packed integration (what OccGridEstimator.sampling -> forward_rays ->
rendering run, and render_rays with FUSED_OCC_CONE off).  All three modes of the launch are compared: frame (per-ray
outputs), extras (+ the packed per-sample arrays) and sampler (the kept samples).  Grids are 16^3 and calls hold 256 rays:
what can go wrong - block boundaries of the cone march, the variable widths in the cull and the compaction, rays carried
between batches, truncation, empty rays - does not depend on the size."""
import ctypes as C
import math

import pytest
import torch

from oracle import fsnerf_oracle as O

import debug_lib
import test_occ_fused as TF
from test_occ_cone_gpu import BOX1, N_RAYS, STEP, estimator, field, mixed_rays, small_setup

pytestmark = pytest.mark.gpu
EXTRAS = ("weights", "alphas", "trans", "sigmas", "rgbs")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import fs_nerf_amd  # noqa: F401
    return torch.device("cuda:0")


def thin_model(dev, precision="fp16x3"):
    """4 x 128 network with a thin positive medium (test_occ_fused's carry case): the cull keeps most samples, so far -
    wide - intervals reach the full pass."""
    return TF.make_model(4, 128, 9, dev, precision=precision, gain=2.0, shift=1.0)


def multi_launch(est, m, od, dd, step, max_steps, *, near=0.0, cone=0.0, u=None, t_min=None, t_max=None, eps=1e-4,
                 athre=0.0):
    """The multi-launch sequence (OccGridEstimator.sampling's, with `max_steps` explicit) -> per-ray outputs, packed
    samples, extras and the marched count per ray."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.render import rendering as Rm
    R = od.shape[0]
    ri, t0, t1, n_cand = ops.occgrid_march(od, dd, est.aabb, est.resolution, est.levels, est.bits, near, 1e10, step, u,
                                           max_steps, t_min=t_min, t_max=t_max, cone_angle=cone)
    if (eps > 0.0 or athre > 0.0) and ri.numel() > 0:
        sig = m.forward_rays(od, dd, ri, t0, t1, full=False).reshape(-1)
        keep = ops.packed_visibility(sig, t0, t1, ri, R, eps, athre)
        ri, t0, t1 = ri[keep], t0[keep], t1[keep]
    if ri.numel() == 0:  # (no sample anywhere: pure background)
        ex = {k: torch.empty(0, device=od.device) for k in EXTRAS[:4]}
        ex["rgbs"] = torch.empty(0, 3, device=od.device)
        return (torch.ones(R, 3, device=od.device), torch.zeros(R, 1, device=od.device),
                torch.zeros(R, 1, device=od.device)), (ri, t0, t1), ex, n_cand

    def rgb_sigma_fn(a, b, c):
        out = m.forward_rays(od, dd, c, a, b, full=True)
        return out[..., :3], out[..., -1]

    rgb, op, dep, ex = Rm.rendering(t0, t1, ri, R, rgb_sigma_fn, torch.full((3,), 1.0))
    return (rgb, op, dep), (ri, t0, t1), ex, n_cand


def three_modes(est, m, o, d, dev, step, max_steps, what="", **kw):
    """Frame, extras and sampler mode of the one launch against the multi-launch sequence, bit for bit -> (t_starts,
    t_ends, marched counts) of the sequence."""
    from fs_nerf_amd import ops
    od, dd = o.to(dev), d.to(dev)
    kw = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    with torch.no_grad():
        (rgb, op, dep), (ri, t0, t1), ex, n_cand = multi_launch(est, m, od, dd, step, max_steps, **kw)
        args = dict(aabb=est.aabb, res=est.resolution, levels=est.levels, bits=est.bits, near_plane=kw.get("near", 0.0),
                    far_plane=1e10, step=step, max_steps=max_steps, u=kw.get("u"), early_stop_eps=kw.get("eps", 1e-4),
                    alpha_thre=kw.get("athre", 0.0), cone_angle=kw.get("cone", 0.0), t_min=kw.get("t_min"),
                    t_max=kw.get("t_max"))
        pm = m.packed()
        f_rgb, f_op, f_dep, cnt = ops.render_occ_fused(pm, od, dd, bkgd=(1.0, 1.0, 1.0), want_counts=True, **args)
        e_rgb, e_op, e_dep, e_cnt, (e_ri, e_t0, e_t1, e_ex) = ops.render_occ_fused(pm, od, dd, bkgd=(1.0, 1.0, 1.0),
                                                                                   want_extras=True, **args)
        s_ri, s_t0, s_t1 = ops.occ_sample_fused(pm, od, dd, **args)
    torch.cuda.synchronize()
    n_kept = torch.bincount(ri, minlength=od.shape[0])
    print(f"{what}: {int(n_cand.sum())} marched, {ri.numel()} kept, max per ray {int(n_cand.max())}; "
          f"frame max |d rgb| {float((f_rgb - rgb).abs().max()):.3e}")
    assert torch.equal(cnt["n_cand"].long(), n_cand) and torch.equal(cnt["n_kept"].long(), n_kept), what
    assert torch.equal(e_cnt["n_cand"].long(), n_cand) and torch.equal(e_cnt["n_kept"].long(), n_kept), what
    assert torch.equal(s_ri, ri) and torch.equal(s_t0, t0) and torch.equal(s_t1, t1), f"sampler mode: {what}"
    assert torch.equal(f_rgb, rgb) and torch.equal(f_op, op) and torch.equal(f_dep, dep), f"frame mode: {what}"
    assert torch.equal(e_rgb, rgb) and torch.equal(e_op, op) and torch.equal(e_dep, dep), f"extras mode: {what}"
    assert e_ri.dtype == torch.int64 and torch.equal(e_ri, ri) and torch.equal(e_t0, t0) and torch.equal(e_t1, t1), what
    for k in EXTRAS:
        assert e_ex[k].shape == ex[k].shape and torch.equal(e_ex[k], ex[k]), (what, k)
    return t0, t1, n_cand


@pytest.mark.parametrize("cone", [0.01, 0.05])
@pytest.mark.parametrize("kind", ["random", "ones", "zeros"])
def test_three_launch_modes_are_the_multi_launch_sequence(dev, kind, cone):
    est = estimator(BOX1, 16, 3, field(kind), dev)
    m = thin_model(dev)
    o, d = mixed_rays()
    u = torch.rand(N_RAYS, generator=torch.Generator().manual_seed(1))
    ms = est.max_steps(STEP, cone)
    for uu in (None, u):
        for eps, athre in ((1e-4, 1e-3), (0.0, 0.0)):  # (both zero: no density pass, every marched sample is kept)
            t0, t1, n_cand = three_modes(est, m, o, d, dev, STEP, ms, f"{kind} cone {cone} u {uu is not None} cull {eps, athre}",
                                         cone=cone, u=uu, eps=eps, athre=athre)
            if kind == "zeros":
                assert t0.numel() == 0
                continue
            widths = t1 - t0
            assert float(widths.max()) > 1.5 * float(widths.min()), "variable-width samples reach every pass"
            assert int(n_cand[200:254].max()) == 0 and int(n_cand[254]) > 0 and int(n_cand[255]) > 0  # misses, axis ray, inside
            if kind == "ones":
                assert int(n_cand.max()) > 128, "several blocks of 64"
                if eps > 0.0:
                    assert t0.numel() < int(n_cand.sum()), "the cull drops samples"
                else:
                    assert t0.numel() == int(n_cand.sum())


def carry_case(dev):
    """A full three-level grid at step 0.005 with cone_angle 0.002: up to 1472 intervals per ray (2774 lattice points
    without the cone angle, past the 2048 one ray group holds, so only the cone march fits)."""
    est = estimator(BOX1, 16, 3, field("ones"), dev)
    ms = est.max_steps(0.005, 0.002)
    assert ms == 1472 and est.max_steps(0.005) == 2774
    return est, ms


def test_rays_with_more_than_half_a_batch_are_carried(dev):
    """A ray with more than 1024 candidates shares its batch (2048) with no second one of its kind: every such ray is
    carried into a batch of its own, re-marched there, and the results are still the sequence's."""
    from fs_nerf_amd.render import rendering as Rm
    est, ms = carry_case(dev)
    assert ms <= Rm.FUSED_OCC_MAX_STEPS < est.max_steps(0.005)
    o, d = mixed_rays()
    _, _, n_cand = three_modes(est, thin_model(dev), o, d, dev, 0.005, ms, "carry", cone=0.002)
    assert int((n_cand > 1024).sum()) >= 2 and int(n_cand.max()) <= ms, int(n_cand.max())


@pytest.mark.parametrize("cone", [0.0, 0.01])
def test_truncated_march(dev, cone):
    """max_steps = 100 ends inside the second block of 64: the launch equals the truncated march."""
    est = estimator(BOX1, 16, 3, field("ones"), dev)
    o, d = mixed_rays()
    u = torch.rand(N_RAYS, generator=torch.Generator().manual_seed(1))
    _, _, n_cand = three_modes(est, thin_model(dev), o, d, dev, STEP, 100, f"truncated cone {cone}", cone=cone, u=u, eps=0.0)
    assert int(n_cand.max()) == 100 and int((n_cand == 100).sum()) > 50


def ray_bounds():
    """tests/test_occ_cone_gpu.py's recipe: +-inf entries, about one ray in eight with t_max < t_min (no samples)."""
    gen = torch.Generator().manual_seed(3)
    torch.rand(N_RAYS, generator=gen)
    t_min = torch.rand(N_RAYS, generator=gen) * 8.0
    t_max = t_min + torch.rand(N_RAYS, generator=gen) * 8.0 - 1.0
    t_min[::7], t_max[::5], t_min[3::11], t_max[4::13] = -math.inf, math.inf, math.inf, -math.inf
    assert int((t_max < t_min).sum()) > 10
    return t_min, t_max


@pytest.mark.parametrize("cone", [0.0, 0.02])
def test_per_ray_bounds(dev, cone):
    est = estimator(BOX1, 16, 3, field("random"), dev)
    m = thin_model(dev)
    o, d = mixed_rays()
    u = torch.rand(N_RAYS, generator=torch.Generator().manual_seed(1))
    t_min, t_max = ray_bounds()
    ms = est.max_steps(STEP, cone)
    free = three_modes(est, m, o, d, dev, STEP, ms, f"no bounds cone {cone}", cone=cone, u=u, athre=1e-3)
    for lo, hi in ((t_min, t_max), (t_min, None), (None, t_max)):
        t0, _, n_cand = three_modes(est, m, o, d, dev, STEP, ms, f"bounds {lo is not None, hi is not None} cone {cone}",
                                    cone=cone, u=u, t_min=lo, t_max=hi, athre=1e-3)
        assert t0.numel() > 0 and 0 < int(n_cand.sum()) < int(free[2].sum()), "the bounds tighten the march"
        if lo is not None and hi is not None:
            assert int(n_cand[(t_max < t_min).to(dev)].max()) == 0, "an empty range: pure background"


def test_tile_layouts(dev):
    """256-sample tiles (a 256-wide network in single-pass bf16: two sample groups per wave) and the default fp16x3's
    128-sample tiles, with variable-width samples."""
    from fs_nerf_amd.core.models import NeRF
    est = estimator(BOX1, 16, 3, field("random"), dev)
    o, d = mixed_rays()
    u = torch.rand(N_RAYS, generator=torch.Generator().manual_seed(1))
    sd = O.init_nerf_state_dict(2, 256, [], 10, 4, seed=4)
    sd["sigma.weight"] *= 2.0
    sd["sigma.bias"] += 1.0
    wide = NeRF(3, 3, 2, 256, (), precision="bf16", pos_fn={"n_freqs": 10, "log_space": True},
                dir_fn={"n_freqs": 4, "log_space": True})
    wide.load_state_dict(sd)
    wide = wide.to(dev).eval()
    ms = est.max_steps(STEP, 0.01)
    three_modes(est, wide, o, d, dev, STEP, ms, "bf16, 2 x 256", cone=0.01, u=u, athre=1e-3)
    m = TF.make_model(8, 256, 4, dev, gain=2.0, shift=1.0)
    assert m.precision == "fp16x3"
    three_modes(est, m, o, d, dev, STEP, ms, "fp16x3, 8 x 256", cone=0.01, u=u, athre=1e-3)


OPTS = dict(cone_angle=0.02, near_plane=0.5, alpha_thre=1e-3)


def test_render_rays_with_the_switch_on(dev, monkeypatch):
    from fs_nerf_amd.render import rendering as Rm
    m, est, o, d = small_setup(dev, train=False)
    run = lambda **kw: Rm.render_rays(o, d, est, m, white_bkgd=True, render_step_size=STEP, device=dev, sampling_kwargs=OPTS, **kw)
    assert Rm._rays_route(est, m, None, False, True, 256, STEP, OPTS) == "estimator-sampling"
    with torch.no_grad():
        (rgb_u, op_u, dep_u, ex_u), ri_u, tv_u = run()
        monkeypatch.setattr(Rm, "FUSED_OCC_CONE", True)
        assert Rm._rays_route(est, m, None, False, False, 256, STEP, OPTS) == "occ-frame"
        assert Rm._rays_route(est, m, None, False, True, 256, STEP, OPTS) == "occ-extras"
        (rgb_f, op_f, dep_f, _), ri_f, _ = run(want_extras=False)
        (rgb_e, op_e, dep_e, ex_e), ri_e, tv_e = run()
    assert ri_u.numel() > 1000 and float(tv_u.min()) >= 0.5
    assert ri_f is None and torch.equal(rgb_f, rgb_u) and torch.equal(op_f, op_u) and torch.equal(dep_f, dep_u)
    assert torch.equal(ri_e, ri_u) and torch.equal(tv_e, tv_u)
    assert torch.equal(rgb_e, rgb_u) and torch.equal(op_e, op_u) and torch.equal(dep_e, dep_u)
    for k in EXTRAS:
        assert torch.equal(ex_e[k], ex_u[k]), k


def test_training_call_through_the_fused_sampler(dev, monkeypatch):
    from fs_nerf_amd.render import rendering as Rm
    m, est, o, d = small_setup(dev, train=True)
    monkeypatch.setattr(Rm, "FUSED_OCC_SAMPLER_MIN_RAYS", 0)
    outs = []
    for on, route in ((False, "estimator-sampling"), (True, "occ-sampler")):
        monkeypatch.setattr(Rm, "FUSED_OCC_CONE", on)
        assert Rm._rays_route(est, m, None, True, True, 256, STEP, OPTS) == route
        est.generator = torch.Generator(device=dev).manual_seed(21)
        m.zero_grad(set_to_none=True)
        (rgb, _, _, ex), ri, tv = Rm.render_rays(o, d, est, m, train=True, white_bkgd=True, render_step_size=STEP, device=dev,
                                                 sampling_kwargs=OPTS)
        outs.append((ri, tv, rgb))
    (ri_u, tv_u, rgb_u), (ri_f, tv_f, rgb_f) = outs
    assert ri_u.numel() > 1000
    assert torch.equal(ri_f, ri_u) and torch.equal(tv_f, tv_u) and torch.equal(rgb_f.detach(), rgb_u.detach())
    assert rgb_f.requires_grad
    target = torch.rand(256, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    torch.nn.functional.mse_loss(rgb_f, target).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert any(float(p.grad.abs().max()) > 0 for p in m.parameters())


def test_bf16_cull_takes_the_options_through_its_sampler(dev, monkeypatch):
    """`NeRF.cull_precision = "bf16"` with the switch on: the sampler launch runs on the single-pass blob with the cone
    angle and the cull thresholds, its samples are the multi-launch sequence's with the density pass in that mode, and
    what render_rays returns is the full pass + integration of exactly those samples in the model's own mode."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.render import rendering as Rm
    est = estimator(BOX1, 16, 3, field("ones"), dev)
    m = TF.make_model(8, 256, 4, dev, gain=2.0, shift=1.0)
    m.cull_precision = "bf16"
    opts = dict(cone_angle=0.01, alpha_thre=1e-3)
    o, d = mixed_rays()
    od, dd = o.to(dev), d.to(dev)
    monkeypatch.setattr(Rm, "FUSED_OCC_CONE", True)
    assert Rm._rays_route(est, m, None, False, True, N_RAYS, STEP, opts) == "occ-sampler"
    with torch.no_grad():
        (rgb, op, dep, ex), ri, tv = Rm.render_rays(o, d, est, m, white_bkgd=True, render_step_size=STEP, device=dev,
                                                    sampling_kwargs=opts)
        ri_h, t0, t1, n_cand = ops.occgrid_march(od, dd, est.aabb, 16, 3, est.bits, 0.0, 1e10, STEP, None,
                                                 est.max_steps(STEP, 0.01), cone_angle=0.01)
        sig = ops.mlp_fwd_rays(m.packed_cull(), od, dd, ri_h, t0, t1, False, m._mask(m.pos_mask, dev),
                               m._mask(m.dir_mask, dev)).reshape(-1)
        keep = ops.packed_visibility(sig, t0, t1, ri_h, N_RAYS, 1e-4, 1e-3)
        ri_h, t0, t1 = ri_h[keep], t0[keep], t1[keep]
        (rgb_h, op_h, dep_h, ex_h), _, tv_h = Rm._render_samples((ri_h, t0, t1), od, dd, m, False, True, False, dev)
    print(f"bf16 cull: {int(n_cand.sum())} marched, {ri_h.numel()} kept by hand, {ri.numel()} by the sampler launch")
    assert 1000 < ri_h.numel() < int(n_cand.sum()), "the cull drops samples"
    assert torch.equal(ri, ri_h) and torch.equal(tv, tv_h)
    assert torch.equal(rgb, rgb_h) and torch.equal(op, op_h) and torch.equal(dep, dep_h)
    for k in EXTRAS:
        assert torch.equal(ex[k], ex_h[k]), k


def test_frame_through_one_launch(dev, monkeypatch):
    from fs_nerf_amd.render import rendering as Rm
    m, est, _, _ = small_setup(dev, train=False)
    pose, hwf = O.pose_from_spherical(4.0311289, 50.0, 123.0), (30, 41, 50.0)
    assert Rm._frame_route(est, m, None, False, False, STEP, OPTS) == "chunked"
    with torch.no_grad():
        rgb_c, dep_c, flagged = Rm._chunked_frame("chunked", hwf, pose, 512, est, m, None, False, False, False, True, STEP,
                                                  dev, OPTS)
        monkeypatch.setattr(Rm, "FUSED_OCC_CONE", True)
        assert Rm._frame_route(est, m, None, False, False, STEP, OPTS) == "camera-occupancy"
        img, depth = Rm.render_frame(hwf, 2.0, 6.0, pose, 512, est, m, white_bkgd=True, render_step_size=STEP, device=dev,
                                     sampling_kwargs=OPTS)
    assert not flagged and float((rgb_c != 1.0).float().mean()) > 0.05, "part of the frame shows the medium"
    assert torch.equal(img.reshape(-1, 3), rgb_c) and torch.equal(depth.reshape(-1), dep_c.reshape(-1).clamp(2.0, 6.0))


def test_plain_and_extended_entry_points_agree(dev):
    """fsn_render_rays_occgrid and fsn_render_rays_occgrid_ex (cone_angle 0, null pointers) through the C ABI, frame and
    sampler mode, with fsn_occ_gather_samples and fsn_occ_gather_ex behind the latter: the same results."""
    from fs_nerf_amd import _lib as L
    from fs_nerf_amd.ops import _p, _stream
    est = estimator(BOX1, 16, 3, field("random"), dev)
    m = thin_model(dev)
    o, d = mixed_rays()
    od, dd = o.to(dev), d.to(dev)
    u = torch.rand(N_RAYS, generator=torch.Generator().manual_seed(1)).to(dev)
    pm, ms, lib = m.packed(), est.max_steps(STEP), L.lib()
    got = []
    for ex in (False, True):
        a = L.OccRenderArgs()
        a.R, a.rays_o, a.rays_d, a.u = N_RAYS, od.data_ptr(), dd.data_ptr(), u.data_ptr()
        for i in range(6):
            a.aabb[i] = BOX1[i]
        a.res, a.levels, a.bits = 16, 3, est.bits.data_ptr()
        a.near_plane, a.far_plane, a.step, a.max_steps, a.early_stop_eps, a.alpha_thre = 0.0, 1e10, STEP, ms, 1e-4, 1e-3
        a.bkgd[0] = a.bkgd[1] = a.bkgd[2] = 1.0
        out = {k: torch.full((N_RAYS, n), -1.0, device=dev) for k, n in (("colors", 3), ("opacity", 1), ("depth", 1))}
        a.colors, a.opacity, a.depth = (out[k].data_ptr() for k in ("colors", "opacity", "depth"))
        n_cand, n_kept = torch.zeros(N_RAYS, dtype=torch.int32, device=dev), torch.zeros(N_RAYS, dtype=torch.int32, device=dev)
        a.n_cand, a.n_kept = n_cand.data_ptr(), n_kept.data_ptr()
        wc, status = torch.empty(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        a.work_counter, a.status = wc.data_ptr(), status.data_ptr()
        launch = (lambda: lib.fsn_render_rays_occgrid_ex(C.byref(pm.desc), pm.prec, _p(pm.blob), C.byref(a), 0.0, None, None,
                                                          None, _stream())) if ex else \
            (lambda: lib.fsn_render_rays_occgrid(C.byref(pm.desc), pm.prec, _p(pm.blob), C.byref(a), _stream()))
        L.check(launch(), "frame mode")
        slots = torch.full((N_RAYS, ms), -1.0, device=dev)
        a.sample_t0, a.sample_cap = slots.data_ptr(), ms
        s_kept = torch.zeros(N_RAYS, dtype=torch.int32, device=dev)
        a.n_kept = s_kept.data_ptr()
        L.check(launch(), "sampler mode")
        incl = torch.cumsum(s_kept, 0, dtype=torch.int64)
        n, offs = int(incl[-1]), (incl - s_kept).contiguous()
        ri = torch.full((n,), -1, dtype=torch.int64, device=dev)
        ts, te = torch.full((n,), -1.0, device=dev), torch.full((n,), -1.0, device=dev)
        if ex:
            L.check(lib.fsn_occ_gather_ex(_p(s_kept), _p(offs), _p(slots), None, ms, N_RAYS, STEP, _p(ri), _p(ts), _p(te), None,
                                          None, _stream()), "gather")
        else:
            L.check(lib.fsn_occ_gather_samples(_p(s_kept), _p(offs), _p(slots), ms, N_RAYS, STEP, _p(ri), _p(ts), _p(te),
                                               _stream()), "gather")
        torch.cuda.synchronize()
        got.append((out["colors"], out["opacity"], out["depth"], n_cand, n_kept, s_kept, ri, ts, te))
    assert int(got[0][4].sum()) > 1000 and torch.equal(got[0][4], got[0][5])
    assert all(torch.equal(p, q) for p, q in zip(*got))
    assert torch.equal(got[0][8], got[0][7] + STEP)


def test_lds_indices_stay_inside_with_cone_and_bounds():
    """The debug library (every FSN_AT / FSN_SPAN of k_render_occ range-checked, the candidates' ends included - they
    share storage with the kept samples' densities): the carry case and a bounds case through all three modes in a child
    process; the record must stay empty.  (tests/test_debug_build.py holds the negative control.)"""
    rep = debug_lib.run_worker("occ_cone_debug_worker.py")
    got = rep["render"] + rep["occ"]
    assert got == [0] * 8, f"k_render_occ indexed outside an LDS array: {got} (count, line, index, extent)"
    debug_lib.assert_no_other_unit_recorded(rep)
    assert rep["carried"] >= 2
