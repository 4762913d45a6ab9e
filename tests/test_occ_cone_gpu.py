"""GPU: the occupancy march with per-ray bounds and cone-angle steps (fsn_occgrid_march_ex), fsn_ray_aabb_intersect and
the `sampling_kwargs` of the product path.  The kernels are compared with the float32 NumPy restatement of
tests/occ_cone_ref.py bit for bit (the definition: include/fsnerf_hip.h); the grids are small, because the arithmetic
that can go wrong - block boundaries, the wave-uniform exit, clipping, zero direction components, the level lookup - does
not depend on their size; one case runs the reference's real configuration (128^3, four levels)."""
import functools
import math

import pytest
import torch

from oracle import fsnerf_oracle as O

import occ_cone_ref as CR
import test_occ_fused as TF
from test_occgrid import _orbit_rays, _sphere_binaries

pytestmark = pytest.mark.gpu
BOX1 = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
STEP = 0.02
N_RAYS = 256
MISS = slice(200, 254)  # mixed_rays: the rays that look away from the grid


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import fs_nerf_amd  # noqa: F401
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def mixed_rays():
    """256 rays: 120 with the origin inside the outermost box (+-4) of the three-level grid over +-1, 80 from radius 10
    (outside every box), 54 of those looking away (misses), one axis-parallel ray with two zero direction components
    and one with its origin inside the region of interest."""
    far = 10.0 / 4.0311289
    o1, d1 = _orbit_rays(120, 2)
    o2, d2 = _orbit_rays(80, 3)
    o3, d3 = _orbit_rays(54, 4)
    o = torch.cat([o1, o2 * far, o3 * far, torch.tensor([[0.2, -0.3, 6.0], [0.1, 0.2, -0.3]])])
    d = torch.cat([d1, d2, -d3, torch.tensor([[0.0, 0.0, -1.0], [0.4364, -0.8729, 0.2182]])])
    assert o.shape[0] == N_RAYS and float(o1.abs().max()) < 4.0 and float((o2 * far).abs().max()) > 4.0
    return o.contiguous(), d.contiguous()


@functools.lru_cache(maxsize=None)
def field(kind):
    if kind == "random":
        return torch.rand(3, 16, 16, 16, generator=torch.Generator().manual_seed(11)) < 0.3
    return torch.ones(3, 16, 16, 16, dtype=torch.bool) if kind == "ones" else torch.zeros(3, 16, 16, 16, dtype=torch.bool)


def estimator(aabb, res, levels, bins, dev):
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    est = OccGridEstimator(aabb, res, levels).to(dev)
    est.set_binaries(bins)
    return est


def same(got, want):
    return all(g.dtype == w.dtype and torch.equal(g.cpu(), w) for g, w in zip(got, want))


@pytest.mark.parametrize("cone", [0.0, 0.01, 0.05])
@pytest.mark.parametrize("kind", ["random", "ones", "zeros"])
def test_march_matches_the_restatement(dev, kind, cone):
    bins = field(kind)
    est = estimator(BOX1, 16, 3, bins, dev)
    o, d = mixed_rays()
    u = torch.rand(N_RAYS, generator=torch.Generator().manual_seed(1))
    for uu in (None, u):
        for near in (0.0, 0.7):
            got = est.sampling(o.to(dev), d.to(dev), render_step_size=STEP, near_plane=near, far_plane=1e10,
                               cone_angle=cone, u=None if uu is None else uu.to(dev))
            ms = est.max_steps(STEP, cone, near)
            want = CR.march(o, d, BOX1, 16, 3, bins, near, 1e10, STEP, uu, ms, cone_angle=cone)
            assert got[0].numel() == want[0].numel() and same(got, want), (kind, cone, uu is not None, near)
            n = torch.bincount(want[0], minlength=N_RAYS)
            assert int(n[MISS].max()) == 0
            if kind == "ones" and near == 0.0:
                # a full grid keeps every lattice point (the other fields and the later near plane march the same
                # lattice, with fewer points kept): several blocks of 64 and the exit test behind them
                assert int(n.max()) > 128, int(n.max())
            if kind == "zeros":
                assert want[0].numel() == 0
            elif near == 0.0:
                assert int(n[254]) > 0 and int(n[255]) > 0 and int((n[:120] > 0).sum()) == 120


def test_plain_and_extended_entry_points_agree(dev):
    """fsn_occgrid_march and fsn_occgrid_march_ex (null bounds, cone 0) called through the C ABI, count and fill pass:
    the same samples, and those of the restatement."""
    import ctypes as C
    from fs_nerf_amd import _lib
    from fs_nerf_amd.ops import _p, _stream
    bins = field("random")
    est = estimator(BOX1, 16, 3, bins, dev)
    o, d = mixed_rays()
    od, dd = o.to(dev), d.to(dev)
    ms = est.max_steps(STEP)
    ab = (C.c_float * 6)(*BOX1)
    lib = _lib.lib()
    for uu in (None, torch.rand(N_RAYS, generator=torch.Generator().manual_seed(1))):
        ud = None if uu is None else uu.to(dev)
        head = (_p(od), _p(dd), N_RAYS, ab, 16, 3, _p(est.bits), 0.0, 1e10, STEP, _p(ud), ms)
        got = []
        for fn, extra in ((lib.fsn_occgrid_march, ()), (lib.fsn_occgrid_march_ex, (None, None, 0.0))):
            counts = torch.zeros(N_RAYS, device=dev, dtype=torch.int64)
            _lib.check(fn(*head, *extra, _p(counts), None, None, None, None, _stream()), "count pass")
            offsets = (torch.cumsum(counts, 0) - counts).contiguous()
            n = int(counts.sum())
            ri = torch.full((n,), -1, device=dev, dtype=torch.int64)
            t0, t1 = torch.full((n,), -1.0, device=dev), torch.full((n,), -1.0, device=dev)
            _lib.check(fn(*head, *extra, None, _p(offsets), _p(ri), _p(t0), _p(t1), _stream()), "fill pass")
            got.append((counts, ri, t0, t1))
        want = CR.march(o, d, BOX1, 16, 3, bins, 0.0, 1e10, STEP, uu, ms, cone_angle=0.0)
        assert want[0].numel() > 1000
        assert all(torch.equal(a, b) for a, b in zip(*got)), uu is not None
        assert torch.equal(got[0][0].cpu(), torch.bincount(want[0], minlength=N_RAYS)) and same(got[0][1:], want)


def test_march_real_configuration(dev):
    """run-nerf.py:92-98: 128^3, four levels over +-1.5, step 5e-3, with nerfacc's cone angle for unbounded scenes."""
    aabb = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
    bins = _sphere_binaries(128, 4)
    est = estimator(aabb, 128, 4, bins, dev)
    o, d = _orbit_rays(64, 5)
    u = torch.rand(64, generator=torch.Generator().manual_seed(2))
    ms = est.max_steps(5e-3, 0.004)
    assert ms <= 1280 + 64
    got = est.sampling(o.to(dev), d.to(dev), render_step_size=5e-3, cone_angle=0.004, u=u.to(dev))
    want = CR.march(o, d, aabb, 128, 4, bins, 0.0, 1e10, 5e-3, u, ms, cone_angle=0.004)
    assert want[0].numel() > 2000 and same(got, want)


@pytest.mark.parametrize("cone", [0.0, 0.01])
def test_per_ray_bounds(dev, cone):
    from fs_nerf_amd.render.occgrid import ray_aabb_intersect
    bins = field("random")
    est = estimator(BOX1, 16, 3, bins, dev)
    o, d = mixed_rays()
    gen = torch.Generator().manual_seed(3)
    u = torch.rand(N_RAYS, generator=gen)
    t_min = torch.rand(N_RAYS, generator=gen) * 8.0
    t_max = t_min + torch.rand(N_RAYS, generator=gen) * 8.0 - 1.0  # about one in eight: t_max < t_min
    t_min[::7], t_max[::5], t_min[3::11], t_max[4::13] = -math.inf, math.inf, math.inf, -math.inf
    assert int((t_max < t_min).sum()) > 10
    ms = est.max_steps(STEP, cone)
    for uu in (None, u):
        ud = None if uu is None else uu.to(dev)
        free = est.sampling(o.to(dev), d.to(dev), render_step_size=STEP, cone_angle=cone, u=ud)
        for lo, hi in ((t_min, t_max), (t_min, None), (None, t_max)):
            got = est.sampling(o.to(dev), d.to(dev), render_step_size=STEP, cone_angle=cone, u=ud,
                               t_min=None if lo is None else lo.to(dev), t_max=None if hi is None else hi.to(dev))
            want = CR.march(o, d, BOX1, 16, 3, bins, 0.0, 1e10, STEP, uu, ms, t_min=lo, t_max=hi, cone_angle=cone)
            assert 0 < want[0].numel() < free[0].numel() and same(got, want)
        # the outermost box's own range tightens nothing
        outer = [v for v in est.level_aabb(2)[0] + est.level_aabb(2)[1]]
        t0, t1, hit = ray_aabb_intersect(o.to(dev), d.to(dev), torch.tensor([outer]))
        assert bool(hit[:120].all())
        got = est.sampling(o.to(dev), d.to(dev), render_step_size=STEP, cone_angle=cone, u=ud, t_min=t0[:, 0], t_max=t1[:, 0])
        assert all(torch.equal(g, f) for g, f in zip(got, free))


def test_ray_aabb_intersect_matches_the_restatement(dev):
    from fs_nerf_amd.render.occgrid import ray_aabb_intersect
    o, d = mixed_rays()
    o2, d2 = _orbit_rays(44, 9)
    o, d = torch.cat([o, o2]).clone(), torch.cat([d, d2]).clone()
    d[10:40:3, 0] = 0.0  # zero direction components, origin inside / outside the slab
    d[11:40:3, 1] = 0.0
    o[10:25, 0] = 0.5
    boxes = torch.tensor([BOX1, [-4.0, -4.0, -4.0, 4.0, 4.0, 4.0], [0.25, -0.5, -2.0, 1.5, 0.75, 0.5]])
    assert o.shape[0] == 300
    for kw in ({}, dict(near_plane=0.5, far_plane=6.0), dict(near_plane=3.0, far_plane=9.0, miss_value=-1.0)):
        got = ray_aabb_intersect(o.to(dev), d.to(dev), boxes, **kw)
        want = CR.ray_aabb_intersect(o, d, boxes, **kw)
        assert got[0].shape == (300, 3) and got[2].dtype == torch.bool and same(got, want), kw
        frac = float(want[2].float().mean())
        assert 0.1 < frac < 0.9, "hits and misses"
    assert float(want[0][~want[2]].max()) == -1.0


def test_cone_samples_are_contiguous_through_the_compositor(dev):
    """A full grid and a constant density: the intervals of a ray tile [first t_start, last t_end) without gaps, so its
    opacity is 1 - exp(-sigma (last t_end - first t_start)) - to 1e-5 of the transmittance 1 - opacity (float32
    accumulation over at most a few hundred terms, the bound tests/test_composite_grad_gpu.py uses for such sums)."""
    from fs_nerf_amd.render import rendering as Rm
    est = estimator(BOX1, 16, 3, field("ones"), dev)
    o, d = mixed_rays()
    sigma = 0.1
    ri, t0, t1 = est.sampling(o.to(dev), d.to(dev), render_step_size=STEP, cone_angle=0.01)
    n = torch.bincount(ri, minlength=N_RAYS)
    assert 128 < int(n.max()) < 1000
    fn = lambda a, b, c: (torch.full((a.numel(), 3), 0.5, device=dev), torch.full_like(a, sigma))
    with torch.no_grad():
        _, opacity, _, _ = Rm.rendering(t0, t1, ri, N_RAYS, fn)
    first = torch.full((N_RAYS,), math.inf, device=dev, dtype=torch.float64).scatter_reduce(0, ri, t0.double(), "amin")
    last = torch.full((N_RAYS,), -math.inf, device=dev, dtype=torch.float64).scatter_reduce(0, ri, t1.double(), "amax")
    has = n > 0
    trans = torch.exp(-sigma * (last - first)[has])
    err = ((opacity.reshape(-1).double()[has] - (1.0 - trans)).abs() / trans).max()
    print(f"contiguity: max |opacity - expected| / (1 - opacity) = {float(err):.3e} over {int(has.sum())} rays")
    assert float(trans.min()) > 0.2 and float(err) <= 1e-5, float(err)
    assert float(opacity.reshape(-1)[~has].abs().max()) == 0.0


def small_setup(dev, train):
    from fs_nerf_amd.core.models import NeRF
    sd = O.init_nerf_state_dict(4, 128, [], 10, 4, seed=4)
    sd["sigma.weight"] *= 16.0
    sd["sigma.bias"] += 1.0
    m = NeRF(3, 3, 4, 128, (), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
    m.load_state_dict(sd)
    m = m.to(dev).train(train)
    est = estimator(TF.AABB, 16, 2, _sphere_binaries(16, 2), dev).train(train)
    o, d = _orbit_rays(256, 7)
    return m, est, o, d


def test_render_rays_with_sampling_kwargs_is_the_public_pieces(dev):
    from fs_nerf_amd.core.loss import DistortionLoss
    from fs_nerf_amd.render import rendering as Rm
    m, est, o, d = small_setup(dev, train=True)
    od, dd = o.to(dev), d.to(dev)
    opts = dict(cone_angle=0.02, near_plane=0.5, alpha_thre=1e-3)
    est.generator = torch.Generator(device=dev).manual_seed(21)
    (rgb, opacity, depth, ex), ri, tv = Rm.render_rays(o, d, est, m, train=True, white_bkgd=True, render_step_size=STEP,
                                                       device=dev, sampling_kwargs=opts)
    # by hand: estimator.sampling -> forward_rays(full=True) -> rendering
    est.generator = torch.Generator(device=dev).manual_seed(21)
    sigma_fn = lambda a, b, c: m.forward_rays(od, dd, c, a, b, full=False).squeeze(-1)
    ri_h, t0_h, t1_h = est.sampling(od, dd, sigma_fn=sigma_fn, render_step_size=STEP, stratified=True, **opts)

    def rgb_sigma_fn(a, b, c):
        out = m.forward_rays(od, dd, c, a, b, full=True)
        return out[..., :3], out[..., -1]

    rgb_h, op_h, dep_h, _ = Rm.rendering(t0_h, t1_h, ri_h, 256, rgb_sigma_fn, torch.full((3,), 1.0))
    assert ri.numel() > 1000 and float(t0_h.min()) >= 0.5
    widths = t1_h - t0_h
    assert float(widths.max()) > 1.5 * float(widths.min()), "variable-width samples"
    assert torch.equal(ri, ri_h) and torch.equal(tv, (t0_h + t1_h) / 2.0)
    assert torch.equal(rgb, rgb_h) and torch.equal(opacity, op_h) and torch.equal(depth, dep_h)
    assert rgb.requires_grad
    torch.nn.functional.mse_loss(rgb, torch.rand(256, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(1))).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert any(float(p.grad.abs().max()) > 0 for p in m.parameters())
    # every output differentiable + the distortion loss on the variable-width intervals
    m.zero_grad(set_to_none=True)
    est.generator = torch.Generator(device=dev).manual_seed(21)
    (rgb, opacity, depth, ex), ri, tv = Rm.render_rays(o, d, est, m, train=True, white_bkgd=True, render_step_size=STEP,
                                                       device=dev, full_grad=True, sampling_kwargs=opts)
    assert torch.equal(ex["t_starts"], t0_h) and torch.equal(ex["t_ends"], t1_h)
    dist = DistortionLoss()(ex["weights"], ex["t_starts"], ex["t_ends"], ri, 256)
    assert bool(torch.isfinite(dist)) and float(dist.detach()) > 0
    (rgb.square().mean() + depth.mean() + dist).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_scalar_options_on_the_fused_routes(dev):
    """near_plane / far_plane / alpha_thre are arguments of the fused occupancy kernels: the one-launch routes stay and
    still equal the unfused sequence bit for bit (tests/test_occ_fused.py's claim for the defaults)."""
    from fs_nerf_amd.render import rendering as Rm
    from fs_nerf_amd.utils import utilities as U
    m, est, o, d = small_setup(dev, train=False)
    opts = dict(near_plane=3.0, far_plane=5.0, alpha_thre=1e-3)
    run = lambda **kw: Rm.render_rays(o, d, est, m, white_bkgd=True, render_step_size=STEP, device=dev,
                                      sampling_kwargs=opts, **kw)
    assert Rm._rays_route(est, m, None, False, False, 256, STEP, opts) == "occ-frame"
    assert Rm._rays_route(est, m, None, False, True, 256, STEP, opts) == "occ-extras"
    with torch.no_grad():
        (rgb_u, op_u, dep_u, ex_u), ri_u, tv_u = TF.unfused(run)
        (rgb_d, _, _, _), ri_d, _ = TF.unfused(lambda: Rm.render_rays(o, d, est, m, white_bkgd=True, render_step_size=STEP,
                                                                      device=dev))
        (rgb_f, op_f, dep_f, _), ri_f, _ = run(want_extras=False)
        (rgb_e, op_e, dep_e, ex_e), ri_e, tv_e = run()
    assert 0 < ri_u.numel() < ri_d.numel() and float(tv_u.min()) >= 3.0 and float(tv_u.max()) < 5.0 + STEP
    assert not torch.equal(rgb_u, rgb_d), "the options reach the kernels"
    assert ri_f is None and torch.equal(rgb_f, rgb_u) and torch.equal(op_f, op_u) and torch.equal(dep_f, dep_u)
    assert torch.equal(ri_e, ri_u) and torch.equal(tv_e, tv_u)
    assert torch.equal(rgb_e, rgb_u) and torch.equal(op_e, op_u) and torch.equal(dep_e, dep_u)
    for k in ("weights", "alphas", "trans", "sigmas", "rgbs"):
        assert torch.equal(ex_e[k], ex_u[k]), k
    # the frame: one launch with the rays generated in it == the chunked frame
    pose, hwf = O.pose_from_spherical(4.0311289, 50.0, 123.0), (30, 41, 50.0)
    assert Rm._frame_route(est, m, None, False, False, STEP, opts) == "camera-occupancy"
    with torch.no_grad():
        img, depth = Rm.render_frame(hwf, 2.0, 6.0, pose, 512, est, m, white_bkgd=True, render_step_size=STEP, device=dev,
                                     sampling_kwargs=opts)
        rgb_c, dep_c, flagged = Rm._chunked_frame("chunked", hwf, pose, 512, est, m, None, False, False, False, True, STEP,
                                                  dev, opts)
    assert not flagged and torch.equal(img.reshape(-1, 3), rgb_c) and torch.equal(depth.reshape(-1), dep_c.reshape(-1).clamp(2.0, 6.0))
