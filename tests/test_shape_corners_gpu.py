"""The corners of the network-shape envelope on the GPU.  build_geom (csrc/mlp_layout.hpp) accepts d_hidden in
{128, 256}, 2..16 layers, any skip set below n_layers - 1, 0..10 position and 0..4 direction frequency bands, and
models.NeRF sends all of it to the same kernels; the rest of the suite runs 4x128, 8x256 with skip (4,) and 6x128 with
skips (1, 3).  Five networks at the corners (tests/wstream_ref.py, CORNERS):

  min         2 x 128, no skip        fewest phases: 3 in the single-pass modes (the tile length WStream::begin_tile
                                      had wrong on the one-launch occupancy routes), 6 in the x3 modes
  bare        2 x 128, skip (0,)      no frequency bands at all: identity slots only
  deep        16 x 128, skips 0..14   kMaxLayers, every layer fed by the encoding: the longest stream
  wide-skips  8 x 256, skips 0..6     the largest aux area that fits LDS (3392 of 3456 floats)
  wide-min    2 x 256, no skip        the shortest stream with two sample groups per wave

through every route a NeRF takes: point and ray form against the float64 oracle (a), the occupancy refresh (b), the
fused stratified render (c), the one-launch occupancy render and sampler (d), the training pair (e); and the depth
limit of 256-wide networks (f).  Weights: oracle.init_nerf_state_dict(seed=7).

Bars.  x3 modes: tests/test_gpu_parity.py's (rgb atol 1e-5, sigma atol 1e-4 max|sigma|, rtol 1e-4).  Single-pass
modes: 4 x the error of the oracle's own emulation of the mode (operands rounded to 16 bits, float64 sums) against the
unrounded float64 result on the same inputs - the kernel differs from the emulation by float32 accumulation, which
moves a few operands across a rounding boundary by one unit of the format, the size of the errors the emulation
already holds; a stream that delivers the wrong weights is wrong by the size of the output.

Measured on the MI355X.  (a), largest over the four launches of a model, rgb absolute / sigma over max|sigma|:

  net          fp16x3              bf16x3              fp16                bf16
  min          1.7e-7 / 1.5e-5     3.1e-7 / 2.1e-5     2.1e-5 / 5.6e-4     1.7e-4 / 3.4e-3
  bare         6.0e-8 / 5.2e-7     2.4e-7 / 1.4e-5     1.6e-5 / 6.9e-4     1.2e-4 / 6.2e-3
  deep         2.5e-7 / 1.8e-5     3.5e-7 / 2.1e-5     1.7e-5 / 4.5e-4     1.3e-4 / 3.8e-3
  wide-skips   2.0e-7 / 1.3e-5     2.7e-7 / 1.2e-5     1.1e-5 / 3.0e-4     1.0e-4 / 2.8e-3
  wide-min     2.5e-7 / 2.8e-5     3.1e-7 / 2.7e-5     1.3e-5 / 6.9e-4     1.1e-4 / 6.4e-3

The x3 modes' sigma figures are mostly the float32 rounding of the ray form's midpoints under the 2^9 frequency band
(the point form measures 2.9e-7 .. 5.2e-7 in fp16x3 and 4.0e-6 .. 1.4e-5 in bf16x3). The emulation's own errors on these samples are fp16 rgb 1.0e-5 .. 1.9e-5, sigma 2.7e-4 ..
6.9e-4, bf16 rgb 0.9e-4 .. 1.7e-4, sigma 2.1e-3 .. 6.4e-3: the single-pass kernels measure 1.0 .. 1.2 x the emulation's
error on the same launch (bar: 4 x).  (b) no cell of any grid differs.  (c) fused and generic route agree bit for bit.
(d) fused and unfused agree bit for bit in all four modes of all five networks (13708 candidates, 5374 .. 13162 kept,
the largest batch certainly formed holds 242 candidates).  (e) parameter and input gradients: at most 5.7e-7 (default
mode, bar 2e-4) and 1.9e-5 (bf16x3, bar 1e-3).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import fsnerf_oracle as O
from test_gpu_parity import close
from test_occ_fused import AABB, both_paths, orbit_rays, sphere_grid, unfused
from test_train_step import _rel, _relu_margin
from wstream_ref import CORNERS

pytestmark = pytest.mark.gpu

NETS = ("min", "bare", "deep", "wide-skips", "wide-min")
X3 = ("fp16x3", "bf16x3")
SINGLE = ("fp16", "bf16")
PRECISIONS = X3 + SINGLE
N = 300       # two full 128-sample tiles and a tail (one 256-sample tile and a tail with two groups per wave)
N_RAYS = 7
STEP = 5e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def state(net):
    L, D, skip, nf, nfd = CORNERS[net]
    return O.init_nerf_state_dict(L, D, list(skip), nf, nfd, seed=7)


def cfg(net):
    L, D, skip, nf, nfd = CORNERS[net]
    return dict(n_layers=L, skip=list(skip), n_freqs=nf, n_freqs_dir=nfd, log_space=True)


def make_model(net, dev, precision="fp16x3", sd=None):
    from fs_nerf_amd.core.models import NeRF
    L, D, skip, nf, nfd = CORNERS[net]
    m = NeRF(3, 3, L, D, skip, precision=precision, pos_fn={"n_freqs": nf, "log_space": True},
             dir_fn={"n_freqs": nfd, "log_space": True})
    m.load_state_dict(state(net) if sd is None else sd)
    return m.to(dev).eval()


@functools.lru_cache(maxsize=None)
def host_inputs():
    """The samples of tests/test_tile_groups_gpu.py: 300 points in the box, 300 packed intervals on 7 rays."""
    gen = torch.Generator().manual_seed(20)
    x = torch.rand(N, 3, generator=gen) * 3 - 1.5
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)
    ro = torch.rand(N_RAYS, 3, generator=gen) - 0.5
    rd = torch.nn.functional.normalize(torch.randn(N_RAYS, 3, generator=gen), dim=-1)
    ri = (torch.arange(N) * N_RAYS) // N
    t0 = 0.5 + torch.rand(N, generator=gen) * 2.0
    t1 = t0 + 0.01 + torch.rand(N, generator=gen) * 0.05
    return dict(x=x, d=d, ro=ro, rd=rd, ri=ri, t0=t0, t1=t1)


@functools.lru_cache(maxsize=None)
def reference(net):
    """float64 oracle on both forms' inputs (the ray form's midpoints formed in float64), and per single-pass mode the
    emulation's own error against it: {form: (want [N,4], {mode: (err rgb, err sigma / max|sigma|)})}."""
    i = {k: (v.double() if v.is_floating_point() else v) for k, v in host_inputs().items()}
    sd = {k: v.double() for k, v in state(net).items()}
    forms = {"point": (i["x"], i["d"]),
             "rays": (i["ro"][i["ri"]] + i["rd"][i["ri"]] * (i["t0"] + i["t1"])[:, None] / 2.0, i["rd"][i["ri"]])}
    out = {}
    for form, (x, d) in forms.items():
        want = O.nerf_forward(sd, x, d, **cfg(net))
        smax = float(want[:, 3].abs().max())
        emu = {}
        for mode in SINGLE:
            e = O.nerf_forward(sd, x, d, emulate=mode, **cfg(net))
            emu[mode] = (float((e[:, :3] - want[:, :3]).abs().max()), float((e[:, 3] - want[:, 3]).abs().max()) / smax)
        out[form] = (want, emu)
    return out


@pytest.fixture(scope="module")
def inputs(dev):
    return {k: v.to(dev) for k, v in host_inputs().items()}


@pytest.fixture(scope="module")
def models(dev, inputs):
    """(network, precision) -> (model, its outputs on the 300 samples: point and ray form, full and density only),
    computed once per module.  The first launch calibrates the scaled fp16x3 network on the whole input.  No mode has a
    reason to leave its precision: every layer's largest activation lies in 0.29 .. 2.3 (float64, these samples)."""
    cache = {}

    def get(net, prec):
        if (net, prec) not in cache:
            m = make_model(net, dev, prec)
            i = inputs
            out = {}
            with torch.no_grad():
                for key, launch in ((("point", True), lambda: m(i["x"], i["d"])), (("point", False), lambda: m(i["x"])),
                                    (("rays", True), lambda: m.forward_rays(i["ro"], i["rd"], i["ri"], i["t0"], i["t1"], True)),
                                    (("rays", False), lambda: m.forward_rays(i["ro"], i["rd"], i["ri"], i["t0"], i["t1"], False))):
                    out[key] = launch()
                    assert m.precision == prec, f"{net} {prec} {key}: the model left its precision"
            for k, v in out.items():
                assert v.shape == (N, 4 if k[1] else 1) and bool(torch.isfinite(v).all()), (net, prec, k)
            cache[(net, prec)] = (m, out)
        return cache[(net, prec)]

    yield get
    cache.clear()


# ------------------------------------------------------------------------------------------- a. point form and ray form
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("net", NETS)
def test_point_and_ray_form_against_float64(models, net, prec):
    m, out = models(net, prec)
    ref = reference(net)
    worst = [0.0, 0.0]
    fails = []
    for (form, full), y in out.items():
        want, emu = ref[form]
        y = y.cpu().double()
        smax = float(want[:, 3].abs().max())
        e_sigma = float((y[:, -1] - want[:, 3]).abs().max()) / smax
        e_rgb = float((y[:, :3] - want[:, :3]).abs().max()) if full else 0.0
        worst = [max(worst[0], e_rgb), max(worst[1], e_sigma)]
        if prec in X3:
            print(f"{net} {prec} {form} {'full' if full else 'density'}: rgb {e_rgb:.2e} (atol 1e-5), "
                  f"sigma/max {e_sigma:.2e} (atol 1e-4)")
            try:
                if full:
                    close(y[:, :3], want[:, :3], atol=1e-5, what=f"{net} {prec} {form} rgb")
                close(y[:, -1], want[:, 3], atol=1e-4 * smax, what=f"{net} {prec} {form} sigma")
            except AssertionError as e:
                fails.append(str(e))
        else:
            b_rgb, b_sigma = 4.0 * emu[prec][0], 4.0 * emu[prec][1]
            print(f"{net} {prec} {form} {'full' if full else 'density'}: rgb {e_rgb:.2e} (bar {b_rgb:.2e}), "
                  f"sigma/max {e_sigma:.2e} (bar {b_sigma:.2e})")
            if e_rgb > b_rgb or e_sigma > b_sigma:
                fails.append(f"{net} {prec} {form} full={full}: rgb {e_rgb:.3e} > {b_rgb:.3e} or sigma {e_sigma:.3e} > {b_sigma:.3e}")
    print(f"FIGURE a {net} {prec}: rgb {worst[0]:.2e} sigma {worst[1]:.2e}")
    assert not fails, fails
    assert m.precision == prec


# ------------------------------------------------------------------------------------------- b. occupancy refresh
@pytest.mark.parametrize("prec", ["fp16x3", "bf16"])
@pytest.mark.parametrize("net", NETS)
def test_refresh_uses_the_standalone_densities(dev, models, net, prec):
    """One warm-up refresh of a 16^3 one-level grid from zero: every cell once, occs = max(0, sigma * step).  bf16: the
    fused refresh launch (csrc/occ_refresh.hip, NeRF.occ_eval_fn); fp16x3: a closure over the model.  Either way the
    grid holds, bit for bit, the density-only forward of (a)'s model at the refresh's own points."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    m, _ = models(net, prec)
    res = 16
    est = OccGridEstimator(AABB, res, 1).to(dev).train()
    est.generator = torch.Generator().manual_seed(5)
    cells, x = ops.occgrid_select(est.bits, est.aabb, res, 1, 0, True, res ** 3 // 4, res ** 3 // 4, est.update_seed(0))
    assert torch.equal(cells.sort().values, torch.arange(res ** 3, device=dev))
    with torch.no_grad():
        # (odd split: the standalone forward sees the points in other tiles and lanes than the refresh does)
        sigma = torch.cat([m(x[:1001]), m(x[1001:])]).reshape(-1)
    want = torch.zeros(res ** 3, device=dev)
    want[cells] = torch.clamp(sigma * STEP, min=0.0)
    fn = m.occ_eval_fn(STEP, "bf16") if prec == "bf16" else (lambda p: m(p) * STEP)
    est.update_every_n_steps(0, fn, occ_thre=1e-2)
    n_diff = int((est.occs != want).sum())
    print(f"{net} {prec}: {int((want > 0).sum())} of {res ** 3} cells with positive density, {n_diff} differ")
    assert 0 < int((want > 0).sum()), "the refresh saw positive densities"
    assert torch.equal(est.occs, want), f"{n_diff} cells differ, max {float((est.occs - want).abs().max()):.3e}"
    assert m.precision == prec and (prec != "bf16" or fn.precision == "bf16")


# ------------------------------------------------------------------------------------------- c. fused stratified render
@pytest.mark.parametrize("net", NETS)
def test_fused_stratified_render_matches_the_generic_route(dev, net):
    """tests/test_gpu_parity.py::test_render_rays_generic_model_matches_fused on the corner networks: the fused launch
    (csrc/render.hip, coarse = fine = the network) against the same call with a plain callable in the model slot."""
    from fs_nerf_amd.render import rendering as Rm
    from test_gpu_parity import _rays
    sd = dict(state(net))
    sd["sigma.weight"] = sd["sigma.weight"] * 64.0
    sd["sigma.bias"] = sd["sigma.bias"] + 3.0
    m = make_model(net, dev, sd=sd)

    class Wrapped(torch.nn.Module):  # not a fs_nerf_amd NeRF -> generic path
        def forward(self, x, dirs=None):
            return m(x, dirs)

    R, S, NI = 130, 16, 16
    o, d, gen = _rays(R, 3)
    u, uf = torch.rand(R, generator=gen).to(dev), torch.rand(R, NI, generator=gen).to(dev)
    est = Rm.StratifiedEstimator(2.0, 6.0, S, NI)
    with torch.no_grad():
        a = Rm.render_rays(o, d, est, m, device=dev, u=u, u_fine=uf)
        b = Rm.render_rays(o, d, est, Wrapped().eval(), device=dev, u=u, u_fine=uf)
    print(f"{net}: fused vs generic rgb {float((a[0][0] - b[0][0]).abs().max()):.2e} depth "
          f"{float((a[0][2] - b[0][2]).abs().max()):.2e} t_vals {float((a[2] - b[2]).abs().max()):.2e}; "
          f"opacity up to {float(a[0][1].max()):.3f}")
    assert m.precision == "fp16x3" and float(a[0][1].max()) > 0.5, "the rays hit a medium"
    close(a[0][0], b[0][0], atol=1e-5, what="rgb fused vs generic")
    close(a[0][2], b[0][2], atol=1e-4, what="depth fused vs generic")
    close(a[2], b[2], rtol=1e-5, atol=1e-5, what="t_vals fused vs generic")
    assert torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------- d. one-launch occupancy render
OCC_STEP = 2e-2
OCC_TOL = {"bf16": 2e-3, "fp16": 3e-4}  # tests/test_occ_fused.py: single-pass fused against unfused


def occ_model(net, dev, prec):
    sd = dict(state(net))
    sd["sigma.weight"] = sd["sigma.weight"] * 64.0
    sd["sigma.bias"] = sd["sigma.bias"] + 3.0
    return make_model(net, dev, prec, sd)


def first_batches(n_cand, cus):
    """Candidates of the batches the launch certainly formed.  A workgroup pulls take = remaining / (2 x workgroups)
    rays (at most 8), looking at the queue before it advances it, and fewer than 8 rays are a batch of their own
    (csrc/render_occ.hip).  While the queue's head is below R - take0 x 2 x workgroups every look gives take0 =
    R / (2 x workgroups), whichever workgroup pulls: the batches are the runs of take0 rays from ray 0 on."""
    R = n_cand.numel()
    grid = min((R + 7) // 8, cus)
    take0 = min(max(R // (2 * grid), 1), 8)
    assert take0 < 8, "these launches hand out fewer than 8 rays per pull"
    last = R - take0 * 2 * grid  # a pull that starts at or below `last` has seen at most `last`: take0 rays
    c = n_cand.cpu().long()
    return [int(c[b:b + take0].sum()) for b in range(0, last + 1, take0)]


@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("net", NETS)
def test_one_launch_occupancy_render_is_the_unfused_sequence(dev, net, prec):
    """tests/test_occ_fused.py's scene: the fused launch (density tiles, cull, full tiles of one blob in a data-dependent
    order: WStream::begin_tile) against march -> density pass -> visibility -> full pass -> integration as separate
    launches.  `min` in bf16 / fp16 has 3-phase density tiles: the case begin_tile wraps at once for."""
    from fs_nerf_amd import _lib, ops
    m = occ_model(net, dev, prec)
    est = sphere_grid(32, 1, dev)
    o, d = orbit_rays(700, 5)
    (rgb_u, op_u, dep_u, ri), (rgb_f, op_f, dep_f) = both_paths(o, d, est, m, dev, OCC_STEP)
    _, _, _, cnt = ops.render_occ_fused(m.packed(), o.to(dev), d.to(dev), aabb=est.aabb, res=est.resolution, levels=est.levels,
                                        bits=est.bits, near_plane=0.0, far_plane=1e10, step=OCC_STEP,
                                        max_steps=est.max_steps(OCC_STEP), bkgd=(1.0, 1.0, 1.0), want_counts=True)
    n_cand, n_kept = int(cnt["n_cand"].sum()), int(cnt["n_kept"].sum())
    batches = first_batches(cnt["n_cand"], _lib.lib().fsn_device_cus())
    e_rgb, e_op, e_dep = (float((a - b).abs().max()) for a, b in ((rgb_f, rgb_u), (op_f, op_u), (dep_f, dep_u)))
    print(f"FIGURE d {net} {prec}: fused vs unfused rgb {e_rgb:.2e} opacity {e_op:.2e} depth {e_dep:.2e}; candidates {n_cand}, "
          f"kept {n_kept}, largest of the first {len(batches)} batches {max(batches)} candidates")
    assert m.precision == prec
    assert n_cand > n_kept > 0, "density tiles ran, the cull dropped samples and some survived"
    assert max(batches) > 128, "a batch with two density tiles in a row"
    if prec in X3:
        assert torch.equal(cnt["n_kept"].long(), torch.bincount(ri, minlength=o.shape[0]))
        assert torch.equal(rgb_f, rgb_u) and torch.equal(op_f, op_u) and torch.equal(dep_f, dep_u)
    else:
        assert e_rgb <= OCC_TOL[prec] and e_op <= OCC_TOL[prec]


@pytest.mark.parametrize("prec", ["bf16", "fp16x3"])
def test_one_launch_occupancy_sampler_of_the_smallest_network(dev, prec):
    """The sampler mode of the launch (density tiles only: in bf16 every tile of `min` has 3 phases) against
    OccGridEstimator.sampling with the standalone density pass: same kept samples; then through render_rays, where a
    training call of any size takes the fused sampler once FUSED_OCC_SAMPLER_MIN_RAYS is 0."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.render import rendering as Rm
    m = occ_model("min", dev, prec)
    est = sphere_grid(32, 1, dev)
    o, d = orbit_rays(700, 5)
    od, dd = o.to(dev), d.to(dev)
    with torch.no_grad():
        ri_u, ts_u, te_u = est.sampling(od, dd, sigma_fn=lambda a, b, c: m.forward_rays(od, dd, c, a, b, full=False).squeeze(-1),
                                        render_step_size=OCC_STEP)
        ri_f, ts_f, te_f = ops.occ_sample_fused(m.packed(), od, dd, aabb=est.aabb, res=est.resolution, levels=est.levels,
                                                bits=est.bits, near_plane=0.0, far_plane=1e10, step=OCC_STEP,
                                                max_steps=est.max_steps(OCC_STEP))
    print(f"min {prec}: {ri_u.numel()} samples kept by the unfused sampling, {ri_f.numel()} by the fused sampler")
    assert ri_u.numel() > 500
    assert torch.equal(ri_f, ri_u)
    assert torch.equal(ts_f, ts_u) and torch.equal(te_f, te_u)
    m.train()
    est.train()
    outs = []
    keep = (Rm.FUSED_OCC_SAMPLER, Rm.FUSED_OCC_SAMPLER_MIN_RAYS)
    try:
        Rm.FUSED_OCC_SAMPLER_MIN_RAYS = 0
        for flag in (True, False):
            Rm.FUSED_OCC_SAMPLER = flag
            est.generator = torch.Generator(device=dev).manual_seed(9)
            (rgb, _, _, _), ri, tv = Rm.render_rays(o, d, est, m, train=True, white_bkgd=True, render_step_size=OCC_STEP, device=dev)
            outs.append((rgb.detach(), ri, tv))
    finally:
        Rm.FUSED_OCC_SAMPLER, Rm.FUSED_OCC_SAMPLER_MIN_RAYS = keep
    assert outs[0][1].numel() > 500 and m.precision == prec
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][0], outs[1][0])


@pytest.mark.parametrize("prec", ["bf16", "fp16x3"])
def test_one_launch_occupancy_extras_of_the_smallest_network(dev, prec):
    """The extras mode of the launch (render_rays' full return tuple: one launch + one gather) against the unfused
    sequence: the same samples; per-ray and per-sample outputs bit for bit in fp16x3, within tests/test_occ_fused.py's
    single-pass bar in bf16."""
    from fs_nerf_amd.render import rendering as Rm
    m = occ_model("min", dev, prec)
    est = sphere_grid(32, 1, dev)
    o, d = orbit_rays(700, 5)

    def run():
        with torch.no_grad():
            return Rm.render_rays(o, d, est, m, white_bkgd=True, render_step_size=OCC_STEP, device=dev)

    (rgb_u, op_u, dep_u, ex_u), ri_u, tv_u = unfused(run)
    assert Rm.FUSED_OCC_EXTRAS and o.shape[0] * est.max_steps(OCC_STEP) <= Rm.FUSED_OCC_EXTRAS_MAX_SLOTS
    (rgb_f, op_f, dep_f, ex_f), ri_f, tv_f = run()
    e_rgb, e_op = float((rgb_f - rgb_u).abs().max()), float((op_f - op_u).abs().max())
    print(f"min {prec}: {ri_u.numel()} samples unfused, {ri_f.numel()} in the extras mode; rgb {e_rgb:.2e} opacity {e_op:.2e}")
    assert ri_u.numel() > 500 and m.precision == prec
    assert torch.equal(ri_f, ri_u) and torch.equal(tv_f, tv_u)
    if prec in X3:
        assert torch.equal(rgb_f, rgb_u) and torch.equal(op_f, op_u) and torch.equal(dep_f, dep_u)
        for k in ("weights", "alphas", "trans", "sigmas", "rgbs"):
            assert ex_f[k].shape == ex_u[k].shape and torch.equal(ex_f[k], ex_u[k]), k
    else:
        assert e_rgb <= OCC_TOL[prec] and e_op <= OCC_TOL[prec]
        for k in ("weights", "alphas", "trans", "sigmas", "rgbs"):
            assert ex_f[k].shape == ex_u[k].shape and bool(torch.isfinite(ex_f[k]).all()), k


# ------------------------------------------------------------------------------------------- e. training
TRAIN = [(None, 2e-4, 2e-5), ("bf16x3", 1e-3, 1e-4)]  # tests/test_train_step.py TRAIN_MODES / test_input_grad.py MODES


@functools.lru_cache(maxsize=None)
def train_reference(net, margin):
    """N samples whose every ReLU pre-activation is at least `margin` from zero, a cotangent, and float64 autograd's
    gradients of (out * c).sum() with respect to the parameters and the inputs."""
    L, D, skip, nf, nfd = CORNERS[net]
    gen = torch.Generator().manual_seed(21)
    x = torch.rand(4 * N, 3, generator=gen) * 3 - 1.5
    d = torch.nn.functional.normalize(torch.randn(4 * N, 3, generator=gen), dim=-1)
    keep = _relu_margin(state(net), x, d, L, list(skip), nf, nfd) > margin
    share = float(keep.float().mean())
    x, d = x[keep][:N].contiguous(), d[keep][:N].contiguous()
    assert x.shape[0] == N, f"{net}: {share:.2f} of the candidates pass the margin {margin:g}"
    c = torch.randn(N, 4, generator=gen)
    sdr = {k: v.double().clone().requires_grad_(True) for k, v in state(net).items()}
    x64, d64 = x.double().requires_grad_(True), d.double().requires_grad_(True)
    want = O.nerf_forward(sdr, x64, d64, **cfg(net))
    (want * c.double()).sum().backward()
    return x, d, c, want.detach(), {k: v.grad for k, v in sdr.items()}, x64.grad, d64.grad, share


@pytest.mark.parametrize("tp,tol,margin", TRAIN)
@pytest.mark.parametrize("net", NETS)
def test_training_gradients_against_float64_autograd(dev, net, tp, tol, margin):
    x, d, c, want, g_par, g_x, g_d, share = train_reference(net, margin)
    m = make_model(net, dev).train()
    m.train_precision = tp
    xg, dg = x.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    out = m(xg, dg)
    assert out.requires_grad and out.shape == (N, 4)
    (out * c.to(dev)).sum().backward()
    e_out = _rel(out, want)
    errs = {name: _rel(p.grad, g_par[name]) for name, p in m.named_parameters()}
    e_x, e_d = _rel(xg.grad, g_x), _rel(dg.grad, g_d)
    worst = max(errs, key=errs.get)
    print(f"FIGURE e {net} {tp}: {share:.2f} of the candidates kept; out {e_out:.2e}, parameter gradients up to "
          f"{errs[worst]:.2e} ({worst}), d x {e_x:.2e}, d dirs {e_d:.2e} (bar {tol:g})")
    assert set(errs) == set(g_par)
    assert e_out < (1e-4 if tp == "bf16x3" else 1e-5)
    for name, err in errs.items():
        assert err < tol, (name, err)
    assert e_x < tol and e_d < tol, (e_x, e_d)


# ------------------------------------------------------------------------------------------- f. the real depth limit
def test_a_256_wide_network_deeper_than_8_layers_is_refused(dev, models):
    """The aux area (biases, heads) of a network lives in kAuxCapFloats = 3456 floats of LDS: (n_layers + 5) x 256 + 36
    fits up to 8 layers.  9x256 packs (the packer's envelope is 2..16 layers) and every kernel entry point refuses it;
    nothing is left behind."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.core.models import NeRF
    from fs_nerf_amd.render import rendering as Rm
    from test_gpu_parity import _rays
    i = host_inputs()
    x, d = i["x"].to(dev), i["d"].to(dev)
    o, dr, gen = _rays(16, 3)
    est = Rm.StratifiedEstimator(2.0, 6.0, 16, 16)
    for prec in ("fp16x3", "bf16"):
        m9 = NeRF(3, 3, 9, 256, (4,), precision=prec, pos_fn={"n_freqs": 10, "log_space": True},
                  dir_fn={"n_freqs": 4, "log_space": True})
        m9.load_state_dict(O.init_nerf_state_dict(9, 256, [4], 10, 4, seed=7))
        m9 = m9.to(dev).eval()
        with torch.no_grad():
            with pytest.raises(RuntimeError, match="too deep"):
                m9(x, d)
            with pytest.raises(RuntimeError, match="too deep"):
                m9(x)
            with pytest.raises(RuntimeError, match="too deep"):
                Rm.render_rays(o, dr, est, m9, device=dev)
        assert m9.precision == prec
    assert ops.range_ok(dev)
    m, out = models("wide-skips", "fp16x3")
    with torch.no_grad():
        y = m(x, d)
    assert torch.equal(y, out[("point", True)]), "an 8x256 call right after the refused ones"
