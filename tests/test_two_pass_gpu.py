"""precision="fp16x2" (FSN_PREC_FP16X2, inference only) on the GPU: k_mlp_fwd and k_render_fused at both widths, the
nine hand-scheduled X2 k-loop blocks (tools/gen_kloop.py), the compiler-scheduled forms and the mode's range guard.

The mode streams the FSN_PREC_FP16X3 blob, leaves the weights' low fragments unread and forms, per GEMM,
ah.wh + 2^-11 al'.wh.  fp16x3 without activation scaling (`x3ns`) forms ah.wh + 2^-11 (al'.wh + ah.wl') and is held
to float64 all over the suite.  With every split weight exactly representable in fp16 (`R(W)`, tests/test_two_pass_cpu.py:
layers.*.weight, connection.weight, branch.weight - the GEMMs of csrc/mlp_pack.hpp pack_piece / gemm_to_sd; biases,
sigma.* and rgb.* are aux_value's float32 entries) wl' = 0 and the two modes form the same sums:

  a  x2(R(W)) == x3ns(R(W)), torch.equal                      same sums
  b  x2(W) == x2(R(W)), torch.equal                           the blobs differ in the low fragments only: never read
  c  x2(W) against float64 on R(W) at the x3 bars             (tests/test_shape_corners_gpu.py: rgb 1e-5, sigma 1e-4 max)
  d  a and b on every tensor of the fused render and sampler  the only route to the hand-scheduled X2 blocks
  e  the range guard: fp16x2 -> bf16x3                        (tests/test_parity_fp64.py's fp16x3 test, second half)
  f  training under fp16x2 is fp16x3 training                 (NeRF.train_prec)

Orders, read before asserting (a).  Compiler-scheduled (mlp_dev.hpp): k_mlp_fwd runs the x3 / x2 modes of BOTH widths
through unit_mfma_r (mlp.hip is VariantStandalone: kX3Pf1 and not kKloopAsm), the fused render its 128-wide networks through
unit_mfma; both issue, unit by unit, main = a.hi b.hi into the main tile, then [a.lo b.hi], then a.hi b.lo into the
correction tile, the bracketed product under prec_reads_w_lo only.  Hand-scheduled (render.hip, 256 wide):
gen_kloop.py block() emits per unit the same three in the same order, the middle one under `mode in ("X3", "X3S")`;
the X2 and X3 texts differ in that product, in the reads of the low A set and in the form of the lgkmcnt waits.  For
every one of the 18 texts the sequence of (A, B) operands per accumulator tile of X3 with the a.lo products struck
out IS the X2 sequence, and each correction tile's first product takes the constant 0 as its C operand in both
(checked by running block() for both modes).  So with wl' = 0 the two modes differ by MFMAs whose A operand is all
zeros, which add +0 to a tile: no network needs (c)'s bar in place of (a).

Which launches reach what.  Point and ray form (a - c) never execute a hand-scheduled block; those run in the fused
render only, so (d)'s 8x256 cases are what holds them - 8x256 with skip (4,) reaches all nine shapes
(test_two_pass_cpu.py::test_8x256_reaches_every_hand_scheduled_block).

Powers of two (a).  All split weights x 2^-7 as they are.  The same with 2^7 leaves the fp16 range in exact arithmetic
(float64 layer maxima 2.3e2, 1.2e4, 6.6e5 ... 7.5e17 on these samples; asserted in test_two_pass_cpu.py), so "no range flag" cannot
hold for it in any fp16 mode; 2^7 is applied to every other GEMM instead and 2^-7 to the rest, both ways round
(layer maxima 0.07 .. 228): every GEMM runs with its weights at 2^7 once and at 2^-7 twice, in range.

Measured on the MI355X, largest over the four launches, rgb absolute / sigma over max|sigma|:

  net          x2(W) against float64 on R(W)      against float64 on W (no bar: the weights' rounding)
  8x256        7.0e-8 / 6.1e-6                    8.8e-6 / 3.7e-4
  min          2.0e-7 / 1.5e-5                    1.4e-5 / 3.7e-4
  bare         5.8e-8 / 2.4e-7                    9.5e-6 / 4.9e-4
  deep         2.2e-7 / 1.8e-5                    1.3e-5 / 3.0e-4
  wide-skips   1.8e-7 / 1.3e-5                    7.9e-6 / 2.2e-4
  wide-min     2.5e-7 / 2.9e-5                    8.9e-6 / 5.3e-4

(bars: 1e-5 / 1e-4; the left column is of the size of fp16x3's in tests/test_shape_corners_gpu.py, the sigma figures
mostly the float32 midpoints of the ray form.)  (a), (b), (d), (f): no entry of any tensor differs.  (e): rgb within 2.1e-7 of float64 after the bf16x3 re-run.
The whole file, 28 tests: about 2 s on one MI355X (with tests/test_encoding_reuse_gpu.py: 52 tests in 3.8 s).

Arithmetic-only mutants, one build each.  unit_mfma_r skips a.hi b.lo for FSN_PREC_FP16X2: (a) and (c) fail on all
six networks, (d) passes (the fused render does not go through unit_mfma_r) and test_encoding_reuse_gpu.py's three
fp16x2 cases fail.  prec_reads_w_lo true for FSN_PREC_FP16X2: (b), (c) and (d) fail everywhere.  The generator's X2
16/0 parity-0 text with b.hi in place of b.lo in one correction MFMA: (d)'s two 8x256 cases and
test_encoding_reuse_gpu.py's fp16x2-8x256 fail, nothing else.  No test of another mode fails under any of them.
"""
import functools
import warnings

import pytest
import torch

from oracle import fsnerf_oracle as O
from test_encoding_reuse_gpu import NETS as RENDER_NETS, NEAR, FAR, camera, jitter, render_four_ways, state as medium_state
from test_gpu_parity import close
from test_parity_fp64 import cfg_of, hidden_max, hip_model, scaled_sd
from test_shape_corners_gpu import N, host_inputs
from test_two_pass_cpu import POW2, rounded, scaled
from wstream_ref import CORNERS

pytestmark = pytest.mark.gpu

NETS = dict(CORNERS)
NETS["8x256"] = (8, 256, (4,), 10, 4)
NET_IDS = ("8x256", "min", "bare", "deep", "wide-skips", "wide-min")
LAUNCHES = (("point", True), ("point", False), ("rays", True), ("rays", False))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def state(net):
    L, D, skip, nf, nfd = NETS[net]
    return O.init_nerf_state_dict(L, D, list(skip), nf, nfd, seed=7)


def cfg(net):
    L, D, skip, nf, nfd = NETS[net]
    return dict(n_layers=L, skip=list(skip), n_freqs=nf, n_freqs_dir=nfd, log_space=True)


def make(spec, sd, mode, dev):
    """mode "x2": precision fp16x2; "x3ns": fp16x3 without activation scaling (FSN_PREC_FP16X3)."""
    from fs_nerf_amd.core.models import NeRF
    L, D, skip, nf, nfd = spec
    m = NeRF(3, 3, L, D, skip, precision={"x2": "fp16x2", "x3ns": "fp16x3"}[mode], pos_fn={"n_freqs": nf, "log_space": True},
             dir_fn={"n_freqs": nfd, "log_space": True})
    m.load_state_dict(sd)
    m.act_scaling = False
    return m.to(dev).eval()


def want_prec(m, mode):
    from fs_nerf_amd import _lib
    want = {"x2": ("fp16x2", _lib.FSN_PREC_FP16X2), "x3ns": ("fp16x3", _lib.FSN_PREC_FP16X3)}[mode]
    return (m.precision, m.infer_prec()) == want


def four_launches(m, mode, i, what):
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a range fall-back here is a failure
        with torch.no_grad():
            for key in LAUNCHES:
                form, full = key
                if form == "point":
                    y = m(i["x"], i["d"]) if full else m(i["x"])
                else:
                    y = m.forward_rays(i["ro"], i["rd"], i["ri"], i["t0"], i["t1"], full)
                assert want_prec(m, mode), f"{what} {key}: the model left its precision"
                assert y.shape == (N, 4 if full else 1) and bool(torch.isfinite(y).all()), (what, key)
                out[key] = y
    return out


@pytest.fixture(scope="module")
def inputs(dev):
    return {k: v.to(dev) for k, v in host_inputs().items()}


@pytest.fixture(scope="module")
def runs(dev, inputs):
    """(network, mode, weights "W" / "R") -> the four launches' outputs, once per module."""
    cache = {}

    def get(net, mode, which):
        if (net, mode, which) not in cache:
            sd = state(net) if which == "W" else rounded(state(net))
            cache[(net, mode, which)] = four_launches(make(NETS[net], sd, mode, dev), mode, inputs, f"{net} {mode}({which})")
        return cache[(net, mode, which)]

    yield get
    cache.clear()


def n_diff(a, b):
    return f"{int((a != b).sum())} of {a.numel()} entries differ, by up to {float((a - b).abs().max()):.3e}"


# ------------------------------------------------------------------------------------------- a. same sums
@pytest.mark.parametrize("net", NET_IDS)
def test_x2_forms_the_sums_of_x3_on_fp16_weights(dev, runs, net):
    from fs_nerf_amd import ops
    a, b = runs(net, "x2", "R"), runs(net, "x3ns", "R")
    for key in LAUNCHES:
        assert torch.equal(a[key], b[key]), f"{net} {key}: x2(R(W)) != x3ns(R(W)): {n_diff(a[key], b[key])}"
    assert ops.range_ok(dev)


@pytest.mark.parametrize("case", list(POW2))
def test_x2_forms_the_sums_of_x3_under_powers_of_two(dev, inputs, case):
    """Point form, 8x256, the split weights scaled by exact powers of two before rounding: other exponents in the high
    parts (2^-7: many fp16 subnormals) and in the products of the correction tile."""
    from fs_nerf_amd import ops
    sd = rounded(scaled(state("8x256"), 8, POW2[case]))
    hi = host_inputs()
    mx = O.layer_maxima(sd, hi["x"], hi["d"], **cfg("8x256"))
    assert 2.0 ** -6 < min(mx) and max(mx) < 65504.0 / 64, f"{case}: float64 layer maxima {mx} are well inside the envelope"
    assert ops.range_ok(dev)  # clean slate
    out = {}
    for mode in ("x2", "x3ns"):
        m = make(NETS["8x256"], sd, mode, dev)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            with torch.no_grad():
                out[mode] = (m(inputs["x"], inputs["d"]), m(inputs["x"]))
        assert want_prec(m, mode) and m.range_events == 0
        assert ops.range_ok(dev), f"{case} {mode}: a range flag was raised"
    for a, b in zip(out["x2"], out["x3ns"]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), f"{case}: {n_diff(a, b)}"
    print(f"{case}: layer maxima {min(mx):.3g} .. {max(mx):.3g}; rgb range {float(out['x2'][0][:, :3].min()):.3f} .. "
          f"{float(out['x2'][0][:, :3].max()):.3f}")


# ------------------------------------------------------------------------------------------- b. low fragments unread
@pytest.mark.parametrize("net", NET_IDS)
def test_x2_never_reads_the_weights_low_fragments(runs, net):
    a, b = runs(net, "x2", "W"), runs(net, "x2", "R")
    for key in LAUNCHES:
        assert torch.equal(a[key], b[key]), f"{net} {key}: x2(W) != x2(R(W)): {n_diff(a[key], b[key])}"
    if net == "8x256":  # not vacuous: the low fragments of W matter to the mode that reads them
        c = runs(net, "x3ns", "W")
        for key in LAUNCHES:
            assert not torch.equal(c[key], a[key]), key


# ------------------------------------------------------------------------------------------- c. float64
@functools.lru_cache(maxsize=None)
def truth(net, which):
    """float64 oracle on R(W) / W for both forms (the ray form's midpoints formed in float64)."""
    i = {k: (v.double() if v.is_floating_point() else v) for k, v in host_inputs().items()}
    sd = {k: v.double() for k, v in (rounded(state(net)) if which == "R" else state(net)).items()}
    forms = {"point": (i["x"], i["d"]),
             "rays": (i["ro"][i["ri"]] + i["rd"][i["ri"]] * (i["t0"] + i["t1"])[:, None] / 2.0, i["rd"][i["ri"]])}
    return {form: O.nerf_forward(sd, x, d, **cfg(net)) for form, (x, d) in forms.items()}


@pytest.mark.parametrize("net", NET_IDS)
def test_x2_against_float64_on_the_rounded_weights(runs, net):
    out = runs(net, "x2", "W")
    worst = {"R": [0.0, 0.0], "W": [0.0, 0.0]}
    fails = []
    for (form, full), y in out.items():
        y = y.cpu().double()
        for which in ("R", "W"):
            want = truth(net, which)[form]
            smax = float(want[:, 3].abs().max())
            e_sigma = float((y[:, -1] - want[:, 3]).abs().max()) / smax
            e_rgb = float((y[:, :3] - want[:, :3]).abs().max()) if full else 0.0
            worst[which] = [max(worst[which][0], e_rgb), max(worst[which][1], e_sigma)]
            if which == "W":
                continue  # for the record only: the weights' rounding, not the kernel
            print(f"{net} fp16x2 {form} {'full' if full else 'density'}: rgb {e_rgb:.2e} (atol 1e-5), sigma/max {e_sigma:.2e} (atol 1e-4)")
            try:
                if full:
                    close(y[:, :3], want[:, :3], atol=1e-5, what=f"{net} fp16x2 {form} rgb")
                close(y[:, -1], want[:, 3], atol=1e-4 * smax, what=f"{net} fp16x2 {form} sigma")
            except AssertionError as e:
                fails.append(str(e))
    print(f"FIGURE c {net}: against float64 on R(W) rgb {worst['R'][0]:.2e} sigma/max {worst['R'][1]:.2e}; "
          f"on W rgb {worst['W'][0]:.2e} sigma/max {worst['W'][1]:.2e}")
    assert not fails, fails


# ------------------------------------------------------------------------------------------- d. fused render and sampler
#        id: network, S, NI, image (H, W), masks
RENDER = {"rays5-8x256": ("8x256", 64, 128, (1, 5), False),
          "ragged7-8x256": ("8x256", 40, 24, (1, 7), False),
          "ragged7-4x128": ("4x128", 40, 24, (1, 7), False),
          "ragged7-two-skips": ("8x128-two-skips", 40, 24, (1, 7), False),
          "masks-pixels2x3-two-skips": ("8x128-two-skips", 64, 128, (2, 3), True)}
TENSORS = {"colors", "opacity", "depth", "edges", "weights", "weights_coarse", "sigmas", "rgbs", "alphas", "trans"}


def render_all(net, mode, which, S, NI, H, W, pm, dm, dev):
    """The four launch shapes of the fused render and the sampler-only launch -> {(launch, tensor name): tensor}."""
    from fs_nerf_amd import ops
    pair = []
    for seed in (42, 43):
        sd = medium_state(net, seed)
        pair.append(make(RENDER_NETS[net], sd if which == "W" else rounded(sd), mode, dev))
    pc, pf = pair[0].packed(), pair[1].packed()
    assert want_prec(pair[0], mode) and want_prec(pair[1], mode) and pc.prec == pair[0].infer_prec()
    o, d, outs = render_four_ways(pc, pf, camera(H, W, 123.0, dev), S, NI, dev, pm, dm)
    res = {(key, name): t for key, out in outs.items() for name, t in out.items()}
    for key, out in outs.items():
        assert TENSORS <= set(out), (key, sorted(out))
    u, uf = jitter(H * W, NI, dev)
    edges, wc = ops.sample_fused(pc, o, d, near=NEAR, far=FAR, n_samples=S, n_importance=NI, u=u, u_fine=uf, pos_mask=pm,
                                 dir_mask=dm, want_weights=True)
    res[("sampler", "edges")], res[("sampler", "weights_coarse")] = edges, wc
    for k, t in res.items():
        assert bool(torch.isfinite(t).all()), k
    return res


@pytest.mark.parametrize("case", list(RENDER))
def test_fused_render_and_sampler_in_x2(dev, case):
    from fs_nerf_amd import ops
    net, S, NI, (H, W), masked = RENDER[case]
    pm = O.freq_mask(3, 10, 0.45).to(dev) if masked else None
    dm = O.freq_mask(3, 4, 0.6).to(dev) if masked else None
    assert ops.range_ok(dev)
    x2r, x3r, x2w = (render_all(net, mode, which, S, NI, H, W, pm, dm, dev) for mode, which in (("x2", "R"), ("x3ns", "R"), ("x2", "W")))
    assert ops.range_ok(dev), "no launch raised a range flag"
    assert set(x2r) == set(x3r) == set(x2w) and len(x2r) >= 4 * len(TENSORS) + 2
    opa = float(x2w[(("rays", False), "opacity")].max())
    print(f"{case}: {len(x2r)} tensors; opacity up to {opa:.3f}")
    assert opa > 0.5, "the rays hit a medium"
    for k in x2r:
        assert x2r[k].shape == x3r[k].shape and torch.equal(x2r[k], x3r[k]), f"{case} {k}: x2(R(W)) != x3ns(R(W)): {n_diff(x2r[k], x3r[k])}"
        assert torch.equal(x2w[k], x2r[k]), f"{case} {k}: x2(W) != x2(R(W)): {n_diff(x2w[k], x2r[k])}"
    # the sampler-only launch returns the full launch's edges and coarse weights
    assert torch.equal(x2w[("sampler", "edges")], x2w[(("rays", False), "edges")])
    assert torch.equal(x2w[("sampler", "weights_coarse")], x2w[(("rays", False), "weights_coarse")])


# ------------------------------------------------------------------------------------------- e. range guard
def test_fp16x2_out_of_range_is_detected_and_rerun_in_bf16x3(dev):
    from fs_nerf_amd import ops
    from fs_nerf_amd.core.models import NeRF
    from fs_nerf_amd.render import rendering as Rm
    assert NeRF.FALLBACK["fp16x2"] == "bf16x3"
    L, D = 8, 256
    gen = torch.Generator().manual_seed(12)
    sd_c, sd_f = scaled_sd(L, D, 42, 4e5), scaled_sd(L, D, 43, 4e5)
    pts_h = torch.rand(500, 3, generator=gen) * 2 - 1
    dirs_h = torch.nn.functional.normalize(torch.randn(500, 3, generator=gen), dim=-1)
    assert hidden_max(sd_f, pts_h, L) > 2 * 65504.0
    pts, dirs = pts_h.to(dev), dirs_h.to(dev)
    try:
        assert ops.range_ok(dev)  # clean slate
        m = hip_model(sd_f, L, D, dev, "fp16x2")
        with pytest.warns(RuntimeWarning, match="fp16 range"):
            with torch.no_grad():
                y = m(pts, dirs)
        assert m.precision == "bf16x3" and bool(torch.isfinite(y).all())
        want = O.nerf_forward({k: v.double() for k, v in sd_f.items()}, pts_h.double(), dirs_h.double(), **cfg_of(L))
        e = float((y.cpu().double() - want)[:, :3].abs().max())
        print(f"after the bf16x3 re-run: rgb {e:.2e} (bar 1e-4)")
        assert e < 1e-4
        assert ops.range_ok(dev), "the guard consumed the word"
        # with the guard switched off nothing is read back and nothing is re-run
        m2 = hip_model(sd_f, L, D, dev, "fp16x2")
        m2.range_check = False
        with torch.no_grad():
            m2(pts, dirs)
        assert m2.precision == "fp16x2" and not ops.range_ok(dev)  # ... but the device word recorded it
        # render_rays: the fused stratified launch
        R = 8
        o, d = ops.get_rays(O.pose_from_spherical(4.0311289, 50.0, 123.0), 1, R, 3.0, dev)
        x = (o[:, None, :] + d[:, None, :] * torch.linspace(2.0, 6.0, 16, device=dev)[None, :, None]).reshape(-1, 3).cpu()
        assert hidden_max(sd_f, x, L) > 2 * 65504.0 and hidden_max(sd_c, x, L) > 2 * 65504.0
        mc, mf = hip_model(sd_c, L, D, dev, "fp16x2"), hip_model(sd_f, L, D, dev, "fp16x2")
        u, uf = jitter(R, 128, dev)
        est = Rm.StratifiedEstimator(2.0, 6.0, 64, 128)
        with pytest.warns(RuntimeWarning, match="fp16 range"):
            with torch.no_grad():
                (rgb, op, dep, ex), _, _ = Rm.render_rays(o, d, est, mc, white_bkgd=True, device=dev, model_fine=mf, u=u, u_fine=uf)
        assert mc.precision == "bf16x3" and mf.precision == "bf16x3", "both models continue in the wide-range mode"
        for t in (rgb, op, dep, ex["weights"], ex["sigmas"], ex["rgbs"]):
            assert bool(torch.isfinite(t).all())
        assert ops.range_ok(dev)
    finally:
        ops.range_flags(dev)  # whatever happened above: the next test finds the word clean
    assert ops.range_ok(dev)


# ------------------------------------------------------------------------------------------- f. training
def test_training_under_fp16x2_is_fp16x3_training(dev):
    from fs_nerf_amd import _lib
    spec = RENDER_NETS["4x128"]
    sd = O.init_nerf_state_dict(4, 128, [4], 10, 4, seed=7)
    i = host_inputs()
    c = torch.randn(N, 4, generator=torch.Generator().manual_seed(22)).to(dev)
    res = {}
    for prec in ("fp16x2", "fp16x3"):
        m = make(spec, sd, {"fp16x2": "x2", "fp16x3": "x3ns"}[prec], dev).train()
        assert m.train_prec() == _lib.FSN_PREC_FP16X3
        xg, dg = i["x"].to(dev).requires_grad_(True), i["d"].to(dev).requires_grad_(True)
        out = m(xg, dg)
        assert out.requires_grad and out.shape == (N, 4)
        (out * c).sum().backward()
        assert m.precision == prec
        res[prec] = (out.detach(), xg.grad, dg.grad, {k: p.grad for k, p in m.named_parameters()})
    a, b = res["fp16x2"], res["fp16x3"]
    assert set(a[3]) == set(b[3]) == set(sd)
    for what, ta, tb in [("out", a[0], b[0]), ("d x", a[1], b[1]), ("d dirs", a[2], b[2])] + [(k, a[3][k], b[3][k]) for k in a[3]]:
        assert ta is not None and bool(torch.isfinite(ta).all()) and float(ta.abs().max()) > 0.0, what
        assert torch.equal(ta, tb), f"{what}: {n_diff(ta, tb)}"
