"""Quantitative parity of the whole hot path (north_star: rgb_map, depth_map, weights within 1e-4 relative of the
reference PyTorch CPU path on identical rays / RNG), END TO END - stratified edges, coarse density pass, inverse-CDF
resampling, fine pass, compositing in ONE fused launch, no intermediate result substituted.

Method: the oracle is evaluated twice on the same float32 inputs, in float64 (the truth) and in float32 ("the
reference PyTorch CPU path").  For every output
  (1) the HIP path's error against the truth must be of the size of the float32 oracle's own error:
      max and 99th percentile <= 2 x the oracle's (+ a floor of a few float32 ulps of the output's scale);
  (2) wherever the float32 oracle is within 1e-4 relative (+ the same small absolute floor) of the truth, so is HIP.
Compositing / sampling follow the build's restatement of nerfacc and its own sampler definitions (PARITY UNPINNED
for those rows); the MLP / encoder / ray rows underneath are pinned by the reference-generated goldens.
"""
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import fsnerf_oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-4
# criterion (1): slack of a few float32 ulps of the output's scale on top of "2 x the float32 oracle's error"
FLOOR = {"rgb_map": 3e-7, "opacity": 3e-7, "weights": 3e-7, "depth_map": 3e-6}
# criterion (2): absolute floor next to the 1e-4 relative bound (values that are ~0 have no meaningful relative
# error): 1e-6 of full scale for the [0,1] quantities, 1e-5 for a single weight (a sample's weight moves by up to
# 1.6e-5 in the float32 oracle itself when an importance sample crosses an interval edge), 1e-5 m for depth
ATOL = {"rgb_map": 1e-6, "opacity": 1e-6, "weights": 1e-5, "depth_map": 1e-5}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def make_sd(L, D, seed, sigma_gain=64.0, sigma_shift=3.0):
    sd = O.init_nerf_state_dict(L, D, [4], 10, 4, seed=seed)
    sd["sigma.weight"] = sd["sigma.weight"] * sigma_gain
    sd["sigma.bias"] = sd["sigma.bias"] + sigma_shift
    return sd


def cfg_of(L):
    return dict(n_layers=L, skip=[4], n_freqs=10, n_freqs_dir=4, log_space=True)


def hip_model(sd, L, D, dev, precision, pm=None, dm=None, act_scaling=True):
    """act_scaling (fp16x3 inference): True = round 4's scaled network in FSN_PREC_FP16X3U (the default), False = round
    3's arithmetic (FSN_PREC_FP16X3: low parts scaled by 2^11, correction accumulator), still what training runs."""
    from fs_nerf_amd.core.models import NeRF
    m = NeRF(3, 3, L, D, (4,), precision=precision, pos_fn={"n_freqs": 10, "log_space": True},
             dir_fn={"n_freqs": 4, "log_space": True})
    m.load_state_dict(sd)
    m.set_freq_mask(pm, dm)
    m.act_scaling = act_scaling
    return m.to(dev).eval()


def orbit_rays(R, seed, hw, focal):
    gen = torch.Generator().manual_seed(seed)
    pose = O.pose_from_spherical(4.0311289, 50.0, float(torch.rand(1, generator=gen)) * 360.0)
    o, d = O.get_rays(pose, (hw, hw, focal))
    idx = torch.randperm(hw * hw, generator=gen)[:R]
    return o.reshape(-1, 3)[idx].contiguous(), d.reshape(-1, 3)[idx].contiguous(), gen


def ndc_rays(R, seed):
    gen = torch.Generator().manual_seed(seed)
    hwf = (378, 504, 407.6)
    pose = torch.eye(4)
    pose[:3, 3] = torch.tensor([0.1, -0.05, 0.0])
    o, d = O.get_rays(pose, hwf)
    o, d = O.to_ndc(o.reshape(-1, 3), d.reshape(-1, 3), hwf, 1.0)
    idx = torch.randperm(o.shape[0], generator=gen)[:R]
    return o[idx].contiguous(), d[idx].contiguous(), gen


def oracle(o, d, sd_c, sd_f, cfg, dtype, **kw):
    c = lambda t: None if t is None else t.to(dtype)
    sdc = {k: v.to(dtype) for k, v in sd_c.items()}
    sdf = None if sd_f is None else {k: v.to(dtype) for k, v in sd_f.items()}
    kw = {k: (c(v) if torch.is_tensor(v) else v) for k, v in kw.items()}
    return O.render_rays_oracle(c(o), c(d), sdc, sdf, cfg, **kw)


def outputs(res):
    (rgb, op, dep, ex), _, _ = res
    R = rgb.shape[0]
    f = lambda t: t.detach().cpu().double().numpy()
    return {"rgb_map": f(rgb), "opacity": f(op).reshape(R, 1), "depth_map": f(dep).reshape(R, 1),
            "weights": f(ex["weights"]).reshape(R, -1)}


def assert_parity(hip, o32, truth, what, factor=2.0, rtol=RTOL, atol_scale=1.0, tail="elementwise"):
    """(1) error-size and (2) 1e-4 criteria of the module docstring, for every output.
    tail="count" (trained networks): the coarse pdf of a trained density is peaked, most importance samples fall into
    intervals of mass ~1e-4, where the inverse CDF turns a 1e-7 difference of the coarse cdf into a 1e-4 shift of the
    sample and of the weights on either side of it - in the float32 oracle as in the kernel, in DIFFERENT elements.
    The float32 oracle is then itself outside 1e-4 on a tail of elements; criterion (2) becomes: HIP's tail is no
    larger - at most twice as many elements outside the tolerance as the float32 oracle has (+ 1 in 5000)."""
    H, P, T = outputs(hip), outputs(o32), outputs(truth)
    report = {}
    for k in ("rgb_map", "depth_map", "weights", "opacity"):
        assert H[k].shape == T[k].shape, f"{what} {k}: shape {H[k].shape} vs {T[k].shape}"
        assert np.isfinite(H[k]).all(), f"{what} {k}: non-finite values"
        eh, ep = np.abs(H[k] - T[k]), np.abs(P[k] - T[k])
        fl = FLOOR[k] * max(1.0, float(np.abs(T[k]).max()) if k != "depth_map" else 1.0)
        report[k] = (eh.max(), ep.max(), np.percentile(eh, 99), np.percentile(ep, 99))
        assert eh.max() <= factor * ep.max() + fl, \
            f"{what} {k}: max error {eh.max():.3e} vs float32 oracle's {ep.max():.3e} (x{factor} + {fl:.1e})"
        assert np.percentile(eh, 99) <= factor * np.percentile(ep, 99) + fl, \
            f"{what} {k}: p99 error {np.percentile(eh, 99):.3e} vs float32 oracle's {np.percentile(ep, 99):.3e}"
        tol = rtol * np.abs(T[k]) + atol_scale * ATOL[k]
        ok32 = ep <= tol
        nh, n32 = int((eh > tol).sum()), int((~ok32).sum())
        report[k] = report[k] + (nh, n32)
        if tail == "count":
            assert nh <= 2 * n32 + eh.size // 5000, f"{what} {k}: {nh} of {eh.size} elements outside 1e-4, the " \
                                                    f"float32 oracle has {n32}"
        else:
            bad = ok32 & (eh > tol)
            assert not bad.any(), f"{what} {k}: {int(bad.sum())} of {bad.size} elements outside 1e-4 where the float32 " \
                                  f"oracle is inside (worst {float((eh - tol)[bad].max()):.3e} over)"
        assert ok32.mean() > 0.99, f"{what} {k}: the float32 oracle itself is outside 1e-4 on {1 - ok32.mean():.4f}"
    return report


# BASELINE.json configurations: (net, S, NI, two nets, rays, near, far, mask ratio)
CASES = {
    "C1": ("4x128", 64, 0, False, "orbit100", 2.0, 6.0, None),       # configs[0]: 100x100, 64 coarse, 4x128, mask off
    "C2": ("8x256", 64, 0, False, "orbit400", 2.0, 6.0, 0.5),        # configs[1]: 400x400, 64 coarse, 8x256, mask on
    "C3": ("8x256", 64, 128, True, "orbit800", 2.0, 6.0, None),      # configs[2]: 800x800, 64+128, two 8x256 (headline)
    "C4": ("8x256", 64, 128, False, "ndc", 0.0, 1.0, None),          # configs[3]: forward-facing NDC rays, 64+128
    # configs[4]'s SHAPE in the parity modes (its stated dtype, bf16, has its own tests below): 128+256 samples =
    # kMaxRaySamples, one ray per workgroup group, a different tile split (render.hip launch_render) - VERDICT r3 weak #7
    "C5": ("8x256", 128, 256, True, "orbit1600", 2.0, 6.0, None),
}
DIMS = {"4x128": (4, 128), "8x256": (8, 256)}


def run_case(name, dev, precision, R=192, jitter=True, act_scaling=True):
    from fs_nerf_amd.render import rendering as Rm
    tag, S, NI, two, rk, near, far, mr = CASES[name]
    if name == "C5":
        R = min(R, 96)  # (the float64 oracle evaluates 96 x (128 + 384) samples)
    L, D = DIMS[tag]
    sd_c = make_sd(L, D, 42)
    sd_f = make_sd(L, D, 43) if two else None
    if rk == "ndc":
        o, d, gen = ndc_rays(R, 7)
    else:
        hw = int(rk[5:])
        o, d, gen = orbit_rays(R, 7, hw, 0.5 * hw / np.tan(0.5 * 0.6911112))
    u = torch.rand(R, generator=gen) if jitter else None
    uf = torch.rand(R, NI, generator=gen) if (jitter and NI) else None
    pm = O.freq_mask(3, 10, mr) if mr else None
    dm = O.freq_mask(3, 4, mr) if mr else None
    kw = dict(near=near, far=far, n_samples=S, n_importance=NI, u=u, u_fine=uf, white_bkgd=True, pos_mask=pm,
              dir_mask=dm)
    truth = oracle(o, d, sd_c, sd_f, cfg_of(L), torch.float64, **kw)
    o32 = oracle(o, d, sd_c, sd_f, cfg_of(L), torch.float32, **kw)
    mc = hip_model(sd_c, L, D, dev, precision, pm, dm, act_scaling)
    mf = hip_model(sd_f, L, D, dev, precision, pm, dm, act_scaling) if two else None
    est = Rm.StratifiedEstimator(near, far, S, NI)
    with torch.no_grad():
        hip = Rm.render_rays(o, d, est, mc, white_bkgd=True, device=dev, model_fine=mf,
                             u=None if u is None else u.to(dev), u_fine=None if uf is None else uf.to(dev))
    assert mc.precision == precision, "no range fallback expected here"
    return hip, o32, truth


# (round 3's arithmetic - act_scaling False, what the training kernels run - on the headline and the NDC shape with jitter;
# the default, scaled arithmetic on every shape with and without)
@pytest.mark.parametrize("name,jitter,act_scaling", [(n, j, True) for n in ("C1", "C2", "C3", "C4", "C5") for j in (True, False)] +
                         [("C3", True, False), ("C4", True, False), ("C1", False, False)])
def test_end_to_end_fp16x3_is_float32_grade(dev, name, jitter, act_scaling):
    """The default parity mode on every BASELINE configuration's shape, end to end (for C3 / C4 that is coarse pass ->
    resampling -> fine pass on the kernel's own importance samples): error of the size of the float32 oracle's.  Both
    arithmetic variants of the mode: the scaled network of round 4 (the default) and round 3's."""
    hip, o32, truth = run_case(name, dev, "fp16x3", jitter=jitter, act_scaling=act_scaling)
    assert_parity(hip, o32, truth, f"{name} fp16x3")
    # the sample positions themselves (t_vals) and the ray indices of the 3-tuple
    (_, _, _, ex), ri, tv = hip
    (_, _, _, tex), tri, ttv = truth
    assert torch.equal(ri.cpu(), tri)
    et = (tv.cpu().double() - ttv).abs()
    e32 = (o32[2].double() - ttv).abs()
    assert float(et.max()) <= 2.0 * float(e32.max()) + 3e-6, (float(et.max()), float(e32.max()))


@pytest.mark.parametrize("name,jitter", [("C1", True), ("C2", True), ("C3", True), ("C4", True), ("C5", True), ("C5", False)])
def test_end_to_end_bf16x3_fallback_mode(dev, name, jitter):
    """bf16x3 (the mode the fp16 range guard falls back to; ~2^-16 per product): at most 10 x the float32 oracle's
    error, inside 1e-4 relative with three times the absolute floors (3e-5 on a single weight: measured 2.2e-5).  Every
    BASELINE shape (C1 / C2 and the 128+256 shape were not covered)."""
    hip, o32, truth = run_case(name, dev, "bf16x3", jitter=jitter)
    assert_parity(hip, o32, truth, f"{name} bf16x3", factor=10.0, atol_scale=3.0)


# ------------------------------------------------------------------ fp16x3 range envelope
def scaled_sd(L, D, seed, s):
    """Hidden activations ~ s x those of the default-init net: layer 0 and every later hidden bias scaled by s (ReLU
    is positively homogeneous, so every hidden activation scales by exactly s), sigma / connection weights by 1/s so
    that the outputs stay those of the unscaled net (up to rounding)."""
    sd = make_sd(L, D, seed)
    sd["layers.0.weight"] = sd["layers.0.weight"] * s
    for i in range(L):
        sd[f"layers.{i}.bias"] = sd[f"layers.{i}.bias"] * s
    for i in range(1, L):
        if i - 1 in (4,):  # the skip layer sees [h, x_in]: the x_in columns must carry the factor themselves
            w = sd[f"layers.{i}.weight"].clone()
            w[:, D:] = w[:, D:] * s
            sd[f"layers.{i}.weight"] = w
    sd["sigma.weight"] = sd["sigma.weight"] / s
    sd["connection.weight"] = sd["connection.weight"] / s
    return sd


def hidden_max(sd, x, L):
    sd64 = {k: v.double() for k, v in sd.items()}
    pe = O.posenc(x.double(), 10, True)
    h, mx = pe, 0.0
    for i in range(L):
        h = torch.relu(h @ sd64[f"layers.{i}.weight"].T + sd64[f"layers.{i}.bias"])
        mx = max(mx, float(h.max()))
        if i == 4:
            h = torch.cat([h, pe], dim=-1)
    return mx


@pytest.mark.parametrize("scale,factor,act_scaling", [(1e2, 3.0, True), (1e4, 3.0, True), (1e6, 3.0, True), (1e9, 3.0, True),
                                                       (1e4, 3.0, False)])
def test_fp16x3_envelope_large_activations(dev, scale, factor, act_scaling):
    """Trained networks have activations far above the default initialisation's ~1: with hidden activations of 1e2
    and 1e4 (still inside the fp16 range) the parity mode must stay float32-grade (3 x the float32 oracle's error),
    end to end.  At 1e4 the test network's sigma / connection weights are ~2e-5, i.e. fp16-subnormal high parts: until
    round 3 their low parts fell below fp16's 6e-8 resolution (error 5e-6 on rgb_map, asserted at 40 x); the low parts
    are now stored scaled by 2^11 (csrc/mlp_layout.hpp) and the case is float32-grade like the others.
    Round 4 (act_scaling, the default): per-layer power-of-two scales folded into the packed network bring every layer
    back to 2^4 .. 2^10 whatever its own scale - activations of 1e6 and 1e9, beyond fp16 altogether, are as native as 1."""
    from fs_nerf_amd.render import rendering as Rm
    L, D, R, S, NI = 8, 256, 192, 64, 128
    o, d, gen = orbit_rays(R, 11, 800, 1111.111)
    u, uf = torch.rand(R, generator=gen), torch.rand(R, NI, generator=gen)
    sd_c, sd_f = scaled_sd(L, D, 42, scale / 3.0), scaled_sd(L, D, 43, scale / 3.0)
    x = o[:, None, :] + d[:, None, :] * torch.linspace(2.0, 6.0, 16)[None, :, None]
    hm = hidden_max(sd_f, x.reshape(-1, 3), L)
    assert 0.3 * scale < hm < (3.0 * scale if act_scaling else 65504.0 / 2), f"test net: hidden max {hm:.3g} for scale {scale:g}"
    kw = dict(near=2.0, far=6.0, n_samples=S, n_importance=NI, u=u, u_fine=uf, white_bkgd=True)
    truth = oracle(o, d, sd_c, sd_f, cfg_of(L), torch.float64, **kw)
    o32 = oracle(o, d, sd_c, sd_f, cfg_of(L), torch.float32, **kw)
    mc, mf = hip_model(sd_c, L, D, dev, "fp16x3", act_scaling=act_scaling), hip_model(sd_f, L, D, dev, "fp16x3", act_scaling=act_scaling)
    est = Rm.StratifiedEstimator(2.0, 6.0, S, NI)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a range fallback here would be a failure
        with torch.no_grad():
            hip = Rm.render_rays(o, d, est, mc, white_bkgd=True, device=dev, model_fine=mf, u=u.to(dev), u_fine=uf.to(dev))
    assert mc.precision == "fp16x3" and mf.precision == "fp16x3" and mc.range_events == 0 and mf.range_events == 0
    assert_parity(hip, o32, truth, f"activations ~{scale:g}", factor=factor)


@pytest.mark.parametrize("s,act_scaling", [(1e-2, True), (1e-4, True), (1e-6, True), (1e-9, True),
                                           (1e-2, False), (1e-3, False), (1e-4, False)])
def test_fp16x3_envelope_small_activations(dev, s, act_scaling):
    """The LOW end of the envelope (the reference's weight-norm regulariser pushes this way).
    Hidden activations ~ s x the default initialisation's.  Unscaled fp16 low parts are subnormal below ~0.1 (an
    activation of 1e-3 kept ~15 bits: sigma errors of 4e-4 relative, silently); with the low parts scaled by 2^11 and
    the correction products in their own accumulator the mode is float32-grade natively down to s = 1e-3 (layer
    maxima 1e-4 .. 2e-3), checked here END TO END on the headline shape with the same criterion as everywhere else.
    Below that the kernels REPORT it (FSN_STATUS_FP16_SMALL: a layer whose largest activation over a wavefront's 16
    samples is an fp16 subnormal, < 2^-14) and the host re-runs in bf16x3 with a RuntimeWarning - checked to bf16x3's
    stated accuracy.  Either way never silent.
    Round 4 (act_scaling, the default): the scaled network has no low end - activations of 1e-4, 1e-6 and 1e-9 are native
    fp16x3 like everything else (the calibration puts every layer at 2^10), no report, no fall-back."""
    from fs_nerf_amd.render import rendering as Rm
    L, D, R, S, NI = 8, 256, 192, 64, 128
    o, d, gen = orbit_rays(R, 13, 800, 1111.111)
    u, uf = torch.rand(R, generator=gen), torch.rand(R, NI, generator=gen)
    sd_c, sd_f = scaled_sd(L, D, 42, s), scaled_sd(L, D, 43, s)
    x = o[:, None, :] + d[:, None, :] * torch.linspace(2.0, 6.0, 16)[None, :, None]
    hm = hidden_max(sd_f, x.reshape(-1, 3), L)
    assert 0.3 * s < hm < 30 * s, f"test net: hidden max {hm:.3g} for s {s:g}"
    kw = dict(near=2.0, far=6.0, n_samples=S, n_importance=NI, u=u, u_fine=uf, white_bkgd=True)
    truth = oracle(o, d, sd_c, sd_f, cfg_of(L), torch.float64, **kw)
    o32 = oracle(o, d, sd_c, sd_f, cfg_of(L), torch.float32, **kw)
    mc, mf = hip_model(sd_c, L, D, dev, "fp16x3", act_scaling=act_scaling), hip_model(sd_f, L, D, dev, "fp16x3", act_scaling=act_scaling)
    est = Rm.StratifiedEstimator(2.0, 6.0, S, NI)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with torch.no_grad():
            hip = Rm.render_rays(o, d, est, mc, white_bkgd=True, device=dev, model_fine=mf, u=u.to(dev), u_fine=uf.to(dev))
    fell_back = mc.precision == "bf16x3"
    if act_scaling:
        assert not fell_back and not rec and mc.range_events == 0 and mf.range_events == 0, "the scaled network has no low end"
    if s >= 1e-3:
        assert not fell_back and not rec, f"s={s:g} is inside the native envelope (hidden max {hm:.3g})"
    if fell_back:
        assert mf.precision == "bf16x3" and any("below 2^-14" in str(w.message) for w in rec), "reported, not silent"
        # (bf16x3's own grade, ~2^-16 per product whatever the scale: 4 x the absolute floors here - measured: one
        # weight of 36,864 at 3.3e-5 - against 3 x on the default-scale nets of test_end_to_end_bf16x3_fallback_mode)
        assert_parity(hip, o32, truth, f"activations ~{s:g}, reported bf16x3 re-run", factor=10.0, atol_scale=4.0)
    else:
        assert not rec
        assert_parity(hip, o32, truth, f"activations ~{s:g}, native fp16x3", factor=3.0)
    if s <= 1e-4 and not act_scaling:
        assert fell_back, "below the envelope the mode must say so"


@pytest.mark.parametrize("s,act_scaling", [(v, True) for v in (1e9, 1e6, 1e4, 1e2, 1.0, 1e-2, 1e-3, 1e-6, 1e-9)] +
                         [(v, False) for v in (1e4, 1.0, 1e-3)])
def test_fp16x3_sigma_relative_error_over_the_envelope(dev, s, act_scaling):
    """NeRF.forward alone, 20,000 points, the density head's RELATIVE error (a weight's error is of the same order):
    fp16x3 within 4 x the float32 oracle's error against a float64 evaluation over the whole native envelope
    (tools/emulate_split.py tabulates the same arithmetic on the CPU: rounds 1-2 had 3e-3 at s = 1e-2)."""
    L, D, n = 8, 256, 20000
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(n, 3, generator=gen) * 3.0 - 1.5
    dv = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
    sd = scaled_sd(L, D, 42, s)
    want = O.nerf_forward({k: v.double() for k, v in sd.items()}, x.double(), dv.double(), **cfg_of(L))
    o32 = O.nerf_forward(sd, x, dv, **cfg_of(L)).double()
    m = hip_model(sd, L, D, dev, "fp16x3", act_scaling=act_scaling)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with torch.no_grad():
            y = m(x.to(dev), dv.to(dev)).cpu().double()
    assert m.precision == "fp16x3" and m.range_events == 0
    den = want[:, 3].abs().clamp_min(1e-2 * float(want[:, 3].abs().max()))
    es, e32 = ((y[:, 3] - want[:, 3]).abs() / den), ((o32[:, 3] - want[:, 3]).abs() / den)
    assert float(es.max()) <= 4.0 * float(e32.max()) and float(es.mean()) <= 2.0 * float(e32.mean()), \
        f"s={s:g}: sigma rel. error max {float(es.max()):.2e} mean {float(es.mean()):.2e} vs float32 oracle " \
        f"{float(e32.max()):.2e} / {float(e32.mean()):.2e}"
    er, er32 = (y[:, :3] - want[:, :3]).abs(), (o32[:, :3] - want[:, :3]).abs()
    assert float(er.max()) <= 4.0 * float(er32.max()) + 1e-7, (s, float(er.max()), float(er32.max()))


def test_fp16x3_out_of_range_is_detected_and_rerun_in_bf16x3(dev):
    """Hidden activations beyond 65504 cannot be held in fp16 parts: the kernels raise the device status word, the
    host re-runs the call in bf16x3 (float32's range) with a RuntimeWarning, and the result is finite and correct
    to bf16x3's accuracy - never inf / NaN, never silent."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.render import rendering as Rm
    L, D, R, S, NI = 8, 256, 96, 64, 128
    o, d, gen = orbit_rays(R, 12, 800, 1111.111)
    u, uf = torch.rand(R, generator=gen), torch.rand(R, NI, generator=gen)
    sd_c, sd_f = scaled_sd(L, D, 42, 4e5), scaled_sd(L, D, 43, 4e5)
    x = o[:, None, :] + d[:, None, :] * torch.linspace(2.0, 6.0, 16)[None, :, None]
    assert hidden_max(sd_f, x.reshape(-1, 3), L) > 2 * 65504.0
    kw = dict(near=2.0, far=6.0, n_samples=S, n_importance=NI, u=u, u_fine=uf, white_bkgd=True)
    truth = oracle(o, d, sd_c, sd_f, cfg_of(L), torch.float64, **kw)
    o32 = oracle(o, d, sd_c, sd_f, cfg_of(L), torch.float32, **kw)
    # (round 3's arithmetic, `act_scaling = False`: the scaled network of round 4 has no such limit - its own guard is
    # tested in test_scaled_fp16x3_*)
    mc, mf = hip_model(sd_c, L, D, dev, "fp16x3", act_scaling=False), hip_model(sd_f, L, D, dev, "fp16x3", act_scaling=False)
    est = Rm.StratifiedEstimator(2.0, 6.0, S, NI)
    assert ops.range_ok(dev)  # clean slate
    with pytest.warns(RuntimeWarning, match="fp16 range"):
        with torch.no_grad():
            hip = Rm.render_rays(o, d, est, mc, white_bkgd=True, device=dev, model_fine=mf, u=u.to(dev), u_fine=uf.to(dev))
    assert mc.precision == "bf16x3" and mf.precision == "bf16x3", "the models continue in the wide-range mode"
    assert_parity(hip, o32, truth, "after the bf16x3 re-run", factor=10.0, atol_scale=3.0)
    # the standalone NeRF.forward has the same guard
    m = hip_model(sd_f, L, D, dev, "fp16x3", act_scaling=False)
    pts = (torch.rand(500, 3, generator=gen) * 2 - 1).to(dev)
    dirs = torch.nn.functional.normalize(torch.randn(500, 3, generator=gen), dim=-1).to(dev)
    with pytest.warns(RuntimeWarning, match="fp16 range"):
        y = m(pts, dirs)
    assert m.precision == "bf16x3" and bool(torch.isfinite(y).all())
    want = O.nerf_forward({k: v.double() for k, v in sd_f.items()}, pts.cpu().double(), dirs.cpu().double(), **cfg_of(L))
    assert float((y.cpu().double() - want)[:, :3].abs().max()) < 1e-4
    # with the guard switched off nothing is read back and nothing is re-run (the caller's choice)
    m2 = hip_model(sd_f, L, D, dev, "fp16x3", act_scaling=False)
    m2.range_check = False
    m2(pts, dirs)
    assert m2.precision == "fp16x3" and not ops.range_ok(dev)  # ... but the device word still recorded it


def test_deferred_range_check_does_not_wait_per_call_and_is_never_silent(dev):
    """`range_check = "deferred"` (batch rendering in small launches): a call returns without
    waiting for the GPU; the NEXT call looks at the (asynchronously read back) word of the previous one, warns, switches
    the models to bf16x3 and renders correctly from then on; a chunked render_frame looks once at its end and renders
    the frame again.  In-range networks never warn."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.render import rendering as Rm
    L, D, R, S, NI = 8, 256, 96, 64, 128
    o, d, gen = orbit_rays(R, 12, 800, 1111.111)
    u, uf = torch.rand(R, generator=gen), torch.rand(R, NI, generator=gen)
    kw = dict(near=2.0, far=6.0, n_samples=S, n_importance=NI, u=u, u_fine=uf, white_bkgd=True)
    est = Rm.StratifiedEstimator(2.0, 6.0, S, NI)
    assert ops.range_ok(dev) and ops.range_poll(dev) == 0

    def models(scale):
        mc, mf = (hip_model(scaled_sd(L, D, sd_, scale), L, D, dev, "fp16x3", act_scaling=False) for sd_ in (42, 43))
        mc.range_check = mf.range_check = "deferred"
        mc.weight_check = mf.weight_check = False  # (scaled_sd's 1/s on the connection weights is not what is tested here)
        return mc, mf

    render = lambda mc, mf: Rm.render_rays(o, d, est, mc, white_bkgd=True, device=dev, model_fine=mf, u=u.to(dev), u_fine=uf.to(dev))
    mc, mf = models(1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with torch.no_grad():
            a, b = render(mc, mf), render(mc, mf)
    assert torch.equal(a[0][0], b[0][0]) and ops.range_poll(dev) == 0 and mc.precision == "fp16x3"
    mc, mf = models(4e5)
    with torch.no_grad():
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            render(mc, mf)  # overflows on the device; nobody has looked yet
        assert mc.precision == "fp16x3"
        with pytest.warns(RuntimeWarning, match="EARLIER render_rays call"):
            good = render(mc, mf)
    assert mc.precision == "bf16x3" and mf.precision == "bf16x3"
    sd_c, sd_f = scaled_sd(L, D, 42, 4e5), scaled_sd(L, D, 43, 4e5)
    truth = oracle(o, d, sd_c, sd_f, cfg_of(L), torch.float64, **kw)
    o32 = oracle(o, d, sd_c, sd_f, cfg_of(L), torch.float32, **kw)
    assert_parity(good, o32, truth, "after the deferred fallback", factor=10.0, atol_scale=3.0)
    assert ops.range_poll(dev) == 0 and ops.range_ok(dev)
    # chunked frame (foreign estimator path is not needed: an NDC frame goes through get_rays -> to_ndc -> chunks)
    mc, mf = models(4e5)
    pose = torch.eye(4)
    with torch.no_grad():
        with pytest.warns(RuntimeWarning, match="end of the frame"):
            img, depth = Rm.render_frame((24, 32, 30.0), 0.0, 1.0, pose, 256, Rm.StratifiedEstimator(0.0, 1.0, 32, 32), mc,
                                         ndc=True, white_bkgd=True, device=dev, model_fine=mf)
    assert mc.precision == "bf16x3" and bool(torch.isfinite(img).all()) and bool(torch.isfinite(depth).all())
    assert ops.range_poll(dev) == 0 and ops.range_ok(dev)


# ------------------------------------------------------------------ round 4: the scaled network's own guard
def drift_(m, s, D=256):
    """scaled_sd's transformation applied IN PLACE to a live model: every hidden activation x s, outputs unchanged."""
    with torch.no_grad():
        m.layers[0].weight.mul_(s)
        for l in m.layers:
            l.bias.mul_(s)
        m.layers[5].weight[:, D:].mul_(s)  # the skip layer's x_in columns
        m.sigma.weight.div_(s)
        m.connection.weight.div_(s)


def test_scaled_fp16x3_drift_after_calibration_is_detected_and_recalibrated(dev):
    """"a network whose scale drifts after calibration is REPORTED (the two-sided guard)".  The
    per-layer scales of the fp16x3 inference path are calibrated once; when the weights then change under them (training,
    in-place edits) the packed network is re-packed with the OLD scales.  Hidden activations 1e3 x larger reach fp16
    infinity (bit 0), 1e9 x smaller fall below a wavefront maximum of 2^-4 (bit 1): either way the launch says so, the
    host re-calibrates on the call's own inputs and re-runs - fp16x3 is kept, the result is float32-grade, inf / NaN or a
    low-precision result is never returned, and `range_events` counts the event.  With `range_check = False` nothing
    is looked at (the caller's choice) and the device word keeps the record."""
    from fs_nerf_amd import ops
    L, D, n = 8, 256, 6000
    gen = torch.Generator().manual_seed(4)
    x = (torch.rand(n, 3, generator=gen) * 3.0 - 1.5).to(dev)
    dv = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1).to(dev)
    m = hip_model(make_sd(L, D, 42), L, D, dev, "fp16x3")
    assert ops.range_ok(dev)

    def check(y, what):
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        want = O.nerf_forward({k: v.double() for k, v in sd.items()}, x.cpu().double(), dv.cpu().double(), **cfg_of(L))
        o32 = O.nerf_forward(sd, x.cpu(), dv.cpu(), **cfg_of(L)).double()
        assert bool(torch.isfinite(y).all()), what
        e, e32 = (y.cpu().double() - want).abs(), (o32 - want).abs()
        den = want[:, 3].abs().clamp_min(1e-2 * float(want[:, 3].abs().max()))
        assert float((e[:, 3] / den).max()) <= 4.0 * float((e32[:, 3] / den).max()), what + ": sigma"
        assert float(e[:, :3].max()) <= 4.0 * float(e32[:, :3].max()) + 1e-7, what + ": rgb"

    with warnings.catch_warnings():
        warnings.simplefilter("error")  # re-calibration is not a warning; a bf16x3 fall-back would be
        with torch.no_grad():
            check(m(x, dv), "fresh calibration")
            assert m.calibrations == 1 and m.range_events == 0 and m.precision == "fp16x3"
            for s in (1e3, 1e-9):
                e_old, ev, cal = list(m.act_state.exps), m.range_events, m.calibrations
                drift_(m, s)
                y = m(x, dv)
                assert m.precision == "fp16x3" and m.range_events == ev + 1 and m.calibrations == cal + 1, f"drift x{s:g}"
                shift = [en - eo for en, eo in zip(m.act_state.exps[:L], e_old[:L])]
                assert all(abs(sh + np.log2(s)) <= 1.0 for sh in shift), (s, shift)
                check(y, f"after a drift of x{s:g}")
                assert ops.range_ok(dev)
            # an in-envelope drift (x 1/8: layer maxima at 2^7) needs nothing
            ev = m.range_events
            drift_(m, 0.125)
            check(m(x, dv), "in-envelope drift")
            assert m.range_events == ev
    # a probe that does not cover the data (here: a calibration target with no headroom at all) moves the target
    m2 = hip_model(make_sd(L, D, 43), L, D, dev, "fp16x3")
    m2.act_target_exp = 17
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with torch.no_grad():
            check2 = m2(x, dv)
    assert m2.act_target_exp == 13 and m2.range_events == 1 and m2.precision == "fp16x3" and bool(torch.isfinite(check2).all())
    # the caller's choice not to look
    m3 = hip_model(make_sd(L, D, 42), L, D, dev, "fp16x3")
    with torch.no_grad():
        m3(x, dv)
        drift_(m3, 1e3)
        m3.range_check = False
        m3(x, dv)
    assert m3.range_events == 0 and not ops.range_ok(dev)  # ... but the device word recorded it


def test_scaled_fp16x3_deferred_check_and_chunked_frames(dev):
    """The deferred range check with the scaled network: a drifted network's first call returns without anybody looking;
    the NEXT call warns that the earlier outputs are invalid, re-calibrates and is correct.  And ADVICE r3 (medium): a
    chunked frame in which an EARLY chunk leaves the envelope - the following chunk's poll consumes its flag - must still
    be rendered again as a whole (round 3 returned the invalid chunk inside the image)."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.render import rendering as Rm
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    L, D, R, S, NI = 8, 256, 96, 64, 128
    o, d, gen = orbit_rays(R, 12, 800, 1111.111)
    u, uf = torch.rand(R, generator=gen), torch.rand(R, NI, generator=gen)
    est = Rm.StratifiedEstimator(2.0, 6.0, S, NI)
    mc, mf = hip_model(make_sd(L, D, 42), L, D, dev, "fp16x3"), hip_model(make_sd(L, D, 43), L, D, dev, "fp16x3")
    mc.range_check = mf.range_check = "deferred"
    assert ops.range_ok(dev) and ops.range_poll(dev) == 0
    render = lambda: Rm.render_rays(o, d, est, mc, white_bkgd=True, device=dev, model_fine=mf, u=u.to(dev), u_fine=uf.to(dev))
    with torch.no_grad():
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            a, b = render(), render()
            assert torch.equal(a[0][0], b[0][0]) and mc.range_events == 0
            drift_(mc, 1e3), drift_(mf, 1e3)
            render()  # overflows on the device; nobody has looked yet
        assert mc.range_events == 0
        with pytest.warns(RuntimeWarning, match="EARLIER render_rays call"):
            good = render()
    assert mc.precision == "fp16x3" and mf.precision == "fp16x3" and mc.range_events == 1 and mf.range_events == 1
    kw = dict(near=2.0, far=6.0, n_samples=S, n_importance=NI, u=u, u_fine=uf, white_bkgd=True)
    sd_c, sd_f = ({k: v.detach().cpu() for k, v in m_.state_dict().items()} for m_ in (mc, mf))
    truth = oracle(o, d, sd_c, sd_f, cfg_of(L), torch.float64, **kw)
    o32 = oracle(o, d, sd_c, sd_f, cfg_of(L), torch.float32, **kw)
    assert_parity(good, o32, truth, "after the deferred re-calibration", factor=3.0)
    assert ops.range_poll(dev) == 0 and ops.range_ok(dev)
    # chunked frame through the occupancy estimator (NDC: get_rays -> to_ndc -> chunks -> one fused launch per chunk);
    # round 3's arithmetic at 4e5 x the default scale overflows in EVERY chunk it runs - chunk 1 posts the flag, chunk 2's
    # poll consumes it and switches to bf16x3, the end-of-frame look finds nothing pending
    occ = OccGridEstimator(roi_aabb=torch.tensor([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]), resolution=16, levels=1).to(dev)
    occ.set_binaries(torch.ones(1, 16, 16, 16, dtype=torch.bool))
    occ.eval()
    hwf, pose = (24, 32, 30.0), torch.eye(4)
    frame = lambda m_: Rm.render_frame(hwf, 0.0, 1.0, pose, 256, occ, m_, ndc=True, white_bkgd=True, render_step_size=0.05, device=dev)
    bad = hip_model(scaled_sd(L, D, 42, 4e5), L, D, dev, "fp16x3", act_scaling=False)
    bad.range_check, bad.weight_check = "deferred", False
    with torch.no_grad():
        with pytest.warns(RuntimeWarning):
            img, depth = frame(bad)
        assert bad.precision == "bf16x3" and bool(torch.isfinite(img).all()) and bool(torch.isfinite(depth).all())
        ref_m = hip_model(scaled_sd(L, D, 42, 4e5), L, D, dev, "bf16x3")
        img_ref, depth_ref = frame(ref_m)
    assert torch.equal(img, img_ref) and torch.equal(depth, depth_ref), "the frame is the bf16x3 frame, chunk 1 included"
    assert ops.range_poll(dev) == 0 and ops.range_ok(dev)


def test_deferred_single_launch_frame_recalibrates_on_its_own_rays(dev):
    """`render_frame` as ONE launch under the deferred range check, with a calibration that does not fit the frame: the
    network's raw-position columns dominate layer 0 and the frame's rays reach 20,000 x the default probe's box, so the
    scales measured on the default probe overflow at once.  The one look per frame finds the flag, re-calibrates on the
    FRAME'S OWN rays (not on the default probe again, where three target moves would not have reached) and looks at the
    repeat too: the frame that is returned is valid - equal, to float32 grade, to the frame of the synchronous guard."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.render import rendering as Rm
    L, D = 8, 256
    sd = make_sd(L, D, 42)
    sd["layers.0.weight"][:, :3] *= 64.0
    # (a scene the float32 reference itself can render out there: a constant small density - a raw density of -1e5 over an
    # interval of 625 is exp(+inf) in any arithmetic; make_sd's layers attenuate, so the colours do not saturate)
    sd["sigma.weight"].zero_()
    sd["sigma.bias"].fill_(0.002)
    est = Rm.StratifiedEstimator(2.0, 40000.0, 64, 0)
    hwf, pose = (24, 32, 30.0), torch.eye(4)
    frame = lambda m_: Rm.render_frame(hwf, 2.0, 40000.0, pose, 1 << 20, est, m_, white_bkgd=True, device=dev)
    m = hip_model(sd, L, D, dev, "fp16x3")
    m.calibrate()  # default probe: positions in [-2, 2]^3
    m.range_check = "deferred"
    ref = hip_model(sd, L, D, dev, "fp16x3")  # synchronous guard: calibrates on the frame's rays in its first call
    assert ops.range_poll(dev) == 0
    with torch.no_grad():
        with pytest.warns(RuntimeWarning, match="re-calibrated"):
            img, depth = frame(m)
        img_ref, depth_ref = frame(ref)
    assert m.precision == "fp16x3" and ref.precision == "fp16x3" and m.range_events >= 1
    assert bool(torch.isfinite(img).all()) and bool(torch.isfinite(depth).all()) and float(img.std()) > 0.02
    assert torch.allclose(img, img_ref, rtol=1e-4, atol=2e-5) and torch.allclose(depth, depth_ref, rtol=1e-4, atol=1e-3)
    assert ops.range_poll(dev) == 0 and ops.range_ok(dev)
    # new weights forget the target moves the old ones needed
    moved = m.act_target_exp
    m.load_state_dict(make_sd(L, D, 43))
    assert m.act_target_exp == m.ACT_TARGET_EXP and (moved == m.ACT_TARGET_EXP or m.act_state.moved_by == 0)


# ------------------------------------------------------------------ BASELINE config 5: bf16 weights / activations
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_config5_single_pass_vs_rounding_emulating_oracle(dev, prec):
    """configs[4]: 1600x1600-style rays, 128+256 samples, bf16 weights/activations.  Oracle = the same math with the
    16-bit operand rounding emulated on the CPU (oracle.nerf_forward(emulate=...)).  The kernel and
    the emulation differ only in float32 summation order - and in the few operands that such a last-bit difference
    pushes across a 16-bit rounding boundary (one bf16 ulp = 2^-8 of that activation), so the tolerance is stated
    per output: coarse weights / rgb_map / opacity 2e-3 (bf16), 3e-4 (fp16) absolute on [0,1] quantities - against
    3e-2 when the float32 oracle was the yardstick."""
    from fs_nerf_amd.render import rendering as Rm
    L, D, R, S, NI = 8, 256, 128, 128, 256
    o, d, gen = orbit_rays(R, 5, 1600, 2222.2)
    sd_c, sd_f = make_sd(L, D, 42), make_sd(L, D, 43)
    mc, mf = hip_model(sd_c, L, D, dev, prec), hip_model(sd_f, L, D, dev, prec)
    est = Rm.StratifiedEstimator(2.0, 6.0, S, NI)
    with torch.no_grad():
        out = Rm.render_rays(o, d, est, mc, white_bkgd=True, device=dev, model_fine=mf)
    (rgb, op, dep, ex), ri, tv = out
    assert ex["weights"].shape == (R * (S + NI),) and ex["edges"].shape == (R, S + NI + 1)
    kw = dict(near=2.0, far=6.0, n_samples=S, n_importance=NI, white_bkgd=True, emulate=prec)
    emu = O.render_rays_oracle(o, d, sd_c, sd_f, cfg_of(L), **kw)
    tol = {"bf16": 2e-3, "fp16": 3e-4}[prec]
    wc = emu[0][3]["weights_coarse"]
    assert float((ex["weights_coarse"].cpu() - wc).abs().max()) <= tol, "coarse pass vs the emulating oracle"
    # fine pass + integration on the kernel's own sample set (resampling amplifies a coarse-weight ulp in empty space)
    emu2 = O.render_rays_oracle(o, d, sd_c, sd_f, cfg_of(L), edges_override=ex["edges"].cpu(), **kw)
    assert float((rgb.cpu() - emu2[0][0]).abs().max()) <= tol, "rgb_map"
    assert float((op.cpu() - emu2[0][1]).abs().max()) <= tol, "opacity"
    assert float((ex["weights"].cpu().reshape(R, -1) - emu2[0][3]["weights"]).abs().max()) <= tol, "weights"
    # and end to end against the float32 oracle, the mode's own (stated) accuracy: 8 / 11 mantissa bits
    o32 = O.render_rays_oracle(o, d, sd_c, sd_f, cfg_of(L), near=2.0, far=6.0, n_samples=S, n_importance=NI,
                               white_bkgd=True)
    assert float((rgb.cpu() - o32[0][0]).abs().max()) <= {"bf16": 2e-3, "fp16": 3e-4}[prec] * 4


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_config5_end_to_end_bound_on_every_output(dev, prec):
    """configs[4] END TO END - coarse pass, resampling on the kernel's OWN coarse weights, fine pass,
    integration, nothing handed over - with a bound on weights and depth_map too.  Yardstick: the rounding-emulating
    oracle evaluated in float64 (operands rounded to the 16-bit format, products and sums exact to double: the
    arithmetic the mode DEFINES) against the same oracle in float32 (one legitimate float32 evaluation of that
    definition: its distance from the float64 one is what summation order and the last-bit rounding flips it causes
    are worth, resampling amplification included).  The kernel is another float32 evaluation (own summation order,
    hardware sine in the encodings): its error against the float64 emulation must be of that size - max and 99th
    percentile within 2 x the float32 emulation's (+ the floors of the parity criterion), per output.  (Measured:
    0.8 - 1.5 x on every output, e.g. bf16 weights 4.1e-4 against 4.2e-4, depth 1.4e-4 against 9.8e-5.)"""
    from fs_nerf_amd.render import rendering as Rm
    L, D, R, S, NI = 8, 256, 128, 128, 256
    o, d, gen = orbit_rays(R, 5, 1600, 2222.2)
    u, uf = torch.rand(R, generator=gen), torch.rand(R, NI, generator=gen)
    sd_c, sd_f = make_sd(L, D, 42), make_sd(L, D, 43)
    mc, mf = hip_model(sd_c, L, D, dev, prec), hip_model(sd_f, L, D, dev, prec)
    est = Rm.StratifiedEstimator(2.0, 6.0, S, NI)
    with torch.no_grad():
        hip = Rm.render_rays(o, d, est, mc, white_bkgd=True, device=dev, model_fine=mf, u=u.to(dev), u_fine=uf.to(dev))
    kw = dict(near=2.0, far=6.0, n_samples=S, n_importance=NI, u=u, u_fine=uf, white_bkgd=True, emulate=prec)
    emu64 = oracle(o, d, sd_c, sd_f, cfg_of(L), torch.float64, **kw)
    emu32 = oracle(o, d, sd_c, sd_f, cfg_of(L), torch.float32, **kw)
    H, P, T = outputs(hip), outputs(emu32), outputs(emu64)
    worst = {}
    for k in ("rgb_map", "depth_map", "weights", "opacity"):
        eh, ep = np.abs(H[k] - T[k]), np.abs(P[k] - T[k])
        fl = FLOOR[k] * 10
        worst[k] = (float(eh.max()), float(ep.max()), float(np.percentile(eh, 99)), float(np.percentile(ep, 99)))
        assert eh.max() <= 2.0 * ep.max() + fl and np.percentile(eh, 99) <= 2.0 * np.percentile(ep, 99) + fl, \
            f"{prec} {k}: max / p99 error vs the float64 emulation {eh.max():.2e} / {np.percentile(eh, 99):.2e}, the " \
            f"float32 emulation's {ep.max():.2e} / {np.percentile(ep, 99):.2e}"
    print("config5", prec, {k: tuple(f"{x:.1e}" for x in v) for k, v in worst.items()})


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_single_pass_two_groups_per_wave_ragged_shapes(dev, prec):
    """The single-pass modes of 256-wide networks run 32 samples per wave in 256-sample tiles (two 16-sample groups
    sharing every weight operand): sizes that end inside a group, a wave or a tile, ray counts below the rays of one
    workgroup, sample counts that do not divide the tile - each against the rounding-emulating oracle."""
    from fs_nerf_amd.render import rendering as Rm
    L, D = 8, 256
    sd = make_sd(L, D, 42)
    m = hip_model(sd, L, D, dev, prec)
    tol = {"bf16": 2e-3, "fp16": 3e-4}[prec]
    gen = torch.Generator().manual_seed(11)
    for n in (1, 15, 17, 255, 256, 257, 700):
        x = torch.rand(n, 3, generator=gen) * 3 - 1.5
        dv = torch.nn.functional.normalize(torch.randn(n, 3, generator=gen), dim=-1)
        with torch.no_grad():
            y4 = m(x.to(dev), dv.to(dev)).cpu()
            y1 = m(x.to(dev)).cpu()
            y4b, y1b = m(x.to(dev), dv.to(dev)).cpu(), m(x.to(dev)).cpu()
        assert torch.equal(y4, y4b) and torch.equal(y1, y1b), f"n={n}: not reproducible from launch to launch"
        e4 = O.nerf_forward(sd, x, dv, emulate=prec, **cfg_of(L))
        assert y4.shape == (n, 4) and y1.shape == (n, 1)
        # rgb in [0,1]: tol.  sigma: the test nets' density head has a x64 gain, so one flipped 16-bit rounding of a
        # hidden activation moves it by up to ~16 tol (its effect on a weight, sigma x interval length, is what the
        # render checks below and the config-5 test bound by tol)
        assert float((y4[:, :3] - e4[:, :3]).abs().max()) <= tol, f"n={n} rgb"
        assert float((y4[:, 3] - e4[:, 3]).abs().max()) <= 16 * tol, f"n={n} sigma"
        assert float((y1[:, 0] - e4[:, 3]).abs().max()) <= 16 * tol, f"n={n} density-only pass"
        assert float((y1[:, 0] - y4[:, 3]).abs().max()) == 0.0, f"n={n} density-only pass == full pass sigma"
    sd_f = make_sd(L, D, 43)
    mf = hip_model(sd_f, L, D, dev, prec)
    for R, S, NI in ((1, 64, 128), (3, 96, 32), (5, 128, 256), (7, 40, 0), (9, 200, 56)):
        o, d, _ = orbit_rays(R, 3 + R, 400, 555.5)
        est = Rm.StratifiedEstimator(2.0, 6.0, S, NI)
        with torch.no_grad():
            (rgb, op, dep, ex), _, _ = Rm.render_rays(o, d, est, m, white_bkgd=True, device=dev, model_fine=mf if NI else None)
        kw = dict(near=2.0, far=6.0, n_samples=S, n_importance=NI, white_bkgd=True, emulate=prec)
        emu = O.render_rays_oracle(o, d, sd, sd_f if NI else None, cfg_of(L), edges_override=ex["edges"].cpu() if NI else None, **kw)
        what = f"R={R} S={S} NI={NI}"
        assert float((rgb.cpu() - emu[0][0]).abs().max()) <= tol, what + " rgb_map"
        assert float((op.cpu() - emu[0][1]).abs().max()) <= tol, what + " opacity"
        assert float((ex["weights"].cpu().reshape(R, -1) - emu[0][3]["weights"]).abs().max()) <= tol, what + " weights"


def test_config5_full_frame_1600_properties(dev):
    """BASELINE configs[4] at full size: 1600x1600, 128+256 samples, two 8x256 networks in bf16, one fused launch with
    the rays generated in it.  Size-independent properties on all 2,560,000 rays; 48 of them re-rendered alone must
    reproduce their pixels bit for bit and agree with the rounding-emulating oracle."""
    from fs_nerf_amd.render import rendering as Rm
    L, D, S, NI = 8, 256, 128, 256
    sd_c, sd_f = make_sd(L, D, 42), make_sd(L, D, 43)
    mc, mf = hip_model(sd_c, L, D, dev, "bf16"), hip_model(sd_f, L, D, dev, "bf16")
    est = Rm.StratifiedEstimator(2.0, 6.0, S, NI)
    pose = O.pose_from_spherical(4.0311289, 50.0, 77.0)
    hwf = (1600, 1600, 0.5 * 1600 / np.tan(0.5 * 0.6911112))
    with torch.no_grad():
        img, depth = Rm.render_frame(hwf, 2.0, 6.0, pose, 1 << 30, est, mc, white_bkgd=True, device=dev, model_fine=mf)
    assert img.shape == (1600, 1600, 3) and depth.shape == (1600, 1600)
    assert bool(torch.isfinite(img).all()) and bool(torch.isfinite(depth).all())
    assert float(depth.min()) >= 2.0 and float(depth.max()) <= 6.0
    assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0 + 1e-6
    o, d = Rm.U.get_rays(pose, hwf, dev)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    idx = torch.randperm(1600 * 1600, generator=torch.Generator().manual_seed(2))[:48].to(dev)
    with torch.no_grad():
        (rgb, op, dep, ex), _, _ = Rm.render_rays(o[idx], d[idx], est, mc, white_bkgd=True, device=dev, model_fine=mf)
    assert torch.equal(rgb, img.reshape(-1, 3)[idx]), "a ray renders the same alone and inside the frame"
    assert torch.equal(dep.reshape(-1).clamp(2.0, 6.0), depth.reshape(-1)[idx])
    with torch.no_grad():
        img2, _ = Rm.render_frame(hwf, 2.0, 6.0, pose, 1 << 30, est, mc, white_bkgd=True, device=dev, model_fine=mf)
    assert torch.equal(img, img2), "reproducible from launch to launch"
    w = ex["weights"].reshape(48, S + NI)
    assert float((w.sum(-1, keepdim=True) - op).abs().max()) < 1e-5, "opacity = sum of weights"
    assert bool((ex["edges"][:, 1:] >= ex["edges"][:, :-1]).all()), "sorted sample union"
    kw = dict(near=2.0, far=6.0, n_samples=S, n_importance=NI, white_bkgd=True, emulate="bf16")
    emu = O.render_rays_oracle(o[idx].cpu(), d[idx].cpu(), sd_c, sd_f, cfg_of(L), edges_override=ex["edges"].cpu(), **kw)
    assert float((rgb.cpu() - emu[0][0]).abs().max()) <= 2e-3, "rgb_map vs the emulating oracle"
    assert float((w.cpu() - emu[0][3]["weights"]).abs().max()) <= 2e-3, "weights vs the emulating oracle"


# ------------------------------------------------------------------ the headline configuration at full size
def test_full_frame_800_two_8x256_properties_and_parity(dev):
    """BASELINE configs[2] as bench.py runs it: an 800x800 frame, 64+128 samples, TWO 8x256 networks, one fused launch.
    Size-independent properties on all 640,000 rays plus the error-ratio parity check on 512 rays drawn from them."""
    from fs_nerf_amd.render import rendering as Rm
    L, D = 8, 256
    sd_c, sd_f = make_sd(L, D, 42), make_sd(L, D, 43)
    mc, mf = hip_model(sd_c, L, D, dev, "fp16x3"), hip_model(sd_f, L, D, dev, "fp16x3")
    est = Rm.StratifiedEstimator(2.0, 6.0, 64, 128)
    pose = O.pose_from_spherical(4.0311289, 50.0, 30.0)
    hwf = (800, 800, 0.5 * 800 / np.tan(0.5 * 0.6911112))
    with torch.no_grad():
        img, depth = Rm.render_frame(hwf, 2.0, 6.0, pose, 1 << 30, est, mc, white_bkgd=True, device=dev, model_fine=mf)
        img2, depth2 = Rm.render_frame(hwf, 2.0, 6.0, pose, 123457, est, mc, white_bkgd=True, device=dev, model_fine=mf)
    assert img.shape == (800, 800, 3) and depth.shape == (800, 800)
    assert bool(torch.isfinite(img).all()) and bool(torch.isfinite(depth).all())
    assert torch.equal(img, img2) and torch.equal(depth, depth2), "deterministic and chunking-invariant"
    assert float(depth.min()) >= 2.0 and float(depth.max()) <= 6.0
    assert float(img.min()) >= 0.0 and float(img.max()) <= 1.0 + 1e-6
    o, d = Rm.U.get_rays(pose, hwf, dev)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    idx = torch.randperm(640000, generator=torch.Generator().manual_seed(1))[:512]
    with torch.no_grad():
        sub = Rm.render_rays(o[idx.to(dev)], d[idx.to(dev)], est, mc, white_bkgd=True, device=dev, model_fine=mf)
    (rgb, op, dep, ex), _, _ = sub
    assert torch.equal(rgb, img.reshape(-1, 3)[idx.to(dev)]), "a ray renders the same alone and inside the frame"
    w = ex["weights"].reshape(512, 192)
    assert float((w.sum(-1, keepdim=True) - op).abs().max()) < 1e-5, "opacity = sum of weights"
    assert bool((ex["edges"][:, 1:] >= ex["edges"][:, :-1]).all()), "sorted sample union"
    oc, dc = o[idx.to(dev)].cpu(), d[idx.to(dev)].cpu()
    kw = dict(near=2.0, far=6.0, n_samples=64, n_importance=128, white_bkgd=True)
    truth = oracle(oc, dc, sd_c, sd_f, cfg_of(L), torch.float64, **kw)
    o32 = oracle(oc, dc, sd_c, sd_f, cfg_of(L), torch.float32, **kw)
    assert_parity(sub, o32, truth, "800x800 frame, 512 rays")


def test_rendering_accepts_int32_ray_indices_with_backward(dev):
    """nerfacc-style callers may pass int32 ray indices into `rendering`; forward and backward widen them instead of
    reinterpreting the buffer."""
    from fs_nerf_amd.render import rendering as Rm
    gen = torch.Generator().manual_seed(3)
    counts = torch.tensor([5, 0, 64, 17, 1])
    R, N = len(counts), int(counts.sum())
    ri64 = torch.repeat_interleave(torch.arange(R), counts)
    t0 = torch.arange(N) * 0.02 + torch.rand(N, generator=gen) * 0.01
    t1 = t0 + 0.02
    sig = (torch.rand(N, generator=gen) * 20.0)
    rgb = torch.rand(N, 3, generator=gen)
    outs = []
    for ri in (ri64, ri64.to(torch.int32)):
        s, c = sig.clone().to(dev).requires_grad_(True), rgb.clone().to(dev).requires_grad_(True)
        col, op, dep, ex = Rm.rendering(t0.to(dev), t1.to(dev), ri.to(dev), R, lambda a, b, i: (c, s),
                                        torch.ones(3, device=dev))
        (col.sum() + 0.5 * op.sum()).backward()
        outs.append((col.detach(), s.grad.clone(), c.grad.clone()))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    with pytest.raises((RuntimeError, TypeError)):
        Rm.rendering(t0.to(dev), t1.to(dev), ri64.to(dev).float(), R, lambda a, b, i: (rgb.to(dev), sig.to(dev)), None)


def test_two_phase_and_camera_modes_are_bitwise_the_plain_launch(dev):
    """The optional launch shapes change scheduling only: rays generated in the launch from the pose == get_rays
    tensors; "all coarse passes, then all fine passes" (edges handed over through HBM) == group by group."""
    from fs_nerf_amd import ops
    L, D = 4, 128
    mc, mf = hip_model(make_sd(L, D, 42), L, D, dev, "fp16x3"), hip_model(make_sd(L, D, 43), L, D, dev, "fp16x3")
    pose = O.pose_from_spherical(4.0311289, 50.0, 123.0)
    H, W, focal = 150, 201, 260.0
    kw = dict(near=2.0, far=6.0, n_samples=64, n_importance=128, bkgd=(1.0, 1.0, 1.0), want_extras=False)
    o, d = ops.get_rays(pose, H, W, focal, dev)
    base = ops.render_fused(mc.packed(), mf.packed(), o, d, two_phase=False, **kw)
    cam = ops.render_fused(mc.packed(), mf.packed(), None, None, camera=(pose, H, W, focal, 0, H, dev), two_phase=False, **kw)
    two = ops.render_fused(mc.packed(), mf.packed(), None, None, camera=(pose, H, W, focal, 0, H, dev), two_phase=True, **kw)
    rows = ops.render_fused(mc.packed(), mf.packed(), None, None, camera=(pose, H, W, focal, 40, 30, dev), two_phase=True, **kw)
    for k in range(3):
        assert torch.equal(base[k], cam[k]) and torch.equal(base[k], two[k])
        assert torch.equal(rows[k], base[k][40 * W:70 * W]), "a row block of the frame (a rank's shard)"
    ex = ops.render_fused(mc.packed(), mf.packed(), o, d, two_phase=True, near=2.0, far=6.0, n_samples=64,
                          n_importance=128, bkgd=(1.0, 1.0, 1.0), want_extras=True)
    ex1 = ops.render_fused(mc.packed(), mf.packed(), o, d, two_phase=False, near=2.0, far=6.0, n_samples=64,
                           n_importance=128, bkgd=(1.0, 1.0, 1.0), want_extras=True)
    for k in ("weights", "edges", "weights_coarse", "rgbs"):
        assert torch.equal(ex[3][k], ex1[3][k]), k


@pytest.mark.gpu
def test_weights_below_the_fp16_envelope_are_reported(dev):
    """A layer whose LARGEST weight is below 2^-20 (high parts deep in fp16's subnormals: fewer than 15 bits relative to
    the layer's weights): the weights' own check at pack time reports it - bf16x3 with a warning, never silently."""
    sd = make_sd(8, 256, 42)
    sd["layers.2.weight"] = sd["layers.2.weight"] * 1e-5   # largest entry ~6e-7
    sd["layers.2.bias"] = sd["layers.2.bias"] * 1e-5
    sd["layers.3.weight"] = sd["layers.3.weight"] * 1e5    # the next layer brings the scale back
    m = hip_model(sd, 8, 256, dev, "fp16x3", act_scaling=False)
    x = torch.rand(500, 3) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(500, 3), dim=-1)
    with pytest.warns(RuntimeWarning, match="largest weight is below"):
        with torch.no_grad():
            y = m(x.to(dev), d.to(dev))
    assert m.precision == "bf16x3"
    want = O.nerf_forward({k: v.double() for k, v in sd.items()}, x.double(), d.double(), **cfg_of(8))
    assert float((y.cpu().double() - want).abs().max()) < 2e-3 * max(1.0, float(want.abs().max()))
    ok = hip_model(make_sd(8, 256, 42), 8, 256, dev, "fp16x3", act_scaling=False)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        with torch.no_grad():
            ok(x.to(dev), d.to(dev))
            # the scaled network of round 4 takes the tiny layer in its stride: the layer's scale brings it back
            ms = hip_model(sd, 8, 256, dev, "fp16x3")
            ys = ms(x.to(dev), d.to(dev))
    assert ok.precision == "fp16x3" and ms.precision == "fp16x3" and ms.range_events == 0
    o32 = O.nerf_forward(sd, x, d, **cfg_of(8)).double()
    assert float((ys.cpu().double() - want).abs().max()) <= 4.0 * float((o32 - want).abs().max()) + 1e-7
