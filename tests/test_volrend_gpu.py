"""GPU: the packed volume-rendering primitives (csrc/packed_scan.hip, render/volrend.py) and `rendering(rgb_alpha_fn=)`
against the compositor's own kernels (bit for bit) and the float64 restatements of tests/volrend_ref.py, whose autograd
is the truth for every gradient.

Inputs: volrend_ref.density_case / alpha_case - 70 rays x S in {5, 64, 65, 192} (fewer samples than lanes, one per lane,
a ragged last lane, three per lane), 20 % of the samples dropped, ray 3 empty, ray 7 all-zero sigma, 5 % negative
values, one alpha of exactly 1.0 in the middle of ray 11 - and dense_case (9 full rows) where the three addressing modes
must describe the same rays.  Metric: test_train_step._rel, max |a - b| / max |b|; bars 1e-5 (forward values) and 2e-4
(gradients), the project's own for this arithmetic class (tests/test_composite_grad_gpu.py).  Every figure is printed
before it is asserted.  Measured on the MI355X: every forward figure of this file at or below 3.2e-7, every gradient
figure at or below 3.9e-7 (the product scans' dense backward), the integration test's colours, opacity and depth
identical to rendering()'s; no sample of the visibility check lies within 1e-6 of a threshold.  Two equalities hold by
construction and are pinned with torch.equal: the dense compositor against the packed one (one kernel), the density
form's weights backward against the compositor backward (one device routine)."""
import functools

import pytest
import torch

import fs_nerf_amd  # noqa: F401

import composite_ref as CR
import volrend_ref as VR
from test_train_step import _rel

SIZES = VR.SIZES
TOL_GRAD, TOL_FWD = 2e-4, 1e-5
BK = torch.tensor([1.0, 0.5, 0.25])
SCANS = [("inclusive_sum", False, False), ("exclusive_sum", False, True), ("inclusive_prod", True, False),
         ("exclusive_prod", True, True)]


def _dev():
    return torch.device("cuda:0")


def _g(t):
    return t.to(_dev())


def _check(label, got, ref, tol):
    e = _rel(got, ref)
    print(f"{label}: {e:.3e}")
    assert bool(torch.isfinite(got).all()), label
    assert e < tol, (label, e)


@functools.lru_cache(maxsize=None)
def _density(S):
    """the density case on the device with the compositor's forward: built once per size, never modified"""
    from fs_nerf_amd import ops
    case = VR.density_case(S)
    g = {k: _g(case[k]) for k in ("sig", "rgb", "t0", "t1", "ri", "prefix")}
    _, _, _, ex = ops.composite_packed(g["sig"], g["rgb"], g["t0"], g["t1"], g["ri"], case["R"], None)
    return case, g, ex


@functools.lru_cache(maxsize=None)
def _alpha_reference(S, which, prefix):
    """float64 autograd from the SAME float32 alphas -> (weights, trans, d_alphas)"""
    case = VR.alpha_case(S)
    a = case["alphas"].double().requires_grad_(True)
    w, tr = VR.weights_from_alpha(a, case["ri"], case["R"], case["prefix"].double() if prefix else None)
    loss = sum((out * case[c].double()).sum() for out, c, k in ((w, "g", "weights"), (tr, "g2", "trans")) if k in which)
    return w.detach(), tr.detach(), torch.autograd.grad(loss, a)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
def test_density_form_equals_the_compositor_bit_for_bit(S):
    from fs_nerf_amd import ops
    from fs_nerf_amd.render import volrend as V
    case, g, ex = _density(S)
    R = case["R"]
    info = V.pack_info(g["ri"], R)
    for kw in (dict(ray_indices=g["ri"], n_rays=R), dict(packed_info=info), dict(ray_indices=g["ri"])):
        w, tr, al = V.render_weight_from_density(g["t0"], g["t1"], g["sig"], **kw)
        assert torch.equal(w, ex["weights"]) and torch.equal(tr, ex["trans"]) and torch.equal(al, ex["alphas"]), list(kw)
        tr2, al2 = V.render_transmittance_from_density(g["t0"], g["t1"], g["sig"], **kw)
        assert torch.equal(tr2, ex["trans"]) and torch.equal(al2, ex["alphas"])
        for eps, thre in ((1e-4, 0.01), (1e-4, 0.0), (0.3, 0.2)):
            keep = V.render_visibility_from_density(g["t0"], g["t1"], g["sig"], early_stop_eps=eps, alpha_thre=thre, **kw)
            want = ops.packed_visibility(g["sig"], g["t0"], g["t1"], g["ri"], R, eps, thre)
            assert keep.dtype == torch.bool and torch.equal(keep, want), (eps, thre)
    assert 0 < int(want.sum()) < want.numel()
    ref = CR.forward64(case, None)
    for k, v in (("weights", w), ("trans", tr), ("alphas", al)):
        _check(f"S={S} forward {k}", v, ref[k], TOL_FWD)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1] + SIZES)
def test_dense_compositor_equals_the_packed_one_bit_for_bit(S):
    """one kernel behind both entry points: dense rows [9, S] and the same samples flattened under ray_indices"""
    from fs_nerf_amd import ops
    case = VR.dense_case(S)
    R = case["R"]
    rgb = torch.rand(R * S, 3, generator=torch.Generator().manual_seed(600 + S))
    sig, t0, t1, rgb = (_g(t) for t in (case["sig"], case["t0"], case["t1"], rgb))
    dense = ops.composite(sig.reshape(R, S), rgb.reshape(R, S, 3), t0.reshape(R, S), t1.reshape(R, S), _g(BK))
    ri = torch.arange(R).repeat_interleave(S)
    packed = ops.composite_packed(sig, rgb, t0, t1, _g(ri), R, _g(BK))
    for name, a, b in zip(("colors", "opacity", "depth"), dense, packed):
        assert torch.equal(a, b), name
    for k in ("weights", "alphas", "trans"):
        assert dense[3][k].shape == (R, S) and torch.equal(dense[3][k].reshape(-1), packed[3][k]), k
    assert float(packed[1].min()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("which", ["all", "weights", "trans", "alphas"])
def test_density_weights_backward_equals_the_compositor_backward_bit_for_bit(S, which):
    """one routine behind both: without a colour cotangent the compositor's q_i = 0 - 0 + 0 + u_i is u_i exactly, so
    d_sigmas agree to the bit (torch.equal: the two accumulate from a literal 0 in different places, +-0 alike)"""
    from fs_nerf_amd import ops
    case, g, _ = _density(S)
    cot = {k: (_g(v) if which in ("all", k) else None) for k, v in case["cot"].items()}
    spans = ops.RaySpans(case["sig"].numel(), case["R"], ray_indices=g["ri"])
    mine = ops.packed_weights_bwd(g["sig"], g["t0"], g["t1"], spans, False, None, cot["weights"], cot["trans"], cot["alphas"])
    theirs, _ = ops.composite_packed_bwd_full(g["sig"], g["rgb"], g["t0"], g["t1"], g["ri"], case["R"], None, None, None,
                                              d_weights=cot["weights"], d_alphas=cot["alphas"], d_trans=cot["trans"])
    assert torch.equal(mine, theirs) and float(mine.abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
def test_pack_info_is_exact(S):
    from fs_nerf_amd.render import volrend as V
    case = VR.alpha_case(S)
    want = torch.tensor([(a, b - a) for a, b in VR.ray_slices(case["ri"], case["R"])], dtype=torch.int64)
    info = V.pack_info(_g(case["ri"]), case["R"])
    assert info.dtype == torch.int64 and torch.equal(info.cpu(), want)
    assert int(info[CR.EMPTY_RAY, 1]) == 0 and int(info[CR.EMPTY_RAY, 0]) == int(info[CR.EMPTY_RAY + 1, 0])
    assert torch.equal(V.pack_info(_g(case["ri"])).cpu(), want[:int(case["ri"].max()) + 1])
    more = V.pack_info(_g(case["ri"]), case["R"] + 3).cpu()  # rays past the last index: empty, at the end
    assert torch.equal(more[:case["R"]], want) and torch.equal(more[case["R"]:], torch.tensor([[case["N"], 0]] * 3))
    none = V.pack_info(_g(case["ri"][:0]), 4)
    assert none.shape == (4, 2) and int(none.abs().max()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
def test_three_addressing_modes_give_identical_bits(S):
    """nothing dropped: ray_indices, packed_info (from pack_info) and dense rows describe the same rays"""
    from fs_nerf_amd.render import volrend as V
    case = VR.dense_case(S)
    R = case["R"]
    ri = _g(case["ri"])
    info = V.pack_info(ri, R)
    assert torch.equal(info.cpu(), torch.stack([torch.arange(R) * S, torch.full((R,), S)], 1))
    gcot = _g(case["g"])

    def three(fn, *flat):
        """fn(*tensors, **addressing) forward and backward (cotangent gcot on every output) under the three modes"""
        res = []
        for mode in ("ri", "info", "dense"):
            ins = [t.clone().requires_grad_(True) for t in flat]
            shaped = [t.reshape(R, S) for t in ins] if mode == "dense" else ins
            outs = fn(mode, *shaped)
            outs = outs if isinstance(outs, tuple) else (outs,)
            assert all(o.shape == shaped[0].shape for o in outs)
            sum((o.reshape(-1) * gcot).sum() for o in outs).backward()
            res.append([o.detach().reshape(-1) for o in outs] + [t.grad for t in ins])
        for other in res[1:]:
            assert all(torch.equal(a, b) for a, b in zip(res[0], other))
        return res[0]

    addr = lambda mode: {"ri": dict(ray_indices=ri, n_rays=R), "info": dict(packed_info=info), "dense": {}}[mode]
    t0, t1 = _g(case["t0"]), _g(case["t1"])
    tt = lambda mode, t: t.reshape(R, S) if mode == "dense" else t
    three(lambda m, s: V.render_weight_from_density(tt(m, t0), tt(m, t1), s, **addr(m)), _g(case["sig"]))
    three(lambda m, a: V.render_weight_from_alpha(a, **addr(m)), _g(case["alphas"]))
    saddr = lambda mode: {"ri": dict(indices=ri), "info": dict(packed_info=info), "dense": {}}[mode]
    for name, prod, _ in SCANS:
        out, _ = three(lambda m, x: getattr(V, name)(x, **saddr(m)), _g(case["x_prod" if prod else "x_sum"]))
        if name == "exclusive_prod":  # the dense tensor against the same data packed, and against float64
            _check(f"S={S} dense exclusive_prod", out, VR.scan(case["x_prod"].double(), case["ri"], R, True, True), TOL_FWD)
    keeps = [V.render_visibility_from_alpha(tt(m, _g(case["alphas"])), early_stop_eps=0.05, alpha_thre=0.01, **addr(m))
             for m in ("ri", "info", "dense")]
    assert keeps[2].shape == (R, S) and all(torch.equal(keeps[0], k.reshape(-1)) for k in keeps[1:])
    assert 0 < int(keeps[0].sum()) < keeps[0].numel()
    vals = torch.randn(R * S, 3, generator=torch.Generator().manual_seed(S)).to(ri.device)
    flat = V.accumulate_along_rays(_g(case["alphas"]), vals, ri, R)
    dense = V.accumulate_along_rays(_g(case["alphas"]).reshape(R, S), vals.reshape(R, S, 3))
    assert dense.shape == (R, 3) and torch.equal(flat, dense)


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("name,prod,exclusive", SCANS)
def test_scans_forward_and_backward(S, name, prod, exclusive):
    """packed (ragged rays, by indices and by packed_info) and dense, against float64; the product scans also on
    x = 1 - alphas, whose ray 11 holds a factor of exactly 0: that ray's gradient is finite and within the bar"""
    from fs_nerf_amd.render import volrend as V
    fn = getattr(V, name)
    case, dense = VR.alpha_case(S), VR.dense_case(S)
    R, ri = case["R"], case["ri"]
    info = V.pack_info(_g(ri), R)
    inputs = [("plain", case["x_prod" if prod else "x_sum"])] + ([("zero-factor", 1.0 - case["alphas"])] if prod else [])
    for label, x in inputs:
        x64 = x.double().requires_grad_(True)
        ref = VR.scan(x64, ri, R, prod, exclusive)
        (ref * case["g"].double()).sum().backward()
        eleven = ri == VR.ONE_RAY
        for mode, kw in (("indices", dict(indices=_g(ri))), ("packed_info", dict(packed_info=info))):
            xg = _g(x).requires_grad_(True)
            out = fn(xg, **kw)
            (out * _g(case["g"])).sum().backward()
            _check(f"S={S} {name} {label} {mode} forward", out, ref.detach(), TOL_FWD)
            _check(f"S={S} {name} {label} {mode} backward", xg.grad, x64.grad, TOL_GRAD)
            if label == "zero-factor":
                assert float(x[case["one"]]) == 0.0 and float(x64.grad[eleven].abs().max()) > 0
                _check(f"S={S} {name} {label} {mode} backward, ray 11", xg.grad[eleven], x64.grad[eleven], TOL_GRAD)
    x = dense["x_prod" if prod else "x_sum"]
    x64 = x.double().requires_grad_(True)
    ref = VR.scan(x64, dense["ri"], dense["R"], prod, exclusive)
    (ref * dense["g"].double()).sum().backward()
    xg = _g(x).reshape(dense["R"], S).requires_grad_(True)
    out = fn(xg)
    (out * _g(dense["g"]).reshape(dense["R"], S)).sum().backward()
    _check(f"S={S} {name} dense forward", out.reshape(-1), ref.detach(), TOL_FWD)
    _check(f"S={S} {name} dense backward", xg.grad.reshape(-1), x64.grad, TOL_GRAD)


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("which", ["weights", "trans", "alphas", "all"])
def test_from_density_backward_vs_float64_autograd(S, which):
    """cotangents on weights, trans and alphas, each alone and all together, against composite_ref.autograd_reference
    (float64 autograd on oracle.rendering_packed); ray 7 (all-zero sigma) measured on its own as well"""
    from fs_nerf_amd.render import volrend as V
    case, g, _ = _density(S)
    cot = case["cot"] if which == "all" else {which: case["cot"][which]}
    gs = CR.autograd_reference(case, cot, None)[0]
    sg = g["sig"].clone().requires_grad_(True)
    outs = dict(zip(("weights", "trans", "alphas"),
                    V.render_weight_from_density(g["t0"], g["t1"], sg, ray_indices=g["ri"], n_rays=case["R"])))
    sum((outs[k] * _g(v)).sum() for k, v in cot.items()).backward()
    seven = case["ri"] == CR.ZERO_RAY
    assert int(seven.sum()) > 0
    _check(f"S={S} from density, d_{which}", sg.grad, gs, TOL_GRAD)
    _check(f"S={S} from density, d_{which}, ray 7", sg.grad[seven], gs[seven], TOL_GRAD)
    if which == "all":  # the two-output form: the same kernel with d_weights NULL
        sg2 = g["sig"].clone().requires_grad_(True)
        tr, al = V.render_transmittance_from_density(g["t0"], g["t1"], sg2, packed_info=V.pack_info(g["ri"], case["R"]))
        ((tr * _g(cot["trans"])).sum() + (al * _g(cot["alphas"])).sum()).backward()
        gs2 = CR.autograd_reference(case, {k: cot[k] for k in ("trans", "alphas")}, None)[0]
        _check(f"S={S} transmittance from density, d_trans + d_alphas", sg2.grad, gs2, TOL_GRAD)


@pytest.mark.gpu
def test_prefix_trans_forward_and_backward():
    """S = 65, both forms: trans and weights carry the prefix, the gradient too, and none goes to the prefix"""
    from fs_nerf_amd.render import volrend as V
    S = 65
    case, g, _ = _density(S)
    R, ri = case["R"], case["ri"]
    s64 = case["sig"].double().requires_grad_(True)
    ref = VR.weights_from_density(s64, case["t0"].double(), case["t1"].double(), ri, R, case["prefix"].double())
    sum((o * case["cot"][k].double()).sum() for o, k in zip(ref, ("weights", "trans", "alphas"))).backward()
    sg, pg = g["sig"].clone().requires_grad_(True), g["prefix"].clone().requires_grad_(True)
    outs = V.render_weight_from_density(g["t0"], g["t1"], sg, ray_indices=g["ri"], n_rays=R, prefix_trans=pg)
    sum((o * _g(case["cot"][k])).sum() for o, k in zip(outs, ("weights", "trans", "alphas"))).backward()
    for o, r, k in zip(outs, ref, ("weights", "trans", "alphas")):
        _check(f"prefix, from density, forward {k}", o, r.detach(), TOL_FWD)
    _check("prefix, from density, d_sigmas", sg.grad, s64.grad, TOL_GRAD)
    assert pg.grad is None
    acase = VR.alpha_case(S)
    w64, tr64, ga = _alpha_reference(S, ("weights", "trans"), True)
    ag = _g(acase["alphas"]).requires_grad_(True)
    w, tr = V.render_weight_from_alpha(ag, ray_indices=_g(acase["ri"]), n_rays=R, prefix_trans=_g(acase["prefix"]))
    ((w * _g(acase["g"])).sum() + (tr * _g(acase["g2"])).sum()).backward()
    _check("prefix, from alpha, forward weights", w, w64, TOL_FWD)
    _check("prefix, from alpha, forward trans", tr, tr64, TOL_FWD)
    _check("prefix, from alpha, d_alphas", ag.grad, ga, TOL_GRAD)


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
def test_from_alpha_forward_backward_and_visibility(S):
    """against float64 autograd computed from the same float32 alphas; ray 11 (alpha == 1.0 in its middle) on its own"""
    from fs_nerf_amd.render import volrend as V
    case = VR.alpha_case(S)
    R, ri = case["R"], _g(case["ri"])
    eleven = case["ri"] == VR.ONE_RAY
    for which in (("weights",), ("trans",), ("weights", "trans")):
        w64, tr64, ga = _alpha_reference(S, which, False)
        ag = _g(case["alphas"]).requires_grad_(True)
        w, tr = V.render_weight_from_alpha(ag, ray_indices=ri, n_rays=R)
        sum((o * _g(case[c])).sum() for o, c, k in ((w, "g", "weights"), (tr, "g2", "trans")) if k in which).backward()
        _check(f"S={S} from alpha, forward weights", w, w64, TOL_FWD)
        _check(f"S={S} from alpha, forward trans", tr, tr64, TOL_FWD)
        _check(f"S={S} from alpha, d_{'+'.join(which)}", ag.grad, ga, TOL_GRAD)
        _check(f"S={S} from alpha, d_{'+'.join(which)}, ray 11", ag.grad[eleven], ga[eleven], TOL_GRAD)
        assert float(ga[eleven].abs().max()) > 0
    after = torch.nonzero(eleven).reshape(-1)
    after = after[after > case["one"]]
    assert float(tr.detach()[after].abs().max()) == 0.0 and float(w.detach()[after].abs().max()) == 0.0  # behind alpha == 1: exactly dark
    w64, tr64, ga = _alpha_reference(S, ("trans",), False)
    ag = _g(case["alphas"]).requires_grad_(True)
    tr = V.render_transmittance_from_alpha(ag, packed_info=V.pack_info(ri, R))
    (tr * _g(case["g2"])).sum().backward()
    _check(f"S={S} transmittance from alpha, forward", tr, tr64, TOL_FWD)
    _check(f"S={S} transmittance from alpha, d_trans", ag.grad, ga, TOL_GRAD)
    # the visibility rule, exactly, away from the thresholds
    eps, thre = 1e-4, 0.01
    a64 = case["alphas"].double()
    near = ((tr64 - eps).abs() <= 1e-6 * eps) | ((a64 - thre).abs() <= 1e-6 * thre)
    print(f"S={S} visibility: {int(near.sum())} of {near.numel()} samples within 1e-6 of a threshold")
    assert int(near.sum()) <= 0.01 * near.numel()
    keep = V.render_visibility_from_alpha(_g(case["alphas"]), ray_indices=ri, n_rays=R, early_stop_eps=eps, alpha_thre=thre)
    want = (tr64 >= eps) & (a64 >= thre)
    assert keep.dtype == torch.bool and torch.equal(keep.cpu()[~near], want[~near])
    assert 0 < int(want.sum()) < want.numel() and not bool(keep[after].any())


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("C", [1, 3, 7, None])
def test_accumulate_along_rays(S, C):
    from fs_nerf_amd.render import volrend as V
    case = VR.alpha_case(S)
    R, ri = case["R"], case["ri"]
    w = case["x_sum"]
    v = None if C is None else case["values"][C]
    gr = case["g_rays"][1 if C is None else C]
    w64 = w.double().requires_grad_(True)
    v64 = None if v is None else v.double().requires_grad_(True)
    ref = VR.accumulate(w64, v64, ri, R)
    (ref * gr.double()).sum().backward()
    wg = _g(w).requires_grad_(True)
    vg = None if v is None else _g(v).requires_grad_(True)
    out = V.accumulate_along_rays(wg, vg, _g(ri), R)
    assert out.shape == (R, 1 if C is None else C)
    (out * _g(gr)).sum().backward()
    _check(f"S={S} C={C} accumulate forward", out, ref.detach(), TOL_FWD)
    _check(f"S={S} C={C} accumulate d_weights", wg.grad, w64.grad, TOL_GRAD)
    if v is not None:
        _check(f"S={S} C={C} accumulate d_values", vg.grad, v64.grad, TOL_GRAD)
    assert float(out.detach()[CR.EMPTY_RAY].abs().max()) == 0.0 and float(ref.detach().abs().max()) > 0.1
    # weights alone require grad: d_values is not computed, and the other way round
    if v is not None:
        wg2 = _g(w).requires_grad_(True)
        (V.accumulate_along_rays(wg2, _g(v), _g(ri), R) * _g(gr)).sum().backward()
        assert torch.equal(wg2.grad, wg.grad)
        vg2 = _g(v).requires_grad_(True)
        (V.accumulate_along_rays(_g(w), vg2, _g(ri), R) * _g(gr)).sum().backward()
        assert torch.equal(vg2.grad, vg.grad)
    none = V.accumulate_along_rays(_g(w[:0]), None if v is None else _g(v[:0]), _g(ri[:0]), 5)
    assert none.shape == (5, 1 if C is None else C) and float(none.abs().max()) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("bkgd", [None, BK])
def test_rendering_with_rgb_alpha_fn(S, bkgd):
    """all four outputs and the extras against float64; gradients to rgbs and alphas through a loss on colours + depth
    + weights"""
    from fs_nerf_amd.render import rendering as Rm
    case = VR.alpha_case(S)
    R, ri = case["R"], case["ri"]
    gen = torch.Generator().manual_seed(500 + S)
    gc, gd = torch.randn(R, 3, generator=gen), torch.randn(R, 1, generator=gen)
    a64, c64 = case["alphas"].double().requires_grad_(True), case["rgb"].double().requires_grad_(True)
    ref = VR.rendering_from_alpha(c64, a64, case["t0"].double(), case["t1"].double(), ri, R, bkgd)
    assert float(ref[1].detach()[torch.arange(R) != CR.EMPTY_RAY].min()) > 0.05  # (depth carries 1 / opacity)
    ((ref[0] * gc.double()).sum() + (ref[2] * gd.double()).sum() + (ref[3] * case["g"].double()).sum()).backward()
    ag, cg = _g(case["alphas"]).requires_grad_(True), _g(case["rgb"]).requires_grad_(True)
    colors, opacity, depth, ex = Rm.rendering(_g(case["t0"]), _g(case["t1"]), _g(ri), R, rgb_alpha_fn=lambda a, b, c: (cg, ag),
                                              render_bkgd=None if bkgd is None else _g(bkgd))
    assert set(ex) == {"weights", "trans", "alphas", "rgbs"} and ex["alphas"] is ag and ex["rgbs"] is cg
    assert colors.shape == (R, 3) and opacity.shape == (R, 1) and depth.shape == (R, 1)
    assert all(t.requires_grad for t in (colors, opacity, depth, ex["weights"], ex["trans"]))
    ((colors * _g(gc)).sum() + (depth * _g(gd)).sum() + (ex["weights"] * _g(case["g"])).sum()).backward()
    for name, got, want in (("colors", colors, ref[0]), ("opacity", opacity, ref[1]), ("depth", depth, ref[2]),
                            ("weights", ex["weights"], ref[3]), ("trans", ex["trans"], ref[4])):
        _check(f"S={S} rgb_alpha_fn forward {name}", got, want.detach(), TOL_FWD)
    _check(f"S={S} rgb_alpha_fn d_alphas", ag.grad, a64.grad, TOL_GRAD)
    _check(f"S={S} rgb_alpha_fn d_rgbs", cg.grad, c64.grad, TOL_GRAD)
    want_empty = torch.zeros(3) if bkgd is None else bkgd
    assert torch.equal(colors.detach()[CR.EMPTY_RAY].cpu(), want_empty) and float(depth.detach()[CR.EMPTY_RAY]) == 0.0


@pytest.mark.gpu
def test_rendering_with_rgb_alpha_fn_on_an_all_empty_batch():
    from fs_nerf_amd.render import rendering as Rm
    dev = _dev()
    e = torch.zeros(0, device=dev)
    fn = lambda a, b, c: (torch.zeros(0, 3, device=dev, requires_grad=True), torch.zeros(0, device=dev, requires_grad=True))
    colors, opacity, depth, ex = Rm.rendering(e, e, torch.zeros(0, dtype=torch.int64, device=dev), 6, rgb_alpha_fn=fn,
                                              render_bkgd=_g(BK))
    assert torch.equal(colors.detach().cpu(), BK.expand(6, 3)) and float(depth.abs().max()) == 0.0
    assert float(opacity.abs().max()) == 0.0 and ex["weights"].numel() == 0
    colors.sum().backward()  # legal: the empty inputs carry the graph


@pytest.mark.gpu
def test_occupancy_samples_rerendered_by_the_primitives():
    """a sample set of OccGridEstimator.sampling (16^3, one level) through rendering(full_grad=False) and through
    render_weight_from_density + accumulate_along_rays: colours, opacity, depth within 1e-5, d_sigmas within 2e-4"""
    from fs_nerf_amd.render import rendering as Rm
    from fs_nerf_amd.render import volrend as V
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    from test_occgrid import AABB, _orbit_rays, _sphere_binaries
    dev = _dev()
    est = OccGridEstimator(roi_aabb=torch.tensor(AABB), resolution=16, levels=1).to(dev)
    est.set_binaries(_sphere_binaries(16, 1))
    R = 300
    o, d = (_g(t) for t in _orbit_rays(R, 2))
    ri, t0, t1 = est.sampling(o, d, render_step_size=2e-2)
    N = ri.numel()
    assert N > 5000 and int(torch.bincount(ri, minlength=R).min()) == 0  # some rays miss the sphere
    x = o[ri] + d[ri] * ((t0 + t1) / 2.0)[:, None]
    sig = (6.0 * torch.exp(-2.0 * (x * x).sum(-1)) * (1.0 + 0.5 * torch.sin(9.0 * x[:, 0]))).contiguous()
    rgb = torch.sigmoid(3.0 * x).contiguous()
    gen = torch.Generator().manual_seed(9)
    gc, go = _g(torch.randn(R, 3, generator=gen)), _g(torch.randn(R, 1, generator=gen))
    s1 = sig.clone().requires_grad_(True)
    colors, opacity, depth, _ = Rm.rendering(t0, t1, ri, R, rgb_sigma_fn=lambda a, b, c: (rgb, s1), render_bkgd=_g(BK))
    ((colors * gc).sum() + (opacity * go).sum()).backward()
    s2 = sig.clone().requires_grad_(True)
    w, _, _ = V.render_weight_from_density(t0, t1, s2, ray_indices=ri, n_rays=R)
    op2 = V.accumulate_along_rays(w, None, ri, R)
    col2 = V.accumulate_along_rays(w, rgb, ri, R) + _g(BK) * (1.0 - op2)
    dep2 = V.accumulate_along_rays(w, ((t0 + t1) / 2.0)[:, None], ri, R) / op2.clamp_min(CR.EPS)
    ((col2 * gc).sum() + (op2 * go).sum()).backward()
    _check("integration colours", col2, colors, TOL_FWD)
    _check("integration opacity", op2, opacity, TOL_FWD)
    _check("integration depth", dep2, depth, TOL_FWD)
    _check("integration d_sigmas", s2.grad, s1.grad, TOL_GRAD)
    assert float(s1.grad.abs().max()) > 0
