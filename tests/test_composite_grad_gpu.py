"""GPU: the full backward of the packed compositor (fsn_composite_packed_bwd_full), `rendering(full_grad=True)`, the
distortion loss (fsn_distortion_fwd / _bwd) and one training step through render_rays(full_grad=True), against float64
autograd on oracle.rendering_packed and the float64 restatements of tests/composite_ref.py.

Inputs: tests/composite_ref.ragged_case - 70 rays x S in {5, 64, 65, 192} (fewer samples than lanes, one per lane, a
ragged last lane, three per lane), 20 % of the samples dropped, ray 3 empty, ray 7 with opacity exactly 0 (the O < eps
branch of the depth gradient), 5 % negative sigmas.  Metric: test_train_step._rel, max |a - b| / max |b|; bars 2e-4
(gradients) and 1e-5 (forward values).  Ray 7 is measured apart: its depth gradient is m/eps ~ 5e7.

One case is measured on another scale, and DESIGN.md ("Full compositor backward") records it next to the equations:
d_opacity ALONE at S >= 64.  Every regular ray is saturated there (opacity > 0.9999), the true gradient
dt_i g_O (1 - O) is 1e-6 .. 1e-17, and the formula - the lean kernel's, which G2 pins bit for bit - forms it as the
difference of two terms of size dt_i |g_O|, each rounded to float32.  The error is a few float32 eps of THOSE terms,
so that case's denominator is max dt_i |g_O| (the gradient's size at T = 1), with the same 2e-4 bar; S = 5 (opacity
0.17 .. 0.9) checks the same term on the plain metric.  Measured on the MI355X at S = 64, 65, 192: 1.9e-2, 4.9e-2 and
1.1e4 on the plain metric (max |reference| 1.4e-6, 6.0e-7, 9.3e-18; the test prints them), 1.6e-7, 1.8e-7 and 1.5e-7 on
the terms' scale.  Every other figure of this file is below 1.1e-6 (gradients) and 1.7e-6 (values)."""
import functools

import pytest
import torch

import fs_nerf_amd  # noqa: F401
from oracle import fsnerf_oracle as O

import composite_ref as CR
from test_train_step import _rel

SIZES = [5, 64, 65, 192]
BK = torch.tensor([1.0, 0.5, 0.25])
TOL_GRAD, TOL_FWD = 2e-4, 1e-5
REGULAR_MIN_OPACITY = 0.05


@functools.lru_cache(maxsize=None)
def _setup(S):
    """the case, its cotangents, the float64 forward and the GPU forward: built once per size, never modified"""
    from fs_nerf_amd import ops
    dev = torch.device("cuda:0")
    case = CR.ragged_case(S)
    cot = CR.random_cotangents(case, 100 + S)
    ref = CR.forward64(case, BK)
    op = ref["opacity"].reshape(-1)
    regular = torch.ones(case["R"], dtype=torch.bool)
    regular[[CR.EMPTY_RAY, CR.ZERO_RAY]] = False
    # the depth gradient carries 1/O: this keeps the comparison well conditioned (change the seed, not the bound)
    assert float(op[regular].min()) >= REGULAR_MIN_OPACITY, float(op[regular].min())
    assert float(op[CR.ZERO_RAY]) == 0.0 and int((case["ri"] == CR.EMPTY_RAY).sum()) == 0
    g = {k: case[k].to(dev) for k in ("sig", "rgb", "t0", "t1", "ri")}
    colors, opacity, depth, ex = ops.composite_packed(g["sig"], g["rgb"], g["t0"], g["t1"], g["ri"], case["R"], BK)
    fwd = dict(colors=colors, opacity=opacity, depth=depth, weights=ex["weights"], alphas=ex["alphas"], trans=ex["trans"])
    return case, cot, ref, g, fwd


@functools.lru_cache(maxsize=None)
def _reference_grads(S, which):
    case, cot, _, _, _ = _setup(S)
    return CR.autograd_reference(case, _select(case, cot, which), BK)[:2]


def _select(case, cot, which):
    if which == "all":
        return cot
    if which == "colors+opacity":
        return {k: cot[k] for k in ("colors", "opacity")}
    if which == "depth-ray7":
        d = torch.zeros_like(cot["depth"])
        d[CR.ZERO_RAY] = cot["depth"][CR.ZERO_RAY]
        return {"depth": d}
    return {which: cot[which]}


def _full(S, sel, bkgd=BK):
    from fs_nerf_amd import ops
    case, _, _, g, fwd = _setup(S)
    d = {k: v.to(g["sig"].device) for k, v in sel.items()}
    return ops.composite_packed_bwd_full(g["sig"], g["rgb"], g["t0"], g["t1"], g["ri"], case["R"], bkgd, d.get("colors"),
                                         d.get("opacity"), opacity=fwd["opacity"], depth=fwd["depth"],
                                         d_depth=d.get("depth"), d_weights=d.get("weights"), d_alphas=d.get("alphas"),
                                         d_trans=d.get("trans"))


def _err(a, b, scale=None):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    den = b.abs().max().clamp(min=1e-12) if scale is None else scale
    return float((a - b).abs().max() / den)


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
def test_forward_values_of_the_ragged_case(S):
    _, _, ref, _, fwd = _setup(S)
    for k in CR.COTANGENTS:
        e = _rel(fwd[k].reshape(ref[k].shape), ref[k])
        print(f"S={S} forward {k}: {e:.3e}")
        assert e < TOL_FWD, (k, e)
    assert float(fwd["opacity"][CR.ZERO_RAY]) == 0.0 and float(fwd["depth"][CR.ZERO_RAY]) == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("which", ["all"] + list(CR.COTANGENTS) + ["depth-ray7"])
def test_full_backward_vs_float64_autograd(S, which):
    """G1: all six cotangents, each alone with the others NULL, d_depth alone on ray 7; background (1, 0.5, 0.25)."""
    case, cot, ref, _, _ = _setup(S)
    sel = _select(case, cot, which)
    gs, gr = _reference_grads(S, which)
    ds, dr = _full(S, sel)
    ri = case["ri"]
    seven = ri == CR.ZERO_RAY
    scale = None
    if which == "opacity" and S >= 64:  # (module docstring: the saturated rays' opacity-only gradient)
        assert float(ref["opacity"].reshape(-1)[ri[~seven]].min()) > 0.9999
        dt = (case["t1"] - case["t0"]).double()
        scale = (dt * cot["opacity"].reshape(-1)[ri].abs().double())[~seven].max()
        print(f"S={S} opacity alone on the plain metric: {_err(ds[~seven], gs[~seven]):.3e} "
              f"(max |reference| {float(gs[~seven].abs().max()):.3e})")
    figures = dict(regular_sig=_err(ds[~seven], gs[~seven], scale), regular_rgb=_err(dr[~seven], gr[~seven]),
                   ray7_sig=_err(ds[seven], gs[seven]), ray7_rgb=_err(dr[seven], gr[seven]))
    if which == "all":  # the empty ray's neighbours, each on its own
        for r in (CR.EMPTY_RAY - 1, CR.EMPTY_RAY + 1):
            assert int((ri == r).sum()) > 0
            figures[f"ray{r}_sig"] = _err(ds[ri == r], gs[ri == r])
            figures[f"ray{r}_rgb"] = _err(dr[ri == r], gr[ri == r])
    print(f"S={S} {which}: " + " ".join(f"{k}={v:.3e}" for k, v in figures.items()))
    assert bool(torch.isfinite(ds).all()) and bool(torch.isfinite(dr).all())
    if which in ("all", "depth", "depth-ray7"):
        assert float(gs[seven].abs().max()) > 1e4  # the O < eps branch: m / eps
    for k, v in figures.items():
        assert v < TOL_GRAD, (k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
def test_full_entry_point_equals_the_lean_one_bit_for_bit(S):
    """G2: with only d_colors / d_opacity given.  Both entry points launch one kernel, so the equality shows that the
    lean one hands its arguments through; the lean result is also held to float64 autograd on its own."""
    from fs_nerf_amd import ops
    case, cot, _, g, _ = _setup(S)
    dev = g["sig"].device
    dc, dop = cot["colors"].to(dev), cot["opacity"].to(dev)
    for bkgd in (BK, None):
        for op in (dop, None):
            lean = ops.composite_packed_bwd(g["sig"], g["rgb"], g["t0"], g["t1"], g["ri"], case["R"], bkgd, dc, op)
            full = ops.composite_packed_bwd_full(g["sig"], g["rgb"], g["t0"], g["t1"], g["ri"], case["R"], bkgd, dc, op)
            assert torch.equal(full[0], lean[0]) and torch.equal(full[1], lean[1])
            assert float(lean[0].abs().max()) > 0
    gs, gr = _reference_grads(S, "colors+opacity")
    ds, dr = ops.composite_packed_bwd(g["sig"], g["rgb"], g["t0"], g["t1"], g["ri"], case["R"], BK, dc, dop)
    es, er = _rel(ds, gs), _rel(dr, gr)
    print(f"S={S} lean entry point against float64 autograd: d_sigmas={es:.3e} d_rgbs={er:.3e}")
    assert es < TOL_GRAD and er < TOL_GRAD, (es, er)


@pytest.mark.gpu
def test_rendering_full_grad(monkeypatch):
    """G3: every output differentiable; a depth-only loss backpropagates; unused cotangents reach the kernel as NULL;
    the default is what test_train_step.py::test_composite_gradients_vs_autograd states."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.render import rendering as Rm
    S = 65
    case, cot, _, g, _ = _setup(S)
    dev = g["sig"].device
    calls = []
    real = ops.composite_packed_bwd_full

    def spy(*a, **kw):
        calls.append((a, kw))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "composite_packed_bwd_full", spy)

    def render(full_grad):
        sg, rg = g["sig"].clone().requires_grad_(True), g["rgb"].clone().requires_grad_(True)
        out = Rm.rendering(g["t0"], g["t1"], g["ri"], case["R"], lambda a, b, c: (rg, sg), BK.to(dev), full_grad=full_grad)
        return sg, rg, out

    sg, rg, (colors, opacity, depth, ex) = render(True)
    assert set(ex) == {"weights", "alphas", "trans", "sigmas", "rgbs"}
    assert all(t.requires_grad for t in (colors, opacity, depth, ex["weights"], ex["alphas"], ex["trans"]))
    d_gt = cot["depth"].to(dev)
    (depth * d_gt).sum().backward()
    assert len(calls) == 1
    a, kw = calls[0]
    assert a[7] is None and a[8] is None  # d_colors, d_opacity
    assert kw["d_depth"] is not None and kw["opacity"] is not None and kw["depth"] is not None
    assert kw["d_weights"] is None and kw["d_alphas"] is None and kw["d_trans"] is None
    gs, gr = _reference_grads(S, "depth")
    seven = case["ri"] == CR.ZERO_RAY
    for sel in (seven, ~seven):
        assert _rel(sg.grad[sel], gs[sel]) < TOL_GRAD
    assert float(rg.grad.abs().max()) == 0.0
    # weights and colours together: two cotangents, the rest NULL
    sg, rg, (colors, opacity, depth, ex) = render(True)
    ((ex["weights"] * cot["weights"].to(dev)).sum() + (colors * cot["colors"].to(dev)).sum()).backward()
    a, kw = calls[1]
    assert a[7] is not None and a[8] is None and kw["d_depth"] is None and kw["d_weights"] is not None
    gs2 = _reference_grads(S, "weights")[0] + _reference_grads(S, "colors")[0]
    assert _rel(sg.grad[~seven], gs2[~seven]) < TOL_GRAD
    # the default: depth and the extras are detached, the lean backward runs
    sg, rg, (colors, opacity, depth, ex) = render(False)
    assert colors.requires_grad and opacity.requires_grad
    assert not depth.requires_grad and not ex["weights"].requires_grad and not ex["alphas"].requires_grad
    assert not ex["trans"].requires_grad
    (colors * cot["colors"].to(dev)).sum().backward()
    assert len(calls) == 2
    with pytest.raises(RuntimeError):
        render(False)[2][2].sum().backward()  # depth alone: nothing requires grad


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
def test_distortion_value_gradient_and_determinism(S):
    """G4: on the packed inputs with the GPU forward's weights."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.core.loss import DistortionLoss
    case, cot, _, g, fwd = _setup(S)
    R, dev = case["R"], g["sig"].device
    w = fwd["weights"].detach().clone().requires_grad_(True)
    val = ops.distortion(w, g["t0"], g["t1"], g["ri"], R)
    assert val.shape == (R, 1) and val.requires_grad
    w64 = fwd["weights"].detach().cpu().double()
    t0, t1, ri = case["t0"].double(), case["t1"].double(), case["ri"]
    ref = CR.distortion_value(w64, t0, t1, ri, R)
    gr = cot["opacity"]  # a per-ray cotangent
    (val * gr.to(dev)).sum().backward()
    ref_g = CR.distortion_grad(w64, t0, t1, ri, R, gr.double())
    ev, eg = _rel(val.reshape(-1), ref), _rel(w.grad, ref_g)
    print(f"S={S} distortion: value={ev:.3e} d_weights={eg:.3e}")
    assert ev < TOL_FWD and eg < TOL_GRAD
    assert float(val.detach()[CR.EMPTY_RAY]) == 0.0 and float(val.detach()[CR.ZERO_RAY]) == 0.0 and float(ref.max()) > 1e-3
    w2 = fwd["weights"].detach().clone().requires_grad_(True)
    val2 = ops.distortion(w2, g["t0"], g["t1"], g["ri"], R)
    (val2 * gr.to(dev)).sum().backward()
    assert torch.equal(val2, val) and torch.equal(w2.grad, w.grad)
    mean = DistortionLoss()(fwd["weights"], g["t0"], g["t1"], g["ri"], R)
    assert mean.shape == () and abs(float(mean) - float(ref.mean())) < TOL_FWD * float(ref.max())
    none = ops.distortion(w[:0], g["t0"][:0], g["t1"][:0], g["ri"][:0], 4)  # no samples at all: zeros
    assert none.shape == (4, 1) and float(none.detach().abs().max()) == 0.0


@pytest.mark.gpu
def test_training_step_with_depth_opacity_and_distortion_terms():
    """G5: the reference's training call (render_rays with the occupancy estimator, train=True) with full_grad=True and
    a loss on rgb, depth, opacity and the distortion of the weights, each term per ray and weighted by the ReLU-margin
    ray mask of test_occgrid.py::test_training_step_gradients_through_the_occupancy_path (4 x 128 case): every
    parameter gradient within 2e-4 of float64 autograd on the oracle over the same samples, and layers.0.weight's
    gradient away from the colour-only one by more than 10 x that bar."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.core.models import NeRF
    from fs_nerf_amd.core.optim import FusedAdam
    from fs_nerf_amd.render import rendering as Rm
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    from test_occgrid import AABB, _orbit_rays, _relu_margin_rel, _sphere_binaries
    dev = torch.device("cuda:0")
    L, D, skip = 4, 128, ()
    sd = O.init_nerf_state_dict(L, D, list(skip), 10, 4, seed=6)
    sd["sigma.weight"] *= 16.0
    sd["sigma.bias"] += 1.0
    m = NeRF(3, 3, L, D, skip, pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
    m.load_state_dict(sd)
    m = m.to(dev).train()
    opt = FusedAdam(m.parameters(), lr=1e-3)
    est = OccGridEstimator(roi_aabb=torch.tensor(AABB), resolution=32, levels=1).to(dev)
    est.set_binaries(_sphere_binaries(32, 1))
    est.train()
    R, step = 800, 2e-2
    o, d = _orbit_rays(R, 3)
    est.generator = torch.Generator(device=dev).manual_seed(2)
    with torch.no_grad():
        (_, _, _, ex0), ri0, tv0 = Rm.render_rays(o, d, est, m, train=True, white_bkgd=True, render_step_size=step, device=dev)
    assert "t_starts" not in ex0  # the default path's extras keys do not change
    ri0, tv0 = ri0.cpu(), tv0.cpu()
    risky = _relu_margin_rel(sd, o[ri0] + d[ri0] * tv0[:, None], d[ri0], L, skip) < 4e-6
    ray_ok = torch.ones(R, dtype=torch.bool)
    ray_ok[ri0[risky]] = False
    assert int(ray_ok.sum()) >= 40, int(ray_ok.sum())
    gen = torch.Generator().manual_seed(4)
    ok = ray_ok[:, None].float()
    c = torch.randn(R, 3, generator=gen) * ok
    d_gt = 2.0 + 4.0 * torch.rand(R, 1, generator=gen)
    est.generator = torch.Generator(device=dev).manual_seed(2)
    opt.zero_grad()
    (rgb, opacity, depth, ex), ri, tv = Rm.render_rays(o, d, est, m, train=True, white_bkgd=True, render_step_size=step,
                                                       device=dev, full_grad=True)
    assert torch.equal(ri.cpu(), ri0) and torch.equal(tv.cpu(), tv0) and ri.numel() > 2000
    assert all(t.requires_grad for t in (rgb, opacity, depth, ex["weights"], ex["alphas"], ex["trans"]))
    dist = ops.distortion(ex["weights"], ex["t_starts"], ex["t_ends"], ri, R)
    okd = ok.to(dev)
    loss = (rgb * c.to(dev)).sum() + (((depth - d_gt.to(dev)) ** 2 + (opacity - 1.0) ** 2 + dist) * okd).sum()
    loss.backward()
    cfg = dict(n_layers=L, skip=list(skip), n_freqs=10, n_freqs_dir=4)
    sdr = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items()}
    oo, dd = o.double(), d.double()
    t0, t1 = ex["t_starts"].detach().cpu().double(), ex["t_ends"].detach().cpu().double()

    def fn(a, b, cc):
        # the network at the positions the GPU evaluated (and the ray mask was computed for): the float32 midpoints
        # render_rays returned.  (a + b)/2 in float64 lies half an ulp of t away, which the 2^9 frequency of the
        # encoding turns into 1e-4 of phase: ReLU units change branch.  The integration takes the edges themselves.
        y = O.nerf_forward(sdr, oo[cc] + dd[cc] * tv0.double()[:, None], dd[cc], **cfg)
        return y[:, :3], y[:, 3]

    col, op64, dep64, ex64 = O.rendering_packed(t0, t1, ri0, R, fn, torch.ones(3, dtype=torch.float64))
    colour_term = (col * c.double()).sum()
    dist64 = CR.distortion_value(ex64["weights"], t0, t1, ri0, R)[:, None]
    extra = (((dep64 - d_gt.double()) ** 2 + (op64 - 1.0) ** 2 + dist64) * ok.double()).sum()
    colour_only = torch.autograd.grad(colour_term, sdr["layers.0.weight"], retain_graph=True)[0]
    (colour_term + extra).backward()
    print(f"loss gpu {float(loss.detach()):.9e} oracle {float((colour_term + extra).detach()):.9e} rays in the loss {int(ray_ok.sum())} "
          f"min opacity there {float(op64.detach()[ray_ok].min()):.3e}")
    errs = {name: _rel(p.grad, sdr[name].grad) for name, p in m.named_parameters()}
    for name, e in errs.items():
        print(f"  {name}: {e:.3e}")
    moved = _rel(m.layers[0].weight.grad, colour_only)
    print(f"  layers.0.weight against the colour-only gradient: {moved:.3e}")
    for name, e in errs.items():
        assert e < TOL_GRAD, (name, e)
    assert moved > 10 * TOL_GRAD, moved
