"""Gradients of the training pair with respect to the network's INPUTS (csrc/input_grad.hip): sample positions and
directions in the point form, rays_o / rays_d in the ray form, against float64 autograd on the oracle; the frozen-network
route, NeRF.density_gradient, the render_rays wiring and the C-ABI.

Bars = tests/test_train_step.py's TRAIN_MODES: error relative to the tensor's largest entry below 2e-4 in the default
fp16x3 mode and 1e-3 in bf16x3, on samples whose every ReLU pre-activation is at least `margin` (2e-5 / 1e-4) away from
zero (a unit within the forward's error of zero takes the other branch and changes the sample's whole gradient)."""
import ctypes as C
import functools

import pytest
import torch

import fs_nerf_amd  # noqa: F401
from oracle import fsnerf_oracle as O

MODES = [(None, 2e-4, 2e-5), ("bf16x3", 1e-3, 1e-4)]  # (train precision, tolerance, ReLU margin): TRAIN_MODES' MFMA rows
NETS = [(4, 128, (), 10, 4), (8, 256, (4,), 10, 4), (6, 128, (1, 3), 7, 3)]
N = 300  # three 128-sample tiles, the last partial


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-12))


def _relu_margin(sd, x, d, n_layers, skip, nf, nfd, log_space=True, pos_mask=None, dir_mask=None):
    """min |pre-activation| over every ReLU unit of the network, per sample (float64, CPU)."""
    sd = {k: v.double() for k, v in sd.items()}
    dm = lambda m: None if m is None else m.double()
    pe = O.posenc(x.double(), nf, log_space, dm(pos_mask))
    h, margin = pe, torch.full((x.shape[0],), 1e9, dtype=torch.float64)
    for i in range(n_layers):
        z = torch.nn.functional.linear(h, sd[f"layers.{i}.weight"], sd[f"layers.{i}.bias"])
        margin = torch.minimum(margin, z.abs().amin(dim=1))
        h = torch.relu(z)
        if i in skip:
            h = torch.cat([h, pe], dim=-1)
    f = torch.nn.functional.linear(h, sd["connection.weight"], sd["connection.bias"])
    zb = torch.nn.functional.linear(torch.cat([f, O.posenc(d.double(), nfd, log_space, dm(dir_mask))], dim=-1),
                                    sd["branch.weight"], sd["branch.bias"])
    return torch.minimum(margin, zb.abs().amin(dim=1))


def _band_mask(nf):
    """posenc-layout mask: the highest band zero, the one below it 0.37, everything else one."""
    m = torch.ones(3 * (1 + 2 * nf))
    m[3 + 6 * (nf - 1):3 + 6 * nf] = 0.0
    m[3 + 6 * (nf - 2):3 + 6 * (nf - 1)] = 0.37
    return m


@functools.lru_cache(maxsize=None)
def _state(net):
    L, D, skip, nf, nfd = net
    sd = O.init_nerf_state_dict(L, D, list(skip), nf, nfd, seed=3)
    sd["sigma.weight"] *= 16.0
    return sd


def _model(net, log_space=True, masked=False):
    from fs_nerf_amd.core.models import NeRF
    L, D, skip, nf, nfd = net
    m = NeRF(3, 3, L, D, skip, pos_fn={"n_freqs": nf, "log_space": log_space}, dir_fn={"n_freqs": nfd, "log_space": log_space})
    m.load_state_dict(_state(net))
    if masked:
        m.set_freq_mask(_band_mask(nf), _band_mask(nfd))
    return m.to(torch.device("cuda:0"))


def _cfg(net, log_space=True, masked=False):
    L, D, skip, nf, nfd = net
    cfg = dict(n_layers=L, skip=list(skip), n_freqs=nf, n_freqs_dir=nfd, log_space=log_space)
    if masked:
        cfg.update(pos_mask=_band_mask(nf).double(), dir_mask=_band_mask(nfd).double())
    return cfg


@functools.lru_cache(maxsize=None)
def _samples(net, margin, n=N, log_space=True, masked=False):
    """n margin-selected samples out of 12 n candidates (seed 3), the rule of test_nerf_gradients_vs_autograd."""
    L, D, skip, nf, nfd = net
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(12 * N, 3, generator=gen) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(12 * N, 3, generator=gen), dim=-1)
    mk = (_band_mask(nf), _band_mask(nfd)) if masked else (None, None)
    keep = _relu_margin(_state(net), x, d, L, skip, nf, nfd, log_space, *mk) > margin
    x, d = x[keep][:n].contiguous(), d[keep][:n].contiguous()
    assert x.shape[0] == n
    return x, d


@functools.lru_cache(maxsize=None)
def _reference(net, margin, cscale, n=N, log_space=True, masked=False):
    """-> (x, d, c, d x, d dirs) with the float64 autograd gradients of (out * c).sum() on the oracle."""
    x, d = _samples(net, margin, n, log_space, masked)
    c = torch.randn(n, 4, generator=torch.Generator().manual_seed(7)) * cscale
    x64, d64 = x.double().requires_grad_(True), d.double().requires_grad_(True)
    ref = O.nerf_forward(_state(net), x64, d64, **_cfg(net, log_space, masked))
    (ref * c.double()).sum().backward()
    return x, d, c, x64.grad, d64.grad


def _point_case(net, tp, tol, margin, cscale, log_space=True, masked=False):
    dev = torch.device("cuda:0")
    x, d, c, gx, gd = _reference(net, margin, cscale, N, log_space, masked)
    m = _model(net, log_space, masked).train()
    m.train_precision = tp
    xg, dg = x.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    out = m(xg, dg)
    assert out.requires_grad and out.shape == (N, 4)
    (out * c.to(dev)).sum().backward()
    assert xg.grad is not None and dg.grad is not None and xg.grad.shape == (N, 3) and dg.grad.shape == (N, 3)
    ex, ed = _rel(xg.grad, gx), _rel(dg.grad, gd)
    print(f"net {net} mode {tp} cscale {cscale:g} log_space {log_space} masked {masked}: d_x {ex:.3e} d_dirs {ed:.3e}")
    assert ex < tol, ("x", ex)
    assert ed < tol, ("dirs", ed)
    # the parameter gradients do not notice: same bits as the same step with inputs that need no gradient
    with_inputs = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    (m(x.to(dev), d.to(dev)) * c.to(dev)).sum().backward()
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, with_inputs[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("tp,tol,margin", MODES)
@pytest.mark.parametrize("cscale", [1.0, 1e-7, 1e3])
@pytest.mark.parametrize("net", NETS)
def test_point_form_input_gradients_vs_float64(net, cscale, tp, tol, margin):
    _point_case(net, tp, tol, margin, cscale)


@pytest.mark.gpu
@pytest.mark.parametrize("tp,tol,margin", MODES)
def test_point_form_linear_frequencies(tp, tol, margin):
    _point_case(NETS[2], tp, tol, margin, 1.0, log_space=False)


@pytest.mark.gpu
@pytest.mark.parametrize("tp,tol,margin", MODES)
def test_point_form_frequency_mask(tp, tol, margin):
    _point_case(NETS[1], tp, tol, margin, 1.0, masked=True)


@pytest.mark.gpu
@pytest.mark.parametrize("tp,tol,margin", MODES)
def test_point_form_weight_slices_staged_per_job(tp, tol, margin):
    """8 x 256 with two skip-fed layers: three position slices and the direction slice are 208 KiB in the x3 modes, more
    than the kernel keeps in LDS - it stages one GEMM's slice at a time instead of holding all of them."""
    _point_case((8, 256, (2, 5), 10, 4), tp, tol, margin, 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_tile_tails(n):
    dev = torch.device("cuda:0")
    tp, tol, margin = MODES[0]
    x, d, c, gx, gd = _reference(NETS[1], margin, 1.0, n)
    m = _model(NETS[1]).train()
    xg, dg = x.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    (m(xg, dg) * c.to(dev)).sum().backward()
    assert xg.grad.shape == (n, 3) and bool(torch.isfinite(xg.grad).all()) and bool(torch.isfinite(dg.grad).all())
    ex, ed = _rel(xg.grad, gx), _rel(dg.grad, gd)
    print(f"n {n}: d_x {ex:.3e} d_dirs {ed:.3e}")
    assert ex < tol and ed < tol, (ex, ed)


# ray form: 37 rays; sample counts with 0, 1, 64 and 150 (samples 69 .. 218: across the tile boundary at 128), two
# neighbouring empty rays and an empty last one; 308 samples = three tiles
RAY_COUNTS = [4, 0, 0, 1, 64, 150, 2] + [3] * 29 + [0]


@functools.lru_cache(maxsize=None)
def _ray_case(net, margin):
    """rays and, per ray, sorted disjoint intervals whose float32 midpoints clear the ReLU margin -> (o, d, ri, t0, t1)."""
    L, D, skip, nf, nfd = net
    gen = torch.Generator().manual_seed(3)
    R = len(RAY_COUNTS)
    o = torch.rand(R, 3, generator=gen) * 0.4 - 0.2
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=-1)
    ri, t0, t1 = [], [], []
    for r, cnt in enumerate(RAY_COUNTS):
        if cnt == 0:
            continue
        e = torch.sort(torch.rand(12 * cnt + 9, generator=gen) * 1.1 + 0.1).values
        a, b = e[:-1], e[1:]
        x = o[r] + d[r] * (a + b)[:, None] / 2.0  # float32, the forward's operation order
        ok = _relu_margin(_state(net), x, d[r].expand_as(x), L, skip, nf, nfd) > margin
        assert int(ok.sum()) >= cnt, (r, int(ok.sum()))
        a, b = a[ok][:cnt], b[ok][:cnt]
        ri.append(torch.full((cnt,), r, dtype=torch.int64)); t0.append(a); t1.append(b)
    return o, d, torch.cat(ri), torch.cat(t0).contiguous(), torch.cat(t1).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("tp,tol,margin", MODES)
def test_ray_form_gradients_vs_float64(tp, tol, margin):
    dev = torch.device("cuda:0")
    net = NETS[1]
    o, d, ri, t0, t1 = _ray_case(net, margin)
    R, n = o.shape[0], ri.numel()
    assert R == 37 and n == sum(RAY_COUNTS)
    c = torch.randn(n, 4, generator=torch.Generator().manual_seed(7))
    o64, d64 = o.double().requires_grad_(True), d.double().requires_grad_(True)
    mid = ((t0 + t1) / 2.0).double()  # the float32 midpoint the forward forms
    ref = O.nerf_forward(_state(net), o64[ri] + d64[ri] * mid[:, None], d64[ri], **_cfg(net))
    (ref * c.double()).sum().backward()
    m = _model(net).train()
    m.train_precision = tp

    def run():
        og, dg = o.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
        m.zero_grad(set_to_none=True)
        out = m.forward_rays(og, dg, ri.to(dev), t0.to(dev), t1.to(dev))
        out.mul(c.to(dev)).sum().backward()
        return og.grad, dg.grad

    go, gd = run()
    assert go is not None and gd is not None and go.shape == (R, 3) and gd.shape == (R, 3)
    eo, ed = _rel(go, o64.grad), _rel(gd, d64.grad)
    print(f"mode {tp}: d_rays_o {eo:.3e} d_rays_d {ed:.3e}")
    assert eo < tol and ed < tol, (eo, ed)
    empty = torch.tensor([k == 0 for k in RAY_COUNTS])
    assert int(empty.sum()) == 3
    assert bool((go.cpu()[empty] == 0).all()) and bool((gd.cpu()[empty] == 0).all())
    go2, gd2 = run()
    assert torch.equal(go, go2) and torch.equal(gd, gd2), "fixed summation order: the same bits"


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["rays_d only", "rays_o only"])
@pytest.mark.parametrize("tp,tol,margin", MODES)
def test_ray_form_one_ray_tensor_requires_grad(tp, tol, margin, which):
    """A fixed camera centre (rotation-only pose refinement) or fixed directions: the tensor that asks gets its WHOLE
    gradient - d rays_d = sum (m_i d_x_i + d_dirs_i) needs the per-sample position gradient although rays_o asks for
    nothing - within the bar of float64 and with the bits of the call in which both ask; the other gets none."""
    dev = torch.device("cuda:0")
    net = NETS[1]
    o, d, ri, t0, t1 = _ray_case(net, margin)
    c = torch.randn(ri.numel(), 4, generator=torch.Generator().manual_seed(7))
    o64, d64 = o.double().requires_grad_(True), d.double().requires_grad_(True)
    mid = ((t0 + t1) / 2.0).double()
    ref = O.nerf_forward(_state(net), o64[ri] + d64[ri] * mid[:, None], d64[ri], **_cfg(net))
    (ref * c.double()).sum().backward()
    m = _model(net).train()
    m.train_precision = tp

    def run(need_o, need_d):
        og, dg = o.to(dev).requires_grad_(need_o), d.to(dev).requires_grad_(need_d)
        m.zero_grad(set_to_none=True)
        m.forward_rays(og, dg, ri.to(dev), t0.to(dev), t1.to(dev)).mul(c.to(dev)).sum().backward()
        return og.grad, dg.grad, {k: p.grad.clone() for k, p in m.named_parameters()}

    jo, jd, jp = run(True, True)
    go, gd, gp = run(which == "rays_o only", which == "rays_d only")
    got, other, joint, want = (gd, go, jd, d64.grad) if which == "rays_d only" else (go, gd, jo, o64.grad)
    assert other is None and got is not None
    e = _rel(got, want)
    print(f"mode {tp} {which}: {e:.3e}")
    assert e < tol, e
    assert torch.equal(got, joint)
    assert all(torch.equal(gp[k], jp[k]) for k in jp)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["dirs only", "x only"])
def test_point_form_one_input_requires_grad(which):
    dev = torch.device("cuda:0")
    tp, tol, margin = MODES[0]
    x, d, c, gx, gd = _reference(NETS[1], margin, 1.0)
    m = _model(NETS[1]).train()

    def run(need_x, need_d):
        xg, dg = x.to(dev).requires_grad_(need_x), d.to(dev).requires_grad_(need_d)
        m.zero_grad(set_to_none=True)
        (m(xg, dg) * c.to(dev)).sum().backward()
        return xg.grad, dg.grad

    jx, jd = run(True, True)
    ox, od = run(which == "x only", which == "dirs only")
    got, other, joint, want = (od, ox, jd, gd) if which == "dirs only" else (ox, od, jx, gx)
    assert other is None and _rel(got, want) < tol and torch.equal(got, joint)


@pytest.mark.gpu
@pytest.mark.parametrize("tp", ["bf16", "fp16"])
def test_single_pass_modes_input_gradients(tp):
    """The single-pass 16-bit instantiations of k_input_grad.  Not parity modes (2^-8 / 2^-11 per product through ten
    chained GEMMs, ReLU units change branch), so the criterion is the project's for these modes
    (test_single_pass_training_modes_run): direction and scale of the whole gradient - cosine above 0.995 and norm
    within 5 % - here against float64 autograd, point form and ray form."""
    dev = torch.device("cuda:0")
    net = NETS[1]
    x, d, c, gx, gd = _reference(net, 2e-5, 1.0)
    m = _model(net).train()
    m.train_precision = tp
    xg, dg = x.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    (m(xg, dg) * c.to(dev)).sum().backward()
    o, dd, ri, t0, t1 = _ray_case(net, 2e-5)
    cr = torch.randn(ri.numel(), 4, generator=torch.Generator().manual_seed(7))
    o64, d64 = o.double().requires_grad_(True), dd.double().requires_grad_(True)
    ref = O.nerf_forward(_state(net), o64[ri] + d64[ri] * ((t0 + t1) / 2.0).double()[:, None], d64[ri], **_cfg(net))
    (ref * cr.double()).sum().backward()
    og, rg = o.to(dev).requires_grad_(True), dd.to(dev).requires_grad_(True)
    m.forward_rays(og, rg, ri.to(dev), t0.to(dev), t1.to(dev)).mul(cr.to(dev)).sum().backward()
    for name, got, want in (("d_x", xg.grad, gx), ("d_dirs", dg.grad, gd), ("d_rays_o", og.grad, o64.grad),
                            ("d_rays_d", rg.grad, d64.grad)):
        a, b = got.detach().cpu().double().reshape(-1), want.reshape(-1)
        assert bool(torch.isfinite(a).all()), name
        cos, ratio = float((a * b).sum() / (a.norm() * b.norm())), float(a.norm() / b.norm())
        print(f"{tp} {name}: cosine {cos:.5f} norm ratio {ratio:.4f}")
        assert cos > 0.995 and abs(ratio - 1.0) < 0.05, (name, cos, ratio)


@pytest.mark.gpu
def test_frozen_network_density_gradient_and_null_weights_route():
    dev = torch.device("cuda:0")
    tp, tol, margin = MODES[0]
    net = NETS[1]
    x, d, c, gx, gd = _reference(net, margin, 1.0)
    # float64 gradient of sigma alone
    x64 = x.double().requires_grad_(True)
    sig64 = O.nerf_forward(_state(net), x64, d.double(), **_cfg(net))[:, 3]
    (gs64,) = torch.autograd.grad(sig64.sum(), x64)
    assert float(gs64.norm(dim=-1).min()) >= 0.6  # normals are well defined on these samples
    frozen = _model(net).eval()
    for p in frozen.parameters():
        p.requires_grad_(False)
    # the same call on the frozen and on a trainable network: one chain, the same bits (each model's first backward
    # calibrates its per-stage factors on this very cotangent)
    xg, dg = x.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    (frozen(xg, dg) * c.to(dev)).sum().backward()
    assert _rel(xg.grad, gx) < tol and _rel(dg.grad, gd) < tol
    assert all(p.grad is None for p in frozen.parameters())
    trainable = _model(net).train()
    xt, dt = x.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True)
    (trainable(xt, dt) * c.to(dev)).sum().backward()
    assert torch.equal(xg.grad, xt.grad) and torch.equal(dg.grad, dt.grad)
    assert all(p.grad is not None for p in trainable.parameters())
    sigma, grad = frozen.density_gradient(x.to(dev))
    assert sigma.shape == (N,) and grad.shape == (N, 3) and not grad.requires_grad
    assert _rel(sigma, sig64) < 1e-5
    e = _rel(grad, gs64)
    print(f"density gradient {e:.3e}")
    assert e < tol, e
    assert all(p.grad is None for p in frozen.parameters())
    # density_gradient on a TRAINING model leaves its parameters' gradients alone too
    # ... and is no training step: the training backward's per-stage factors, its call count and the optimizer's step
    # flag are the ones it found (input-only calls keep factors and a range word of their own)
    from fs_nerf_amd import ops
    before = {k: p.grad.clone() for k, p in trainable.named_parameters()}
    st = trainable.train_state
    factors, calls, flag = st.train.stage[0].clone(), st.train.calls, ops.step_flag(dev).clone()
    _, g2 = trainable.density_gradient(x.to(dev))
    assert _rel(g2, gs64) < tol and all(torch.equal(p.grad, before[k]) for k, p in trainable.named_parameters())
    assert torch.equal(st.train.stage[0], factors) and st.train.calls == calls
    assert torch.equal(ops.step_flag(dev), flag) and st.inputs.stage is not None


def _wiring_setup(kind, dev):
    from fs_nerf_amd.core.models import NeRF
    from fs_nerf_amd.render import rendering as Rm
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    from test_occgrid import AABB, _orbit_rays, _sphere_binaries

    def net(seed):
        sd = O.init_nerf_state_dict(4, 128, [], 10, 4, seed=seed)
        sd["sigma.weight"] *= 16.0
        sd["sigma.bias"] += 1.0
        m = NeRF(3, 3, 4, 128, (), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
        m.load_state_dict(sd)
        return m.to(dev).train()

    R = 96
    o, d = _orbit_rays(R, 3)
    gen = torch.Generator().manual_seed(9)
    gt = torch.rand(R, 3, generator=gen).to(dev)
    if kind == "occ":
        est = OccGridEstimator(roi_aabb=torch.tensor(AABB), resolution=32, levels=1).to(dev)
        est.set_binaries(_sphere_binaries(32, 1))
        est.train()
        coarse, fine = net(6), None
        kw = dict(render_step_size=5e-2)

        def reseed():
            est.generator = torch.Generator(device=dev).manual_seed(2)
    else:
        est = Rm.StratifiedEstimator(2.0, 6.0, 16, 8).train()
        coarse, fine = net(6), net(7)
        kw = dict(model_fine=fine, u=torch.rand(R, generator=gen).to(dev), u_fine=torch.rand(R, 8, generator=gen).to(dev))
        reseed = lambda: None
    return Rm, est, coarse, fine, o.to(dev), d.to(dev), gt, kw, reseed


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["occ", "stratified"])
def test_render_rays_carries_ray_gradients(kind):
    dev = torch.device("cuda:0")
    Rm, est, coarse, fine, o, d, gt, kw, reseed = _wiring_setup(kind, dev)
    net = fine if fine is not None else coarse
    R = o.shape[0]
    loss_of = lambda rgb, depth: torch.nn.functional.mse_loss(rgb, gt) + depth.mean()

    def step(rays_need_grad):
        og, dg = o.clone().requires_grad_(rays_need_grad), d.clone().requires_grad_(rays_need_grad)
        net.zero_grad(set_to_none=True)
        reseed()
        (rgb, _, depth, ex), ri, _ = Rm.render_rays(og, dg, est, coarse, train=True, white_bkgd=True, device=dev,
                                                    full_grad=True, **kw)
        loss_of(rgb, depth).backward()
        return og.grad, dg.grad, {k: p.grad.clone() for k, p in net.named_parameters()}, (ri, ex["t_starts"], ex["t_ends"])

    step(True)  # (first backward of a model in an fp16 mode calibrates its per-stage factors)
    go, gd, pg, (ri, t0, t1) = step(True)
    assert ri.numel() > 200 and go is not None and gd is not None
    assert float(go.abs().max()) > 0 and float(gd.abs().max()) > 0
    # by hand on the samples the call returned: the same kernels in the same order
    og, dg = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    net.zero_grad(set_to_none=True)

    def rgb_sigma_fn(a, b, cc):
        out = net.forward_rays(og, dg, cc, a, b, full=True)
        return out[..., :3], out[..., -1]

    rgb, _, depth, _ = Rm.rendering(t0, t1, ri, n_rays=R, rgb_sigma_fn=rgb_sigma_fn, render_bkgd=torch.full((3,), 1.0),
                                    full_grad=True)
    loss_of(rgb, depth).backward()
    assert torch.equal(og.grad, go) and torch.equal(dg.grad, gd)
    # the parameters' gradients do not notice the rays' request
    _, _, pg0, (ri0, _, _) = step(False)
    assert torch.equal(ri0, ri)
    for k in pg:
        assert torch.equal(pg[k], pg0[k]), k


@pytest.mark.gpu
def test_c_abi_partial_outputs_flagged_status_and_empty_call():
    from fs_nerf_amd import ops, _lib as Lb
    dev = torch.device("cuda:0")
    net = NETS[0]
    L, D, skip, nf, nfd = net
    m = _model(net)
    ws, bs = m._tensors()
    ws_, bs_ = [w.detach() for w in ws], [b.detach() for b in bs]
    desc = ops.make_desc(L, D, skip, m.pos_encoder.freqs, m.dir_encoder.freqs)
    x, d = (t.to(dev) for t in _samples(net, 2e-5))
    c = torch.randn(N, 4, generator=torch.Generator().manual_seed(7)).to(dev)
    prec = Lb.FSN_PREC_FP16X3
    lib = Lb.lib()
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])

    def call(want_x, want_d, flag=0):
        word = torch.zeros(1, dtype=torch.int32, device=dev)
        out, work = ops.nerf_train_fwd(desc, prec, ws_, bs_, x, d, None, None, status=word)
        assert int(word.item()) == 0
        word.fill_(flag)
        gx = torch.full((N, 3), 7.0, device=dev) if want_x else None
        gd = torch.full((N, 3), 7.0, device=dev) if want_d else None
        rc = lib.fsn_nerf_train_bwd_inputs(C.byref(desc), prec, arr(ws_), N, P(work), P(out), P(c), None, None, None, 0, None,
                                           None, P(word), P(x), P(d), None, None, None, None, None, None, None, P(gx), P(gd),
                                           None)
        assert rc == 0, lib.fsn_last_error()
        torch.cuda.synchronize()
        return gx, gd

    gx, gd = call(True, True)
    assert float(gx.abs().max()) > 0 and float(gd.abs().max()) > 0 and bool((gx != 7.0).all())
    gx1, none = call(True, False)
    none2, gd1 = call(False, True)
    assert none is None and none2 is None and torch.equal(gx1, gx) and torch.equal(gd1, gd)
    assert call(False, False) == (None, None)  # the chain alone (what a frozen network's calibration pass runs)
    zx, zd = call(True, True, flag=Lb.FSN_STATUS_FP16_RANGE)  # a flagged step: zeros, like the weight gradients
    assert bool((zx == 0).all()) and bool((zd == 0).all())
    rc = lib.fsn_nerf_train_bwd_inputs(C.byref(desc), prec, arr(ws_), 0, None, None, None, None, None, None, 0, None, None,
                                       None, None, None, None, None, None, None, None, None, None, None, None, None)
    assert rc == 0
    # a mixed-up call is an error with a message, not a launch
    rc = lib.fsn_nerf_train_bwd_inputs(C.byref(desc), prec, arr(ws_), N, P(x), P(x), P(c), None, None, None, 0, None, None,
                                       None, None, None, None, None, None, None, None, None, None, P(gx), P(gd), None)
    assert rc != 0 and b"x and dirs" in lib.fsn_last_error()
    # fsn_ray_grad_reduce without samples: every ray is empty
    o3 = torch.full((5, 3), 7.0, device=dev)
    d3 = torch.full((5, 3), 7.0, device=dev)
    assert lib.fsn_ray_grad_reduce(None, None, None, None, None, 0, 5, P(o3), P(d3), None) == 0
    torch.cuda.synchronize()
    assert bool((o3 == 0).all()) and bool((d3 == 0).all())


@pytest.mark.gpu
def test_double_backward_raises():
    dev = torch.device("cuda:0")
    x, d = (t.to(dev) for t in _samples(NETS[0], 2e-5))
    m = _model(NETS[0]).train()
    xg = x.clone().requires_grad_(True)
    out = m(xg, d)
    (g,) = torch.autograd.grad((out * out).sum(), xg, create_graph=True)  # (a cotangent that itself carries a graph)
    assert g.requires_grad
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        g.sum().backward()
