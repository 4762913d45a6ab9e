"""GPU: the proposal-network sampler (csrc/propnet.hip, render/pdf.py, render/propnet.py) and the "propnet" route of
render_rays / render_frame.

The sampler's s-edges, centres and t-edges are compared with the float32 restatement of tests/propnet_ref.py with
torch.equal (no transcendental, no contraction, correctly rounded division: bit for bit), for both transforms, with
and without a per-ray jitter; fsn_prop_resample with the composition of the public primitives it fuses, torch.equal;
searchsorted ids exactly.  The interlevel loss and its gradient are compared with the float64 restatement (its
autograd is the truth) under test_train_step._rel, max |a - b| / max |b|, bars 1e-5 (forward) and 2e-4 (gradient), the
project's own for this arithmetic class (tests/test_volrend_gpu.py).  Every figure is printed before it is asserted.
Inputs: propnet_ref.histogram_case / loss_case - 70 rays, S in {1, 5, 64, 65, 192}, n in {1, 7, 64, 65, 200}.

Measured on the MI355X: the sampler differs from the restatement in 0 of its values, every case; the loss within
1.2e-7 and its gradient within 2.1e-7 of the float64 reference (35 to 63 % of the intervals carry a loss wherever the
proposal has more than one interval, largest gradient entry 46); the device cdfs within 7.8e-7 of the CPU float32 ones,
falling by at most 1.2e-7 between two edges (the rounding of the walk's cross-lane prefix); end to end the interlevel
loss 1.843725e-02 against the float64 reference's 1.843725e-02 (2.1e-8 apart)."""
import functools

import pytest
import torch

import fs_nerf_amd  # noqa: F401

import propnet_ref as PR
from test_train_step import _rel

TOL_FWD, TOL_GRAD = 1e-5, 2e-4
PAIRS = [(S, n) for S in PR.S_SIZES for n in PR.N_SIZES]


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
def _case(S):
    """the histogram case on the device: built once per size, never modified"""
    case = PR.histogram_case(S)
    return case, {k: _g(case[k]) for k in ("s_edges", "t_edges", "sigmas", "cdfs", "b")}


@pytest.mark.gpu
@pytest.mark.parametrize("S", PR.S_SIZES)
def test_importance_sample_equals_the_float32_restatement(S):
    from fs_nerf_amd import ops
    from fs_nerf_amd.render import pdf
    case, g = _case(S)
    for n in PR.N_SIZES:
        for jit in (False, True):
            want_e, want_x = PR.importance_sample_f32(case["s_edges"], case["cdfs"], n, case["b"] if jit else None)
            for tf in (None, "uniform", "lindisp"):
                s, x, t = ops.importance_sample(g["s_edges"], g["cdfs"], n, g["b"] if jit else None, tf, PR.NEAR, PR.FAR)
                bad = int((s.cpu() != want_e).sum())
                print(f"S={S} n={n} jitter={jit} {tf}: {bad} of {want_e.numel()} s-edges differ")
                assert torch.equal(s.cpu(), want_e), (S, n, jit, tf)
                assert torch.equal(x.cpu(), want_x), (S, n, jit, tf)
                if tf is None:
                    assert t is None
                else:
                    assert torch.equal(t.cpu(), PR.stot_f32(tf, want_e, PR.NEAR, PR.FAR)), (S, n, jit, tf)
            iv, sm = pdf.importance_sampling(pdf.RayIntervals(vals=g["s_edges"]), g["cdfs"], n, stratified=jit,
                                             u=g["b"] if jit else None)
            assert isinstance(iv, pdf.RayIntervals) and isinstance(sm, pdf.RaySamples)
            assert torch.equal(iv.vals.cpu(), want_e) and torch.equal(sm.vals.cpu(), want_x)
    iv, sm = pdf.importance_sampling(pdf.RayIntervals(vals=g["s_edges"]), g["cdfs"], 7, stratified=True)  # its own draw
    assert bool((iv.vals[:, 1:] >= iv.vals[:, :-1]).all()) and float(iv.vals.min()) >= 0 and float(iv.vals.max()) <= 1


@pytest.mark.gpu
def test_non_monotone_cdf_stays_finite_and_inside_the_support():
    from fs_nerf_amd import ops
    gen = torch.Generator().manual_seed(5)
    v = torch.sort(torch.rand(PR.R, 66, generator=gen), dim=1).values
    v[:, 0], v[:, -1] = 0.0, 1.0  # (s-space, as the estimator calls it)
    c = torch.rand(PR.R, 66, generator=gen)  # outside the contract: not sorted, no 0 / 1 at the ends
    for n in (1, 7, 65):
        s, x, t = ops.importance_sample(_g(v), _g(c), n, None, "uniform", PR.NEAR, PR.FAR)
        for out in (s, x):
            assert bool(torch.isfinite(out).all())
            assert bool((out.cpu() >= v[:, :1]).all()) and bool((out.cpu() <= v[:, -1:]).all()), n
        assert bool(torch.isfinite(t).all()) and float(t.min()) >= PR.NEAR and float(t.max()) <= PR.FAR
        # sorted on any row: the binary search is monotone in u, and a centre stays inside its own key interval
        assert bool((s[:, 1:] >= s[:, :-1]).all()) and bool((x[:, 1:] >= x[:, :-1]).all()), n


@pytest.mark.gpu
@pytest.mark.parametrize("S", PR.S_SIZES)
def test_prop_resample_equals_the_composed_primitives(S):
    from fs_nerf_amd import ops
    from fs_nerf_amd.render import volrend as V
    case, g = _case(S)
    t0, t1 = g["t_edges"][:, :-1].contiguous(), g["t_edges"][:, 1:].contiguous()
    trans, _ = V.render_transmittance_from_density(t0, t1, g["sigmas"])
    cdfs = 1.0 - torch.cat([trans, torch.zeros_like(trans[:, :1])], dim=-1)
    # (monotone only up to the rounding of the walk's cross-lane prefix, a tree sum: trans may rise by a few ulp between
    # two lanes.  The sampler's output is sorted all the same - its search is monotone in u on ANY row - asserted below.
    # Bound: a fall is T |d run| + an ulp of T, with |d run| a few 2^-24 run and T run <= 1/e: well under 1e-6.)
    dip = float((cdfs[:, :-1] - cdfs[:, 1:]).max())
    print(f"S={S} largest fall of the device cdf between two edges: {dip:.3e}")
    assert dip < 1e-6 and bool((cdfs[:, 0] == 0).all()) and bool((cdfs[:, -1] == 1).all())
    _check(f"S={S} cdfs against the CPU float32 cdfs", cdfs, case["cdfs"], TOL_FWD)
    for n in PR.N_SIZES:
        for jit, tf in ((False, "lindisp"), (True, "uniform"), (True, None)):
            b = g["b"] if jit else None
            got_c, got_s, got_x, got_t = ops.prop_resample(g["s_edges"], g["t_edges"], g["sigmas"], n, b, tf, PR.NEAR,
                                                           PR.FAR, want_centres=True)
            s, x, t = ops.importance_sample(g["s_edges"], cdfs, n, b, tf, PR.NEAR, PR.FAR)
            assert torch.equal(got_c, cdfs), (S, n)
            assert torch.equal(got_s, s) and torch.equal(got_x, x), (S, n, jit, tf)
            assert (got_t is None and t is None) if tf is None else torch.equal(got_t, t), (S, n, jit, tf)
            assert bool((s[:, 1:] >= s[:, :-1]).all()), (S, n)


@pytest.mark.gpu
@pytest.mark.parametrize("S", PR.S_SIZES)
def test_searchsorted_ids(S):
    from fs_nerf_amd.render import pdf
    case, g = _case(S)
    keys = case["s_edges"]
    gen = torch.Generator().manual_seed(40 + S)
    # queries below, above and equal to key edges, and random ones in between; a tied pair of keys in ray 3
    q = torch.cat([torch.full((PR.R, 1), -0.5), keys, torch.rand(PR.R, 70, generator=gen), torch.full((PR.R, 1), 1.5),
                   torch.ones(PR.R, 1)], 1)
    if S >= 5:
        keys = keys.clone()
        keys[3, 2] = keys[3, 3]
    want_l, want_r = PR.searchsorted_ref(keys, q)
    il, ir = pdf.searchsorted(pdf.RayIntervals(vals=_g(keys)), pdf.RaySamples(vals=_g(q)))
    assert il.dtype == torch.int64 and ir.dtype == torch.int64 and il.shape == q.shape
    assert torch.equal(il.cpu(), want_l) and torch.equal(ir.cpu(), want_r)
    assert int(il[:, 0].max()) == 0 and int(ir[:, 0].max()) == 0 and int(il[:, -1].min()) == S and int(ir[:, -2].min()) == S
    il2, ir2 = pdf.searchsorted(_g(keys), _g(q[:, :1]))  # plain tensors, one query per ray
    assert torch.equal(il2.cpu(), want_l[:, :1]) and torch.equal(ir2.cpu(), want_r[:, :1])


@pytest.mark.gpu
@pytest.mark.parametrize("S,n", PAIRS)
def test_interlevel_loss_and_gradient(S, n):
    from fs_nerf_amd.render import pdf
    from fs_nerf_amd.render.propnet import _pdf_loss
    case = PR.loss_case(S, n)
    q, cq, k, g = (case[x].double() for x in ("q", "cq", "k", "g"))
    ck64 = case["ck"].double().requires_grad_(True)
    want = PR.pdf_loss64(q, cq, k, ck64)
    (want_grad,) = torch.autograd.grad((want * g).sum(), ck64)
    ck = _g(case["ck"]).requires_grad_(True)
    got = _pdf_loss(pdf.RayIntervals(vals=_g(case["q"])), _g(case["cq"]), pdf.RayIntervals(vals=_g(case["k"])), ck)
    (got_grad,) = torch.autograd.grad((got * _g(case["g"])).sum(), ck)
    frac = float((want > 0).double().mean())
    print(f"S={S} n={n}: {100 * frac:.1f} % of the intervals have a loss, largest gradient entry {float(want_grad.abs().max()):.3g}")
    assert got.shape == (PR.R, n) and got_grad.shape == (PR.R, S + 1)
    if float(want.detach().abs().max()) > 0:
        _check(f"S={S} n={n} loss", got, want.detach(), TOL_FWD)
        _check(f"S={S} n={n} d loss / d cdfs_key", got_grad, want_grad, TOL_GRAD)
    else:
        assert float(got.detach().abs().max()) == 0.0 and float(got_grad.abs().max()) == 0.0
    if n >= 7 and S >= 5:
        assert frac > 0.1


def _nerf(seed):
    from fs_nerf_amd.core.models import NeRF
    torch.manual_seed(seed)
    m = NeRF(3, 3, 4, 128, (), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
    with torch.no_grad():
        m.sigma.weight.mul_(16.0)
        m.sigma.bias.add_(1.0)
    return m.to(_dev())


def _rays(n, seed=3):
    gen = torch.Generator().manual_seed(seed)
    o = torch.tensor([0.0, 0.0, 4.0]) + 0.1 * torch.randn(n, 3, generator=gen)
    d = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, -1.0]) + 0.2 * torch.randn(n, 3, generator=gen), dim=-1)
    return _g(o), _g(d)


@pytest.mark.gpu
def test_end_to_end_route_update_and_cache():
    from fs_nerf_amd.render import rendering as Rm
    from fs_nerf_amd.render.propnet import PropNetEstimator, prop_sigma_fn
    R, NP, NS = 64, 32, 16
    prop, fine = _nerf(11).train(), _nerf(12).train()
    opt = torch.optim.Adam(prop.parameters(), lr=1e-2)
    est = PropNetEstimator(opt, None, prop_models=[prop], prop_samples=(NP,), num_samples=NS, near_plane=PR.NEAR,
                           far_plane=PR.FAR, sampling_type="lindisp").train()
    assert [id(p) for p in est.parameters()] == [id(p) for p in prop.parameters()]
    o, d = _rays(R)
    gen = torch.Generator().manual_seed(9)
    u = [_g(torch.rand(R, generator=gen)) for _ in range(2)]
    # the route against sampling + rendering by hand
    (rgb, op, dep, ex), ri, tv = Rm.render_rays(o, d, est, fine, train=True, white_bkgd=True, device=_dev(), u=u)
    assert len(est.prop_cache) == 2 and est.prop_cache[0][1].requires_grad and est.prop_cache[1][1] is None
    assert torch.equal(ri, torch.arange(R, device=_dev()).repeat_interleave(NS)) and ex["trans"].shape == (R * NS,)
    hand = PropNetEstimator(prop_models=[prop], prop_samples=(NP,), num_samples=NS).train()
    t0, t1 = hand.sampling([prop_sigma_fn(prop, o, d)], (NP,), NS, R, PR.NEAR, PR.FAR, "lindisp", stratified=True,
                           requires_grad=True, u=u, device=_dev())
    assert t0.shape == (R, NS) and bool((t1 >= t0).all()) and float(t0.min()) >= PR.NEAR - 1e-4 and float(t1.max()) <= PR.FAR + 1e-4
    assert torch.equal(tv, ((t0 + t1) / 2.0).reshape(-1))

    def rgb_sigma_fn(t_starts, t_ends, ray_indices):
        out = fine.forward_rays(o, d, ray_indices, t_starts, t_ends, full=True)
        return out[..., :3], out[..., -1]

    h_rgb, h_op, h_dep, _ = Rm.rendering(t0.reshape(-1), t1.reshape(-1), ri, R, rgb_sigma_fn=rgb_sigma_fn,
                                         render_bkgd=torch.ones(3))
    assert torch.equal(rgb, h_rgb) and torch.equal(op, h_op) and torch.equal(dep, h_dep)
    # the no-grad sampler gives the same intervals (the fused level against the differentiable composition)
    t0n, t1n = hand.sampling([prop_sigma_fn(prop, o, d)], (NP,), NS, R, PR.NEAR, PR.FAR, "lindisp", u=u, device=_dev())
    print(f"no-grad sampling against the training pair's sigmas: {_rel(t0n, t0):.3e}")
    hand.prop_cache.clear()
    # the main step, then the proposal update
    torch.nn.functional.mse_loss(rgb, torch.full_like(rgb, 0.5)).backward()
    fine_grads = [p.grad.clone() for p in fine.parameters()]
    assert any(bool((g0 != 0).any()) for g0 in fine_grads)
    assert all(p.grad is None for p in prop.parameters())
    trans = ex["trans"].reshape(R, NS)
    # compute_loss's reference: float64, from the cached float32 intervals and cdfs
    (iv_p, cdf_p), (iv_f, _) = est.prop_cache
    cq = (1.0 - torch.cat([trans.detach().cpu(), torch.zeros(R, 1)], 1)).double()  # (the float32 cdfs the loss is given)
    want = float(PR.pdf_loss64(iv_f.vals.cpu().double(), cq, iv_p.vals.cpu().double(), cdf_p.detach().cpu().double()).mean())
    assert want > 0
    before = [p.detach().clone() for p in prop.parameters()]
    loss = est.update_every_n_steps(trans, requires_grad=True)
    print(f"interlevel loss {loss:.6e}, float64 reference {want:.6e}, rel {abs(loss - want) / want:.3e}")
    assert loss > 0 and loss == loss and abs(loss - want) < TOL_FWD * want
    assert len(est.prop_cache) == 0
    # Every parameter sigma depends on - the trunk and the sigma head - has a finite gradient with non-zero entries and
    # has moved.  The colour head (connection / branch / rgb) cannot: the cotangent of the training pair is on the sigma
    # column alone, so its gradient is an exact zero and Adam leaves it where it was.
    for (name, p), b4 in zip(prop.named_parameters(), before):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        if name.startswith(("layers.", "sigma.")):
            assert bool((p.grad != 0).any()) and not torch.equal(p.detach(), b4), name
        else:
            assert name.startswith(("connection.", "branch.", "rgb.")), name
            assert not bool((p.grad != 0).any()) and torch.equal(p.detach(), b4), name
    assert all(torch.equal(p.grad, g0) for p, g0 in zip(fine.parameters(), fine_grads))
    # requires_grad off: nothing is cached, by the switch, by eval mode and under no_grad
    est.proposal_requires_grad = False
    Rm.render_rays(o, d, est, fine, train=True, white_bkgd=True, device=_dev(), u=u)
    assert len(est.prop_cache) == 0 and est.update_every_n_steps(trans, requires_grad=False) == 0.0
    est.proposal_requires_grad = True
    with torch.no_grad():
        Rm.render_rays(o, d, est, fine, train=True, white_bkgd=True, device=_dev(), u=u)
    assert len(est.prop_cache) == 0
    with pytest.raises(ValueError):
        Rm.render_rays(o, d, est, fine, device=_dev(), sampling_kwargs={"cone_angle": 0.01})
    with pytest.raises(ValueError):
        Rm.render_rays(o, d, est, fine, device=_dev(), sampling_kwargs={"alpha_thre": 0.01})


@pytest.mark.gpu
def test_render_frame_and_zero_rays():
    from fs_nerf_amd import ops
    from fs_nerf_amd.render import pdf
    from fs_nerf_amd.render import rendering as Rm
    from fs_nerf_amd.render.propnet import PropNetEstimator, _pdf_loss
    prop, fine = _nerf(11).eval(), _nerf(12).eval()
    est = PropNetEstimator(prop_models=[prop], prop_samples=(32,), num_samples=16, near_plane=PR.NEAR, far_plane=PR.FAR).eval()
    pose = torch.eye(4)
    pose[2, 3] = 4.0
    with torch.no_grad():
        rgb, depth = Rm.render_frame((12, 12, 12.0), PR.NEAR, PR.FAR, pose, 100, est, fine, white_bkgd=True, device=_dev())
        far = Rm.render_frame((12, 12, 12.0), PR.NEAR, PR.FAR, pose, 100, est, fine, device=_dev(),
                              sampling_kwargs={"near_plane": 3.0, "far_plane": 5.0})[1]
    assert rgb.shape == (12, 12, 3) and depth.shape == (12, 12)
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(depth).all())
    assert float(depth.min()) >= PR.NEAR and float(depth.max()) <= PR.FAR and bool(torch.isfinite(far).all())
    # R = 0: empty tensors, no launch
    e = torch.zeros(0, 5, device=_dev())
    s, x, t = ops.importance_sample(e, e, 7, None, "uniform", PR.NEAR, PR.FAR)
    assert s.shape == (0, 8) and x.shape == (0, 7) and t.shape == (0, 8)
    c, s, x, t = ops.prop_resample(e, e, torch.zeros(0, 4, device=_dev()), 7, None, "lindisp", PR.NEAR, PR.FAR)
    assert c.shape == (0, 5) and s.shape == (0, 8) and x is None and t.shape == (0, 8)
    il, ir = pdf.searchsorted(e, e)
    assert il.shape == (0, 5) and ir.shape == (0, 5)
    ck = e.clone().requires_grad_(True)
    loss = _pdf_loss(pdf.RayIntervals(vals=e), e, pdf.RayIntervals(vals=e), ck)
    assert loss.shape == (0, 4)
    loss.sum().backward()
    assert ck.grad.shape == (0, 5)
    t0, t1 = est.sampling([lambda a, b: torch.zeros_like(a)], (32,), 16, 0, PR.NEAR, PR.FAR, device=_dev())
    assert t0.shape == (0, 16) and t1.shape == (0, 16)
