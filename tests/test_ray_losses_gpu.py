"""GPU: the few-shot geometry losses (csrc/ray_losses.hip: fsn_ray_entropy_*, fsn_depth_kl_*, fsn_patch_tv_*) through
ops.py and core/loss.py, against the float64 restatements of tests/ray_losses_ref.py.

Inputs: the float32 outputs of ops.composite_packed on tests/composite_ref.ragged_case(S), S in {5, 64, 65, 192} (fewer
samples than lanes, one per lane, a ragged last lane, three per lane; ray 3 empty, ray 7 with every value exactly 0,
about 5 % negative entries).  The float64 reference takes those same float32 tensors cast to float64, so only the loss
arithmetic is compared.  Metric: test_train_step._rel, max |a - b| / max |b|; bars 1e-5 (values) and 2e-4 (gradients),
the project's bars for the distortion loss on this skeleton (the float32 CPU restatement of the same formulas stays
below 7e-7 / 6.2e-7 on this case with this file's cotangents).  Ray 7 of the entropy is measured apart: with s = 0 its gradient is
-log(eps)/eps g ~ 1e11, every other ray's entries are some tens.

Measured on the MI355X (the tests print the figures): see DESIGN.md 6.1, "Few-shot geometry losses"."""
import functools

import pytest
import torch

import fs_nerf_amd  # noqa: F401
from oracle import fsnerf_oracle as O

import composite_ref as CR
import ray_losses_ref as RL
from test_train_step import _rel

SIZES = [5, 64, 65, 192]
BK = torch.tensor([1.0, 0.5, 0.25])
TOL_GRAD, TOL_FWD = 2e-4, 1e-5
THRESHOLD = 0.1
TV_SHAPES = [(1, 2, 2), (3, 8, 8), (2, 5, 13), (1, 16, 16), (2, 1, 7), (2, 7, 1)]


@functools.lru_cache(maxsize=None)
def _setup(S):
    """the case, the GPU forward (float32) and its CPU copy, the depth KL targets and a per-ray cotangent: built once
    per size, never modified"""
    from fs_nerf_amd import ops
    dev = torch.device("cuda:0")
    case = CR.ragged_case(S)
    g = {k: case[k].to(dev) for k in ("sig", "rgb", "t0", "t1", "ri")}
    _, opacity, depth, ex = ops.composite_packed(g["sig"], g["rgb"], g["t0"], g["t1"], g["ri"], case["R"], BK)
    fwd = dict(opacity=opacity, depth=depth, weights=ex["weights"], alphas=ex["alphas"])
    cpu = {k: v.detach().cpu() for k, v in fwd.items()}
    assert int((case["ri"] == CR.EMPTY_RAY).sum()) == 0 and float(cpu["opacity"][CR.ZERO_RAY]) == 0.0
    assert bool((cpu["alphas"][case["ri"] == CR.ZERO_RAY] == 0).all())
    kl_depth, kl_var = RL.kl_targets(CR.forward64(case, BK)["depth"], 200 + S)
    gray = torch.randn(case["R"], generator=torch.Generator().manual_seed(300 + S))
    return case, g, fwd, cpu, kl_depth, kl_var, gray


def _bits_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("which", ["alphas", "weights"])
def test_entropy_value_gradient_and_determinism(S, which):
    """Values within 1e-5, gradients within 2e-4 of float64; ray 7 (s = 0) against its own maximum; gradient exactly 0
    where v < 0, passing where v == 0; two calls are equal bit for bit.
    Measured on the MI355X: values <= 1.7e-7, gradients of the regular rays <= 2.5e-7, ray 7 <= 9.9e-8 (alphas and
    weights, bits and nats, all four sizes; ray 7's reference gradient reaches 1.1e11 ... 6.0e11, the other rays'
    at most 75)."""
    from fs_nerf_amd import ops
    case, g, fwd, cpu, _, _, gray = _setup(S)
    R, ri, dev = case["R"], case["ri"], g["sig"].device
    v64 = cpu[which].double()
    seven = ri == CR.ZERO_RAY
    for log2 in (True, False):
        v = fwd[which].detach().clone().requires_grad_(True)
        val = ops.ray_entropy(v, g["ri"], R, log2=log2)
        assert val.shape == (R, 1) and val.requires_grad
        (val * gray.to(dev)[:, None]).sum().backward()
        ref = RL.entropy_value(v64, ri, R, log2=log2)
        ref_g = RL.entropy_grad(v64, ri, R, gray.double(), log2=log2)
        ev = _rel(val.reshape(-1), ref)
        eg, e7 = _rel(v.grad.cpu()[~seven], ref_g[~seven]), _rel(v.grad.cpu()[seven], ref_g[seven])
        print(f"S={S} entropy of {which} log2={log2}: value={ev:.3e} d_values={eg:.3e} ray7={e7:.3e} "
              f"(max |reference|: ray 7 {float(ref_g[seven].abs().max()):.3e}, the rest {float(ref_g[~seven].abs().max()):.3e})")
        assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(v.grad).all())
        assert ev < TOL_FWD and eg < TOL_GRAD and e7 < TOL_GRAD, (ev, eg, e7)
        assert float(ref_g[seven].abs().max()) > 1e10 and float(ref.max()) > 0.5
        assert float(val.detach()[CR.EMPTY_RAY]) == 0.0 and float(val.detach()[CR.ZERO_RAY]) == 0.0
        neg = (cpu[which] < 0)
        assert int(neg.sum()) > 0 and _bits_zero(v.grad[neg.to(dev)])  # torch.clamp(min=0)'s rule: nothing below 0 ...
        assert bool((v.grad.cpu()[seven] != 0).all())  # ... and the gradient passes at v == 0
        v2 = fwd[which].detach().clone().requires_grad_(True)
        val2 = ops.ray_entropy(v2, g["ri"], R, log2=log2)
        (val2 * gray.to(dev)[:, None]).sum().backward()
        assert torch.equal(val2, val) and torch.equal(v2.grad, v.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
def test_entropy_opacity_mask(S):
    """RayEntropyLoss on the alphas with the forward's opacity and threshold 0.1: ray 7 and every ray below the
    threshold have value 0 and gradient bitwise 0; the mean equals the reference's.
    Measured on the MI355X: values <= 1.5e-7, gradients <= 1.5e-7 (two rays masked at every size)."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.core.loss import RayEntropyLoss
    case, g, fwd, cpu, _, _, gray = _setup(S)
    R, ri, dev = case["R"], case["ri"], g["sig"].device
    c = cpu["opacity"].reshape(-1) > THRESHOLD
    assert not bool(c[CR.ZERO_RAY]) and not bool(c[CR.EMPTY_RAY]) and int(c.sum()) > 40
    v = fwd["alphas"].detach().clone().requires_grad_(True)
    per_ray = ops.ray_entropy(v, g["ri"], R, ray_weight=c.to(dev))
    (per_ray * gray.to(dev)[:, None]).sum().backward()
    off = ~c[ri]
    assert int(off.sum()) > 0 and _bits_zero(v.grad[off.to(dev)]) and _bits_zero(per_ray.detach()[(~c).to(dev)])
    v64 = cpu["alphas"].double()
    ref = RL.entropy_value(v64, ri, R, c=c)
    ref_g = RL.entropy_grad(v64, ri, R, gray.double(), c=c)
    ev, eg = _rel(per_ray.reshape(-1), ref), _rel(v.grad, ref_g)
    print(f"S={S} masked entropy: value={ev:.3e} d_values={eg:.3e} rays masked {int((~c).sum())}")
    assert ev < TOL_FWD and eg < TOL_GRAD
    v2 = fwd["alphas"].detach().clone().requires_grad_(True)
    mean = RayEntropyLoss(threshold=THRESHOLD)(v2, g["ri"], R, opacity=fwd["opacity"])
    assert mean.shape == () and abs(float(mean.detach()) - float(ref.mean())) < TOL_FWD * float(ref.max())
    mean.backward()
    assert _bits_zero(v2.grad[off.to(dev)]) and _rel(v2.grad, RL.entropy_grad(v64, ri, R, torch.full((R,), 1.0 / R).double(), c=c)) < TOL_GRAD


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
def test_depth_kl_value_gradient_and_determinism(S):
    """depth = the reference depth + 0.3 randn, var cycling through 1e-4, 1e-2 and 1, rays 10-14 unsupervised (depth 0,
    NaN, +inf, -1; var 0): those give value 0 and gradient bitwise 0, everything is finite (with var = 1e-4 some
    Gaussians underflow to exactly 0, which is expected).
    Measured on the MI355X: values <= 4.5e-7, gradients <= 4.0e-7 (all four sizes)."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.core.loss import DepthKLLoss
    case, g, fwd, cpu, depth, var, gray = _setup(S)
    R, ri, dev = case["R"], case["ri"], g["sig"].device
    d_dev, v_dev = depth.to(dev), var.to(dev)

    def run():
        w = fwd["weights"].detach().clone().requires_grad_(True)
        val = ops.depth_kl(w, g["t0"], g["t1"], g["ri"], R, d_dev, v_dev)
        (val * gray.to(dev)[:, None]).sum().backward()
        return w, val

    w, val = run()
    assert val.shape == (R, 1) and val.requires_grad
    w64, t0, t1 = cpu["weights"].double(), case["t0"].double(), case["t1"].double()
    ref = RL.depth_kl_value(w64, t0, t1, ri, R, depth.double(), var.double())
    ref_g = RL.depth_kl_grad(w64, t0, t1, ri, R, depth.double(), var.double(), gray.double())
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(ref_g).all())
    ev, eg = _rel(val.reshape(-1), ref), _rel(w.grad, ref_g)
    print(f"S={S} depth KL: value={ev:.3e} d_weights={eg:.3e} (max |reference| {float(ref.abs().max()):.3e} / "
          f"{float(ref_g.abs().max()):.3e})")
    assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(w.grad).all())
    assert ev < TOL_FWD and eg < TOL_GRAD, (ev, eg)
    ok = RL.kl_supervised(depth, var)
    assert not bool(ok[list(RL.INVALID_RAYS)].any()) and int(ok.sum()) > 40
    assert _bits_zero(val.detach()[(~ok).to(dev)]) and _bits_zero(w.grad[(~ok[ri]).to(dev)])
    assert _bits_zero(w.grad[(cpu["weights"] < 0).to(dev)]) and float(ref.abs().max()) > 1e-3
    w2, val2 = run()
    assert torch.equal(val2, val) and torch.equal(w2.grad, w.grad)
    mean = DepthKLLoss()(fwd["weights"], g["t0"], g["t1"], g["ri"], R, d_dev, v_dev)
    want = float(ref.sum()) / int(ok.sum())
    assert mean.shape == () and abs(float(mean) - want) < TOL_FWD * float(ref.abs().max())
    # one float for every ray: expanded on the device
    a = ops.depth_kl(fwd["weights"], g["t0"], g["t1"], g["ri"], R, d_dev, 0.01)
    b = ops.depth_kl(fwd["weights"], g["t0"], g["t1"], g["ri"], R, d_dev, torch.full((R,), 0.01, device=dev))
    assert torch.equal(a, b) and float(a.abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", TV_SHAPES)
def test_patch_smoothness_value_gradient_and_determinism(shape):
    """The smallest patch, 64 anchors or fewer, more than 64, and patches without an anchor (value 0, gradient 0);
    contiguous and as a strided slice of a larger tensor.
    Measured on the MI355X: values <= 7.2e-8, gradients <= 7.2e-8."""
    from fs_nerf_amd import ops
    from fs_nerf_amd.core.loss import PatchDepthSmoothnessLoss
    dev = torch.device("cuda:0")
    B, P, Q = shape
    gen = torch.Generator().manual_seed(sum(shape))
    big = 2.0 + 4.0 * torch.rand(B, 2 * P, 2 * Q + 1, generator=gen)
    gb = torch.randn(B, generator=gen)
    d_cpu = big[:, ::2, 1::2].contiguous()
    ref = RL.patch_tv_value(d_cpu.double())
    ref_g = RL.patch_tv_grad(d_cpu.double(), gb.double())

    def run(strided):
        if strided:
            leaf = big.to(dev).requires_grad_(True)
            d = leaf[:, ::2, 1::2]
            assert not d.is_contiguous()
        else:
            leaf = d = d_cpu.to(dev).requires_grad_(True)
        val = ops.patch_depth_smoothness(d)
        (val * gb.to(dev)).sum().backward()
        return leaf, val

    leaf, val = run(False)
    assert val.shape == (B,) and leaf.grad.shape == (B, P, Q)
    if P == 1 or Q == 1:
        assert _bits_zero(val.detach()) and _bits_zero(leaf.grad) and float(ref.abs().max()) == 0.0
    else:
        ev, eg = _rel(val, ref), _rel(leaf.grad, ref_g)
        print(f"patches {shape}: value={ev:.3e} d_depth={eg:.3e}")
        assert ev < TOL_FWD and eg < TOL_GRAD, (ev, eg)
    leaf2, val2 = run(False)
    assert torch.equal(val2, val) and torch.equal(leaf2.grad, leaf.grad)
    big_leaf, val3 = run(True)
    assert torch.equal(val3, val) and torch.equal(big_leaf.grad[:, ::2, 1::2], leaf.grad)
    rest = big_leaf.grad.clone()
    rest[:, ::2, 1::2] = 0.0
    assert float(rest.abs().max()) == 0.0
    mean = PatchDepthSmoothnessLoss()(d_cpu.to(dev))
    want = float(ref.mean()) / max((P - 1) * (Q - 1), 1)
    assert mean.shape == () and abs(float(mean) - want) <= TOL_FWD * abs(want)


@pytest.mark.gpu
def test_empty_inputs():
    """N == 0: zeros of shape [n_rays, 1] and an empty gradient; n_rays == 0: empty outputs."""
    from fs_nerf_amd import ops
    dev = torch.device("cuda:0")
    e = torch.zeros(0, device=dev)
    ei = torch.zeros(0, device=dev, dtype=torch.int64)
    four = torch.full((4,), 3.0, device=dev)
    for fn in (lambda v: ops.ray_entropy(v, ei, 4), lambda v: ops.ray_entropy(v, ei, 4, ray_weight=four),
               lambda v: ops.depth_kl(v, e, e, ei, 4, four, 0.01)):
        v = e.clone().requires_grad_(True)
        out = fn(v)
        assert out.shape == (4, 1) and _bits_zero(out.detach())
        out.sum().backward()
        assert v.grad.shape == (0,)
    assert ops.ray_entropy(e, ei, 0).shape == (0, 1) and ops.depth_kl(e, e, e, ei, 0, e, 0.01).shape == (0, 1)
    # samples that no ray owns get a gradient of zero
    v = torch.rand(8, device=dev).requires_grad_(True)
    out = ops.ray_entropy(v, torch.zeros(8, device=dev, dtype=torch.int64), 0)
    assert out.shape == (0, 1)
    out.sum().backward()
    assert v.grad.shape == (8,) and _bits_zero(v.grad)
    assert ops.patch_depth_smoothness(torch.zeros(0, 4, 4, device=dev)).shape == (0,)


def _chain_cpu(case, dtype, depth, var, c):
    """entropy of the alphas (masked) + depth KL of the weights through oracle.rendering_packed, on the CPU in `dtype`
    -> d loss / d sigmas"""
    sig = case["sig"].to(dtype).requires_grad_(True)
    rgb = case["rgb"].to(dtype).requires_grad_(True)
    t0, t1, ri, R = case["t0"].to(dtype), case["t1"].to(dtype), case["ri"], case["R"]
    _, _, _, ex = O.rendering_packed(t0, t1, ri, R, lambda a, b, i: (rgb, sig), BK.to(dtype))
    ent = RL.entropy_value(ex["alphas"], ri, R, c=c).mean()
    ok = RL.kl_supervised(depth, var)
    kl = RL.depth_kl_value(ex["weights"], t0, t1, ri, R, depth.to(dtype), var.to(dtype)).sum() / int(ok.sum().clamp(min=1))
    (ent + kl).backward()
    return sig.grad


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 65])
def test_losses_through_the_compositor(S):
    """rendering(full_grad=True) on leaf sigmas / rgbs, loss = RayEntropyLoss(alphas, masked by opacity) +
    DepthKLLoss(weights): d_sigmas against float64 autograd through oracle.rendering_packed and the restatements.
    The bar is taken from the same chain in float32 torch on the CPU: in saturated rays the depth KL cotangent
    1 / (w + 1e-5) meets weights near 1e-17, which no fixed bar anticipates - the GPU error may be at most 4 x the
    float32 error (which is tighter than the project's 2e-4 whenever the float32 error is below 5e-5).
    Measured, MI355X / float32 on the CPU: S = 5: 6.8e-6 / 5.8e-6, S = 65: 2.19e-5 / 2.19e-5."""
    from fs_nerf_amd.core.loss import DepthKLLoss, RayEntropyLoss
    from fs_nerf_amd.render import rendering as Rm
    case, g, fwd, cpu, depth, var, _ = _setup(S)
    R, dev = case["R"], g["sig"].device
    op64 = CR.forward64(case, BK)["opacity"].reshape(-1)
    assert float((op64 - THRESHOLD).abs().min()) > 1e-3  # the mask is the same in every precision
    c = op64 > THRESHOLD
    ref = _chain_cpu(case, torch.float64, depth, var, c)
    e32 = _rel(_chain_cpu(case, torch.float32, depth, var, c), ref)
    sg, rg = g["sig"].clone().requires_grad_(True), g["rgb"].clone().requires_grad_(True)
    _, opacity, _, ex = Rm.rendering(g["t0"], g["t1"], g["ri"], R, lambda a, b, i: (rg, sg), BK.to(dev), full_grad=True)
    assert torch.equal(opacity.detach().cpu().reshape(-1) > THRESHOLD, c)
    loss = (RayEntropyLoss(threshold=THRESHOLD)(ex["alphas"], g["ri"], R, opacity=opacity)
            + DepthKLLoss()(ex["weights"], g["t0"], g["t1"], g["ri"], R, depth.to(dev), var.to(dev)))
    loss.backward()
    e_gpu = _rel(sg.grad, ref)
    print(f"S={S} through the compositor: d_sigmas gpu={e_gpu:.3e} float32 cpu={e32:.3e} (max |reference| "
          f"{float(ref.abs().max()):.3e})")
    assert bool(torch.isfinite(sg.grad).all()) and float(ref.abs().max()) > 0
    bar = 4.0 * e32
    if e32 < 5e-5:
        assert bar <= TOL_GRAD
    assert e_gpu <= bar, (e_gpu, e32)
