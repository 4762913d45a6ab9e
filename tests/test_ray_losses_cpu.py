"""CPU: the equations of the few-shot geometry losses ("Few-shot geometry losses") - ray entropy, depth
KL, patch depth smoothness - restated in tests/ray_losses_ref.py: the closed-form gradients against float64 autograd
of the restatements, the per-ray loop form of the entropy against the segmented one; the argument validation of the six
C-ABI entry points, which needs no GPU; and the host layer's refusals."""
import ctypes as C

import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L

import composite_ref as CR
import ray_losses_ref as RL
from test_train_step import _rel

SIZES = [5, 64, 65, 192]
BK = torch.tensor([1.0, 0.5, 0.25])
TV_SHAPES = [(1, 2, 2), (3, 8, 8), (2, 5, 13), (1, 16, 16), (2, 1, 7), (2, 7, 1)]


def _case64(S):
    case = CR.ragged_case(S)
    outs = CR.forward64(case, BK)
    g = torch.randn(case["R"], generator=torch.Generator().manual_seed(S)).double()
    return case, outs, g


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("which", ["alphas", "weights"])
@pytest.mark.parametrize("masked", [False, True])
def test_entropy_closed_form_gradient_and_loop_form(S, which, masked):
    """the closed-form gradient against autograd, the loop form against the segmented one; ray 7 (every value 0: the
    gradient is -log(eps)/eps g ~ 1e11) apart from the rest; with the opacity mask, ray 7 and the rays below the
    threshold have value 0 and gradient 0"""
    case, outs, g = _case64(S)
    ri, R = case["ri"], case["R"]
    c = (outs["opacity"].reshape(-1) > 0.1) if masked else None
    v = outs[which].clone().requires_grad_(True)
    assert int((v.detach() < 0).sum()) > 0  # the raw-sigma network's negative entries
    for log2 in (True, False):
        v.grad = None
        val = RL.entropy_value(v, ri, R, c=c, log2=log2)
        assert _rel(val.detach(), RL.entropy_loop(v.detach(), ri, R, c=c, log2=log2)) < 1e-12
        (val * g).sum().backward()
        closed = RL.entropy_grad(v.detach(), ri, R, g, c=c, log2=log2)
        seven = ri == CR.ZERO_RAY
        assert _rel(closed[~seven], v.grad[~seven]) < 1e-12
        assert bool((closed[v.detach() < 0] == 0).all()) and bool((v.grad[v.detach() < 0] == 0).all())
        assert float(val.detach()[CR.EMPTY_RAY]) == 0.0 and float(val.detach()[CR.ZERO_RAY]) == 0.0
        if masked:
            off = ~c[ri]
            assert not bool(c[CR.ZERO_RAY]) and bool((closed[off] == 0).all()) and bool((v.grad[off] == 0).all())
            assert bool((val.detach()[~c] == 0).all())
        else:
            assert _rel(closed[seven], v.grad[seven]) < 1e-12 and float(closed[seven].abs().max()) > 1e10
            assert float(closed[~seven].abs().max()) < 1e3  # (why ray 7 is measured apart)
    assert float(val.detach().max()) > 0.5


@pytest.mark.parametrize("S", SIZES)
def test_depth_kl_closed_form_gradient(S):
    """the closed-form gradient against autograd; rays 10-14 are unsupervised: value 0, gradient 0; all finite"""
    case, outs, g = _case64(S)
    ri, R = case["ri"], case["R"]
    t0, t1 = case["t0"].double(), case["t1"].double()
    depth, var = (t.double() for t in RL.kl_targets(outs["depth"], 200 + S))
    w = outs["weights"].clone().requires_grad_(True)
    val = RL.depth_kl_value(w, t0, t1, ri, R, depth, var)
    (val * g).sum().backward()
    closed = RL.depth_kl_grad(w.detach(), t0, t1, ri, R, depth, var, g)
    assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(w.grad).all()) and bool(torch.isfinite(closed).all())
    assert _rel(closed, w.grad) < 1e-12
    ok = RL.kl_supervised(depth, var)
    assert not bool(ok[list(RL.INVALID_RAYS)].any()) and int(ok.sum()) > 40
    assert bool((val.detach()[~ok] == 0).all()) and bool((closed[~ok[ri]] == 0).all()) and bool((w.grad[~ok[ri]] == 0).all())
    assert bool((closed[w.detach() < 0] == 0).all()) and float(val.detach().abs().max()) > 1e-3


@pytest.mark.parametrize("shape", TV_SHAPES)
def test_patch_smoothness_closed_form_gradient(shape):
    gen = torch.Generator().manual_seed(sum(shape))
    d = (2.0 + 4.0 * torch.rand(*shape, generator=gen)).double().requires_grad_(True)
    g = torch.randn(shape[0], generator=gen).double()
    val = RL.patch_tv_value(d)
    (val * g).sum().backward()
    closed = RL.patch_tv_grad(d.detach(), g)
    if shape[1] == 1 or shape[2] == 1:
        assert float(val.detach().abs().max()) == 0.0 and float(closed.abs().max()) == 0.0
        assert float(d.grad.abs().max()) == 0.0
    else:
        assert _rel(closed, d.grad) < 1e-12
        p0 = d.detach()[0]  # patch 0, anchor by anchor
        brute = sum((p0[a, b] - p0[a, b + 1]) ** 2 + (p0[a, b] - p0[a + 1, b]) ** 2
                    for a in range(shape[1] - 1) for b in range(shape[2] - 1))
        assert abs(float(brute) - float(val.detach()[0])) < 1e-12 * float(val.detach()[0])


def test_entry_points_validate_without_gpu():
    """null pointers and bad sizes are -1 with the entry point's name; N == 0 or n_rays == 0 is a no-op (nothing is
    launched: validation comes first)"""
    lib = L.lib()
    ent_f, ent_b = lib.fsn_ray_entropy_fwd, lib.fsn_ray_entropy_bwd
    kl_f, kl_b = lib.fsn_depth_kl_fwd, lib.fsn_depth_kl_bwd
    tv_f, tv_b = lib.fsn_patch_tv_fwd, lib.fsn_patch_tv_bwd
    calls = {
        "fsn_ray_entropy_fwd": lambda N, R: ent_f(None, None, N, R, None, 1e-10, 1.0, None, None),
        "fsn_ray_entropy_bwd": lambda N, R: ent_b(None, None, N, R, None, 1e-10, 1.0, None, None, None),
        "fsn_depth_kl_fwd": lambda N, R: kl_f(None, None, None, None, N, R, None, None, 1e-5, None, None),
        "fsn_depth_kl_bwd": lambda N, R: kl_b(None, None, None, None, N, R, None, None, 1e-5, None, None, None),
    }
    for name, call in calls.items():
        assert call(0, 8) == 0 and call(8, 0) == 0 and call(0, 0) == 0, name
        assert call(8, 2) == -1 and (name + ": null pointer").encode() in lib.fsn_last_error(), name
        assert call(-1, 2) == -1 and (name + ": bad sizes").encode() in lib.fsn_last_error(), name
        assert call(8, -2) == -1 and (name + ": bad sizes").encode() in lib.fsn_last_error(), name
    host = (C.c_float * 8)()  # stands for a device array: the call is refused before anything reads it
    idx = (C.c_int64 * 8)()
    p, q = C.cast(host, C.c_void_p), C.cast(idx, C.c_void_p)
    assert ent_f(p, q, 8, 2, None, 1e-10, 1.0, None, None) == -1 and b"fsn_ray_entropy_fwd: null pointer" in lib.fsn_last_error()
    assert ent_b(p, q, 8, 2, None, 1e-10, 1.0, p, None, None) == -1 and b"fsn_ray_entropy_bwd: null pointer" in lib.fsn_last_error()
    assert kl_f(p, p, p, q, 8, 2, None, p, 1e-5, p, None) == -1 and b"fsn_depth_kl_fwd: null pointer" in lib.fsn_last_error()
    assert kl_b(p, p, p, q, 8, 2, p, p, 1e-5, None, p, None) == -1 and b"fsn_depth_kl_bwd: null pointer" in lib.fsn_last_error()
    assert ent_f(p, q, 8, 2, None, 0.0, 1.0, p, None) == -1 and b"fsn_ray_entropy_fwd: eps" in lib.fsn_last_error()
    assert kl_f(p, p, p, q, 8, 2, p, p, 0.0, p, None) == -1 and b"fsn_depth_kl_fwd: eps" in lib.fsn_last_error()
    assert tv_f(None, 0, 4, 4, None, None) == 0 and tv_b(None, 0, 4, 4, None, None, None) == 0
    assert tv_f(None, 2, 4, 4, None, None) == -1 and b"fsn_patch_tv_fwd: null pointer" in lib.fsn_last_error()
    assert tv_b(None, 2, 4, 4, None, None, None) == -1 and b"fsn_patch_tv_bwd: null pointer" in lib.fsn_last_error()
    assert tv_b(p, 2, 2, 2, None, p, None) == -1 and b"fsn_patch_tv_bwd: null pointer" in lib.fsn_last_error()
    for B, P, Q in ((-1, 4, 4), (2, 0, 4), (2, 4, 0), (2, -3, 4)):
        assert tv_f(p, B, P, Q, p, None) == -1 and b"fsn_patch_tv_fwd: bad sizes" in lib.fsn_last_error()
        assert tv_b(p, B, P, Q, p, p, None) == -1 and b"fsn_patch_tv_bwd: bad sizes" in lib.fsn_last_error()
    assert tv_f(p, 1 << 40, 4, 4, p, None) == -1 and b"fsn_patch_tv_fwd: bad sizes" in lib.fsn_last_error()


def test_host_layer_refuses_cpu_tensors_and_mismatched_lengths():
    from fs_nerf_amd import ops
    from fs_nerf_amd.core.loss import DepthKLLoss, PatchDepthSmoothnessLoss, RayEntropyLoss
    case = CR.ragged_case(5)
    N, R, ri, t0, t1 = case["sig"].numel(), case["R"], case["ri"], case["t0"], case["t1"]
    v, depth, var = torch.rand(N), 2.0 + torch.rand(R), torch.full((R,), 0.01)
    with pytest.raises(RuntimeError):
        ops.ray_entropy(v, ri, R)
    with pytest.raises(RuntimeError):
        RayEntropyLoss()(v, ri, R, opacity=torch.rand(R, 1))
    with pytest.raises(RuntimeError):
        ops.depth_kl(v, t0, t1, ri, R, depth, var)
    with pytest.raises(RuntimeError):
        DepthKLLoss()(v, t0, t1, ri, R, depth, 0.01)
    with pytest.raises(RuntimeError):
        ops.patch_depth_smoothness(torch.rand(2, 4, 4))
    with pytest.raises(RuntimeError):
        PatchDepthSmoothnessLoss()(torch.rand(2, 4, 4))
    with pytest.raises(ValueError):
        ops.ray_entropy(v[:-1], ri, R)
    with pytest.raises(ValueError):
        ops.ray_entropy(v, ri, R, ray_weight=torch.ones(R - 1))
    with pytest.raises(ValueError):
        RayEntropyLoss()(v, ri[:-1], R)
    with pytest.raises(ValueError):
        RayEntropyLoss()(v, ri, R, opacity=torch.rand(R + 1, 1))
    with pytest.raises(ValueError):
        ops.depth_kl(v, t0[:-1], t1, ri, R, depth, var)
    with pytest.raises(ValueError):
        ops.depth_kl(v, t0, t1, ri, R, depth[:-1], var)
    with pytest.raises(ValueError):
        DepthKLLoss()(v, t0, t1, ri, R, depth, var[:-1])
    with pytest.raises(ValueError):
        ops.patch_depth_smoothness(torch.rand(4, 4))
    with pytest.raises(ValueError):
        PatchDepthSmoothnessLoss()(torch.rand(2, 4, 4, 1))
