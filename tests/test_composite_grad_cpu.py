"""CPU: the equations of the full compositor backward and of the distortion loss ("Full compositor
backward"), restated in float64 in tests/composite_ref.py, against autograd on oracle.rendering_packed and the O(S^2)
distortion; and the argument validation of the new C-ABI entry points, which needs no GPU."""
import ctypes as C

import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L

import composite_ref as CR
from test_train_step import _rel

BK = torch.tensor([1.0, 0.5, 0.25])


def _f64(case):
    return (case["sig"].double(), case["rgb"].double(), case["t0"].double(), case["t1"].double(), case["ri"], case["R"])


@pytest.mark.parametrize("S", [5, 65])
@pytest.mark.parametrize("which", ["all"] + list(CR.COTANGENTS))
def test_closed_form_compositor_backward_vs_autograd(S, which):
    """C1: all six cotangents at once, then each one alone, float64.  The density is chosen so that no ray saturates
    (sum sigma dt ~ 1.6 * 0.01 * S): d opacity / d sigma_i = dt_i (1 - O) reaches autograd and the closed form alike as
    the difference of two O(1) numbers, so its relative error is eps / (1 - O), and 1e-12 needs 1 - O well above 1e-4."""
    case = CR.ragged_case(S, density=0.01)
    op = CR.forward64(case, BK)["opacity"].reshape(-1)
    assert float((1.0 - op).min()) > 1e-2
    cot = CR.random_cotangents(case, 100 + S)
    if which != "all":
        cot = {which: cot[which]}
    gs, gr, _ = CR.autograd_reference(case, cot, BK)
    d = {k: v.double() for k, v in cot.items()}
    ds, dr = CR.composite_bwd_closed(*_f64(case), bkgd=BK.double(), g=d.get("colors"), g_O=d.get("opacity"),
                                     g_D=d.get("depth"), u=d.get("weights"), a=d.get("alphas"), tau=d.get("trans"))
    seven = case["ri"] == CR.ZERO_RAY  # (its depth gradient is m/eps ~ 5e7: measured apart from the rest)
    assert int(seven.sum()) > 0 and int((case["ri"] == CR.EMPTY_RAY).sum()) == 0
    for sel in (seven, ~seven):
        assert _rel(ds[sel], gs[sel]) < 1e-12 and _rel(dr[sel], gr[sel]) < 1e-12, which


@pytest.mark.parametrize("S", [5, 65])
def test_distortion_value_and_gradient(S):
    """C2: the scan form against the O(S^2) double sum; the closed-form gradient against autograd; float64."""
    case = CR.ragged_case(S)
    outs = CR.forward64(case, BK)
    t0, t1, ri, R = case["t0"].double(), case["t1"].double(), case["ri"], case["R"]
    w = outs["weights"].clone().requires_grad_(True)
    val = CR.distortion_value(w, t0, t1, ri, R)
    assert _rel(val, CR.distortion_bruteforce(w.detach(), t0, t1, ri, R)) < 1e-12
    assert float(val.detach()[CR.EMPTY_RAY]) == 0.0 and float(val.detach().abs().max()) > 1e-3
    g = torch.randn(R, generator=torch.Generator().manual_seed(S)).double()
    (val * g).sum().backward()
    assert _rel(CR.distortion_grad(w.detach(), t0, t1, ri, R, g), w.grad) < 1e-12


def test_new_entry_points_validate_without_gpu():
    """C3: null pointers are an error, empty problems are a no-op, d_depth without the forward's opacity / depth is
    refused by name (nothing is launched: validation comes first)."""
    lib = L.lib()
    full = lib.fsn_composite_packed_bwd_full
    nul = [None] * 5
    assert full(*nul, 0, 8, None, None, None, None, None, None, None, None, None, None, None, None) == 0
    assert full(*nul, 8, 0, None, None, None, None, None, None, None, None, None, None, None, None) == 0
    assert full(*nul, -1, 8, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert full(*nul, 8, 2, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"fsn_composite_packed_bwd_full: null pointer" in lib.fsn_last_error()
    host = (C.c_float * 8)()  # stands for a device array: the call is refused before anything reads it
    p = C.cast(host, C.c_void_p)
    for opacity, depth in ((None, None), (p, None), (None, p)):
        assert full(p, p, p, p, p, 8, 2, None, p, None, opacity, depth, p, None, None, None, p, p, None) == -1
        msg = lib.fsn_last_error()
        assert b"fsn_composite_packed_bwd_full" in msg and b"d_depth" in msg and b"opacity" in msg, msg
    fwd, bwd = lib.fsn_distortion_fwd, lib.fsn_distortion_bwd
    assert fwd(None, None, None, None, 0, 8, None, None) == 0 and fwd(None, None, None, None, 8, 0, None, None) == 0
    assert bwd(None, None, None, None, 0, 8, None, None, None) == 0 and bwd(None, None, None, None, 8, 0, None, None, None) == 0
    assert fwd(None, None, None, None, 8, 2, None, None) == -1 and b"fsn_distortion_fwd: null pointer" in lib.fsn_last_error()
    assert bwd(None, None, None, None, 8, 2, None, None, None) == -1 and b"fsn_distortion_bwd: null pointer" in lib.fsn_last_error()
    assert fwd(None, None, None, None, -1, 2, None, None) == -1 and bwd(None, None, None, None, 8, -2, None, None, None) == -1


def test_host_layer_refuses_cpu_tensors_and_keeps_the_default_surface():
    import inspect

    from fs_nerf_amd import ops
    from fs_nerf_amd.core.loss import DistortionLoss
    from fs_nerf_amd.render import rendering as Rm
    case = CR.ragged_case(5)
    with pytest.raises(RuntimeError):
        ops.distortion(torch.rand(case["sig"].numel()), case["t0"], case["t1"], case["ri"], case["R"])
    with pytest.raises(RuntimeError):
        DistortionLoss()(torch.rand(case["sig"].numel()), case["t0"], case["t1"], case["ri"], case["R"])
    with pytest.raises(RuntimeError):
        ops.composite_packed_bwd_full(case["sig"], case["rgb"], case["t0"], case["t1"], case["ri"], case["R"], None, None, None)
    assert inspect.signature(Rm.rendering).parameters["full_grad"].default is False
    pr = inspect.signature(Rm.render_rays).parameters["full_grad"]
    assert pr.default is False and pr.kind is inspect.Parameter.KEYWORD_ONLY
