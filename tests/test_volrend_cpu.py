"""CPU: the restatements of tests/volrend_ref.py against oracle.rendering_packed and against a brute-force double loop
for the product scan's gradient (the ray with the zero factor included); the argument validation of the packed
primitives' C-ABI entry points, which needs no GPU; the Python layer's refusals."""
import ctypes as C

import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L

import composite_ref as CR
import volrend_ref as VR
from test_train_step import _rel


@pytest.mark.parametrize("S", [5, 65])
def test_density_restatement_equals_the_oracle(S):
    case = VR.density_case(S)
    ref = CR.forward64(case, None)
    w, tr, al = VR.weights_from_density(case["sig"].double(), case["t0"].double(), case["t1"].double(), case["ri"], case["R"])
    for name, a in (("weights", w), ("trans", tr), ("alphas", al)):
        assert _rel(a, ref[name]) < 1e-14, name
    op = VR.accumulate(w, None, case["ri"], case["R"])
    assert _rel(op, ref["opacity"]) < 1e-14 and float(op[CR.EMPTY_RAY]) == 0.0


@pytest.mark.parametrize("S", [5, 65])
def test_alpha_restatement_equals_the_oracle_on_the_density_case(S):
    """alphas = 1 - exp(-sigma dt) in float64: the product form of the transmittance is the oracle's exponential form"""
    case = VR.density_case(S)
    ref = CR.forward64(case, None)
    w, tr = VR.weights_from_alpha(ref["alphas"], case["ri"], case["R"])
    assert _rel(w, ref["weights"]) < 1e-12 and _rel(tr, ref["trans"]) < 1e-12


@pytest.mark.parametrize("S", [5, 65])
@pytest.mark.parametrize("exclusive", [True, False])
def test_product_scan_gradient_vs_bruteforce_with_a_zero_factor(S, exclusive):
    """float64 autograd through cumprod against the double loop that leaves the k-th factor out; ray 11 holds a factor
    of exactly 0 (alpha == 1), where a division-based gradient would be nan"""
    case = VR.alpha_case(S)
    x = (1.0 - case["alphas"]).double()
    assert float(x[case["one"]]) == 0.0 and int(case["ri"][case["one"]]) == VR.ONE_RAY
    xr = x.clone().requires_grad_(True)
    g = case["g"].double()
    (VR.scan(xr, case["ri"], case["R"], True, exclusive) * g).sum().backward()
    brute = VR.prod_grad_bruteforce(x, g, case["ri"], case["R"], exclusive)
    assert bool(torch.isfinite(xr.grad).all())
    eleven = case["ri"] == VR.ONE_RAY
    assert float(brute[eleven].abs().max()) > 0
    assert _rel(xr.grad[eleven], brute[eleven]) < 1e-12 and _rel(xr.grad, brute) < 1e-12


def test_alpha_case_is_what_the_gpu_tests_assume():
    for S in VR.SIZES:
        case = VR.alpha_case(S)
        assert int((case["ri"] == CR.EMPTY_RAY).sum()) == 0 and float(case["alphas"][case["one"]]) == 1.0
        assert int((case["alphas"] < 0).sum()) > 0
        # the visibility thresholds of the GPU test: no float64 value within 1e-6 relative of either
        _, tr = VR.weights_from_alpha(case["alphas"].double(), case["ri"], case["R"])
        near = ((tr - 1e-4).abs() <= 1e-6 * 1e-4) | ((case["alphas"].double() - 0.01).abs() <= 1e-6 * 0.01)
        assert int(near.sum()) == 0


SPAN_NONE = (None, None)  # ray_indices, packed_info


def _entry_points(lib, p):
    """name -> a call of the entry point with `span` = (ray_indices, packed_info, N, R, dense_S) and data pointers `d`
    (None: all data pointers NULL)"""
    return {
        "fsn_packed_scan_fwd": lambda span, d: lib.fsn_packed_scan_fwd(d, *span, L.FSN_SCAN_PROD, 1, d, None),
        "fsn_packed_scan_bwd": lambda span, d: lib.fsn_packed_scan_bwd(d, d, *span, L.FSN_SCAN_PROD, 0, d, None),
        "fsn_packed_weights_fwd": lambda span, d: lib.fsn_packed_weights_fwd(d, d, d, *span, 0, None, d, d, d, None),
        "fsn_packed_weights_bwd": lambda span, d: lib.fsn_packed_weights_bwd(d, d, d, *span, 1, None, d, d, d, d, None),
        "fsn_packed_visibility_alpha": lambda span, d: lib.fsn_packed_visibility_alpha(d, *span, 1e-4, 0.0, d, None),
        "fsn_accumulate_fwd": lambda span, d: lib.fsn_accumulate_fwd(d, d, 3, *span, d, None),
        "fsn_accumulate_bwd": lambda span, d: lib.fsn_accumulate_bwd(d, d, d, 3, *span, d, d, None),
    }


def test_new_entry_points_validate_without_gpu():
    """empty input returns 0; a null pointer returns -1 and the message carries the function's name; two addressing
    modes at once (or none) return -1; nothing is launched: validation comes first"""
    lib = L.lib()
    host = (C.c_int64 * 16)()  # stands for a device array: every call here is refused before anything reads it
    p = C.cast(host, C.c_void_p)
    for name, call in _entry_points(lib, p).items():
        assert call((None, None, 0, 8, 0), None) == 0, name          # N == 0
        assert call((None, None, 8, 0, 0), None) == 0, name          # R == 0
        assert call((p, None, 0, 8, 0), None) == 0, name
        assert call((None, None, -1, 8, 0), None) == -1, name        # bad sizes
        assert call((None, None, 8, 2, -4), None) == -1, name
        assert call((p, None, 8, 2, 0), None) == -1, name            # null data pointers
        msg = lib.fsn_last_error()
        assert name.encode() + b": null pointer" in msg, msg
        assert call((None, None, 8, 2, 4), None) == -1 and name.encode() in lib.fsn_last_error(), name
        for span in ((p, p, 8, 2, 0), (p, None, 8, 2, 4), (None, p, 8, 2, 4), (p, p, 0, 0, 0)):  # two modes at once
            assert call(span, p) == -1, (name, span)
            msg = lib.fsn_last_error()
            assert name.encode() in msg and b"more than one" in msg, msg
        assert call((None, None, 8, 2, 0), p) == -1 and name.encode() in lib.fsn_last_error()  # no addressing at all
        assert call((None, None, 8, 2, 3), p) == -1 and b"dense" in lib.fsn_last_error()  # 8 != 2 * 3
    assert lib.fsn_packed_scan_fwd(p, p, None, 8, 2, 0, 7, 1, p, None) == -1 and b"fsn_packed_scan_fwd: op 7" in lib.fsn_last_error()
    assert lib.fsn_packed_scan_bwd(p, p, p, None, 8, 2, 0, -1, 1, p, None) == -1
    assert lib.fsn_accumulate_fwd(p, None, 3, p, None, 8, 2, 0, p, None) == -1 and b"fsn_accumulate_fwd" in lib.fsn_last_error()
    assert lib.fsn_accumulate_fwd(p, p, 0, p, None, 8, 2, 0, p, None) == -1
    assert lib.fsn_accumulate_bwd(p, p, p, 3, p, None, 8, 2, 0, None, None, None) == -1  # neither output
    assert b"fsn_accumulate_bwd: null pointer" in lib.fsn_last_error()
    pack = lib.fsn_pack_info
    assert pack(None, 0, 8, None, None) == 0 and pack(None, 8, 0, None, None) == 0
    assert pack(None, 8, 2, None, None) == -1 and b"fsn_pack_info: null pointer" in lib.fsn_last_error()
    assert pack(p, 8, 2, None, None) == -1 and pack(None, -1, 2, None, None) == -1


def test_python_layer_refuses_cpu_tensors():
    from fs_nerf_amd.render import volrend as V
    case = VR.alpha_case(5)
    a, ri, R = case["alphas"], case["ri"], case["R"]
    t0, t1 = case["t0"], case["t1"]
    calls = [lambda: V.pack_info(ri, R),
             lambda: V.inclusive_sum(a, indices=ri), lambda: V.exclusive_sum(a.reshape(1, -1)),
             lambda: V.inclusive_prod(a, indices=ri), lambda: V.exclusive_prod(a, indices=ri),
             lambda: V.render_transmittance_from_density(t0, t1, a, ray_indices=ri, n_rays=R),
             lambda: V.render_transmittance_from_alpha(a, ray_indices=ri, n_rays=R),
             lambda: V.render_weight_from_density(t0, t1, a, ray_indices=ri, n_rays=R),
             lambda: V.render_weight_from_alpha(a, ray_indices=ri, n_rays=R),
             lambda: V.render_visibility_from_density(t0, t1, a, ray_indices=ri, n_rays=R),
             lambda: V.render_visibility_from_alpha(a, ray_indices=ri, n_rays=R),
             lambda: V.accumulate_along_rays(a, case["rgb"], ri, R), lambda: V.accumulate_along_rays(a, None, ri, R)]
    for i, call in enumerate(calls):
        with pytest.raises(RuntimeError, match="GPU tensor"):
            call()


def test_rendering_needs_exactly_one_callback_and_sampling_keeps_refusing_alpha_fn():
    import inspect

    from fs_nerf_amd.render import rendering as Rm
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    case = VR.alpha_case(5)
    fn = lambda a, b, c: (case["rgb"], case["alphas"])
    with pytest.raises(ValueError, match="exactly one"):
        Rm.rendering(case["t0"], case["t1"], case["ri"], case["R"])
    with pytest.raises(ValueError, match="exactly one"):
        Rm.rendering(case["t0"], case["t1"], case["ri"], case["R"], rgb_sigma_fn=fn, rgb_alpha_fn=fn)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        Rm.rendering(case["t0"], case["t1"], case["ri"], case["R"], rgb_alpha_fn=fn)
    names = list(inspect.signature(Rm.rendering).parameters)
    assert names[-1] == "rgb_alpha_fn" and names[:7] == ["t_starts", "t_ends", "ray_indices", "n_rays", "rgb_sigma_fn",
                                                         "render_bkgd", "full_grad"]
    est = OccGridEstimator(roi_aabb=torch.tensor([-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]), resolution=16, levels=1)
    with pytest.raises(NotImplementedError):
        est.sampling(torch.zeros(2, 3), torch.ones(2, 3), alpha_fn=lambda a, b, c: a)
