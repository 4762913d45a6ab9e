"""CPU: the proposal-network sampler's restatements (tests/propnet_ref.py) have the properties the kernels are held to,
the "propnet" route is taken exactly for a PropNetEstimator, the new entry points validate their arguments without a
GPU, and the Python surface refuses CPU tensors and the packed form."""
import ctypes as C

import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L

import propnet_ref as PR


@pytest.mark.parametrize("S", PR.S_SIZES)
def test_restated_sampler_is_sorted_and_inside_the_support(S):
    case = PR.histogram_case(S)
    v, c = case["s_edges"], case["cdfs"]
    assert bool((c[:, 1:] >= c[:, :-1]).all()) and bool((c[:, 0] == 0).all()) and bool((c[:, -1] == 1).all())
    for n in PR.N_SIZES:
        for b in (None, case["b"]):
            e, x = PR.importance_sample_f32(v, c, n, b)
            assert e.shape == (PR.R, n + 1) and x.shape == (PR.R, n) and e.dtype == torch.float32
            assert bool((e[:, 1:] >= e[:, :-1]).all()), (S, n)
            assert bool((x[:, 1:] >= x[:, :-1]).all()), (S, n)
            assert bool((e >= v[:, :1]).all()) and bool((e <= v[:, -1:]).all()), (S, n)
            assert bool((x >= v[:, :1]).all()) and bool((x <= v[:, -1:]).all()), (S, n)
            if n > 1:  # every centre lies in its own interval
                assert bool((x >= e[:, :-1]).all()) and bool((x <= e[:, 1:]).all()), (S, n)
            for tf in ("uniform", "lindisp"):
                t = PR.stot_f32(tf, e, PR.NEAR, PR.FAR)
                assert bool((t[:, 1:] >= t[:, :-1]).all()) and float(t.min()) >= PR.NEAR - 1e-5 and float(t.max()) <= PR.FAR + 1e-5
    e, _ = PR.importance_sample_f32(v, c, 1, case["b"])
    assert torch.equal(e, torch.stack([v[:, 0], v[:, -1]], 1))


def test_first_level_is_a_uniform_lattice():
    unit = torch.tensor([0.0, 1.0]).expand(PR.R, 2).contiguous()
    for n in PR.N_SIZES[1:]:
        e, x = PR.importance_sample_f32(unit, unit, n)
        assert torch.allclose(e, torch.linspace(0, 1, n + 1).expand(PR.R, -1), atol=2e-7, rtol=0)
        assert torch.allclose(x, ((torch.arange(n) + 0.5) / n).expand(PR.R, -1), atol=2e-7, rtol=0)
        assert bool((e[:, 0] == 0).all()) and bool((e[:, -1] <= 1).all())


def test_searchsorted_definition():
    keys = torch.tensor([[0.0, 0.25, 0.25, 1.0]])
    q = torch.tensor([[-1.0, 0.0, 0.1, 0.25, 0.5, 1.0, 2.0]])
    il, ir = PR.searchsorted_ref(keys, q)
    assert il.tolist() == [[0, 0, 0, 2, 2, 3, 3]] and ir.tolist() == [[0, 1, 1, 3, 3, 3, 3]]


@pytest.mark.parametrize("S", PR.S_SIZES)
def test_loss_is_zero_on_itself_and_on_a_coarsening(S):
    case = PR.histogram_case(S)
    k, ck = case["s_edges"].double(), case["cdfs"].double()
    assert float(PR.pdf_loss64(k, ck, k, ck).abs().max()) == 0.0
    if S >= 5:  # the key histogram keeps every other edge of the query's (and both ends)
        keep = sorted(set(range(0, S + 1, 2)) | {S})
        assert float(PR.pdf_loss64(k, ck, k[:, keep], ck[:, keep]).abs().max()) == 0.0


@pytest.mark.parametrize("S,n", [(5, 7), (64, 65), (192, 200), (1, 1), (65, 64)])
def test_analytic_gather_gradient_equals_autograd(S, n):
    case = PR.loss_case(S, n)
    q, cq, k, g = (case[x].double() for x in ("q", "cq", "k", "g"))
    ck = case["ck"].double().requires_grad_(True)
    loss = PR.pdf_loss64(q, cq, k, ck)
    (auto,) = torch.autograd.grad((loss * g).sum(), ck)
    mine = PR.pdf_loss_grad64(q, cq, k, ck.detach(), g)
    assert float((auto - mine).abs().max()) <= 1e-12 * max(1.0, float(auto.abs().max()))
    if n >= 7:
        assert float((loss > 0).double().mean()) > 0.1 and float(auto.abs().max()) > 0  # the gradient is exercised


def test_propnet_route_and_the_pinned_routes():
    from torch import nn
    from fs_nerf_amd.core.models import NeRF
    from fs_nerf_amd.render import rendering as Rm
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    from fs_nerf_amd.render.propnet import PropNetEstimator
    mk = lambda: NeRF(3, 3, 2, 16, (), pos_fn={"n_freqs": 2, "log_space": True}, dir_fn={"n_freqs": 1, "log_space": True})
    est = PropNetEstimator(prop_models=[mk()], prop_samples=(8,), num_samples=4, near_plane=2.0, far_plane=6.0)
    assert isinstance(est, nn.Module) and len(list(est.parameters())) > 0 and est.proposal_requires_grad is True
    for model, fine, grad, extras, opts in ((mk(), None, False, True, None), (mk(), mk(), True, False, None),
                                            (nn.Linear(3, 4), None, True, True, {"cone_angle": 0.01})):
        assert Rm._rays_route(est, model, fine, grad, extras, 4096, 5e-3, opts) == "propnet"
    assert Rm._frame_route(est, mk(), None, False, False, 5e-3, None) == "chunked"
    # what tests/test_render_routes_cpu.py pins, by name
    model = mk()
    strat, occ = Rm.StratifiedEstimator(2.0, 6.0, 8, 16), OccGridEstimator([-1.5] * 3 + [1.5] * 3, resolution=16)
    assert Rm._rays_route(strat, model, None, False, True, 64, 5e-3) == "stratified-fused"
    assert Rm._rays_route(strat, model, None, True, True, 64, 5e-3) == "stratified-sampler"
    assert Rm._rays_route(occ, model, None, False, False, 64, 5e-3) == "occ-frame"
    assert Rm._rays_route(occ, model, None, False, True, 64, 5e-3) == "occ-extras"
    assert Rm._rays_route(occ, model, None, True, True, 4096, 5e-3) == "occ-sampler"
    assert Rm._rays_route(occ, model, None, True, True, 64, 5e-3) == "estimator-sampling"
    assert Rm._rays_route(occ, model, None, False, True, 64, 5e-3, {"cone_angle": 0.01}) == "estimator-sampling"
    with pytest.raises(ValueError):
        PropNetEstimator(prop_models=[mk()], prop_samples=(8, 4))
    with pytest.raises(ValueError):
        PropNetEstimator(sampling_type="log")
    assert float(PropNetEstimator().compute_loss(torch.zeros(3, 4))) == 0.0
    assert PropNetEstimator().update_every_n_steps(torch.zeros(3, 4), requires_grad=True) == 0.0


def test_entry_points_validate_without_gpu():
    lib = L.lib()
    f = (C.c_float * 8)()
    i = (C.c_int64 * 8)()
    N, U, LD = L.FSN_STOT_NONE, L.FSN_STOT_UNIFORM, L.FSN_STOT_LINDISP
    cap = L.FSN_PROP_MAX_ROW
    assert cap >= 1024
    # R == 0: nothing to do, whatever the pointers
    assert lib.fsn_importance_sample(None, None, 0, 4, 4, None, N, 0.0, 0.0, None, None, None, None) == 0
    assert lib.fsn_prop_resample(None, None, None, 0, 4, 4, None, LD, 2.0, 6.0, None, None, None, None, None) == 0
    assert lib.fsn_searchsorted_dense(None, None, 0, 4, 4, None, None, None) == 0
    assert lib.fsn_prop_loss_fwd(None, None, None, None, 0, 4, 4, None, None) == 0
    assert lib.fsn_prop_loss_bwd(None, None, None, None, None, 0, 4, 4, None, None) == 0
    # null pointers
    assert lib.fsn_importance_sample(None, f, 1, 1, 1, None, N, 0.0, 0.0, f, None, None, None) == -1
    assert b"fsn_importance_sample: null" in lib.fsn_last_error()
    assert lib.fsn_importance_sample(f, f, 1, 1, 1, None, U, 2.0, 6.0, f, None, None, None) == -1  # transform without t_edges
    assert lib.fsn_prop_resample(f, f, None, 1, 1, 1, None, N, 0.0, 0.0, f, f, None, None, None) == -1
    assert b"fsn_prop_resample: null" in lib.fsn_last_error()
    assert lib.fsn_searchsorted_dense(f, f, 1, 2, 2, None, i, None) == -1
    assert b"fsn_searchsorted_dense: null" in lib.fsn_last_error()
    assert lib.fsn_prop_loss_fwd(f, f, f, f, 1, 1, 1, None, None) == -1
    assert lib.fsn_prop_loss_bwd(f, f, f, f, None, 1, 1, 1, f, None) == -1
    assert b"fsn_prop_loss_bwd: null" in lib.fsn_last_error()
    # bad sizes
    for S, n in ((0, 4), (4, 0), (-1, 4)):
        assert lib.fsn_importance_sample(f, f, 1, S, n, None, N, 0.0, 0.0, f, None, None, None) == -1
        assert b"bad sizes" in lib.fsn_last_error()
        assert lib.fsn_prop_resample(f, f, f, 1, S, n, None, N, 0.0, 0.0, f, f, None, None, None) == -1
        assert lib.fsn_prop_loss_fwd(f, f, f, f, 1, n, S, f, None) == -1
        assert lib.fsn_prop_loss_bwd(f, f, f, f, f, 1, n, S, f, None) == -1
    assert lib.fsn_importance_sample(f, f, -1, 1, 1, None, N, 0.0, 0.0, f, None, None, None) == -1
    assert lib.fsn_searchsorted_dense(f, f, 1, 0, 2, i, i, None) == -1
    assert lib.fsn_importance_sample(f, f, 1, 1, 1, None, 7, 0.0, 0.0, f, None, f, None) == -1
    # lindisp needs a positive near plane
    assert lib.fsn_importance_sample(f, f, 1, 1, 1, None, LD, 0.0, 6.0, f, None, f, None) == -1
    assert b"lindisp" in lib.fsn_last_error()
    assert lib.fsn_prop_resample(f, f, f, 1, 1, 1, None, LD, -1.0, 6.0, f, f, None, f, None) == -1
    # rows over the cap: unsupported, by name
    for S, n in ((cap + 1, 4), (4, cap + 1)):
        assert lib.fsn_importance_sample(f, f, 1, S, n, None, N, 0.0, 0.0, f, None, None, None) == -2
        assert b"fsn_importance_sample: rows of" in lib.fsn_last_error()
        assert lib.fsn_prop_resample(f, f, f, 1, S, n, None, N, 0.0, 0.0, f, f, None, None, None) == -2
        assert b"fsn_prop_resample: rows of" in lib.fsn_last_error()
        assert lib.fsn_prop_loss_fwd(f, f, f, f, 1, n, S, f, None) == -2
        assert b"fsn_prop_loss_fwd: rows of" in lib.fsn_last_error()
        assert lib.fsn_prop_loss_bwd(f, f, f, f, f, 1, n, S, f, None) == -2
        assert b"fsn_prop_loss_bwd: rows of" in lib.fsn_last_error()


def test_python_surface_refuses_cpu_tensors_and_the_packed_form():
    from fs_nerf_amd.render import pdf
    from fs_nerf_amd.render.propnet import PropNetEstimator, _pdf_loss, _transform_stot
    v = torch.tensor([[0.0, 0.5, 1.0]])
    c = torch.tensor([[0.0, 0.3, 1.0]])
    with pytest.raises(RuntimeError):
        pdf.importance_sampling(pdf.RayIntervals(vals=v), c, 4)
    with pytest.raises(RuntimeError):
        pdf.searchsorted(pdf.RayIntervals(vals=v), pdf.RaySamples(vals=c))
    with pytest.raises(RuntimeError):
        _pdf_loss(pdf.RayIntervals(vals=v), c, pdf.RayIntervals(vals=v), c)
    with pytest.raises(RuntimeError):
        PropNetEstimator().sampling([], [], 4, 2, 2.0, 6.0, device="cpu")
    packed = pdf.RayIntervals(vals=v.reshape(-1), packed_info=torch.tensor([[0, 3]]))
    with pytest.raises(NotImplementedError, match="dense"):
        pdf.importance_sampling(packed, c.reshape(-1), 4)
    with pytest.raises(NotImplementedError, match="dense"):
        pdf.searchsorted(packed, pdf.RaySamples(vals=c))
    with pytest.raises(NotImplementedError, match="dense"):
        pdf.importance_sampling(pdf.RayIntervals(vals=v), c, torch.tensor([4]))
    s = torch.tensor([0.0, 0.5, 1.0])
    assert torch.equal(_transform_stot("uniform", s, 2.0, 6.0), torch.tensor([2.0, 4.0, 6.0]))
    assert torch.allclose(_transform_stot("lindisp", s, 2.0, 6.0), torch.tensor([2.0, 3.0, 6.0]))
    assert torch.equal(_transform_stot("lindisp", s, 2.0, 6.0), PR.stot_f32("lindisp", s, 2.0, 6.0))
