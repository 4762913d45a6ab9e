"""CPU: the equations of the neighbouring-ray KL ("Neighbouring-ray KL") - a ray's termination histogram
over fixed depth bins and the KL divergence between neighbouring pixels of a patch - restated in tests/ray_hist_ref.py:
the closed-form gradients against float64 autograd of the restatements, the float32 loop form against the float64 one,
mass conservation, hand cases; the library's edges against the restatement's, bit for bit; the argument validation of the
six C-ABI entry points, which needs no GPU; and the host layer's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L

import composite_ref as CR
import ray_hist_ref as RH
from test_train_step import _rel

SIZES = [5, 64, 65, 192]
BK = torch.tensor([1.0, 0.5, 0.25])
RANGES = [(2.0, 7.0), (3.0, 5.0)]
SYMBOLS = ("fsn_ray_hist_edges", "fsn_ray_hist_fwd", "fsn_ray_hist_bwd", "fsn_patch_nkl_fwd", "fsn_patch_nkl_bwd",
           "fsn_patch_nkl_pairs")


def _case64(S):
    case = CR.ragged_case(S)
    outs = CR.forward64(case, BK)
    return case, outs


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("bins", [1, 7, 64])
@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("normalize", [True, False])
def test_histogram_closed_form_gradient(S, bins, rng, normalize):
    """the closed-form gradient against float64 autograd through the restatement; ray 7 (s = 0: the gradient is of order
    1 / eps) apart from the rest; nothing below v = 0; ray 3's and ray 7's rows are 0"""
    case, outs = _case64(S)
    ri, R = case["ri"], case["R"]
    t0, t1 = case["t0"].double(), case["t1"].double()
    edges = RH.edges_f32(bins, *rng)
    G = torch.randn(R, bins, generator=torch.Generator().manual_seed(S + bins)).double()
    v = outs["weights"].clone().requires_grad_(True)
    assert int((v.detach() < 0).sum()) > 0
    val = RH.hist_value(v, t0, t1, ri, R, edges, normalize)
    (val * G).sum().backward()
    closed = RH.hist_grad(v.detach(), t0, t1, ri, R, edges, G, normalize)
    seven = ri == CR.ZERO_RAY
    if bins == 1 and normalize and rng == RANGES[0]:
        # one bin over a covering range: P = s / (s + eps), the two terms of the gradient cancel and what is left is
        # rounding noise - measured against the terms themselves, |G_r| / (s_r + eps)
        u = torch.clamp(v.detach(), min=0.0)
        terms = (G[:, 0].abs() / (CR.seg_sum(u, ri, R) + 1e-10))[ri]
        assert float(closed[~seven].abs().max()) < 1e-6 * float(terms[~seven].max())
        assert float((closed - v.grad)[~seven].abs().max()) < 1e-12 * float(terms[~seven].max())
    else:
        assert _rel(closed[~seven], v.grad[~seven]) < 1e-12
    assert float(closed[seven].abs().max()) == 0.0 or _rel(closed[seven], v.grad[seven]) < 1e-12
    assert bool((closed[v.detach() < 0] == 0).all()) and bool((v.grad[v.detach() < 0] == 0).all())
    assert float(val.detach()[CR.EMPTY_RAY].abs().max()) == 0.0 and float(val.detach()[CR.ZERO_RAY].abs().max()) == 0.0
    assert float(val.detach().max()) > 0
    if normalize:
        assert float(val.detach().sum(dim=1).max()) <= 1.0 + 1e-12


@pytest.mark.parametrize("S", [5, 65])
def test_mass_is_conserved_on_a_covering_range_and_dropped_on_a_narrow_one(S):
    """the samples of ragged_case lie in [2, 6]: over [2, 7] sum_b H = sum u within rounding, over [3, 5] some is
    dropped; the float32 loop form agrees with the float64 restatement on shared edges"""
    case, outs = _case64(S)
    ri, R = case["ri"], case["R"]
    assert float(case["t0"].min()) >= 2.0 and float(case["t1"].max()) <= 7.0 and float(case["t1"].max()) > 5.0
    w32 = outs["weights"].float()
    u = torch.clamp(w32.double(), min=0.0)
    mass = CR.seg_sum(u, ri, R)
    for bins in (7, 64):
        full = RH.hist_value(w32.double(), case["t0"].double(), case["t1"].double(), ri, R, RH.edges_f32(bins, 2.0, 7.0), False)
        assert _rel(full.sum(dim=1), mass) < 1e-6  # (the float32 edges tile [2, 7] up to their own rounding)
        part = RH.hist_value(w32.double(), case["t0"].double(), case["t1"].double(), ri, R, RH.edges_f32(bins, 3.0, 5.0), False)
        assert float((mass - part.sum(dim=1)).max()) > 1e-3 and bool((part.sum(dim=1) <= mass + 1e-12).all())
        loop = RH.hist_f32_loop(w32.numpy(), case["t0"].numpy(), case["t1"].numpy(), ri.numpy(), R, bins, 3.0, 5.0)
        e = _rel(torch.from_numpy(loop), part)
        print(f"S={S} bins={bins}: float32 loop against float64 on shared edges {e:.3e}")
        assert e < 1e-5


def _hand(v, t0, t1, bins, t_min, t_max, normalize=False):
    v = torch.tensor(v, dtype=torch.float64)
    t0, t1 = torch.tensor(t0, dtype=torch.float64), torch.tensor(t1, dtype=torch.float64)
    ri = torch.zeros(v.numel(), dtype=torch.int64)
    return RH.hist_value(v, t0, t1, ri, 1, RH.edges_f32(bins, t_min, t_max), normalize)[0]


def test_hand_cases_of_the_histogram():
    """bins of width 1 over [0, 4] (edges exact in float32)"""
    # a sample spanning three bins: [0.5, 2.5) of mass 2 -> 0.5, 1, 0.5
    assert torch.equal(_hand([2.0], [0.5], [2.5], 4, 0.0, 4.0), torch.tensor([0.5, 1.0, 0.5, 0.0], dtype=torch.float64))
    # a sample ending exactly on an edge: nothing in the next bin
    assert torch.equal(_hand([1.0], [1.25], [2.0], 4, 0.0, 4.0), torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float64))
    # a sample reaching past both ends keeps what is inside: [-1, 5) of mass 6 -> 1 per bin
    assert torch.equal(_hand([6.0], [-1.0], [5.0], 4, 0.0, 4.0), torch.ones(4, dtype=torch.float64))
    # width 0, a reversed interval, a NaN and an infinite bound: no mass, gradient 0; the float32 loop agrees
    v = [1.0, 1.0, 1.0, 1.0, 3.0, 2.0]
    t0, t1 = [1.0, 2.0, float("nan"), 0.0, 2.0, 0.25], [1.0, 1.5, 2.0, float("inf"), 3.0, 0.75]
    want = torch.tensor([2.0, 0.0, 3.0, 0.0], dtype=torch.float64)
    assert torch.equal(_hand(v, t0, t1, 4, 0.0, 4.0), want)
    loop = RH.hist_f32_loop(np.array(v), np.array(t0), np.array(t1), np.zeros(6, dtype=np.int64), 1, 4, 0.0, 4.0)
    assert np.array_equal(loop[0], want.numpy().astype(np.float32))
    vt = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    t0t, t1t, ri = torch.tensor(t0, dtype=torch.float64), torch.tensor(t1, dtype=torch.float64), torch.zeros(6, dtype=torch.int64)
    G = torch.tensor([[1.0, 2.0, 3.0, 4.0]], dtype=torch.float64)
    for normalize in (False, True):
        vt.grad = None
        (RH.hist_value(vt, t0t, t1t, ri, 1, RH.edges_f32(4, 0.0, 4.0), normalize) * G).sum().backward()
        closed = RH.hist_grad(vt.detach(), t0t, t1t, ri, 1, RH.edges_f32(4, 0.0, 4.0), G, normalize)
        assert bool((closed[:4] == 0).all()) and bool((vt.grad[:4] == 0).all()) and bool(torch.isfinite(vt.grad).all())
        assert _rel(closed, vt.grad) < 1e-12
    # normalised: P = H / (s + eps), and s counts the mass outside the range too
    p = _hand([1.0, 3.0], [0.0, 5.0], [1.0, 6.0], 4, 0.0, 4.0, normalize=True)
    assert abs(float(p[0]) - 0.25) < 1e-9 and float(p[1:].abs().max()) == 0.0


@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 2, 2), (3, 4, 4), (2, 1, 7), (2, 7, 1), (1, 1, 1)])
@pytest.mark.parametrize("masked", [False, True])
def test_patch_kl_closed_form_gradient(shape, masked):
    """the closed-form gradient against float64 autograd; D(p, p) = 0; (1, 1, 1) has no pair; a masked pixel's pairs are
    skipped: they add nothing to the value and nothing to either pixel's gradient"""
    B, Ph, Pw = shape
    bins = 9
    gen = torch.Generator().manual_seed(sum(shape))
    P = torch.rand(B, Ph, Pw, bins, generator=gen).double()
    P = P * (torch.rand(B, Ph, Pw, bins, generator=gen) > 0.3)  # empty bins: log(eps)
    P = (P / (P.sum(-1, keepdim=True) + 1e-10)).requires_grad_(True)
    G = torch.randn(B, Ph, Pw, generator=gen).double()
    c = None
    if masked:
        c = torch.rand(B, Ph, Pw, generator=gen) > 0.3
        c.reshape(-1)[0] = False
    val = RH.nkl_value(P, c)
    (val * G).sum().backward()
    closed = RH.nkl_grad(P.detach(), G, c)
    n_pairs = RH.pair_count(c, shape)
    if n_pairs == 0:
        assert float(val.detach().abs().max()) == 0.0 and float(closed.abs().max()) == 0.0 and float(P.grad.abs().max()) == 0.0
    else:
        assert _rel(closed, P.grad) < 1e-12 and float(val.detach().abs().max()) > 0
    if not masked:
        assert n_pairs == B * (Ph * (Pw - 1) + (Ph - 1) * Pw)
        same = P.detach()[:, :1, :1].expand(B, Ph, Pw, bins).contiguous()
        assert float(RH.nkl_value(same).abs().max()) == 0.0  # D(p, p) = 0
    else:
        # brute force over the pairs, pixel by pixel
        brute = torch.zeros(B, Ph, Pw, dtype=torch.float64)
        lp = torch.log(P.detach() + 1e-5)
        for b in range(B):
            for i in range(Ph):
                for j in range(Pw):
                    for di, dj in ((0, 1), (1, 0)):
                        if i + di < Ph and j + dj < Pw and bool(c[b, i, j]) and bool(c[b, i + di, j + dj]):
                            brute[b, i, j] += (P.detach()[b, i, j] * (lp[b, i, j] - lp[b, i + di, j + dj])).sum()
        assert float((brute - val.detach()).abs().max()) < 1e-12
        off = ~c
        lonely = off.clone()  # a masked pixel takes part in no pair: gradient 0
        assert float(P.grad[lonely].abs().max()) == 0.0 and float(closed[lonely].abs().max()) == 0.0


def test_the_librarys_edges_are_the_restatements_bit_for_bit():
    from fs_nerf_amd import ops
    for bins, lo, hi in ((1, 2.0, 7.0), (7, 2.0, 7.0), (64, 3.0, 5.0), (65, 2.0, 6.0), (200, 0.05, 1.3), (4096, -3.7, 11.1)):
        got = ops.ray_histogram_edges(bins, t_min=lo, t_max=hi).numpy()
        assert got.dtype == np.float32 and got.shape == (bins + 1,)
        assert np.array_equal(got.view(np.int32), RH.edges_f32(bins, lo, hi).view(np.int32)), (bins, lo, hi)
    assert ops.patch_neighbor_pairs(2, 5, 7) == 2 * (5 * 6 + 4 * 7) and ops.patch_neighbor_pairs(3, 1, 1) == 0


def test_symbols_are_declared_and_exported():
    lib = L.lib()
    for name in SYMBOLS:
        assert name in L.FUNCTIONS and hasattr(lib, name), name


def test_entry_points_validate_without_gpu():
    """null pointers, bad sizes and a bad axis are -1 with the entry point's name; nothing to do is a no-op (nothing is
    launched: validation comes first)"""
    lib = L.lib()
    hf, hb, kf, kb = lib.fsn_ray_hist_fwd, lib.fsn_ray_hist_bwd, lib.fsn_patch_nkl_fwd, lib.fsn_patch_nkl_bwd
    host = (C.c_float * 8)()  # stands for a device array: the call is refused before anything reads it
    idx = (C.c_int64 * 8)()
    p, q = C.cast(host, C.c_void_p), C.cast(idx, C.c_void_p)

    def fwd(N=8, R=2, first=0, rows=2, bins=4, lo=0.0, hi=1.0, eps=1e-10, v=p, ri=q, out=p):
        return hf(v, p, p, ri, N, R, first, rows, bins, lo, hi, 1, eps, out, None)

    def bwd(N=8, R=2, first=0, rows=2, bins=4, lo=0.0, hi=1.0, eps=1e-10, v=p, ri=q, hist=p, g=p, dv=p, normalize=1):
        return hb(v, p, p, ri, N, R, first, rows, bins, lo, hi, normalize, eps, hist, g, dv, None)

    for name, call in (("fsn_ray_hist_fwd", fwd), ("fsn_ray_hist_bwd", bwd)):
        err = lambda text: (name + ": " + text).encode() in lib.fsn_last_error()  # noqa: E731
        assert call(N=0, R=0, rows=0) == 0 and call(N=0, R=0, rows=0, v=None, ri=None) == 0, name
        assert call(N=-1) == -1 and err("bad sizes"), name
        assert call(R=-2) == -1 and err("bad sizes"), name
        assert call(first=1, rows=2) == -1 and err("bad sizes"), name
        assert call(first=-1, rows=1) == -1 and err("bad sizes"), name
        assert call(bins=0) == -1 and err("bad sizes"), name
        assert call(bins=4097) == -1 and err("bad sizes"), name
        assert call(lo=1.0, hi=1.0) == -1 and err("t_min < t_max"), name
        assert call(lo=2.0, hi=1.0) == -1 and err("t_min < t_max"), name
        assert call(hi=float("inf")) == -1 and err("t_min < t_max"), name
        assert call(lo=float("nan")) == -1 and err("t_min < t_max"), name
        assert call(eps=0.0) == -1 and err("eps"), name
        assert call(v=None) == -1 and err("null pointer"), name
        assert call(ri=None) == -1 and err("null pointer"), name
    assert fwd(out=None) == -1 and b"fsn_ray_hist_fwd: null pointer" in lib.fsn_last_error()
    assert bwd(dv=None) == -1 and b"fsn_ray_hist_bwd: null pointer" in lib.fsn_last_error()
    assert bwd(g=None) == -1 and b"fsn_ray_hist_bwd: null pointer" in lib.fsn_last_error()
    assert bwd(hist=None) == -1 and b"fsn_ray_hist_bwd: null pointer" in lib.fsn_last_error()
    assert fwd(rows=0) == 0 and fwd(rows=0, out=None) == 0 and bwd(N=0) == 0 and bwd(N=0, dv=None) == 0
    assert lib.fsn_ray_hist_edges(4, 0.0, 1.0, None) == -1 and b"fsn_ray_hist_edges: null pointer" in lib.fsn_last_error()
    assert lib.fsn_ray_hist_edges(0, 0.0, 1.0, host) == -1 and b"fsn_ray_hist_edges: bad sizes" in lib.fsn_last_error()
    assert lib.fsn_ray_hist_edges(4, 1.0, 0.0, host) == -1 and b"fsn_ray_hist_edges: t_min < t_max" in lib.fsn_last_error()
    assert kf(None, None, 0, 4, 4, 8, 1e-5, None, None) == 0 and kb(None, None, 0, 4, 4, 8, 1e-5, None, None, None) == 0
    assert kf(None, None, 2, 4, 4, 8, 1e-5, None, None) == -1 and b"fsn_patch_nkl_fwd: null pointer" in lib.fsn_last_error()
    assert kb(p, None, 2, 4, 4, 8, 1e-5, None, p, None) == -1 and b"fsn_patch_nkl_bwd: null pointer" in lib.fsn_last_error()
    for B, Ph, Pw, bins in ((-1, 4, 4, 8), (2, 0, 4, 8), (2, 4, 0, 8), (2, 4, 4, 0), (2, 4, 4, 4097), (1 << 40, 4, 4, 8)):
        assert kf(p, None, B, Ph, Pw, bins, 1e-5, p, None) == -1 and b"fsn_patch_nkl_fwd: bad sizes" in lib.fsn_last_error()
        assert kb(p, None, B, Ph, Pw, bins, 1e-5, p, p, None) == -1 and b"fsn_patch_nkl_bwd: bad sizes" in lib.fsn_last_error()
    assert kf(p, None, 2, 4, 4, 8, 0.0, p, None) == -1 and b"fsn_patch_nkl_fwd: eps" in lib.fsn_last_error()
    assert lib.fsn_patch_nkl_pairs(2, 0, 4) == -1 and lib.fsn_patch_nkl_pairs(2, 3, 4) == 2 * (3 * 3 + 2 * 4)


def test_host_layer_refusals():
    from fs_nerf_amd import ops
    from fs_nerf_amd.core.loss import NeighborRayKLLoss
    case = CR.ragged_case(5)
    N, R, ri, t0, t1 = case["sig"].numel(), case["R"], case["ri"], case["t0"], case["t1"]
    v = torch.rand(N)
    with pytest.raises(RuntimeError):
        ops.ray_histogram(v, t0, t1, ri, R, t_min=2.0, t_max=7.0)
    with pytest.raises(RuntimeError):
        ops.patch_neighbor_kl(torch.rand(2, 5, 7, 8))
    with pytest.raises(RuntimeError):
        NeighborRayKLLoss(t_min=2.0, t_max=7.0)(v, t0, t1, ri, R, (2, 5, 7))
    with pytest.raises(TypeError):
        ops.ray_histogram(v, t0, t1, ri, R)  # t_min and t_max are required
    for kw in (dict(t_min=2.0, t_max=2.0), dict(t_min=3.0, t_max=2.0), dict(t_min=2.0, t_max=float("inf")),
               dict(t_min=2.0, t_max=7.0, bins=0), dict(t_min=2.0, t_max=7.0, bins=4097),
               dict(t_min=2.0, t_max=7.0, rays=(60, 11)), dict(t_min=2.0, t_max=7.0, rays=(-1, 4)),
               dict(t_min=2.0, t_max=7.0, eps=0.0)):
        with pytest.raises(ValueError):
            ops.ray_histogram(v, t0, t1, ri, R, **kw)
    with pytest.raises(ValueError):
        ops.ray_histogram(v[:-1], t0, t1, ri, R, t_min=2.0, t_max=7.0)
    with pytest.raises(ValueError):
        NeighborRayKLLoss(t_min=7.0, t_max=2.0)
    with pytest.raises(ValueError):
        NeighborRayKLLoss(bins=0, t_min=2.0, t_max=7.0)
    with pytest.raises(ValueError):
        ops.patch_neighbor_kl(torch.rand(5, 7, 8))
    with pytest.raises(ValueError):
        ops.patch_neighbor_kl(torch.rand(2, 5, 7, 8), pair_weight=torch.ones(2, 5, 6))
    with pytest.raises(ValueError):
        NeighborRayKLLoss(t_min=2.0, t_max=7.0)(v, t0, t1, ri, R, (2, 5, 7), opacity=torch.rand(69))
