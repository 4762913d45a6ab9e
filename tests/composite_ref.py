"""TEST INFRASTRUCTURE ONLY: float64 torch restatements (CPU, per-ray cumsums) of what csrc/composite_grad.hip
computes - the closed-form FULL backward of the packed compositor and the distortion loss with its closed-form
gradient - plus the brute-force O(S^2) distortion and the ragged test inputs the CPU and GPU tests share.

The truth these are checked against is autograd on oracle.rendering_packed (tests/test_composite_grad_cpu.py); the GPU
kernels are checked against that autograd and against the functions here (tests/test_composite_grad_gpu.py)."""
import torch

from oracle import fsnerf_oracle as O

EPS = O.FLT_EPS


def _segments(ri, n_rays):
    """(dense row, dense column, number of columns) of every packed sample: samples of a ray are contiguous."""
    N = ri.numel()
    first = torch.ones(N, dtype=torch.bool)
    first[1:] = ri[1:] != ri[:-1]
    seg_first = torch.nonzero(first).reshape(-1)
    seg_id = torch.cumsum(first.to(torch.int64), 0) - 1
    pos = torch.arange(N) - seg_first[seg_id]
    return seg_id, pos, int(pos.max()) + 1


def seg_excl_cumsum(x, ri, n_rays):
    """per-ray exclusive running sum of the packed x [N] (restarted at every ray boundary, no global cumsum)"""
    if x.numel() == 0:
        return x.clone()
    seg_id, pos, m = _segments(ri, n_rays)
    dense = torch.zeros(int(seg_id[-1]) + 1, m, dtype=x.dtype)
    dense = dense.index_put((seg_id, pos), x)
    return (torch.cumsum(dense, dim=1) - dense)[seg_id, pos]


def seg_sum(x, ri, n_rays):
    return torch.zeros(n_rays, dtype=x.dtype).index_add(0, ri, x)


def composite_bwd_closed(sig, rgb, t0, t1, ri, n_rays, bkgd=None, g=None, g_O=None, g_D=None, u=None, a=None, tau=None):
    """Closed-form backward of oracle.rendering_packed -> (dL/dsigmas [N], dL/drgbs [N,3]) from the cotangents of
    colors g [R,3], opacity g_O [R], depth g_D [R], weights u [N], alphas a [N], trans tau [N] (None = zero)."""
    dt_ = sig.dtype
    N = sig.numel()
    zR, zN = torch.zeros(n_rays, dtype=dt_), torch.zeros(N, dtype=dt_)
    g = torch.zeros(n_rays, 3, dtype=dt_) if g is None else g
    g_O, g_D = (zR if v is None else v.reshape(-1) for v in (g_O, g_D))
    u, a, tau = (zN if v is None else v for v in (u, a, tau))
    b = torch.zeros(3, dtype=dt_) if bkgd is None else bkgd.to(dt_)
    delta, m = t1 - t0, (t0 + t1) / 2.0
    s = sig * delta
    T = torch.exp(-seg_excl_cumsum(s, ri, n_rays))
    e = torch.exp(-s)
    alpha = 1.0 - e
    w = T * alpha
    Op = seg_sum(w, ri, n_rays)
    D = seg_sum(w * m, ri, n_rays) / torch.clamp(Op, min=EPS)
    regular = (Op >= EPS)[ri]
    k = torch.where(regular, (m - D[ri]) / torch.where(regular, Op[ri], torch.ones_like(Op[ri])), m / EPS)
    q = (rgb * g[ri]).sum(-1) - (g @ b)[ri] + g_O[ri] + g_D[ri] * k + u
    A = q * T + a
    BT = (q * alpha + tau) * T
    suffix = seg_sum(BT, ri, n_rays)[ri] - seg_excl_cumsum(BT, ri, n_rays) - BT
    return delta * (A * e - suffix), w[:, None] * g[ri]


def distortion_value(w, t0, t1, ri, n_rays):
    """L_r = sum_i [ 2 w_i (m_i W_i - V_i) + w_i^2 dt_i / 3 ] -> [n_rays]; differentiable torch ops."""
    m = (t0 + t1) / 2.0
    W, V = seg_excl_cumsum(w, ri, n_rays), seg_excl_cumsum(w * m, ri, n_rays)
    return seg_sum(2.0 * w * (m * W - V) + w * w * (t1 - t0) / 3.0, ri, n_rays)


def distortion_grad(w, t0, t1, ri, n_rays, g=None):
    """closed form dL/dw_k = g_r ( 2 (m_k W_k - V_k + V'_k - m_k W'_k) + 2 w_k dt_k / 3 )"""
    m = (t0 + t1) / 2.0
    W, V = seg_excl_cumsum(w, ri, n_rays), seg_excl_cumsum(w * m, ri, n_rays)
    Ws, Vs = seg_sum(w, ri, n_rays)[ri] - W - w, seg_sum(w * m, ri, n_rays)[ri] - V - w * m
    d = 2.0 * (m * W - V + Vs - m * Ws) + 2.0 * w * (t1 - t0) / 3.0
    return d if g is None else d * g.reshape(-1)[ri]


def distortion_bruteforce(w, t0, t1, ri, n_rays):
    """sum_i sum_j w_i w_j |m_i - m_j| + sum_i w_i^2 dt_i / 3 per ray, O(S^2) (equal to distortion_value for midpoints
    sorted within the ray)"""
    out = torch.zeros(n_rays, dtype=w.dtype)
    m = (t0 + t1) / 2.0
    for r in range(n_rays):
        sel = ri == r
        wr, mr = w[sel], m[sel]
        out[r] = (wr[:, None] * wr[None, :] * (mr[:, None] - mr[None, :]).abs()).sum() + (wr * wr * (t1 - t0)[sel]).sum() / 3.0
    return out


R_CASE, EMPTY_RAY, ZERO_RAY = 70, 3, 7


def ragged_case(S, seed=None, density=0.15):
    """The packed test inputs (float32, CPU): 70 rays x S stratified samples in [2, 6], sigma = rand * density S, then about
    20 % of the samples dropped at random, every sample of ray 3 dropped (an empty ray), every sigma of ray 7 set to 0
    (opacity exactly 0: the O < eps branch of the depth gradient) and about 5 % of the remaining sigmas flipped to
    -0.1 sigma (the network emits raw sigma).  -> dict(ri, t0, t1, sig, rgb, R)"""
    gen = torch.Generator().manual_seed(S if seed is None else seed)
    R = R_CASE
    edges = O.stratified_edges(2.0, 6.0, S, R, torch.rand(R, generator=gen))
    ri, t0, t1 = O.edges_to_packed(edges)
    sig = torch.rand(R * S, generator=gen) * (density * S)
    rgb = torch.rand(R * S, 3, generator=gen)
    keep = torch.rand(R * S, generator=gen) > 0.2
    keep[ri == EMPTY_RAY] = False
    flip = torch.rand(R * S, generator=gen) < 0.05
    sig = torch.where(flip, -0.1 * sig, sig)
    sig[ri == ZERO_RAY] = 0.0
    return dict(ri=ri[keep].contiguous(), t0=t0[keep].contiguous(), t1=t1[keep].contiguous(), sig=sig[keep].contiguous(),
                rgb=rgb[keep].contiguous(), R=R)


COTANGENTS = ("colors", "opacity", "depth", "weights", "alphas", "trans")


def random_cotangents(case, seed):
    """float32 random cotangents of the six outputs, keyed like COTANGENTS"""
    gen = torch.Generator().manual_seed(seed)
    R, N = case["R"], case["sig"].numel()
    return dict(colors=torch.randn(R, 3, generator=gen), opacity=torch.randn(R, 1, generator=gen),
                depth=torch.randn(R, 1, generator=gen), weights=torch.randn(N, generator=gen),
                alphas=torch.randn(N, generator=gen), trans=torch.randn(N, generator=gen))


def forward64(case, bkgd):
    """oracle.rendering_packed on the case in float64 -> outputs dict (detached)"""
    c, o, d, ex = O.rendering_packed(case["t0"].double(), case["t1"].double(), case["ri"], case["R"],
                                     lambda a, b, i: (case["rgb"].double(), case["sig"].double()),
                                     None if bkgd is None else bkgd.double())
    return dict(colors=c, opacity=o, depth=d, weights=ex["weights"], alphas=ex["alphas"], trans=ex["trans"])


def autograd_reference(case, cot, bkgd):
    """float64 autograd on oracle.rendering_packed of sum_k <cot[k], output k> over the cotangents present in `cot`
    -> (d_sigmas, d_rgbs, outputs dict in float64)"""
    s64 = case["sig"].double().requires_grad_(True)
    r64 = case["rgb"].double().requires_grad_(True)
    c, o, d, ex = O.rendering_packed(case["t0"].double(), case["t1"].double(), case["ri"], case["R"],
                                     lambda a, b, i: (r64, s64), None if bkgd is None else bkgd.double())
    outs = dict(colors=c, opacity=o, depth=d, weights=ex["weights"], alphas=ex["alphas"], trans=ex["trans"])
    loss = sum((outs[k] * v.double()).sum() for k, v in cot.items())
    gs, gr = torch.autograd.grad(loss, (s64, r64), allow_unused=True)
    gs = torch.zeros_like(s64) if gs is None else gs
    gr = torch.zeros_like(r64) if gr is None else gr
    return gs, gr, {k: v.detach() for k, v in outs.items()}
