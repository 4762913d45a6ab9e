"""TEST INFRASTRUCTURE ONLY: torch restatements (CPU, per-ray loops over torch.cumsum / torch.cumprod) of what
csrc/packed_scan.hip computes, and the inputs the CPU and GPU tests of render/volrend.py share.  The restatements are
differentiable in whatever dtype they are given: in float64, autograd through them is the truth for every gradient.

Density inputs: composite_ref.ragged_case(S) - 70 rays x S in {5, 64, 65, 192}, 20 % of the samples dropped, ray 3
empty, ray 7 all-zero sigma, 5 % negative sigmas.  Alpha inputs: the same rays with alphas = rand * min(1, 8/S), 5 %
negated, ONE alpha of exactly 1.0 in the middle of ray 11 (a zero factor of the transmittance product).  Scan inputs:
randn (sum) and rand + 0.5 (prod)."""
import functools

import torch

import composite_ref as CR

SIZES = [5, 64, 65, 192]
ONE_RAY = 11  # holds the alpha of exactly 1.0
EPS = CR.EPS


def ray_slices(ri, n_rays):
    """[(start, stop)] of every ray in the sorted ri"""
    counts = torch.bincount(ri, minlength=n_rays)[:n_rays]
    stops = torch.cumsum(counts, 0)
    return [(int(e - c), int(e)) for c, e in zip(counts, stops)]


def scan(x, ri, n_rays, prod, exclusive):
    """per-ray inclusive / exclusive sum / product of the flat x"""
    out = []
    for a, b in ray_slices(ri, n_rays):
        if b == a:
            continue
        seg = x[a:b]
        inc = torch.cumprod(seg, 0) if prod else torch.cumsum(seg, 0)
        if exclusive:
            first = torch.ones(1, dtype=x.dtype) if prod else torch.zeros(1, dtype=x.dtype)
            inc = torch.cat([first, inc[:-1]])
        out.append(inc)
    return torch.cat(out) if out else x[:0]


def prod_grad_bruteforce(x, g, ri, n_rays, exclusive):
    """d/dx_k of sum_m g_m out_m for the per-ray product scan, by the O(S^2) double loop with the k-th factor left out
    (no division: a zero factor is fine)"""
    d = torch.zeros_like(x)
    for a, b in ray_slices(ri, n_rays):
        for k in range(a, b):
            seg = x[a:b].clone()
            seg[k - a] = 1.0  # every out_m that holds x_k, with that factor left out (the inner loop, over m at once)
            without = torch.cumprod(seg, 0)
            if exclusive:  # out_m = prod x[a:m]: holds x_k for m > k
                d[k] = (g[k + 1:b] * without[k - a:b - a - 1]).sum()
            else:  # out_m = prod x[a:m+1]: holds x_k for m >= k
                d[k] = (g[k:b] * without[k - a:]).sum()
    return d


def weights_from_density(sig, t0, t1, ri, n_rays, prefix=None):
    """-> (weights, trans, alphas)"""
    sdt = sig * (t1 - t0)
    alphas = 1.0 - torch.exp(-sdt)
    trans = torch.exp(-scan(sdt, ri, n_rays, False, True))
    if prefix is not None:
        trans = trans * prefix
    return trans * alphas, trans, alphas


def weights_from_alpha(alphas, ri, n_rays, prefix=None):
    """-> (weights, trans)"""
    trans = scan(1.0 - alphas, ri, n_rays, True, True)
    if prefix is not None:
        trans = trans * prefix
    return trans * alphas, trans


def accumulate(w, v, ri, n_rays):
    """-> [n_rays, C]; v None: the sum of the weights"""
    v = torch.ones(w.numel(), 1, dtype=w.dtype) if v is None else v
    return torch.zeros(n_rays, v.shape[-1], dtype=w.dtype).index_add(0, ri, w[:, None] * v)


def rendering_from_alpha(rgbs, alphas, t0, t1, ri, n_rays, bkgd=None):
    """-> (colors, opacity, depth, weights, trans)"""
    w, tr = weights_from_alpha(alphas, ri, n_rays)
    colors, opacity = accumulate(w, rgbs, ri, n_rays), accumulate(w, None, ri, n_rays)
    depth = accumulate(w, ((t0 + t1) / 2.0)[:, None], ri, n_rays) / torch.clamp(opacity, min=EPS)
    if bkgd is not None:
        colors = colors + bkgd.to(colors.dtype) * (1.0 - opacity)
    return colors, opacity, depth, w, tr


@functools.lru_cache(maxsize=None)
def density_case(S):
    """composite_ref.ragged_case(S) with a prefix_trans in (0.5, 1] and per-sample cotangents (float32, CPU)"""
    case = dict(CR.ragged_case(S))
    cot = CR.random_cotangents(case, 100 + S)
    gen = torch.Generator().manual_seed(300 + S)
    case["prefix"] = 0.5 + 0.5 * torch.rand(case["sig"].numel(), generator=gen)
    case["cot"] = {k: cot[k] for k in ("weights", "trans", "alphas")}
    return case


@functools.lru_cache(maxsize=None)
def alpha_case(S):
    """the rays of ragged_case(S) with alphas = rand * min(1, 8/S), 5 % negated, one alpha == 1.0 in the middle of ray
    11, ray 3 empty; rgbs, cotangents and the scan inputs on the same rays (float32, CPU)"""
    base = CR.ragged_case(S)
    ri, N, R = base["ri"], base["ri"].numel(), base["R"]
    gen = torch.Generator().manual_seed(200 + S)
    alphas = torch.rand(N, generator=gen) * min(1.0, 8.0 / S)
    flip = torch.rand(N, generator=gen) < 0.05
    alphas = torch.where(flip, -alphas, alphas)
    a, b = ray_slices(ri, R)[ONE_RAY]
    assert b - a >= 3
    one = (a + b) // 2
    alphas[one] = 1.0
    rnd = lambda *shape: torch.randn(*shape, generator=gen)
    return dict(ri=ri, t0=base["t0"], t1=base["t1"], R=R, N=N, alphas=alphas, one=one, rgb=torch.rand(N, 3, generator=gen),
                x_sum=rnd(N), x_prod=torch.rand(N, generator=gen) + 0.5, g=rnd(N), g2=rnd(N),
                prefix=0.5 + 0.5 * torch.rand(N, generator=gen),
                values={C: rnd(N, C) for C in (1, 3, 7)}, g_rays={C: rnd(R, C) for C in (1, 3, 7)})


@functools.lru_cache(maxsize=None)
def dense_case(S, R=9):
    """dense [R, S] rows (nothing dropped): the three addressing modes describe the same rays"""
    gen = torch.Generator().manual_seed(400 + S)
    ri = torch.arange(R).repeat_interleave(S)
    t0 = 2.0 + 4.0 * torch.arange(S, dtype=torch.float32)[None, :].expand(R, S) / S + 0.01 * torch.rand(R, 1, generator=gen)
    return dict(R=R, S=S, ri=ri, t0=t0.reshape(-1).contiguous(), t1=(t0 + 4.0 / S).reshape(-1).contiguous(),
                sig=torch.rand(R * S, generator=gen) * (0.15 * S), alphas=torch.rand(R * S, generator=gen) * min(1.0, 8.0 / S),
                x_sum=torch.randn(R * S, generator=gen), x_prod=torch.rand(R * S, generator=gen) + 0.5,
                g=torch.randn(R * S, generator=gen))
