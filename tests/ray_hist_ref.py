"""TEST INFRASTRUCTURE ONLY: restatements of what csrc/ray_hist.hip computes - a ray's termination histogram over fixed
depth bins and the KL divergence between neighbouring pixels of a patch ("Neighbouring-ray KL").  Three
references:

  * `hist_f32_loop`: the UNNORMALISED histogram in float32 NumPy, sequential loops, the kernel's operation order - the
    kernel is compared with it bit for bit;
  * `hist_value` / `hist_grad` / `nkl_value` / `nkl_grad` / `loss_value`: torch restatements in any float dtype (float64
    in the tests) with the closed-form gradients.  They take the float32 edges `edges_f32` AS GIVEN (cast, never
    recomputed): with edges recomputed in float64 the histogram differs by 2.5e-5 of its largest entry, with shared
    edges float32 arithmetic is within 6.9e-7;
  * the same `*_value` functions are differentiable torch, so float64 autograd through them is the third.

The closed forms are checked against autograd in tests/test_ray_hist_cpu.py, the GPU kernels against all three in
tests/test_ray_hist_gpu.py."""
import numpy as np
import torch

from composite_ref import seg_sum


def edges_f32(bins, t_min, t_max):
    """h = (t_max - t_min) / bins, e_b = t_min + (float)b h, every step float32 -> numpy float32 [bins + 1]"""
    lo, hi = np.float32(t_min), np.float32(t_max)
    h = np.float32(np.float32(hi - lo) / np.float32(bins))
    return np.array([np.float32(lo + np.float32(np.float32(b) * h)) for b in range(bins + 1)], dtype=np.float32)


def hist_f32_loop(v, t0, t1, ri, n_rays, bins, t_min, t_max):
    """H [n_rays, bins] in float32, as the kernel sums it: per ray and bin ONE sequential sum over the ray's samples in
    ascending order, from +0; u = max(v, 0), f = max(min(c, e1) - max(a, e0), 0) / (c - a), term = u f.  The loop runs
    over the packed samples (a ray's are contiguous and ascending); each step updates all bins of the sample's ray at
    once - elementwise float32 operations, so every bin still sees exactly the kernel's sequence of roundings."""
    f32 = np.float32
    v, t0, t1 = (np.asarray(x, dtype=np.float32) for x in (v, t0, t1))
    ri = np.asarray(ri)
    e = edges_f32(bins, t_min, t_max)
    e0, e1 = e[:-1], e[1:]
    H = np.zeros((n_rays, bins), dtype=np.float32)
    zero = f32(0.0)
    with np.errstate(all="ignore"):
        for i in range(v.shape[0]):
            a, c = t0[i], t1[i]
            d = f32(c - a)
            if not (np.isfinite(a) and np.isfinite(c) and d > zero):
                continue
            u = v[i] if v[i] > zero else zero
            ov = np.maximum(np.minimum(c, e1) - np.maximum(a, e0), zero)
            H[ri[i]] = H[ri[i]] + u * (ov / d)
    assert H.dtype == np.float32
    return H


def _parts(v, t0, t1, edges):
    """(ok [N], u [N], f [N, bins]) in v's dtype; `edges` are cast, not recomputed"""
    e = torch.as_tensor(edges).to(v.dtype)
    ok = torch.isfinite(t0) & torch.isfinite(t1) & ((t1 - t0) > 0)
    a, c = torch.where(ok, t0, torch.zeros_like(t0)), torch.where(ok, t1, torch.ones_like(t1))  # (a stand-in: [0, 1))
    d = c - a
    u = torch.where(ok, torch.clamp(v, min=0.0), torch.zeros_like(v))
    ov = torch.clamp(torch.minimum(c[:, None], e[None, 1:]) - torch.maximum(a[:, None], e[None, :-1]), min=0.0)
    f = torch.where(ok[:, None], ov / d[:, None], torch.zeros_like(ov))
    return ok, u, f


def hist_value(v, t0, t1, ri, n_rays, edges, normalize=True, eps=1e-10):
    """P (or H) [n_rays, bins]; differentiable torch ops in v's dtype"""
    _, u, f = _parts(v, t0, t1, edges)
    H = torch.zeros(n_rays, f.shape[1], dtype=v.dtype).index_add(0, ri, u[:, None] * f)
    if not normalize:
        return H
    return H / (seg_sum(u, ri, n_rays) + eps)[:, None]


def hist_grad(v, t0, t1, ri, n_rays, edges, G, normalize=True, eps=1e-10):
    """closed form: d u_i = sum_b G_rb f_ib, with normalize (sum_b G_rb f_ib - sum_b G_rb P_rb) / (s_r + eps);
    d v_i = d u_i where the sample counts and v_i >= 0, 0 elsewhere"""
    ok, u, f = _parts(v, t0, t1, edges)
    G = G.to(v.dtype)
    du = (G[ri] * f).sum(dim=1)
    if normalize:
        P = hist_value(v, t0, t1, ri, n_rays, edges, True, eps)
        du = (du - (G * P).sum(dim=1)[ri]) / (seg_sum(u, ri, n_rays) + eps)[ri]
    return torch.where(ok & (v >= 0), du, torch.zeros_like(du))


def _pair_masks(c, shape, dtype):
    """(right [B,Ph,Pw-1], down [B,Ph-1,Pw]): 1 where the pair is counted"""
    B, Ph, Pw = shape
    c = torch.ones(B, Ph, Pw, dtype=torch.bool) if c is None else (c.reshape(B, Ph, Pw) != 0)
    return (c[:, :, :-1] & c[:, :, 1:]), (c[:, :-1] & c[:, 1:])


def nkl_value(P, c=None, eps=1e-5):
    """out [B, Ph, Pw]: D(P_ij, P_i,j+1) + D(P_ij, P_i+1,j) over the counted pairs, D(p, q) = sum_b p_b (log(p_b + eps)
    - log(q_b + eps)); differentiable torch ops in P's dtype (where, not a product: a skipped pair is not computed)"""
    B, Ph, Pw, _ = P.shape
    right, down = _pair_masks(c, (B, Ph, Pw), P.dtype)
    lp = torch.log(P + eps)
    out = torch.zeros(B, Ph, Pw, dtype=P.dtype)
    dr = (P[:, :, :-1] * (lp[:, :, :-1] - lp[:, :, 1:])).sum(-1)
    dd = (P[:, :-1] * (lp[:, :-1] - lp[:, 1:])).sum(-1)
    out = out + torch.nn.functional.pad(torch.where(right, dr, torch.zeros_like(dr)), (0, 1))
    out = out + torch.nn.functional.pad(torch.where(down, dd, torch.zeros_like(dd)), (0, 0, 0, 1))
    return out


def nkl_grad(P, G, c=None, eps=1e-5):
    """closed form: dD/dp_b = log(p_b + eps) - log(q_b + eps) + p_b / (p_b + eps), dD/dq_b = -p_b / (q_b + eps)"""
    B, Ph, Pw, _ = P.shape
    right, down = _pair_masks(c, (B, Ph, Pw), P.dtype)
    G = G.to(P.dtype).reshape(B, Ph, Pw)
    lp, pe = torch.log(P + eps), P + eps
    out = torch.zeros_like(P)
    gr = torch.where(right, G[:, :, :-1], torch.zeros_like(G[:, :, :-1]))[..., None]
    gd = torch.where(down, G[:, :-1], torch.zeros_like(G[:, :-1]))[..., None]
    out[:, :, :-1] += gr * (lp[:, :, :-1] - lp[:, :, 1:] + P[:, :, :-1] / pe[:, :, :-1])
    out[:, :, 1:] += gr * -(P[:, :, :-1] / pe[:, :, 1:])
    out[:, :-1] += gd * (lp[:, :-1] - lp[:, 1:] + P[:, :-1] / pe[:, :-1])
    out[:, 1:] += gd * -(P[:, :-1] / pe[:, 1:])
    return out


def pair_count(c, shape):
    right, down = _pair_masks(c, shape, torch.float64)
    return int(right.sum()) + int(down.sum())


def loss_value(v, t0, t1, ri, n_rays, edges, shape, first_ray=0, c=None, eps=1e-5):
    """NeighborRayKLLoss: the histograms of the rays first_ray ... first_ray + B Ph Pw - 1, the patch term, the sum over
    max(number of counted pairs, 1); differentiable torch ops in v's dtype"""
    B, Ph, Pw = shape
    P = hist_value(v, t0, t1, ri, n_rays, edges)[first_ray:first_ray + B * Ph * Pw]
    return nkl_value(P.reshape(B, Ph, Pw, -1), c, eps).sum() / max(pair_count(c, shape), 1)
