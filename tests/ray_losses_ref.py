"""TEST INFRASTRUCTURE ONLY: torch restatements (CPU, any float dtype, differentiable by autograd) of what
csrc/ray_losses.hip computes - the ray entropy, the depth KL term and the patch depth smoothness (DESIGN.md 6.1,
"Few-shot geometry losses") - with their closed-form gradients and a per-ray loop form of the entropy.

The closed forms are checked against autograd of the restatements in float64 (tests/test_ray_losses_cpu.py); the GPU
kernels against both (tests/test_ray_losses_gpu.py)."""
import math

import torch

from composite_ref import seg_sum


def _ray_weight(c, n_rays, like):
    return torch.ones(n_rays, dtype=like.dtype) if c is None else c.to(like.dtype).reshape(-1)


def entropy_value(v, ri, n_rays, c=None, eps=1e-10, log2=True):
    """H_r = -scale c_r sum_i p_i log(p_i + eps), p = max(v, 0) / (sum + eps) -> [n_rays]"""
    scale = 1.0 / math.log(2.0) if log2 else 1.0
    u = torch.clamp(v, min=0.0)
    p = u / (seg_sum(u, ri, n_rays) + eps)[ri]
    return -scale * _ray_weight(c, n_rays, v) * seg_sum(p * torch.log(p + eps), ri, n_rays)


def entropy_grad(v, ri, n_rays, g, c=None, eps=1e-10, log2=True):
    """closed form: g_r scale c_r (f'(p_k) - sum_i p_i f'(p_i)) / (s + eps) where v_k >= 0, 0 below;
    f'(p) = -log(p + eps) - p / (p + eps)"""
    scale = 1.0 / math.log(2.0) if log2 else 1.0
    u = torch.clamp(v, min=0.0)
    den = (seg_sum(u, ri, n_rays) + eps)[ri]
    p = u / den
    fp = -torch.log(p + eps) - p / (p + eps)
    k = (g.reshape(-1) * scale * _ray_weight(c, n_rays, v))[ri]
    d = k * (fp - seg_sum(p * fp, ri, n_rays)[ri]) / den
    return torch.where(v >= 0, d, torch.zeros_like(d))


def entropy_loop(v, ri, n_rays, c=None, eps=1e-10, log2=True):
    """the same value ray by ray (the spelling the kernel replaces)"""
    scale = 1.0 / math.log(2.0) if log2 else 1.0
    out = torch.zeros(n_rays, dtype=v.dtype)
    for r in range(n_rays):
        u = torch.clamp(v[ri == r], min=0.0)
        if u.numel() == 0 or (c is not None and float(c[r]) == 0.0):
            continue
        p = u / (u.sum() + eps)
        out[r] = -scale * (1.0 if c is None else float(c[r])) * (p * torch.log(p + eps)).sum()
    return out


def kl_supervised(depth, var):
    return torch.isfinite(depth) & (depth > 0) & torch.isfinite(var) & (var > 0)


def _kl_terms(t0, t1, ri, depth, var):
    """(supervised [n_rays], exp(-(m - depth)^2 / (2 var)) dt [N]) with the unsupervised rays' entries exactly 0"""
    ok = kl_supervised(depth, var)
    d = torch.where(ok, depth, torch.ones_like(depth))[ri]
    s2 = torch.where(ok, var, torch.ones_like(var))[ri]
    dm = (t0 + t1) / 2.0 - d
    gauss = torch.exp(-(dm * dm) / (2.0 * s2)) * (t1 - t0)
    return ok, torch.where(ok[ri], gauss, torch.zeros_like(gauss))


def depth_kl_value(w, t0, t1, ri, n_rays, depth, var, eps=1e-5):
    """L_r = sum_i -log(max(w_i, 0) + eps) exp(-(m_i - depth_r)^2 / (2 var_r)) dt_i on supervised rays, 0 elsewhere"""
    _, gd = _kl_terms(t0, t1, ri, depth, var)
    return seg_sum(-torch.log(torch.clamp(w, min=0.0) + eps) * gd, ri, n_rays)


def depth_kl_grad(w, t0, t1, ri, n_rays, depth, var, g, eps=1e-5):
    """closed form: -g_r exp(...)_k dt_k / (w_k + eps) where w_k >= 0, 0 below"""
    _, gd = _kl_terms(t0, t1, ri, depth, var)
    d = -g.reshape(-1)[ri] * gd / (torch.clamp(w, min=0.0) + eps)
    return torch.where(w >= 0, d, torch.zeros_like(d))


INVALID_RAYS = (10, 11, 12, 13, 14)


def kl_targets(depth_ref, seed):
    """The depth KL test's per-ray targets (float32): the reference depth plus 0.3 randn, var cycling through 1e-4,
    1e-2 and 1, and rays 10-14 unsupervised - depth 0, NaN, +inf, -1, and var 0.  -> (depth [R], var [R])"""
    gen = torch.Generator().manual_seed(seed)
    R = depth_ref.numel()
    depth = depth_ref.reshape(-1).float() + 0.3 * torch.randn(R, generator=gen)
    var = torch.tensor([1e-4, 1e-2, 1.0])[torch.arange(R) % 3].clone()
    depth[10], depth[11], depth[12], depth[13] = 0.0, float("nan"), float("inf"), -1.0
    var[14] = 0.0
    return depth, var


def patch_tv_value(d):
    """S_b = sum_{i<P-1, j<Q-1} (d[i,j] - d[i,j+1])^2 + (d[i,j] - d[i+1,j])^2 -> [B]"""
    a = d[:, :-1, :-1]
    return ((a - d[:, :-1, 1:]) ** 2 + (a - d[:, 1:, :-1]) ** 2).sum(dim=(1, 2))


def patch_tv_grad(d, g):
    """closed form, gather: each pixel sums the up-to-four differences it appears in"""
    B, P, Q = d.shape
    out = torch.zeros_like(d)
    if P > 1 and Q > 1:
        dh = 2.0 * (d[:, :-1, :-1] - d[:, :-1, 1:])  # anchor (i, j) against (i, j+1)
        dv = 2.0 * (d[:, :-1, :-1] - d[:, 1:, :-1])  # anchor (i, j) against (i+1, j)
        out[:, :-1, :-1] += dh + dv
        out[:, :-1, 1:] -= dh
        out[:, 1:, :-1] -= dv
    return out * g.reshape(B, 1, 1)
