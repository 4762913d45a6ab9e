"""CPU restatements of the proposal-network sampler (csrc/propnet.hip, render/pdf.py, render/propnet.py) and the inputs
its tests share.

The sampler and the s -> t transform are restated in FLOAT32, operation for operation, every step one torch op (add,
divide, subtract, multiply: IEEE, unfused): the kernels are compiled without contraction and with correctly rounded
division, no transcendental is involved, so their output is compared with torch.equal.  (A float64 restatement is no
yardstick here: flat and saturated cdf stretches make the inverse cdf discontinuous, and the float32 and float64
samplers differ by up to half the support on these inputs.)  The interlevel loss is restated in float64; its autograd
is the truth for the gradient, and `pdf_loss_grad64` is the analytic gather form the backward kernel implements.

Cases: 70 rays (a partial last block of four) x S in {1, 5, 64, 65, 192} intervals in and n in {1, 7, 64, 65, 200} out
(fewer entries than lanes, one per lane, a ragged last lane, several per lane).  Densities rand^4 * 50 with every ninth
sample zero, ray 7 all zero (a flat cdf: trans == 1), ray 11 saturated in its first interval (cdf 1 from its second
edge on); jitters with b = 0 (ray 0) and b = 1 - 2^-24 (ray 1)."""
import functools

import torch

F32 = torch.float32
R = 70
S_SIZES = (1, 5, 64, 65, 192)
N_SIZES = (1, 7, 64, 65, 200)
NEAR, FAR = 2.0, 6.0


def _f(x):
    return torch.tensor(float(x), dtype=F32)


def stot_f32(transform, s, near, far):
    """_transform_stot in float32, the kernels' operation order"""
    near, far = _f(near), _f(far)
    if transform == "uniform":
        return s * far + (1.0 - s) * near
    assert transform == "lindisp"
    return 1.0 / (s * (1.0 / far) + (1.0 - s) * (1.0 / near))


def searchsorted_ref(keys, q):
    """-> (ids_left, ids_right) of the issue's definition, any float dtype"""
    h = torch.searchsorted(keys.contiguous(), q.contiguous(), right=True)  # number of keys <= q
    return (h - 1).clamp(min=0), h.clamp(max=keys.shape[-1] - 1)


def importance_sample_f32(v, c, n, b=None):
    """v, c [R, S+1] float32, b [R] float32 or None (0.5) -> (edges [R, n+1], centres [R, n]), float32 op for op"""
    assert v.dtype == F32 and c.dtype == F32
    rays, S = v.shape[0], v.shape[1] - 1
    b = torch.full((rays,), 0.5, dtype=F32) if b is None else b.to(F32)
    i = torch.arange(n, dtype=F32)
    u = (i[None, :] + b[:, None]) / _f(n)
    h = torch.searchsorted(c.contiguous(), u.contiguous(), right=True)
    k = (h - 1).clamp(0, S - 1)
    c0, c1 = c.gather(1, k), c.gather(1, k + 1)
    den = c1 - c0
    ratio = (u - c0) / torch.where(den > 0, den, torch.ones_like(den))
    frac = torch.where(den > 0, ratio.clamp(0.0, 1.0), torch.zeros_like(den))
    v0, v1 = v.gather(1, k), v.gather(1, k + 1)
    x = v0 + frac * (v1 - v0)
    lo, hi = v[:, :1], v[:, S:]
    if n == 1:
        return torch.cat([lo, hi], 1), x
    mid = (x[:, :-1] + x[:, 1:]) * 0.5
    e0 = torch.maximum(2.0 * x[:, :1] - mid[:, :1], lo)
    en = torch.minimum(2.0 * x[:, -1:] - mid[:, -1:], hi)
    return torch.cat([e0, mid, en], 1), x


def cdfs_f32(t_edges, sigmas):
    """1 - cat(trans, 0) in float32 on the CPU (a sequential sum: a monotone cdf; not the kernel's bits - exp differs)"""
    sdt = sigmas * (t_edges[:, 1:] - t_edges[:, :-1])
    run = torch.cat([torch.zeros_like(sdt[:, :1]), torch.cumsum(sdt, 1)[:, :-1]], 1)  # (no "inclusive - own": not monotone)
    trans = torch.exp(-run)
    return 1.0 - torch.cat([trans, torch.zeros_like(trans[:, :1])], 1)


@functools.lru_cache(maxsize=None)
def histogram_case(S, transform="lindisp"):
    """A proposal level: s_edges / t_edges [R, S+1], sigmas [R, S], cdfs [R, S+1] (float32, CPU) and jitters b [R]"""
    g = torch.Generator().manual_seed(1000 + S)
    inner = torch.sort(torch.rand(R, S - 1, generator=g), dim=1).values if S > 1 else torch.zeros(R, 0)
    s_edges = torch.cat([torch.zeros(R, 1), inner, torch.ones(R, 1)], 1)
    t_edges = stot_f32(transform, s_edges, NEAR, FAR)
    sig = torch.rand(R, S, generator=g) ** 4 * 50.0
    sig.view(-1)[::9] = 0.0
    sig[7] = 0.0
    sig[11, 0] = 1e4
    b = torch.rand(R, generator=g)
    b[0], b[1] = 0.0, 1.0 - 2.0 ** -24
    assert float(b[1]) < 1.0
    return dict(S=S, s_edges=s_edges, t_edges=t_edges, sigmas=sig, cdfs=cdfs_f32(t_edges, sig), b=b)


@functools.lru_cache(maxsize=None)
def loss_case(S, n):
    """Query intervals / cdfs [R, n+1] and key intervals / cdfs [R, S+1], drawn independently (float32, CPU), and a
    cotangent g [R, n].  A fifth of the query weights and every ninth key density are zero."""
    key = histogram_case(S)
    g = torch.Generator().manual_seed(7000 + 31 * S + n)
    inner = torch.sort(torch.rand(R, n - 1, generator=g), dim=1).values if n > 1 else torch.zeros(R, 0)
    q = torch.cat([torch.zeros(R, 1), inner, torch.ones(R, 1)], 1)
    w = torch.rand(R, n, generator=g) ** 2
    w[torch.rand(R, n, generator=g) < 0.2] = 0.0
    w[:, 0] += 1e-3
    cq = torch.cat([torch.zeros(R, 1), torch.cumsum(w, 1)], 1)
    cq = cq / cq[:, -1:]
    return dict(q=q, cq=cq, k=key["s_edges"], ck=key["cdfs"], g=torch.randn(R, n, generator=g))


def pdf_loss64(q, cq, k, ck):
    """the interlevel loss [R, n]; float64 tensors, differentiable w.r.t. ck"""
    il, _ = searchsorted_ref(k, q[:, :-1])
    _, ir = searchsorted_ref(k, q[:, 1:])
    w = cq[:, 1:] - cq[:, :-1]
    wo = ck.gather(1, ir) - ck.gather(1, il)
    return torch.where(w > 0, (w - wo).clamp(min=0) ** 2 / (w + 1e-7), torch.zeros_like(w))


def pdf_loss_grad64(q, cq, k, ck, g):
    """the analytic gradient w.r.t. ck: coef_i scattered to ids_right(q[i+1]) and, negated, to ids_left(q[i])"""
    il, _ = searchsorted_ref(k, q[:, :-1])
    _, ir = searchsorted_ref(k, q[:, 1:])
    w = cq[:, 1:] - cq[:, :-1]
    wo = ck.gather(1, ir) - ck.gather(1, il)
    coef = torch.where(w > 0, -2.0 * (w - wo).clamp(min=0) / (w + 1e-7) * g, torch.zeros_like(w))
    return torch.zeros_like(ck).scatter_add(1, ir, coef).scatter_add(1, il, -coef)
