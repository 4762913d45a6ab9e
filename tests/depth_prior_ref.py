"""Restatements for the monocular-depth-prior tests (csrc/depth_prior.hip, the aux planes of csrc/raydata.hip): the two
patch losses in torch, in whatever dtype the inputs have (float64: the reference; float32: the yardstick of the bar),
with the closed-form (s, t) of the fit left INSIDE autograd, and the aux gather in NumPy.  Nothing here touches a GPU."""
import numpy as np
import torch

SLACK = 16 * 2.0 ** -24  # the project's standing bar: E_kernel <= 4 E_f32 + SLACK (tests/test_pose_refine_gpu.py)


def valid_mask(depth, prior, weight=None):
    ok = torch.isfinite(depth) & torch.isfinite(prior)
    return ok if weight is None else ok & (weight > 0)


def _clean(depth, prior, weight):
    """(valid, w, depth, prior) with every invalid entry replaced by a harmless number, so that no NaN reaches a sum or
    a gradient (0 * NaN is NaN); the replaced entries carry weight 0."""
    ok = valid_mask(depth, prior, weight)
    w = torch.ones_like(depth) if weight is None else weight.to(depth.dtype)
    w = torch.where(ok, w, torch.zeros_like(w)).detach()
    return ok, w, torch.where(ok, depth, torch.ones_like(depth)), torch.where(ok, prior, torch.zeros_like(prior)).detach()


def ssi_x(depth, inverse, z_min):
    return 1.0 / depth.clamp(min=z_min) if inverse else depth


def ssi_fit(depth, prior, weight=None, inverse=False, z_min=1e-3, rel_eps=1e-10):
    """-> (L [B], s [B], t [B], M [B], degenerate [B] bool, (w, x, p) cleaned): the issue's equations, per patch, in the
    dtype of `depth`.  Degenerate patches have L = s = t = 0."""
    ok, w, d, p = _clean(depth, prior, weight)
    x = ssi_x(d, inverse, z_min)
    dims = (1, 2)
    M = w.sum(dims)
    cnt = ok.sum(dims)
    Ms = torch.where(M > 0, M, torch.ones_like(M))
    mx, mp = (w * x).sum(dims) / Ms, (w * p).sum(dims) / Ms
    dx, dp = x - mx[:, None, None], p - mp[:, None, None]
    vx, cxp = (w * dx * dx).sum(dims) / Ms, (w * dx * dp).sum(dims) / Ms
    deg = (cnt < 2) | ~(M > 0) | ~(vx > rel_eps * mx * mx)
    s = torch.where(deg, torch.zeros_like(vx), cxp / torch.where(deg, torch.ones_like(vx), vx))
    t = torch.where(deg, torch.zeros_like(vx), mp - s * mx)
    r = s[:, None, None] * x + t[:, None, None] - p
    L = torch.where(deg, torch.zeros_like(vx), (w * r * r).sum(dims) / Ms)
    return L, s, t, M, deg, (w, x, p)


def ssi_loss(depth, prior, weight=None, inverse=False, z_min=1e-3, rel_eps=1e-10):
    return ssi_fit(depth, prior, weight, inverse, z_min, rel_eps)[0]


def ssi_mean(depth, prior, weight=None, inverse=False, z_min=1e-3, rel_eps=1e-10):
    """ScaleShiftDepthLoss's reduction: the sum over the non-degenerate patches divided by max(their number, 1)."""
    L, _, _, _, deg, _ = ssi_fit(depth, prior, weight, inverse, z_min, rel_eps)
    return L.sum() / max(int((~deg).sum()), 1)


def ssi_partial_grad(depth, prior, weight=None, inverse=False, z_min=1e-3, rel_eps=1e-10):
    """dL_b/ddepth by the stated formula - the partial derivative at fixed (s, t):
    2 w s (s x + t - p) / M, through x = 1 / max(depth, z_min): times -1 / depth^2, 0 below z_min."""
    with torch.no_grad():
        _, s, t, M, deg, (w, x, p) = ssi_fit(depth, prior, weight, inverse, z_min, rel_eps)
        Ms = torch.where(M > 0, M, torch.ones_like(M))
        g = 2.0 * w * s[:, None, None] * (s[:, None, None] * x + t[:, None, None] - p) / Ms[:, None, None]
        if inverse:
            g = torch.where(depth < z_min, torch.zeros_like(g), -g * x * x)
        return torch.where(deg[:, None, None] | (w == 0), torch.zeros_like(g), g)


def _rank_pairs(depth, prior, weight, prior_gap, prior_is_disparity):
    """(ranked [B, N, N] bool: the prior puts i (row) nearer than j (column), both valid; d [B, N] cleaned)"""
    ok, _, d, p = _clean(depth, prior, weight)
    B = depth.shape[0]
    ok, d, p = ok.reshape(B, -1), d.reshape(B, -1), p.reshape(B, -1)
    pi, pj = p[:, :, None], p[:, None, :]
    near = (pi > pj + prior_gap) if prior_is_disparity else (pi < pj - prior_gap)
    return near & ok[:, :, None] & ok[:, None, :], d


def rank_loss(depth, prior, weight=None, margin=1e-4, prior_gap=0.0, prior_is_disparity=False):
    """-> (out [B], pairs [B] int64): the sum over the ranked ordered pairs of max(0, d_i - d_j + margin), and their
    number; patch by patch (a [N, N] table each) in the dtype of `depth`."""
    outs, pairs = [], []
    for b in range(depth.shape[0]):
        sl = slice(b, b + 1)
        ranked, d = _rank_pairs(depth[sl], prior[sl], None if weight is None else weight[sl], prior_gap, prior_is_disparity)
        hinge = ((d[:, :, None] - d[:, None, :]) + margin).clamp(min=0)
        outs.append(torch.where(ranked, hinge, torch.zeros_like(hinge)).sum())
        pairs.append(ranked.sum())
    if not outs:
        return depth.new_zeros(0), torch.zeros(0, dtype=torch.int64)
    return torch.stack(outs), torch.stack(pairs)


def rank_counts(depth, prior, weight=None, margin=1e-4, prior_gap=0.0, prior_is_disparity=False):
    """The gradient's integers [B, P, Q] int64: per pixel +1 for every active pair (hinge > 0) in which it is the
    nearer pixel, -1 for every active pair in which it is the farther."""
    out = []
    for b in range(depth.shape[0]):
        sl = slice(b, b + 1)
        ranked, d = _rank_pairs(depth[sl], prior[sl], None if weight is None else weight[sl], prior_gap, prior_is_disparity)
        active = ranked & (((d[:, :, None] - d[:, None, :]) + margin) > 0)
        out.append((active.sum(2) - active.sum(1)).reshape(depth.shape[1:]))
    return torch.stack(out) if out else torch.zeros((0,) + tuple(depth.shape[1:]), dtype=torch.int64)


def rank_mean(depth, prior, weight=None, **kw):
    """DepthRankingLoss's reduction: sum_b out / max(sum_b pairs, 1)."""
    out, pairs = rank_loss(depth, prior, weight, **kw)
    return out.sum() / max(int(pairs.sum()), 1)


def rel_error(got, want):
    """The project's measure: max |got - want| relative to the largest |want| (1 where that is 0)."""
    got, want = got.detach().double().reshape(-1), want.detach().double().reshape(-1)
    if want.numel() == 0:
        return 0.0
    scale = float(want.abs().max())
    return float((got - want).abs().max()) / (scale if scale > 0 else 1.0)


# ---------------------------------------------------------------- the aux gather
def aux_rows(planes: np.ndarray, index: np.ndarray) -> np.ndarray:
    """Rows `index` of the planes [n, H, W, A] (or [n, H, W]) as uint32 words [len(index), A]: what a batch serves."""
    planes = np.ascontiguousarray(planes, dtype=np.float32)
    A = 1 if planes.ndim == 3 else planes.shape[3]
    return planes.view(np.uint32).reshape(-1, A)[np.asarray(index, dtype=np.int64)]


def bit_planes(n: int, H: int, W: int, A: int, seed: int = 0) -> np.ndarray:
    """Planes [n, H, W, A] float32 whose words are all different: random bit patterns (NaNs with payloads, Inf and
    denormals among them), with +Inf, -Inf, a quiet NaN and -0 planted."""
    rng = np.random.default_rng(seed)
    words = rng.choice(2 ** 32, size=n * H * W * A, replace=False).astype(np.uint32)
    words[:4] = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0x80000000], dtype=np.uint32)
    assert len(np.unique(words)) == words.size
    return words.view(np.float32).reshape(n, H, W, A)
