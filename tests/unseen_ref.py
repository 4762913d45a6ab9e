"""The unseen-view distribution of csrc/unseen_views.hip restated in float32 NumPy, operation for operation (the library
is built with -ffp-contract=off and its sqrtf and / are correctly rounded, so the kernels match this bit for bit):
the counter-based random numbers over raydata_ref._mix, the slots, the disc rejection with its cap of 16 tries, the
look-at, the anchor draw, and the pinhole / NDC ray of csrc/ray_dev.hpp for the rows of a patch batch.

A distribution is a dict of float32 values, `dist_of(sampler.dist)` reads one out of the struct the kernels take."""
import numpy as np

from raydata_ref import _mix

F = np.float32
TRIES, SLOT_ANCHOR = 16, 38
TINY_LEN2, TINY_CROSS2 = F(1e-20), F(1e-8)
SHELL, BOX = 0, 1


def dist_of(d) -> dict:
    """fsn_unseen_dist (ctypes) -> dict; the arrays as float32 vectors."""
    out = {"mode": int(d.mode)}
    for name in ("jitter", "r_lo", "r_hi", "z_lo", "z_hi"):
        out[name] = F(getattr(d, name))
    for name in ("focus", "up", "e1", "e2", "centre", "lo", "hi"):
        out[name] = np.array(list(getattr(d, name)), dtype=F)
    return out


def base(seed: int, g) -> np.ndarray:
    return _mix(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ _mix(np.asarray(g, dtype=np.uint64)))


def bits(b, slot: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        return _mix(b + np.uint64(slot))


def u(b, slot: int) -> np.ndarray:
    """uniform in [0, 1): the top 24 bits, exact in float32"""
    return (bits(b, slot) >> np.uint64(40)).astype(F) * F(2.0 ** -24)


def below(b, slot: int, n: int) -> np.ndarray:
    """uniform on [0, n): (hi32(bits) * n) >> 32"""
    return (((bits(b, slot) >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _len2(a):
    return (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]


def poses(d: dict, seed: int, g, details: bool = False):
    """pose draws g [n] -> [n,12] float32 (with `details`: also a dict of the intermediates z, r, tries, target)."""
    g = np.asarray(g, dtype=np.uint64).reshape(-1)
    b = base(seed, g)
    n = g.shape[0]
    info = {}
    if d["mode"] == SHELL:
        z = np.minimum(d["z_lo"] + u(b, 0) * (d["z_hi"] - d["z_lo"]), d["z_hi"])
        r = np.minimum(d["r_lo"] + u(b, 1) * (d["r_hi"] - d["r_lo"]), d["r_hi"])
        c, s = np.ones(n, dtype=F), np.zeros(n, dtype=F)
        todo, tries = np.ones(n, dtype=bool), np.zeros(n, dtype=np.int64)
        for k in range(TRIES):
            a_, b_ = F(2.0) * u(b, 6 + 2 * k) - F(1.0), F(2.0) * u(b, 7 + 2 * k) - F(1.0)
            q = a_ * a_ + b_ * b_
            ok = todo & (q > 0) & (q <= 1)
            root = np.sqrt(np.where(ok, q, F(1.0)))
            c, s = np.where(ok, a_ / root, c), np.where(ok, b_ / root, s)
            tries += todo
            todo &= ~ok
        h = np.sqrt(F(1.0) - z * z)
        hc, hs = h * c, h * s
        origin = np.stack([d["centre"][k] + r * ((hc * d["e1"][k] + hs * d["e2"][k]) + z * d["up"][k]) for k in range(3)], -1)
        info.update(z=z, r=r, tries=tries, fallback=todo)
    else:
        origin = np.stack([np.minimum(d["lo"][k] + u(b, k) * (d["hi"][k] - d["lo"][k]), d["hi"][k]) for k in range(3)], -1)
    target = np.stack([d["focus"][k] + d["jitter"] * (F(2.0) * u(b, 3 + k) - F(1.0)) for k in range(3)], -1)
    v = origin - target
    vv = _len2(v)
    far = vv >= TINY_LEN2
    zc = np.where(far[:, None], v / np.sqrt(np.where(far, vv, F(1.0)))[:, None], d["up"][None, :])
    x = _cross(np.broadcast_to(d["up"], zc.shape), zc)
    xx = _len2(x)
    alt = xx < TINY_CROSS2
    x2 = _cross(np.broadcast_to(d["e1"], zc.shape), zc)
    x = np.where(alt[:, None], x2, x)
    xx = np.where(alt, _len2(x2), xx)
    xc = x / np.sqrt(xx)[:, None]
    yc = _cross(zc, xc)
    m = np.stack([xc, yc, zc, origin], -1).reshape(n, 12).astype(F)  # rows [xc_k yc_k zc_k origin_k]
    assert m.dtype == F and origin.dtype == F and zc.dtype == F
    if details:
        info.update(target=target, origin=origin)
        return m, info
    return m


def anchors(seed: int, q, H: int, W: int, P: int, dilation: int):
    """patches q [n] -> (row0 [n], col0 [n]) int64 on the (H - ext + 1) x (W - ext + 1) lattice"""
    ext = (P - 1) * dilation + 1
    b = base(seed, np.asarray(q, dtype=np.uint64).reshape(-1))
    return below(b, SLOT_ANCHOR, H - ext + 1), below(b, SLOT_ANCHOR + 1, W - ext + 1)


def rays(m, row, col, H: int, W: int, focal: float, ndc: bool, near: float = 1.0):
    """pinhole_ray (+ ndc_ray) of csrc/ray_dev.hpp: poses m [n,12], pixels (row, col) [n] -> (o [n,3], d [n,3]) float32.
    The host-side constants are rounded as fsn_ray_patch_batch rounds them: formed in double, then float32."""
    m = np.asarray(m, dtype=F).reshape(-1, 3, 4)
    half_w, half_h, f = F(W * 0.5), F(H * 0.5), F(focal)
    dx = (np.asarray(col).astype(F) - half_w) / f
    dy = -((np.asarray(row).astype(F) - half_h) / f)
    dz = np.full_like(dx, F(-1.0))
    nrm = np.sqrt((dx * dx + dy * dy) + dz * dz)
    dx, dy, dz = dx / nrm, dy / nrm, dz / nrm
    d = np.stack([(dx * m[:, k, 0] + dy * m[:, k, 1]) + dz * m[:, k, 2] for k in range(3)], -1)
    o = m[:, :, 3].copy()
    if ndc:
        sx, sy = F(-1.0 / (W / (2.0 * focal))), F(-1.0 / (H / (2.0 * focal)))
        nr, two_near = F(near), F(2.0 * near)
        ddx, ddy, ddz = d[:, 0], d[:, 1], d[:, 2]
        t = -(nr + o[:, 2]) / ddz
        ox, oy, oz = o[:, 0] + t * ddx, o[:, 1] + t * ddy, o[:, 2] + t * ddz
        o = np.stack([sx * ox / oz, sy * oy / oz, F(1.0) + two_near / oz], -1)
        d = np.stack([sx * (ddx / ddz - ox / oz), sy * (ddy / ddz - oy / oz), -two_near / oz], -1)
    assert o.dtype == F and d.dtype == F
    return o, d


def patch_batch(d: dict, seed: int, first_patch: int, count: int, per_pose: int, H: int, W: int, focal: float, P: int,
                dilation: int, ndc: bool, near: float = 1.0):
    """fsn_unseen_patch_batch -> (rays_o, rays_d [count P^2, 3], poses [count,12], anchors [count] = row0 AW + col0)"""
    q = np.arange(first_patch, first_patch + count, dtype=np.int64)
    m = poses(d, seed, q // per_pose)
    row0, col0 = anchors(seed, q, H, W, P, dilation)
    i, j = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    row = (row0[:, None, None] + i[None] * dilation).reshape(-1)
    col = (col0[:, None, None] + j[None] * dilation).reshape(-1)
    o, dd = rays(np.repeat(m, P * P, axis=0), row, col, H, W, focal, ndc, near)
    ext = (P - 1) * dilation + 1
    return o, dd, m, row0 * (W - ext + 1) + col0
