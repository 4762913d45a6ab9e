"""CPU restatement of the extended occupancy march (fsn_occgrid_march_ex: per-ray bounds, cone-angle steps) and of
fsn_ray_aabb_intersect: float32 NumPy, operation for operation (the library is built without floating-point
contraction, so the results are the kernels' bit for bit).  The definition is in include/fsnerf_hip.h.  Test
infrastructure only, alongside composite_ref.py and raydata_ref.py."""
import numpy as np
import torch

f = np.float32


def _np(t):
    return None if t is None else (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(f)


def _slabs(o, d, lo, hi):
    """One ray against one box: (t_enter, t_exit, miss) - division form; a zero component tests the origin."""
    tmin, tmax, miss = f(-np.inf), f(np.inf), False
    for a in range(3):
        if d[a] == 0:
            miss = miss or bool(o[a] < lo[a]) or bool(o[a] > hi[a])
        else:
            ta, tb = (lo[a] - o[a]) / d[a], (hi[a] - o[a]) / d[a]
            tmin, tmax = np.fmax(tmin, np.fmin(ta, tb)), np.fmin(tmax, np.fmax(ta, tb))
    return tmin, tmax, miss


def _occupied(p, c, h, res, levels, bins):
    """grid_occupied for points p [N,3]: the cell at the finest level containing the point; False outside all boxes."""
    keep = np.zeros(len(p), bool)
    done = np.zeros(len(p), bool)
    s = f(1)
    for l in range(levels):
        lo, hi = c - h * s, c + h * s
        inside = np.all((p >= lo) & (p <= hi), axis=1) & ~done
        q = np.clip(np.floor((p - lo) / (hi - lo) * f(res)).astype(np.int64), 0, res - 1)
        cell = (q[:, 0] * res + q[:, 1]) * res + q[:, 2]
        keep |= inside & bins[l][cell]
        done |= inside
        s = s * f(2)
    return keep


def march(rays_o, rays_d, aabb, res, levels, binaries, near_plane, far_plane, step, u=None, max_steps=16384,
          t_min=None, t_max=None, cone_angle=0.0):
    """-> (ray_indices int64 [N], t_starts [N], t_ends [N]) as torch tensors; binaries bool [levels,res,res,res]."""
    o_all, d_all, u, t_min, t_max = _np(rays_o), _np(rays_d), _np(u), _np(t_min), _np(t_max)
    amin, amax = np.array(aabb[:3], f), np.array(aabb[3:], f)
    c, h = (amin + amax) / f(2), (amax - amin) / f(2)
    bins = (binaries.numpy() if isinstance(binaries, torch.Tensor) else np.asarray(binaries)).reshape(levels, -1)
    step, near_plane, far_plane, cone = f(step), f(near_plane), f(far_plane), f(cone_angle)
    sc = f(1 << (levels - 1))
    lo_box, hi_box = c - h * sc, c + h * sc
    lane = np.arange(64)
    ri, ts_out, te_out = [], [], []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for r in range(o_all.shape[0]):
            o, d = o_all[r], d_all[r]
            tmin, tmax, miss = _slabs(o, d, lo_box, hi_box)
            near_r = near_plane + u[r] * step if (u is not None and not cone > 0) else near_plane
            t_lo, t_hi = np.fmax(tmin, near_r), np.fmin(tmax, far_plane)
            if miss or not (t_hi > t_lo):
                continue
            t_lo = np.fmax(t_lo, t_min[r]) if t_min is not None else t_lo
            t_hi = np.fmin(t_hi, t_max[r]) if t_max is not None else t_hi
            if not (t_hi > t_lo):
                continue
            if cone > 0:
                tb = t_lo + u[r] * np.fmax(t_lo * cone, step) if u is not None else t_lo
                ts, te, ok = [], [], []
                for it in range(0, max_steps, 64):
                    dtb = np.fmax(tb * cone, step)
                    ts_b = tb + lane.astype(f) * dtb
                    ts.append(ts_b)
                    te.append(tb + (lane + 1).astype(f) * dtb)
                    ok.append((it + lane < max_steps) & (ts_b < t_hi))
                    tb = tb + f(64) * dtb
                    if not (tb < t_hi):
                        break
                ts, te, rng = np.concatenate(ts), np.concatenate(te), np.concatenate(ok)
            else:
                k0 = max(int(np.ceil((t_lo - near_r) / step)), 0)
                k = np.arange(k0, k0 + max_steps, dtype=np.int64)
                ts = near_r + k.astype(f) * step
                te = ts + step
                rng = (ts >= t_lo) & (ts < t_hi)  # (the kernel's early exit only skips points that are out of range)
            tm = (ts + te) / f(2)
            keep = rng & _occupied(o[None, :] + d[None, :] * tm[:, None], c, h, res, levels, bins)
            ri.append(np.full(int(keep.sum()), r, np.int64))
            ts_out.append(ts[keep])
            te_out.append(te[keep])
    cat = lambda xs, dt: torch.from_numpy(np.concatenate(xs) if xs else np.zeros(0, dt))
    return cat(ri, np.int64), cat(ts_out, f), cat(te_out, f)


def ray_aabb_intersect(rays_o, rays_d, aabbs, near_plane=-np.inf, far_plane=np.inf, miss_value=np.inf):
    """-> (t_mins [R,M], t_maxs [R,M], hits bool [R,M]) as torch tensors."""
    o_all, d_all, boxes = _np(rays_o), _np(rays_d), _np(aabbs).reshape(-1, 6)
    R, M = o_all.shape[0], boxes.shape[0]
    t0, t1, hits = np.empty((R, M), f), np.empty((R, M), f), np.zeros((R, M), bool)
    near_plane, far_plane, miss_value = f(near_plane), f(far_plane), f(miss_value)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for r in range(R):
            for m in range(M):
                tmin, tmax, miss = _slabs(o_all[r], d_all[r], boxes[m, :3], boxes[m, 3:])
                a, b = np.fmax(tmin, near_plane), np.fmin(tmax, far_plane)
                hits[r, m] = (not miss) and bool(b > a)
                t0[r, m], t1[r, m] = (a, b) if hits[r, m] else (miss_value, miss_value)
    return torch.from_numpy(t0), torch.from_numpy(t1), torch.from_numpy(hits)
