"""CPU restatement of fsn_occgrid_visibility (OccGridEstimator.mark_invisible_cells): NumPy, operation for operation.
With dtype=float32 the results are the kernel's bit for bit (the library is built without floating-point contraction);
with dtype=float64 the same rule is the geometric reference, and it can report the cells whose outcome hangs on a margin
too close to zero for float32 to decide.  The definition is in include/fsnerf_hip.h.  Test infrastructure only, alongside
occ_cone_ref.py."""
import numpy as np

f32, f64 = np.float32, np.float64


def _arr(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=f64)


def cams_opencv(K, c2w):
    """K [3,3] / [N,3,3], c2w [N,3,4] / [N,4,4] (x right, y down, z forward) -> float32 [N,16]: world -> camera
    [R^T | -R^T t] formed in float64 with the estimator's operation order, then fx, fy, cx, cy."""
    K, c2w = _arr(K), _arr(c2w)
    N = c2w.shape[0]
    K = np.broadcast_to(K, (N, 3, 3))
    Rt = np.transpose(c2w[:, :3, :3], (0, 2, 1))
    t = c2w[:, :3, 3]
    tt = -((Rt[:, :, 0] * t[:, None, 0] + Rt[:, :, 1] * t[:, None, 1]) + Rt[:, :, 2] * t[:, None, 2])
    w2c = np.concatenate([Rt, tt[:, :, None]], 2).reshape(N, 12)
    intr = np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], 1)
    return np.concatenate([w2c, intr], 1).astype(f32)


def cams_from_views(poses, hwf):
    """`get_rays` poses (x right, y up, looking down -z) and (H, W, focal) -> the same table: the y and z axes flip, and
    the principal point sits at W/2 + 1/2, H/2 + 1/2 (pixel i's footprint is [i - 1/2, i + 1/2])."""
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
    c2w = _arr(poses)[:, :3, :] * np.array([1.0, -1.0, -1.0, 1.0])
    K = np.array([[focal, 0.0, W / 2.0 + 0.5], [0.0, focal, H / 2.0 + 0.5], [0.0, 0.0, 1.0]])
    return cams_opencv(K, c2w)


def ndc_args(hwf, near=1.0):
    H, W, focal = int(hwf[0]), int(hwf[1]), float(hwf[2])
    return (W / (2.0 * focal), H / (2.0 * focal), float(near))


def visibility(aabb, res, levels, cams, width, height, near_plane=0.0, min_views=1, ndc=None, dtype=f32, tol=None):
    """-> visible bool [levels,res,res,res]; with `tol` also `uncertain` (same shape): some margin of some camera at some
    corner (or, with a near plane, at the centre) lies within tol * max(|its terms|) of zero."""
    dt = dtype
    cams = np.asarray(cams).astype(dt)
    a32 = np.asarray(aabb, f32).astype(f64)
    W, Hh, near_plane = dt(width), dt(height), dt(near_plane)
    shape = (res, res, res)
    vis_all, unc_all = [], []
    idx = np.arange(res)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for l in range(levels):
            cd = (a32[:3] + a32[3:]) / 2.0                      # level_box: double, rounded once
            hd = (a32[3:] - a32[:3]) / 2.0 * float(1 << l)
            lo, hi = (cd - hd).astype(dt), (cd + hd).astype(dt)
            ends = []
            for a in range(3):
                w = (hi[a] - lo[a]) / dt(res)
                sh = [1, 1, 1]
                sh[a] = res
                ends.append([np.broadcast_to((lo[a] + (idx + k).astype(dt) * w).reshape(sh), shape).copy() for k in (0, 1)])
            any_left = np.ones(shape, bool)
            if ndc is not None:
                zmax = dt(1) - dt(1e-6)
                any_left = ends[2][0] <= zmax
                ends[2][1] = np.fmin(ends[2][1], zmax)
            pts = [[ends[0][(k >> 2) & 1], ends[1][(k >> 1) & 1], ends[2][k & 1]] for k in range(8)]
            pts.append([(ends[a][0] + ends[a][1]) / dt(2) for a in range(3)])
            if ndc is not None:
                wf, hf, nr = dt(ndc[0]), dt(ndc[1]), dt(ndc[2])
                for k in range(9):
                    z = (dt(2) * nr) / (pts[k][2] - dt(1))
                    pts[k] = [((-pts[k][0]) * z) * wf, ((-pts[k][1]) * z) * hf, z]
            covering = np.zeros(shape, np.int64)
            too_near = np.zeros(shape, bool)
            unc = np.zeros(shape, bool)
            for m in cams:
                fx, fy, cx, cy = m[12], m[13], m[14], m[15]
                wx, hy = W - cx, Hh - cy
                neg = [np.ones(shape, bool) for _ in range(5)]
                for k in range(9):
                    x, y, z = pts[k]
                    X = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]
                    Y = ((m[4] * x + m[5] * y) + m[6] * z) + m[7]
                    D = ((m[8] * x + m[9] * y) + m[10] * z) + m[11]
                    g = [D - near_plane, fx * X + cx * D, wx * D - fx * X, fy * Y + cy * D, hy * D - fy * Y]
                    if k < 8:
                        for j in range(5):
                            neg[j] &= g[j] < 0
                    else:
                        too_near |= (g[1] >= 0) & (g[2] >= 0) & (g[3] >= 0) & (g[4] >= 0) & (D >= 0) & (D < near_plane)
                    if tol is not None and (k < 8 or near_plane > 0):
                        mx = lambda r: np.maximum(np.maximum(abs(m[r] * x), abs(m[r + 1] * y)),
                                                  np.maximum(abs(m[r + 2] * z), abs(m[r + 3])))
                        sX, sY, sD = mx(0), mx(4), mx(8)
                        scale = [np.maximum(sD, near_plane), np.maximum(abs(fx) * sX, abs(cx) * sD),
                                 np.maximum(abs(wx) * sD, abs(fx) * sX), np.maximum(abs(fy) * sY, abs(cy) * sD),
                                 np.maximum(abs(hy) * sD, abs(fy) * sY)]
                        for j in range(5):
                            unc |= abs(g[j]) <= tol * scale[j]
                        if k == 8:
                            unc |= abs(D) <= tol * sD
                covering += ~(neg[0] | neg[1] | neg[2] | neg[3] | neg[4])
            vis_all.append((covering >= min_views) & ~too_near & any_left)
            unc_all.append(unc & any_left)
    vis = np.stack(vis_all)
    return (vis, np.stack(unc_all)) if tol is not None else vis


def cell_is(mask, pts, aabb, res, levels, dtype=f64):
    """For points [N,3] and a bool grid [levels,res,res,res]: (inside [N,levels], value [N,levels]) - whether level l's
    box holds the point, and the mask at the cell of that level holding it."""
    p = np.asarray(pts).astype(dtype)
    a32 = np.asarray(aabb, f32).astype(f64)
    inside, value = [], []
    for l in range(levels):
        cd = (a32[:3] + a32[3:]) / 2.0
        hd = (a32[3:] - a32[:3]) / 2.0 * float(1 << l)
        lo, hi = (cd - hd).astype(dtype), (cd + hd).astype(dtype)
        inside.append(np.all((p >= lo) & (p <= hi), axis=1))
        q = np.clip(np.floor((p - lo) / (hi - lo) * dtype(res)).astype(np.int64), 0, res - 1)
        value.append(mask[l][q[:, 0], q[:, 1], q[:, 2]])
    return np.stack(inside, 1), np.stack(value, 1)


def pack_bits(mask):
    """bool [..] (a multiple of 32 cells) -> int32 words, bit c & 31 of word c >> 5: the layout of `bits`."""
    b = np.asarray(mask).reshape(-1, 32).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32).view(np.int32)
