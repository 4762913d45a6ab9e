"""Restatements of the depth-warp operator (csrc/warp.hip; include/fsnerf_hip.h has the definition) and the case builder
of tests/test_warp_cpu.py and tests/test_warp_gpu.py:
  warp_f32        NumPy float32, forward and backward, every operation in the kernel's order: the forward is the
                  kernel's bit for bit (the library is built with -ffp-contract=off);
  warp_f64        torch float64, the same formulas; its gradient comes from autograd through them;
  loss_f64        core.loss.WarpConsistencyLoss on warp_f64;
  make_case       rows whose validity and cell are the same in float32 and float64, plus deliberately invalid rows;
  plane_scene     the end-to-end depth-recovery scene, recover_f64 its float64 run.
Nothing here touches a GPU."""
import numpy as np
import torch

f32 = np.float32
QNAN = np.float32(np.nan)  # 0x7fc00000: the canonical quiet NaN uvz stores


# ---------------------------------------------------------------------------------------------- float32, NumPy
def _convert_f32(px, white_bkgd):
    """bytes [n, C] -> colours [n, 3] as the ray batch converts a pixel: byte / 255, then c * a + (1 - a)."""
    c = px[:, :3].astype(f32) / f32(255.0)
    if white_bkgd:
        al = (px[:, 3].astype(f32) / f32(255.0))[:, None]
        rest = f32(1.0) - al
        c = c * al + rest
    return c


def warp_f32(o, d, t, s, poses, images, K, white_bkgd=False, z_min=1e-3, border=0.0, g=None):
    """-> dict(colour, valid, uvz) and, with a cotangent g [n,3], d_depth, d_rays_o, d_rays_d."""
    for a in (o, d, t, poses, K):
        assert a.dtype == np.float32
    assert images.dtype == np.uint8 and s.dtype == np.int64
    n = t.shape[0]
    V, H, W, C = images.shape
    z_min, border = f32(z_min), f32(border)
    in_range = (s >= 0) & (s < V)
    sc = np.where(in_range, s, 0)
    M = poses[sc]
    Kr = K[sc] if K.shape[0] > 1 else np.broadcast_to(K[0], (n, 4))
    fx, fy, cx, cy = (Kr[:, i] for i in range(4))
    with np.errstate(all="ignore"):
        p = [(o[:, k] + t * d[:, k]) - M[:, 4 * k + 3] for k in range(3)]
        xc = (M[:, 0] * p[0] + M[:, 4] * p[1]) + M[:, 8] * p[2]
        yc = (M[:, 1] * p[0] + M[:, 5] * p[1]) + M[:, 9] * p[2]
        zc = (M[:, 2] * p[0] + M[:, 6] * p[1]) + M[:, 10] * p[2]
        z = -zc
        u = cx + fx * (xc / z)
        v = cy - fy * (yc / z)
        u_hi, v_hi = f32(W - 1) - border, f32(H - 1) - border
        valid = (in_range & np.isfinite(t) & (t > 0) & (z >= z_min) & (u >= border) & (u <= u_hi) & (v >= border)
                 & (v <= v_hi))
    us, vs = np.where(valid, u, f32(0)), np.where(valid, v, f32(0))
    x0 = np.minimum(np.floor(us).astype(np.int64), W - 2)
    y0 = np.minimum(np.floor(vs).astype(np.int64), H - 2)
    fu, fv = (us - x0.astype(f32))[:, None], (vs - y0.astype(f32))[:, None]
    c00 = _convert_f32(images[sc, y0, x0], white_bkgd)
    c10 = _convert_f32(images[sc, y0, x0 + 1], white_bkgd)
    c01 = _convert_f32(images[sc, y0 + 1, x0], white_bkgd)
    c11 = _convert_f32(images[sc, y0 + 1, x0 + 1], white_bkgd)
    top = c00 + fu * (c10 - c00)
    bot = c01 + fu * (c11 - c01)
    colour = np.where(valid[:, None], top + fv * (bot - top), f32(0)).astype(f32)
    uvz = np.stack([u, v, z], 1)
    uvz = np.where(np.isnan(uvz), QNAN, uvz)
    uvz = np.where(in_range[:, None], uvz, f32(0)).astype(f32)
    out = {"colour": colour, "valid": valid, "uvz": uvz}
    if g is None:
        return out
    assert g.dtype == np.float32
    with np.errstate(all="ignore"):
        du0, du1 = c10 - c00, c11 - c01
        dcu = du0 + fv * (du1 - du0)
        dcv = bot - top
        gu = (g[:, 0] * dcu[:, 0] + g[:, 1] * dcu[:, 1]) + g[:, 2] * dcu[:, 2]
        gv = (g[:, 0] * dcv[:, 0] + g[:, 1] * dcv[:, 1]) + g[:, 2] * dcv[:, 2]
        gufx, gvfy = gu * fx, gv * fy
        g_xc = gufx / z
        g_yc = -(gvfy / z)
        g_z = (-gufx * xc + gvfy * yc) / (z * z)
        g_zc = -g_z
        gp = np.stack([(M[:, 4 * k] * g_xc + M[:, 4 * k + 1] * g_yc) + M[:, 4 * k + 2] * g_zc for k in range(3)], 1)
        gt = (gp[:, 0] * d[:, 0] + gp[:, 1] * d[:, 1]) + gp[:, 2] * d[:, 2]
        gd = t[:, None] * gp
    zero = f32(0)
    out["d_depth"] = np.where(valid, gt, zero).astype(f32)
    out["d_rays_o"] = np.where(valid[:, None], gp, zero).astype(f32)
    out["d_rays_d"] = np.where(valid[:, None], gd, zero).astype(f32)
    return out


# ---------------------------------------------------------------------------------------------- float64, torch
def _tables_f64(images, white_bkgd):
    """uint8 [V,H,W,C] -> float64 [V,H,W,3]: the colours the bytes stand for, in exact arithmetic up to float64."""
    img = torch.as_tensor(images).to(torch.float64) / 255.0
    if white_bkgd:
        return img[..., :3] * img[..., 3:4] + (1.0 - img[..., 3:4])
    return img[..., :3]


def warp_f64(o, d, t, s, poses, images, K, white_bkgd=False, z_min=1e-3, border=0.0):
    """o, d [n,3], t [n] float64 tensors (autograd flows to them); s [n] int64; poses [V,12], K [1|V,4] (any float
    dtype, read as float64), images uint8 -> (colour [n,3], valid [n] bool, uvz [n,3])."""
    poses, K, s = torch.as_tensor(poses).double(), torch.as_tensor(K).double(), torch.as_tensor(s)
    tab = _tables_f64(images, white_bkgd)
    V, H, W, _ = tab.shape
    in_range = (s >= 0) & (s < V)
    sc = torch.where(in_range, s, torch.zeros_like(s))
    M = poses[sc].view(-1, 3, 4)
    Kr = K[sc] if K.shape[0] > 1 else K[0].expand(s.shape[0], 4)
    def project(t_):
        p = (o + t_[:, None] * d) - M[:, :, 3]
        cam = torch.einsum("nkj,nk->nj", M[:, :, :3], p)  # R^T p
        xc, yc, z_ = cam[:, 0], cam[:, 1], -cam[:, 2]
        return Kr[:, 2] + Kr[:, 0] * (xc / z_), Kr[:, 3] - Kr[:, 1] * (yc / z_), z_

    with torch.no_grad():
        uvz = torch.stack(project(t), 1)
    # (the differentiable pass never sees a non-finite depth: such a row is invalid, a constant, and autograd would turn
    # its 0 x NaN into a NaN gradient where the definition says 0)
    u, v, z = project(torch.where(torch.isfinite(t), t, torch.ones_like(t)))
    valid = (in_range & torch.isfinite(t) & (t > 0) & (z >= z_min) & (u >= border) & (u <= (W - 1) - border)
             & (v >= border) & (v <= (H - 1) - border))
    us, vs = torch.where(valid, u, torch.zeros_like(u)), torch.where(valid, v, torch.zeros_like(v))
    x0 = torch.floor(us.detach()).long().clamp(max=W - 2)
    y0 = torch.floor(vs.detach()).long().clamp(max=H - 2)
    fu, fv = (us - x0)[:, None], (vs - y0)[:, None]
    c00, c10, c01, c11 = tab[sc, y0, x0], tab[sc, y0, x0 + 1], tab[sc, y0 + 1, x0], tab[sc, y0 + 1, x0 + 1]
    top = c00 + fu * (c10 - c00)
    bot = c01 + fu * (c11 - c01)
    colour = torch.where(valid[:, None], top + fv * (bot - top), torch.zeros_like(top))
    uvz = torch.where(in_range[:, None], uvz, torch.zeros(1, dtype=torch.float64))
    return colour, valid, uvz


def grads_f64(case, g, **kw):
    """The float64 reference of a case under the cotangent g [n,3] -> dict(colour, valid, uvz, d_depth, d_rays_o,
    d_rays_d); an invalid row's gradients are exactly 0 (its colour is a constant)."""
    o, d, t = (torch.as_tensor(case[k]).double().requires_grad_() for k in ("o", "d", "t"))
    colour, valid, uvz = warp_f64(o, d, t, case["s"], case["poses"], case["images"], case["K"], case["white_bkgd"],
                                  kw.get("z_min", 1e-3), case["border"])
    go, gd, gt = torch.autograd.grad(colour, (o, d, t), torch.as_tensor(g).double(), allow_unused=True)
    clean = lambda x, like: torch.nan_to_num(torch.zeros_like(like) if x is None else x, nan=0.0, posinf=0.0, neginf=0.0)
    mask = valid[:, None].double()
    return {"colour": colour.detach(), "valid": valid, "uvz": uvz, "d_depth": clean(gt, t) * valid.double(),
            "d_rays_o": clean(go, o) * mask, "d_rays_d": clean(gd, d) * mask}


def loss_f64(rgb, depth, rays_o, rays_d, src_view, poses, images, K, white_bkgd, kind="l1", threshold=None, z_min=1e-3,
             border=0.5, opacity=None):
    """core.loss.WarpConsistencyLoss in float64 (all tensor arguments float64 torch tensors)."""
    src_view = torch.as_tensor(src_view)
    if threshold is not None:
        src_view = torch.where(opacity.detach() > threshold, src_view, torch.full_like(src_view, -1))
    colour, valid, _ = warp_f64(rays_o, rays_d, depth, src_view, poses, images, K, white_bkgd, z_min, border)
    diff = rgb - colour
    per_row = (diff.abs() if kind == "l1" else diff * diff).mean(dim=1)
    return torch.where(valid, per_row, torch.zeros_like(per_row)).sum() / valid.sum().clamp(min=1).double()


# ---------------------------------------------------------------------------------------------- cases
def look_at(centre, target, up=(0.0, 0.0, 1.0)):
    """camera-to-world [3,4] float64 of a camera at `centre` looking at `target` down its own -z, y up."""
    centre, target, up = (np.asarray(a, dtype=np.float64) for a in (centre, target, up))
    zc = centre - target
    zc /= np.linalg.norm(zc)
    xc = np.cross(up, zc)
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    return np.concatenate([np.stack([xc, yc, zc], 1), centre[:, None]], 1)


# (n, V, H, W, C, white_bkgd, per-view K, border): the smallest shapes at which the kernel can go wrong - n: one row, a
# block's tail, one wave, one wave plus a row, more than one block; images: 2 x 2 (the smallest legal cell; only border 0
# leaves room for a target there), 5 x 7, 24 x 32; one and three views; RGB, RGBA with and without the white background;
# a shared and a per-view camera table; both borders
CASES = [(1, 1, 2, 2, 3, False, False, 0.0), (63, 3, 5, 7, 4, True, True, 0.5), (64, 3, 24, 32, 4, False, False, 0.0),
         (65, 1, 5, 7, 3, False, True, 0.5), (257, 3, 24, 32, 4, True, True, 0.5), (257, 3, 2, 2, 4, True, False, 0.0)]
N_INVALID = 11  # the deliberately invalid rows of make_case, each far from its threshold


def make_case(n, V, H, W, C, white_bkgd, per_view_K, border, seed):
    """A case of n rows: inputs as float32 / int64 / uint8 NumPy arrays in a dict.  Valid rows: a target (u*, v*) in
    source view s with fractional parts in [0.05, 0.95] and at least 0.05 px inside the border, back-projected at a
    depth z in [1, 6]; the ray runs from another camera position through that point and `t` is the distance along it.
    With n > N_INVALID, N_INVALID rows are invalid on purpose (kinds in case["kind"]): src_view -1 and V; depth 0, -1,
    NaN, +inf; a point 0.5 behind the source camera; a point 1.5 px outside each of the four borders.
    Asserts that the float32 and float64 restatements agree on `valid` for every row, that it is what the row was
    built to be, and that |u32 - u64|, |v32 - v64| < 0.01 px."""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(0, 2 * np.pi, V)
    centres = np.stack([4.0 * np.cos(ang), 4.0 * np.sin(ang), rng.uniform(0.5, 2.0, V)], 1)
    poses64 = np.stack([look_at(centres[i], rng.uniform(-0.3, 0.3, 3)) for i in range(V)])
    poses = poses64.reshape(V, 12).astype(f32)
    rows = V if per_view_K else 1
    # fx != fy and an off-centre principal point
    K = np.stack([W * rng.uniform(1.0, 1.2, rows), W * rng.uniform(0.8, 0.95, rows), W / 2 + rng.uniform(0.2, 0.4, rows),
                  H / 2 - rng.uniform(0.1, 0.3, rows)], 1).astype(f32)
    images = rng.integers(0, 256, (V, H, W, C), dtype=np.uint8)
    kinds = ["valid"] * n
    if n > N_INVALID:
        for i, kind in zip(rng.permutation(n)[:N_INVALID], ("s=-1", "s=V", "t=0", "t=-1", "t=nan", "t=inf", "behind",
                                                             "left", "right", "above", "below")):
            kinds[i] = kind
    s = rng.integers(0, V, n).astype(np.int64)
    P64, K64 = poses.astype(np.float64).reshape(V, 3, 4), K.astype(np.float64)
    o, d, t = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    lo, hi_u, hi_v = border + 0.05, (W - 1) - border - 0.05, (H - 1) - border - 0.05
    assert lo <= hi_u and lo <= hi_v, "no target fits these images inside this border"
    for r, kind in enumerate(kinds):
        def target(a, b):
            x = rng.uniform(a, b)
            return np.floor(x) + np.clip(x - np.floor(x), 0.05, 0.95)
        us, vs, z = target(lo, hi_u), target(lo, hi_v), rng.uniform(1.0, 6.0)
        if kind == "left":
            us = border - 1.5
        elif kind == "right":
            us = (W - 1) - border + 1.5
        elif kind == "above":
            vs = border - 1.5
        elif kind == "below":
            vs = (H - 1) - border + 1.5
        elif kind == "behind":
            z = -0.5
        fx, fy, cx, cy = K64[s[r] if per_view_K else 0]
        cam = np.array([(us - cx) / fx * z, -(vs - cy) / fy * z, -z])
        X = P64[s[r], :, :3] @ cam + P64[s[r], :, 3]
        # the ray's own camera: a position off the source camera's, at least 1 away from the point
        while True:
            origin = P64[s[r], :, 3] + rng.uniform(-1.5, 1.5, 3)
            if np.linalg.norm(X - origin) > 1.0 and np.linalg.norm(origin - P64[s[r], :, 3]) > 0.3:
                break
        t[r] = np.linalg.norm(X - origin)
        o[r], d[r] = origin, (X - origin) / t[r]
        if kind == "s=-1":
            s[r] = -1
        elif kind == "s=V":
            s[r] = V
        elif kind.startswith("t="):
            t[r] = {"t=0": 0.0, "t=-1": -1.0, "t=nan": np.nan, "t=inf": np.inf}[kind]
    case = {"o": o.astype(f32), "d": d.astype(f32), "t": t.astype(f32), "s": s, "poses": poses, "images": images, "K": K,
            "white_bkgd": bool(white_bkgd), "border": float(border), "kind": kinds}
    r32 = warp_f32(case["o"], case["d"], case["t"], s, poses, images, K, white_bkgd, 1e-3, border)
    with torch.no_grad():
        _, v64, uvz64 = warp_f64(*(torch.as_tensor(case[k]).double() for k in ("o", "d", "t")), s, poses, images, K,
                                 white_bkgd, 1e-3, border)
    want = np.array([k == "valid" for k in kinds])
    assert np.array_equal(r32["valid"], v64.numpy()) and np.array_equal(r32["valid"], want), (r32["valid"], v64, kinds)
    ok = want
    err = np.abs(r32["uvz"][ok, :2].astype(np.float64) - uvz64.numpy()[ok, :2])
    assert err.size == 0 or err.max() < 0.01, err.max()
    # ... and the cell is the same: every valid target is 0.05 px from a cell's edge, the two differ by less than 0.01
    return case


def case_tensors(case, device, dtype=torch.float32):
    o, d, t = (torch.as_tensor(case[k]).to(device, dtype) for k in ("o", "d", "t"))
    return o, d, t, torch.as_tensor(case["s"]).to(device), torch.as_tensor(case["poses"]).to(device), \
        torch.as_tensor(case["images"]).to(device), torch.as_tensor(case["K"]).to(device)


# ---------------------------------------------------------------------------------------------- end to end
# Three 24 x 32 views (focal 30) of the plane z = 0, fronto-parallel (R = I: the cameras look down -z), textured with a
# smooth ramp quantised to bytes: R linear in x, G linear in y, B a low-frequency product.  Rays of view 0, their depth
# started at the plane's times 1 +- 0.1; Adam on the per-ray depth through WarpConsistencyLoss("l2", border=0.5) against
# other_views(1) of view 0.  The error is max |depth - true| / true over the rows whose true point projects at least
# PLANE_MARGIN px inside the source view (a row nearer the border may leave the view on the way and stop moving).
PLANE_HW, PLANE_FOCAL = (24, 32), 30.0
PLANE_CENTRES = ((0.0, 0.0, 4.0), (0.9, 0.0, 4.0), (0.0, 1.0, 4.2))
PLANE_MARGIN = 3.0
E2E_STEPS, E2E_LR = 150, 0.02
# measured by tests/test_warp_cpu.py::test_depth_recovery_f64 (the float64 restatement, E2E_STEPS Adam steps at E2E_LR,
# view 0's own photograph as the rendered colour): from 1.000e-01 to 1.722e-02 - the floor is the byte quantisation of
# the two photographs (half a byte against a ramp of about seven bytes per pixel), not the optimiser
E2E_F64_ERR = 1.73e-2
# the GPU's bound: float32 rounding of the byte-quantised slopes on top of it
E2E_BOUND = 2.0 * E2E_F64_ERR


def plane_texture(x, y):
    return np.stack([0.5 + 0.2 * x, 0.5 + 0.2 * y, 0.5 + 0.1 * x * y], -1)


def plane_scene():
    """-> dict: images uint8 [3,24,32,3], poses [3,4,4] float32, hwf, and of view 0: rays o, d [768,3] float32 (unit d,
    the loaders' arithmetic in float64 rounded once), the true depth t [768], the start depth t0, src [768] int64 (the
    view other_views(1) names for view 0) and `interior`, the rows the error is taken over."""
    H, W = PLANE_HW
    f = PLANE_FOCAL
    hh, ww = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dirs = np.stack([(ww - W / 2) / f, -(hh - H / 2) / f, -np.ones_like(ww)], -1)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    images, poses = [], []
    for c in PLANE_CENTRES:
        c = np.asarray(c)
        tt = -c[2] / dirs[..., 2]
        X = c + tt[..., None] * dirs
        images.append(np.clip(np.rint(plane_texture(X[..., 0], X[..., 1]) * 255.0), 0, 255).astype(np.uint8))
        pose = np.eye(4)
        pose[:3, 3] = c
        poses.append(pose)
    c0 = np.asarray(PLANE_CENTRES[0])
    d0 = dirs.reshape(-1, 3)
    t_true = -c0[2] / d0[:, 2]
    dist = [np.linalg.norm(np.asarray(c) - c0) for c in PLANE_CENTRES[1:]]
    src = 1 + int(np.argmin(dist))
    X = c0 + t_true[:, None] * d0
    cs = np.asarray(PLANE_CENTRES[src])
    p = X - cs
    u, v = W / 2 + f * p[:, 0] / -p[:, 2], H / 2 - f * p[:, 1] / -p[:, 2]
    m = PLANE_MARGIN
    interior = (u >= m) & (u <= W - 1 - m) & (v >= m) & (v <= H - 1 - m)
    sign = np.where((np.arange(H * W) % 2) == 0, 1.1, 0.9)
    return {"images": np.stack(images), "poses": np.stack(poses).astype(f32), "hwf": (H, W, f),
            "o": np.broadcast_to(c0, d0.shape).astype(f32).copy(), "d": d0.astype(f32), "t": t_true.astype(f32),
            "t0": (t_true * sign).astype(f32), "src": np.full(H * W, src, dtype=np.int64), "interior": interior}


def recover_f64(scene, steps=E2E_STEPS, lr=E2E_LR):
    """The float64 run of the end-to-end test -> max relative depth error over the interior rows."""
    H, W, f = scene["hwf"]
    o, d = torch.as_tensor(scene["o"]).double(), torch.as_tensor(scene["d"]).double()
    poses12 = torch.as_tensor(scene["poses"])[:, :3, :4].reshape(-1, 12)
    K = torch.tensor([[f, f, W * 0.5, H * 0.5]], dtype=torch.float64)
    rgb = torch.as_tensor(scene["images"][0]).double().reshape(-1, 3) / 255.0  # view 0's own photograph
    depth =torch.as_tensor(scene["t0"]).double().requires_grad_()
    opt = torch.optim.Adam([depth], lr=lr)
    for _ in range(steps):
        opt.zero_grad()
        loss_f64(rgb, depth, o, d, scene["src"], poses12, scene["images"], K, False, kind="l2", border=0.5).backward()
        opt.step()
    t = torch.as_tensor(scene["t"]).double()
    inside = torch.as_tensor(scene["interior"])
    return float(((depth.detach() - t).abs() / t)[inside].max())
