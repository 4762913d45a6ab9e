"""The learnable-intrinsics layer restated on the CPU: the camera table K(phi) and the rays under K in
torch, in any dtype (float64: the truth, autograd included; float32: the yardstick of float32 rounding), and the rows of
csrc/ray_dev.hpp's pinhole_ray_k / ndc_ray in NumPy float32, operation for operation (the library is built with
-ffp-contract=off), which the batch kernels must match bit for bit."""
import numpy as np
import torch

import pose_refine_ref as PR

F = np.float32


def table(phi, H, W, focal0, tie_focal=True):
    """phi [m,4] -> K = (fx, fy, cx, cy) [m,4] in phi's dtype."""
    fx = focal0 * torch.exp(phi[:, 0])
    fy = fx if tie_focal else focal0 * torch.exp(phi[:, 1])
    return torch.stack([fx, fy, W * 0.5 + W * phi[:, 2], H * 0.5 + H * phi[:, 3]], -1)


def rays(P, K, index, H, W, focal0, ndc, near=1.0):
    """PR.rays with the camera table K [1 or n, 4] in place of (focal, focal, W/2, H/2); the NDC constants stay those of
    the stored focal0."""
    dt = P.dtype
    index = torch.as_tensor(index, dtype=torch.int64)
    view, pix = index // (H * W), index % (H * W)
    h, w = (pix // W).to(dt), (pix % W).to(dt)
    Kv = K[view if K.shape[0] > 1 else torch.zeros_like(view)]
    c = torch.stack([(w - Kv[:, 2]) / Kv[:, 0], -(h - Kv[:, 3]) / Kv[:, 1], -torch.ones_like(w)], -1)
    c = c / c.norm(dim=-1, keepdim=True)
    M = P.reshape(-1, 3, 4)[view]
    d = (M[:, :, :3] @ c[:, :, None])[:, :, 0]
    o = M[:, :, 3]
    if not ndc:
        return o, d
    sx, sy = -1.0 / (W / (2.0 * focal0)), -1.0 / (H / (2.0 * focal0))
    t = -(near + o[:, 2]) / d[:, 2]
    p = o + t[:, None] * d
    no = torch.stack([sx * p[:, 0] / p[:, 2], sy * p[:, 1] / p[:, 2], 1.0 + 2.0 * near / p[:, 2]], -1)
    nd = torch.stack([sx * (d[:, 0] / d[:, 2] - p[:, 0] / p[:, 2]), sy * (d[:, 1] / d[:, 2] - p[:, 1] / p[:, 2]),
                      -2.0 * near / p[:, 2]], -1)
    return no, nd


def rows_f32(P, K, index, H, W, focal0, ndc, near=1.0):
    """The rows the batch kernels write for the flat ray indices `index` over poses P [n,12] and the table K [1 or n, 4]
    (both float32 as the kernel reads them) -> (o [B,3], d [B,3]) float32: pinhole_ray_k, then ndc_ray."""
    P, K = np.asarray(P, dtype=F).reshape(-1, 3, 4), np.asarray(K, dtype=F)
    index = np.asarray(index, dtype=np.int64)
    view, pix = index // (H * W), index % (H * W)
    row, col = pix // W, pix % W
    m = P[view]
    Kv = K[view if K.shape[0] > 1 else np.zeros_like(view)]
    fx, fy, cx, cy = Kv[:, 0], Kv[:, 1], Kv[:, 2], Kv[:, 3]
    dx = (col.astype(F) - cx) / fx
    dy = -((row.astype(F) - cy) / fy)
    dz = np.full_like(dx, F(-1.0))
    nrm = np.sqrt((dx * dx + dy * dy) + dz * dz)
    dx, dy, dz = dx / nrm, dy / nrm, dz / nrm
    d = np.stack([(dx * m[:, k, 0] + dy * m[:, k, 1]) + dz * m[:, k, 2] for k in range(3)], -1)
    o = m[:, :, 3].copy()
    if ndc:
        sx, sy = F(-1.0 / (W / (2.0 * focal0))), F(-1.0 / (H / (2.0 * focal0)))
        nr, two_near = F(near), F(2.0 * near)
        ddx, ddy, ddz = d[:, 0], d[:, 1], d[:, 2]
        t = -(nr + o[:, 2]) / ddz
        ox, oy, oz = o[:, 0] + t * ddx, o[:, 1] + t * ddy, o[:, 2] + t * ddz
        o = np.stack([sx * ox / oz, sy * oy / oz, F(1.0) + two_near / oz], -1)
        d = np.stack([sx * (ddx / ddz - ox / oz), sy * (ddy / ddz - oy / oz), -two_near / oz], -1)
    assert o.dtype == F and d.dtype == F
    return o, d


def camera_grad(P0, xi, phi, index, H, W, focal0, ndc, tie_focal, grad_o, grad_d):
    """(dL/dxi [n,6], dL/dphi [m,4]) by autograd through compose, table and rays, in the dtype of P0 (None gradients =
    zeros; xi None = no correction -> its gradient is None)."""
    phi = phi.detach().clone().requires_grad_(True)
    if xi is not None:
        xi = xi.detach().clone().requires_grad_(True)
    o, d = rays(P0 if xi is None else PR.compose(P0, xi), table(phi, H, W, focal0, tie_focal), index, H, W, focal0, ndc)
    loss = (phi * 0.0).sum() + (0.0 if xi is None else (xi * 0.0).sum())
    if grad_o is not None:
        loss = loss + (o * grad_o.to(o.dtype)).sum()
    if grad_d is not None:
        loss = loss + (d * grad_d.to(d.dtype)).sum()
    loss.backward()
    return None if xi is None else xi.grad, phi.grad


def random_phi(m, rng, focal=0.1, centre=0.03):
    """[m,4] float32: log focal factors ~ N(0, focal^2), principal-point offsets (in image sizes) ~ N(0, centre^2)."""
    return torch.from_numpy(np.concatenate([rng.standard_normal((m, 2)) * focal, rng.standard_normal((m, 2)) * centre],
                                           1).astype(np.float32))


def block_error(got, want, blocks):
    """max |got - want| over each column block, relative to the largest entry of `want`'s block (1 where it is all 0)."""
    got, want = got.double(), want.double()
    out = []
    for sl in blocks:
        scale = float(want[:, sl].abs().max())
        out.append(float((got[:, sl] - want[:, sl]).abs().max()) / (scale if scale > 0 else 1.0))
    return out


FOCAL_PP = (slice(0, 2), slice(2, 4))


def recover(step_fn, params0, n_steps=300, lr=1e-2):
    """PR.recover over several parameters: Adam from params0, step_fn(*params) -> loss.  -> the parameters after."""
    params = [p.detach().clone().requires_grad_(True) for p in params0]
    opt = torch.optim.Adam(params, lr=lr)
    for _ in range(n_steps):
        opt.zero_grad()
        step_fn(*params).backward()
        opt.step()
    return [p.detach() for p in params]
