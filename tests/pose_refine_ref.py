"""The learnable-pose layer restated in torch on the CPU, in any dtype: the composition through
torch.linalg.matrix_exp of the skew matrix, and the rays of csrc/ray_dev.hpp's pinhole_ray / ndc_ray.  The tests
evaluate it in float64 (the truth, autograd included) and in float32 (the yardstick of float32 rounding)."""
import math

import numpy as np
import torch


def skew(w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1),
                        torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def compose(P0, xi):
    """P0 [n,12] (rows 0..2 of camera-to-world), xi [n,6] = (omega, tau) -> [n,12]: [exp([omega]x) R0 | t0 + tau]."""
    M = P0.reshape(-1, 3, 4)
    R = torch.linalg.matrix_exp(skew(xi[:, :3])) @ M[:, :, :3]
    t = M[:, :, 3] + xi[:, 3:]
    return torch.cat([R, t[:, :, None]], dim=2).reshape(-1, 12)


def rays(P, index, H, W, focal, ndc, near=1.0):
    """Rays (o [B,3], d [B,3]) of the flat ray indices `index` (view * H * W + h * W + w) over the poses P [n,12]."""
    dt = P.dtype
    index = torch.as_tensor(index, dtype=torch.int64)
    view, pix = index // (H * W), index % (H * W)
    h, w = (pix // W).to(dt), (pix % W).to(dt)
    c = torch.stack([(w - W * 0.5) / focal, -(h - H * 0.5) / focal, -torch.ones_like(w)], -1)
    c = c / c.norm(dim=-1, keepdim=True)
    M = P.reshape(-1, 3, 4)[view]
    d = (M[:, :, :3] @ c[:, :, None])[:, :, 0]
    o = M[:, :, 3]
    if not ndc:
        return o, d
    sx, sy = -1.0 / (W / (2.0 * focal)), -1.0 / (H / (2.0 * focal))
    t = -(near + o[:, 2]) / d[:, 2]
    p = o + t[:, None] * d
    no = torch.stack([sx * p[:, 0] / p[:, 2], sy * p[:, 1] / p[:, 2], 1.0 + 2.0 * near / p[:, 2]], -1)
    nd = torch.stack([sx * (d[:, 0] / d[:, 2] - p[:, 0] / p[:, 2]), sy * (d[:, 1] / d[:, 2] - p[:, 1] / p[:, 2]),
                      -2.0 * near / p[:, 2]], -1)
    return no, nd


def pose_grad(P0, xi, index, H, W, focal, ndc, grad_o, grad_d):
    """dL/dxi [n,6] by autograd through compose and rays, in the dtype of P0 (None gradients = zeros)."""
    xi = xi.detach().clone().requires_grad_(True)
    o, d = rays(compose(P0, xi), index, H, W, focal, ndc)
    loss = o.sum() * 0.0
    if grad_o is not None:
        loss = loss + (o * grad_o.to(o.dtype)).sum()
    if grad_d is not None:
        loss = loss + (d * grad_d.to(d.dtype)).sum()
    loss.backward()
    return xi.grad


# ---------------------------------------------------------------- fixtures
def random_rotations(n, rng):
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def world_poses(n, seed=0):
    """[n,4,4] float32: random rotations, the camera at 4 R[:, 2] (on the sphere of radius 4, looking at the origin)."""
    rng = np.random.default_rng(seed)
    out = np.tile(np.eye(4), (n, 1, 1))
    out[:, :3, :3] = random_rotations(n, rng)
    out[:, :3, 3] = 4.0 * out[:, :3, 2]
    return torch.from_numpy(out.astype(np.float32))


def forward_poses(n, seed=0):
    """[n,4,4] float32 forward-facing cameras: rotations of sigma = 0.1 rad about random axes, translations of
    sigma = 0.3 - |d_z| and |o_z| of the NDC map stay well away from 0."""
    rng = np.random.default_rng(seed)
    w = torch.from_numpy(rng.standard_normal((n, 3)) * 0.1)
    out = torch.eye(4, dtype=torch.float64).repeat(n, 1, 1)
    out[:, :3, :3] = torch.linalg.matrix_exp(skew(w))
    out[:, :3, 3] = torch.from_numpy(rng.standard_normal((n, 3)) * 0.3)
    return out.float()


def poses12(poses):
    return poses[:, :3, :4].reshape(-1, 12).contiguous()


def random_xi(n, theta, rng, tau=0.1, forward=None):
    """[n,6] float32: omega of length `theta` about random axes, tau ~ N(0, tau^2).
    forward = (P0 [n,12], H, W, focal), for NDC cases: a view's axis is drawn again until every ray of the CORRECTED
    view keeps |d_z| >= 0.5 - the NDC map is singular at d_z = 0, and the fixture's promise for the stored poses
    (forward_poses) is kept for the corrected ones (at 1 rad about one axis in six does)."""
    axis = rng.standard_normal((n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    if forward is not None and theta > 0:
        P0, H, W, focal = forward
        pixels = torch.arange(H * W)
        for v in range(n):
            while True:
                w = torch.from_numpy(axis[v] * theta)[None]
                d = rays(compose(P0[v:v + 1].double(), torch.cat([w, torch.zeros(1, 3, dtype=torch.float64)], 1)),
                         pixels, H, W, focal, False)[1]
                if float(d[:, 2].abs().min()) >= 0.5:
                    break
                axis[v] = rng.standard_normal(3)
                axis[v] /= np.linalg.norm(axis[v])
    return torch.from_numpy(np.concatenate([axis * theta, rng.standard_normal((n, 3)) * tau], 1).astype(np.float32))


TAYLOR_THETA = 0.125  # csrc/pose_refine.hip: kPoseTaylorTheta2 = theta^2 = 2^-6
THETAS = (0.0, 1e-7, TAYLOR_THETA * (1 - 1e-5), TAYLOR_THETA * (1 + 1e-5), 1e-3, 0.3, 1.0)


def block_error(got, want):
    """max |got - want| of the omega block and of the tau block of a [n,6] gradient, each relative to the largest
    entry of `want`'s block (1 where that block is all zero)."""
    got, want = got.double(), want.double()
    out = []
    for sl in (slice(0, 3), slice(3, 6)):
        scale = float(want[:, sl].abs().max())
        out.append(float((got[:, sl] - want[:, sl]).abs().max()) / (scale if scale > 0 else 1.0))
    return out


def recover(step_fn, xi0, n_steps=300, lr=1e-2):
    """Adam on xi from xi0: step_fn(xi) -> loss (a tensor whose backward() fills xi.grad).  -> xi after n_steps."""
    xi = xi0.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([xi], lr=lr)
    for _ in range(n_steps):
        opt.zero_grad()
        step_fn(xi).backward()
        opt.step()
    return xi.detach()
