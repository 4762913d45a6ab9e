"""Float64 restatement of the gradient of the interior-mean SSIM (csrc/ssim_grad.hip), in NumPy on top of
tests/metrics_ref.py: the yardstick of ops.ssim_grad_nchw and core.loss.SSIMLoss.  tests/test_ssim_grad_cpu.py pins it
against float64 torch autograd.

Per channel, with metrics_ref's taps w, radius r, cn, C1, C2 and moments:
  A1 = 2 ux uy + C1,  A2 = 2 cn (uxy - ux uy) + C2,  B1 = ux^2 + uy^2 + C1,  B2 = cn (uxx - ux^2 + uyy - uy^2) + C2,
  S = A1 A2 / (B1 B2);  on the interior [r, H-r) x [r, W-r), zero elsewhere, g = upstream / (C (H-2r) (W-2r)):
  Suxy = 2 cn A1 / (B1 B2),  Suxx = Suyy = -S cn / B2,
  Sux = (2 uy A2 - 2 cn uy A1) / (B1 B2) - 2 S ux / B1 + 2 S cn ux / B2,  Suy: x and y swapped;
  dx = F[g Sux] + 2 x F[g Suxx] + y F[g Suxy],  dy: x and y swapped,  F[m](p) = sum_q w(q - p) m(q) (zero extension).
The condition magnitude of an entry, the same sums over absolute values:
  Tx = F[|g Sux|] + 2 |x| F[|g Suxx|] + |y| F[|g Suxy|],  Ty: x and y swapped."""
import numpy as np

import metrics_ref as MR


def adjoint_filter(m, taps):
    """F[m](p) = sum_q w(q - p) m(q) of a 2-D float64 map that is zero outside its array: separable, zero extension."""
    r = len(taps) // 2
    H, W = m.shape
    p = np.pad(m, r)
    rows = sum(taps[k] * p[:, k:k + W] for k in range(len(taps)))
    return sum(taps[k] * rows[k:k + H, :] for k in range(len(taps)))


def channel_grad(x, y, g, gaussian_weights=True, use_sample_covariance=True, data_range=1.0, K1=0.01, K2=0.03):
    """One 2-D channel, the weight g of every interior pixel of S given: (dx, dy, Tx, Ty), float64 [H, W]."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    taps, win = MR.window(gaussian_weights)
    r = win // 2
    H, W = x.shape
    if min(H, W) < win:
        raise ValueError("win_size exceeds image extent")
    cn = MR.cov_norm(win, use_sample_covariance)
    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    ux, uy = MR.filter2d(x, taps), MR.filter2d(y, taps)
    uxx, uyy, uxy = MR.filter2d(x * x, taps), MR.filter2d(y * y, taps), MR.filter2d(x * y, taps)
    A1, A2 = 2 * ux * uy + C1, 2 * cn * (uxy - ux * uy) + C2
    B1, B2 = ux ** 2 + uy ** 2 + C1, cn * (uxx - ux ** 2 + uyy - uy ** 2) + C2
    S = A1 * A2 / (B1 * B2)
    mask = np.zeros((H, W))
    mask[r:H - r, r:W - r] = g
    Suxy = mask * (2 * cn * A1 / (B1 * B2))
    Suxx = mask * (-S * cn / B2)
    Sux = mask * ((2 * uy * A2 - 2 * cn * uy * A1) / (B1 * B2) - 2 * S * ux / B1 + 2 * S * cn * ux / B2)
    Suy = mask * ((2 * ux * A2 - 2 * cn * ux * A1) / (B1 * B2) - 2 * S * uy / B1 + 2 * S * cn * uy / B2)
    F = lambda m: adjoint_filter(m, taps)  # noqa: E731
    Fxx, Fxy = F(Suxx), F(Suxy)
    dx = F(Sux) + 2 * x * Fxx + y * Fxy
    dy = F(Suy) + 2 * y * Fxx + x * Fxy
    Axx, Axy = F(np.abs(Suxx)), F(np.abs(Suxy))
    Tx = F(np.abs(Sux)) + 2 * np.abs(x) * Axx + np.abs(y) * Axy
    Ty = F(np.abs(Suy)) + 2 * np.abs(y) * Axx + np.abs(x) * Axy
    return dx, dy, Tx, Ty


def ssim_grad(x, y, upstream=1.0, **kw):
    """One image of shape (C, H, W): the gradient of upstream * ssim(x, y) (the mean of S over the interior and the
    channels) -> (dx, dy, Tx, Ty), float64 (C, H, W)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    C, H, W = x.shape
    r = MR.window(kw.get("gaussian_weights", True))[1] // 2
    g = upstream / (C * (H - 2 * r) * (W - 2 * r))
    parts = [channel_grad(x[c], y[c], g, **kw) for c in range(C)]
    return tuple(np.stack([p[k] for p in parts]) for k in range(4))


def ssim_grad_batch(x, y, upstream, **kw):
    """(N, C, H, W) with one upstream weight per image -> (dx, dy, Tx, Ty), float64 (N, C, H, W)."""
    parts = [ssim_grad(x[n], y[n], float(upstream[n]), **kw) for n in range(len(x))]
    return tuple(np.stack([p[k] for p in parts]) for k in range(4))
