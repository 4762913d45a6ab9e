"""Float64 restatement of skimage.metrics.structural_similarity (scikit-image 0.22, the version the reference pins in
environment.yaml) and of the reference's PSNR, in NumPy: the yardstick of fs_nerf_amd.core.metrics.

scikit-image is not a dependency of this project, so no fixture is generated from it: this module follows the published
algorithm of skimage 0.22 (skimage/metrics/_structural_similarity.py) step by step, and tests/test_metrics_cpu.py pins
it with closed forms.  Parity with skimage itself is therefore unpinned.

  window    gaussian_weights=True: scipy.ndimage.gaussian_filter, sigma 1.5, truncate 3.5 -> radius 5, 11 taps
            exp(-t^2 / (2 sigma^2)) normalised to sum 1; False: uniform_filter of size 7.  Both separable, both with
            scipy's mode='reflect' (half-sample symmetric: d c b a | a b c d | d c b a), i.e. numpy's pad 'symmetric'.
  moments   ux, uy, uxx, uyy, uxy = filtered x, y, x*x, y*y, x*y
  cov       cn = NP / (NP - 1), NP = win_size^2 (also for the Gaussian window), or 1 without sample covariance;
            vx = cn (uxx - ux^2), vy = cn (uyy - uy^2), vxy = cn (uxy - ux uy)
  S         ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), C1 = (K1 R)^2, C2 = (K2 R)^2
  mean      S cropped by the radius on every side, mean in float64; multichannel: mean over channels.
"""
import math

import numpy as np

SIGMA, TRUNCATE = 1.5, 3.5
GAUSS_RADIUS = int(TRUNCATE * SIGMA + 0.5)  # 5
GAUSS_WIN = 2 * GAUSS_RADIUS + 1  # 11, skimage: win_size = 2 * int(truncate * sigma + 0.5) + 1
UNIFORM_WIN = 7


def gaussian_taps(sigma=SIGMA, radius=GAUSS_RADIUS):
    t = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 * (t / sigma) ** 2)
    return w / w.sum()


def window(gaussian_weights):
    """(taps, win_size) of the separable window."""
    if gaussian_weights:
        return gaussian_taps(), GAUSS_WIN
    return np.full(UNIFORM_WIN, 1.0 / UNIFORM_WIN), UNIFORM_WIN


def cov_norm(win_size, use_sample_covariance=True):
    NP = win_size ** 2
    return NP / (NP - 1.0) if use_sample_covariance else 1.0


def filter2d(img, taps):
    """Separable correlation of a 2-D float64 image with scipy's mode='reflect' edges."""
    r = len(taps) // 2
    H, W = img.shape
    p = np.pad(img, r, mode="symmetric")
    rows = sum(taps[k] * p[:, k:k + W] for k in range(len(taps)))
    return sum(taps[k] * rows[k:k + H, :] for k in range(len(taps)))


def ssim_map(x, y, data_range=1.0, gaussian_weights=True, use_sample_covariance=True, K1=0.01, K2=0.03):
    """The uncropped SSIM map of one 2-D channel, float64."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    taps, win = window(gaussian_weights)
    if min(x.shape) < win:
        raise ValueError("win_size exceeds image extent")
    cn = cov_norm(win, use_sample_covariance)
    ux, uy = filter2d(x, taps), filter2d(y, taps)
    uxx, uyy, uxy = filter2d(x * x, taps), filter2d(y * y, taps), filter2d(x * y, taps)
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    return (A1 * A2) / (B1 * B2)


def ssim(x, y, data_range=1.0, channel_axis=-1, gaussian_weights=True, use_sample_covariance=True, K1=0.01, K2=0.03,
         full=False):
    """structural_similarity of one image: (H, W) with channel_axis=None, or channels on `channel_axis`."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    kw = dict(data_range=data_range, gaussian_weights=gaussian_weights, use_sample_covariance=use_sample_covariance,
              K1=K1, K2=K2)
    r = window(gaussian_weights)[1] // 2
    if channel_axis is None:
        S = ssim_map(x, y, **kw)
        m = S[r:S.shape[0] - r, r:S.shape[1] - r].mean(dtype=np.float64)
        return (m, S) if full else m
    xs, ys = np.moveaxis(x, channel_axis, -1), np.moveaxis(y, channel_axis, -1)
    maps = [ssim_map(xs[..., c], ys[..., c], **kw) for c in range(xs.shape[-1])]
    m = float(np.mean([S[r:S.shape[0] - r, r:S.shape[1] - r].mean(dtype=np.float64) for S in maps]))
    if full:
        return m, np.moveaxis(np.stack(maps, axis=-1), -1, channel_axis)
    return m


def psnr(pred, gt):
    """-10 log10 of the float64 MSE over every element (run-nerf.py:160)."""
    d = np.asarray(pred, dtype=np.float64) - np.asarray(gt, dtype=np.float64)
    return -10.0 * math.log10(float(np.mean(d * d)))
