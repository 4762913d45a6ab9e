"""CPU: the NumPy restatement of the SSIM gradient (tests/ssim_grad_ref.py) against float64 torch autograd of a torch
restatement of the interior mean, whose forward value is pinned to tests/metrics_ref.py.  An interior pixel's window
never leaves the image, so the torch restatement needs no padding: a 'valid' correlation IS the interior."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics_ref as MR
import ssim_grad_ref as GR

# (H, W, gaussian window)
SHAPES = [(11, 11, True), (12, 17, True), (7, 7, False), (20, 9, False), (33, 45, True), (33, 45, False)]


def torch_interior_ssim(x, y, gaussian_weights, use_sample_covariance, data_range=1.0, K1=0.01, K2=0.03):
    """x, y: float64 (N, C, H, W) -> ssim_n (N,), differentiable."""
    taps, win = MR.window(gaussian_weights)
    w = torch.from_numpy(np.outer(taps, taps))[None, None]
    cn = MR.cov_norm(win, use_sample_covariance)
    C1, C2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    N, C, H, W = x.shape

    def filt(t):
        return F.conv2d(t.reshape(N * C, 1, H, W), w).reshape(N, C, H - win + 1, W - win + 1)
    ux, uy, uxx, uyy, uxy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    return S.mean(dim=(1, 2, 3))


def pair(N, C, H, W, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((N, C, H, W))
    y = np.clip(0.7 * x + 0.3 * rng.random((N, C, H, W)), 0.0, 1.0)
    return x, y


@pytest.mark.parametrize("H,W,gauss", SHAPES)
@pytest.mark.parametrize("sample_cov", [True, False])
def test_restatement_is_float64_autograd(H, W, gauss, sample_cov):
    N, C = 3, 2
    x, y = pair(N, C, H, W, seed=H * 100 + W)
    up = np.array([0.75, -1.5, 2.0])  # per-image upstream weights
    tx, ty = torch.from_numpy(x).requires_grad_(), torch.from_numpy(y).requires_grad_()
    vals = torch_interior_ssim(tx, ty, gauss, sample_cov)
    # the forward value of the torch restatement is metrics_ref's
    for n in range(N):
        ref = MR.ssim(x[n], y[n], channel_axis=0, gaussian_weights=gauss, use_sample_covariance=sample_cov)
        assert abs(vals[n].item() - ref) <= 1e-13
    (vals * torch.from_numpy(up)).sum().backward()
    dx, dy, Tx, Ty = GR.ssim_grad_batch(x, y, up, gaussian_weights=gauss, use_sample_covariance=sample_cov)
    # both sides are float64 evaluations of the same function.  The device bar 2^-38 T allows ~16 roundings (2^-53)
    # amplified by 1 / B2 with B2 down to C2 ~ 2^-10; these textured pairs have B2 >= 2^-8 (variances ~ 0.05), so each
    # side is within 16 * 2^-53 * 2^8 = 2^-41 T of the exact value and the two within 2^-40 T of each other
    assert np.all(np.abs(dx - tx.grad.numpy()) <= 2.0 ** -40 * Tx), np.max(np.abs(dx - tx.grad.numpy()) / Tx)
    assert np.all(np.abs(dy - ty.grad.numpy()) <= 2.0 ** -40 * Ty), np.max(np.abs(dy - ty.grad.numpy()) / Ty)
    assert np.abs(dx).max() > 0 and np.abs(dy).max() > 0
    # gradients reach the border pixels (through the windows of interior pixels) although S is cropped
    assert np.abs(dx[:, :, 0, 0]).min() > 0


@pytest.mark.parametrize("H,W,gauss", SHAPES)
def test_identical_images_have_zero_gradient_up_to_conditioning(H, W, gauss):
    """x == y is the maximum of S (= 1 everywhere): the terms of Sux, each ~ 2 cn ux / C2, cancel."""
    x, _ = pair(1, 3, H, W, seed=H + W)
    dx, dy, Tx, Ty = GR.ssim_grad(x[0], x[0], 1.0, gaussian_weights=gauss)
    assert np.all(np.abs(dx) <= 2.0 ** -38 * Tx) and np.all(np.abs(dy) <= 2.0 ** -38 * Ty)
    assert Tx.min() > 0


def test_gradient_is_linear_in_upstream_and_split_over_channels():
    x, y = pair(1, 3, 12, 17, seed=5)
    a = GR.ssim_grad(x[0], y[0], 1.0)
    b = GR.ssim_grad(x[0], y[0], -2.5)
    # (the weight enters every map entry with one rounding: a handful of 2^-53 T, T being the sum of magnitudes)
    assert np.all(np.abs(b[0] + 2.5 * a[0]) <= 2.0 ** -48 * b[2]) and np.allclose(b[2], 2.5 * a[2], rtol=1e-14, atol=0)
    # a channel's gradient depends on the other channels only through the 1 / C of the mean
    one = GR.ssim_grad(x[0, 1:2], y[0, 1:2], 1.0)
    assert np.all(np.abs(one[0][0] - 3.0 * a[0][1]) <= 2.0 ** -48 * one[2][0])
