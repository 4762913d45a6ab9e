"""Evaluation metrics without a GPU: the float64 restatement of skimage's SSIM (tests/metrics_ref.py) pinned by closed
forms, the argument checks of the new C entry points (fsn_ssim, fsn_psnr), and the Python layer's refusals."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as MR  # noqa: E402

import fs_nerf_amd  # noqa: E402,F401
from fs_nerf_amd import _lib as L  # noqa: E402
from fs_nerf_amd.core import metrics  # noqa: E402

C1, C2 = 0.01 ** 2, 0.03 ** 2


# ---------------------------------------------------------------- the float64 restatement
@pytest.mark.parametrize("a,b", [(0.0, 0.0), (0.3, 0.7), (0.9, 0.9), (1.0, 0.0), (0.25, 0.5)])
@pytest.mark.parametrize("gw", [True, False])
def test_constant_images_give_the_closed_form(a, b, gw):
    x, y = np.full((16, 19), a), np.full((16, 19), b)
    want = (2 * a * b + C1) / (a * a + b * b + C1)
    got = MR.ssim(x, y, channel_axis=None, gaussian_weights=gw)
    assert abs(got - want) <= 1e-12, (got, want)


@pytest.mark.parametrize("gw", [True, False])
@pytest.mark.parametrize("cov", [True, False])
def test_identity_and_symmetry(gw, cov):
    rng = np.random.default_rng(3)
    x, y = rng.random((23, 31, 3)), rng.random((23, 31, 3))
    assert abs(MR.ssim(x, x, gaussian_weights=gw, use_sample_covariance=cov) - 1.0) <= 1e-12
    assert MR.ssim(x, y, gaussian_weights=gw, use_sample_covariance=cov) == \
        MR.ssim(y, x, gaussian_weights=gw, use_sample_covariance=cov)
    assert MR.ssim(x, y, gaussian_weights=gw) < 0.5


def test_gaussian_taps_are_the_closed_form():
    w = MR.gaussian_taps()
    assert w.shape == (11,)
    raw = np.array([math.exp(-t * t / (2 * 1.5 * 1.5)) for t in range(-5, 6)])
    np.testing.assert_allclose(w, raw / raw.sum(), rtol=0, atol=1e-16)
    assert abs(w.sum() - 1.0) <= 1e-15
    assert np.array_equal(w, w[::-1])


def test_window_widths_and_covariance_normalisation():
    assert MR.window(True)[1] == 11 and MR.window(False)[1] == 7
    assert MR.cov_norm(11) == 121 / 120 and MR.cov_norm(7) == 49 / 48
    assert MR.cov_norm(11, False) == 1.0 and MR.cov_norm(7, False) == 1.0


def test_reflect_edges_are_half_sample_symmetric():
    img = np.arange(12.0 * 13).reshape(12, 13) ** 1.5
    taps = np.zeros(11)
    taps[0] = 1.0  # picks the pixel 5 to the left / above: the reflected halo itself
    out = MR.filter2d(img, taps)
    assert out[0, 0] == img[4, 4]  # -5 -> 4
    assert out[2, 3] == img[2, 1]  # -3 -> 2, -2 -> 1
    assert out[11, 12] == img[6, 7]


def test_restatement_matches_scipy_filters():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    img = rng.random((20, 27))
    g = nd.gaussian_filter(img, sigma=1.5, truncate=3.5, mode="reflect")
    np.testing.assert_allclose(MR.filter2d(img, MR.gaussian_taps()), g, rtol=0, atol=1e-14)
    u = nd.uniform_filter(img, size=7, mode="reflect")
    np.testing.assert_allclose(MR.filter2d(img, MR.window(False)[0]), u, rtol=0, atol=1e-14)


def test_too_small_images_are_an_error():
    with pytest.raises(ValueError):
        MR.ssim(np.zeros((10, 40)), np.zeros((10, 40)), channel_axis=None)
    MR.ssim(np.zeros((7, 7)), np.zeros((7, 7)), channel_axis=None, gaussian_weights=False)


# ---------------------------------------------------------------- C entry points, no device needed
def _s4(*v):
    return (C.c_int64 * 4)(*v)


def test_metric_entry_points_validate_without_gpu():
    lib = L.lib()
    fake = C.c_void_p(256)  # never dereferenced: every check below fails before a launch
    st = _s4(3 * 64 * 64, 1, 64 * 3, 3)
    # workspace queries
    assert lib.fsn_ssim_workspace_doubles(2, 3, 64, 65) == 2 * 3 * 2 * 3
    assert lib.fsn_ssim_workspace_doubles(1, 0, 64, 64) < 0
    assert lib.fsn_psnr_workspace_doubles(2, 3, 64, 64) == 2 * 3
    assert lib.fsn_psnr_workspace_doubles(-1, 3, 64, 64) < 0
    # N = 0: a no-op
    assert lib.fsn_ssim(None, None, 0, 3, 64, 64, None, None, L.FSN_SSIM_GAUSSIAN, 1, 1.0, 0.01, 0.03, None, None, None,
                        None, None) == 0
    assert lib.fsn_psnr(None, None, 0, 3, 64, 64, None, None, None, None, None) == 0
    # null pointers
    assert lib.fsn_ssim(None, fake, 1, 3, 64, 64, st, st, L.FSN_SSIM_GAUSSIAN, 1, 1.0, 0.01, 0.03, fake, fake, None, None,
                        None) == -1
    assert lib.fsn_ssim(fake, fake, 1, 3, 64, 64, st, st, L.FSN_SSIM_GAUSSIAN, 1, 1.0, 0.01, 0.03, None, fake, None, None,
                        None) == -1
    assert lib.fsn_ssim(fake, fake, 1, 3, 64, 64, None, st, L.FSN_SSIM_GAUSSIAN, 1, 1.0, 0.01, 0.03, fake, fake, None,
                        None, None) == -1
    assert lib.fsn_ssim(fake, fake, 1, 3, 64, 64, st, st, L.FSN_SSIM_GAUSSIAN, 1, 1.0, 0.01, 0.03, fake, fake, fake,
                        None, None) == -1  # a map without its strides
    assert lib.fsn_psnr(fake, None, 1, 3, 64, 64, st, st, fake, fake, None) == -1
    assert lib.fsn_psnr(fake, fake, 1, 3, 64, 64, st, st, fake, None, None) == -1
    assert b"null" in lib.fsn_last_error()
    # images smaller than the window
    assert lib.fsn_ssim(fake, fake, 1, 3, 10, 64, st, st, L.FSN_SSIM_GAUSSIAN, 1, 1.0, 0.01, 0.03, fake, fake, None, None,
                        None) == -1
    assert lib.fsn_ssim(fake, fake, 1, 3, 64, 6, st, st, L.FSN_SSIM_UNIFORM, 1, 1.0, 0.01, 0.03, fake, fake, None, None,
                        None) == -1
    assert b"smaller than" in lib.fsn_last_error()
    # unknown window
    for code in (2, -1, 7):
        assert lib.fsn_ssim(fake, fake, 1, 3, 64, 64, st, st, code, 1, 1.0, 0.01, 0.03, fake, fake, None, None,
                            None) == -2
    # the debug record exists only in the debug build
    buf = (C.c_uint32 * 4)()
    assert lib.fsn_debug_report(b"metrics", buf) == -2


# ---------------------------------------------------------------- the Python layer
def test_python_metrics_refuse_cpu_tensors():
    x = torch.rand(2, 16, 16, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.ssim(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.psnr(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        metrics.psnr(x, x, reduction="none")


def test_python_metrics_refuse_bad_shapes_and_arguments():
    x4 = torch.rand(2, 16, 16, 3)
    with pytest.raises(ValueError):
        metrics.ssim(x4, x4, channel_axis=2)
    with pytest.raises(ValueError):
        metrics.ssim(x4, x4, channel_axis=None)
    with pytest.raises(ValueError):
        metrics.ssim(x4[0], x4[0], channel_axis=1)
    with pytest.raises(ValueError):
        metrics.ssim(x4[0, :, :, 0], x4[0, :, :, 0], channel_axis=0)
    with pytest.raises(ValueError):
        metrics.ssim(x4[None], x4[None])  # 5-D
    with pytest.raises(ValueError):
        metrics.ssim(x4, x4[:1])  # shape mismatch
    with pytest.raises(ValueError):
        metrics.ssim(x4[:, :10], x4[:, :10])  # 10 rows < 11
    with pytest.raises(ValueError):
        metrics.ssim(x4, x4, data_range=None)
    with pytest.raises(ValueError):
        metrics.ssim(x4, x4, win_size=7)
    with pytest.raises(ValueError):
        metrics.ssim(x4, x4, sigma=2.0)
    with pytest.raises(ValueError):
        metrics.ssim(x4, x4, gaussian_weights=False, win_size=11)
    with pytest.raises(ValueError):
        metrics.ssim(x4, x4, reduction="sum")
    with pytest.raises(ValueError):
        metrics.psnr(x4, x4[:1])
    with pytest.raises(ValueError):
        metrics.psnr(x4[None], x4[None])
    with pytest.raises(ValueError):
        metrics.psnr(x4, x4, reduction="mean")
