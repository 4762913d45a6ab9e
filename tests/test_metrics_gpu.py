"""-m gpu: device-side PSNR and SSIM (fs_nerf_amd.core.metrics, csrc/metrics.hip) against the float64 restatement of
skimage 0.22 in tests/metrics_ref.py, their layouts and determinism, the reference-shaped evaluation() on rendered
frames, and the debug build's LDS index record of the SSIM kernel."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import debug_lib  # noqa: E402
import metrics_ref as MR  # noqa: E402

import fs_nerf_amd  # noqa: E402,F401
from fs_nerf_amd.core import metrics  # noqa: E402

pytestmark = pytest.mark.gpu

MEAN_TOL = 5e-7  # per-image mean SSIM
MAP_TOL = 3e-4  # every pixel of the full=True map
SIZES = [(11, 11), (13, 17), (100, 75), (800, 800)]
KINDS = ["uniform", "smooth", "flat", "identical"]
# (C, N, use_sample_covariance, data_range): every value of each factor appears
COMBOS = [(1, 4, True, 1.0), (3, 4, False, 255.0), (3, 1, True, 255.0), (1, 1, False, 1.0)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def make_pair(kind, N, H, W, C, seed):
    rng = np.random.default_rng(seed)
    if kind in ("uniform", "identical"):
        x = rng.random((N, H, W, C))
        y = x.copy() if kind == "identical" else rng.random((N, H, W, C))
    elif kind == "smooth":
        hh, ww = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
        base = 0.5 + 0.3 * np.sin(6.0 * hh + 1.0)[None, :, :, None] * np.cos(4.0 * ww)[None, :, :, None]
        x = base + 1e-2 * rng.random((N, H, W, C))
        y = base + 1e-2 * rng.random((N, H, W, C))
    else:  # near-flat: where float32 moments cancel
        x = 0.9 + 1e-4 * rng.random((N, H, W, C))
        y = 0.9 + 1e-4 * rng.random((N, H, W, C))
    return x.astype(np.float32), y.astype(np.float32)


def check_against_ref(x, y, dev, gw, cov, dr, what):
    """x, y: float32 numpy (N, H, W, C).  Per-image means, their mean, and the full map against the restatement."""
    N = x.shape[0]
    tx, ty = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    kw = dict(data_range=dr, gaussian_weights=gw, use_sample_covariance=cov)
    per, smap = metrics.ssim(tx, ty, channel_axis=-1, reduction="none", full=True, **kw)
    mean = metrics.ssim(tx, ty, channel_axis=-1, **kw)
    assert per.dtype == torch.float64 and per.shape == (N,) and mean.dim() == 0 and mean.dtype == torch.float64
    assert smap.shape == x.shape and smap.dtype == torch.float32
    per, smap = per.cpu().numpy(), smap.cpu().numpy()
    refs = []
    for n in range(N):
        m, S = MR.ssim(x[n], y[n], channel_axis=-1, full=True, **kw)
        refs.append(m)
        assert abs(per[n] - m) <= MEAN_TOL, f"{what} image {n}: mean {per[n]!r} vs {m!r} ({abs(per[n] - m):.3e})"
        err = np.abs(smap[n].astype(np.float64) - S).max()
        assert err <= MAP_TOL, f"{what} image {n}: map error {err:.3e}"
    assert abs(float(mean) - float(np.mean(refs))) <= MEAN_TOL, what


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("gw", [True, False], ids=["gaussian", "uniform7"])
def test_ssim_matches_the_float64_restatement(dev, size, kind, gw):
    H, W = size
    for i, (C, N, cov, dr) in enumerate(COMBOS):
        if H * W > 10 ** 5 and N > 1:
            N = 2  # keeps the host restatement's time in bounds at 800 x 800
        x, y = make_pair(kind, N, H, W, C, seed=1000 * i + H + W)
        x, y = x * np.float32(dr), y * np.float32(dr)
        check_against_ref(x, y, dev, gw, cov, dr, f"{kind} {H}x{W} C={C} N={N} cov={cov} dr={dr}")


def test_identical_pairs_give_one(dev):
    x = torch.rand(3, 40, 50, 3, device=dev)
    for gw in (True, False):
        v = metrics.ssim(x, x, gaussian_weights=gw, reduction="none")
        assert torch.all((v - 1.0).abs() <= 1e-12), v


def _models(dev):
    from fs_nerf_amd.core.models import NeRF
    out = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        m = NeRF(3, 3, 8, 256, (4,), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
        with torch.no_grad():
            m.sigma.weight.mul_(64.0)
            m.sigma.bias.add_(3.0)
        out.append(m.to(dev).eval())
    return out


def _pose(phi_deg, theta_deg=50.0, radius=4.0311289):
    th, ph = math.radians(theta_deg), math.radians(phi_deg)
    tr = torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, radius], [0, 0, 0, 1.0]])
    rt = torch.tensor([[1, 0, 0, 0], [0, math.cos(th), -math.sin(th), 0], [0, math.sin(th), math.cos(th), 0], [0, 0, 0, 1.0]])
    rp = torch.tensor([[math.cos(ph), -math.sin(ph), 0, 0], [math.sin(ph), math.cos(ph), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    return rp @ (rt @ tr)


HW = 64
HWF = (HW, HW, 0.5 * HW / math.tan(0.5 * 0.6911112))
NEAR, FAR = 2.0, 6.0


def _render(model, pose, dev):
    from fs_nerf_amd.render import rendering as R
    est = R.StratifiedEstimator(NEAR, FAR, 64, 128)
    with torch.no_grad():
        rgb, _ = R.render_frame(HWF, NEAR, FAR, pose, 1 << 20, est, model, white_bkgd=True, device=dev)
    return rgb


def test_ssim_of_rendered_frames_matches_the_restatement(dev):
    teacher, student = _models(dev)
    poses = [_pose(phi) for phi in (0.0, 135.0)]
    a = torch.stack([_render(teacher, p, dev) for p in poses])
    b = torch.stack([_render(student, p, dev) for p in poses])
    x, y = a.cpu().numpy(), b.cpu().numpy()
    for gw in (True, False):
        for cov in (True, False):
            check_against_ref(x, y, dev, gw, cov, 1.0, f"rendered gw={gw} cov={cov}")


def test_layouts_give_bitwise_identical_results(dev):
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.rand(3, 45, 70, 3, device=dev, generator=g)
    y = (x + 0.1 * torch.rand(3, 45, 70, 3, device=dev, generator=g)).clamp(0, 1)
    nhwc = metrics.ssim(x, y, reduction="none", full=True)
    nchw = metrics.ssim(x.permute(0, 3, 1, 2).contiguous(), y.permute(0, 3, 1, 2).contiguous(), channel_axis=1,
                        reduction="none", full=True)
    # non-contiguous: NHWC views of NCHW storage, and a channel-last view whose rows are a strided slice
    xv, yv = x.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1), y.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert not xv.is_contiguous()
    perm = metrics.ssim(xv, yv, reduction="none", full=True)
    big_x, big_y = torch.zeros(3, 90, 70, 3, device=dev), torch.zeros(3, 90, 70, 3, device=dev)
    big_x[:, ::2], big_y[:, ::2] = x, y
    sliced = metrics.ssim(big_x[:, ::2], big_y[:, ::2], reduction="none", full=True)
    for name, (v, m) in (("nchw", nchw), ("permuted", perm), ("sliced", sliced)):
        assert torch.equal(v, nhwc[0]), name
        mm = m.permute(0, 2, 3, 1) if name == "nchw" else m
        assert torch.equal(mm, nhwc[1]), name
    single = [metrics.ssim(x[n], y[n]) for n in range(3)]
    assert all(torch.equal(s, nhwc[0][n]) for n, s in enumerate(single))
    # psnr: layouts and the per-image split
    p0 = metrics.psnr(x, y, reduction="none")
    assert torch.equal(metrics.psnr(xv, yv, reduction="none"), p0)
    assert torch.equal(metrics.psnr(x.permute(0, 3, 1, 2).contiguous(), y.permute(0, 3, 1, 2).contiguous(),
                                    reduction="none"), metrics.psnr(x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2),
                                                                    reduction="none"))
    assert torch.allclose(metrics.psnr(x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2), reduction="none"), p0, rtol=0,
                          atol=1e-5)
    assert torch.equal(metrics.psnr(big_x[:, ::2], big_y[:, ::2]), metrics.psnr(x, y))


def test_repeated_calls_are_bitwise_identical(dev):
    x = torch.rand(4, 800, 800, 3, device=dev)
    y = torch.rand(4, 800, 800, 3, device=dev)
    a = metrics.ssim(x, y, reduction="none", full=True)
    b = metrics.ssim(x, y, reduction="none", full=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(metrics.psnr(x, y, reduction="none"), metrics.psnr(x, y, reduction="none"))
    assert torch.equal(metrics.psnr(x, y), metrics.psnr(x, y))


@pytest.mark.parametrize("shape", [(1, 64, 64, 3), (5, 37, 29, 3), (2, 800, 800, 3), (3, 11, 13, 1)])
def test_psnr_matches_float64(dev, shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.random(shape).astype(np.float32)
    y = np.clip(x + 0.05 * rng.standard_normal(shape), 0, 1).astype(np.float32)
    tx, ty = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    s = metrics.psnr(tx, ty)
    assert s.dim() == 0 and s.dtype == torch.float32 and s.is_cuda
    assert abs(float(s) - MR.psnr(x, y)) <= 1e-5
    per = metrics.psnr(tx, ty, reduction="none")
    assert per.shape == (shape[0],)
    for n in range(shape[0]):
        assert abs(float(per[n]) - MR.psnr(x[n], y[n])) <= 1e-5


def test_inputs_are_converted_and_nan_propagates(dev):
    x = torch.rand(2, 20, 20, 3, device=dev, dtype=torch.float64)
    y = torch.rand(2, 20, 20, 3, device=dev, dtype=torch.float64)
    assert torch.equal(metrics.ssim(x, y), metrics.ssim(x.float(), y.float()))
    assert torch.equal(metrics.psnr(x, y), metrics.psnr(x.float(), y.float()))
    x[1, 10, 10, 0] = float("nan")
    v = metrics.ssim(x, y, reduction="none")
    assert not torch.isnan(v[0]) and torch.isnan(v[1])
    assert torch.isnan(metrics.psnr(x, y))


class _Dataset:
    near, far, ndc = NEAR, FAR, False


class _Loader:
    """The shape of the reference's validation DataLoader: (rgb_gt [1,H,W,3], pose [1,4,4]) per view."""

    def __init__(self, items):
        self.items, self.dataset = items, _Dataset()

    def __iter__(self):
        return iter(self.items)

    def __len__(self):
        return len(self.items)


def test_evaluation_returns_the_reference_triple(dev):
    teacher, student = _models(dev)
    poses = [_pose(phi) for phi in (10.0, 100.0, 250.0)]
    gts = [_render(teacher, p, dev).cpu() for p in poses]  # the loader yields host tensors, as a DataLoader does
    loader = _Loader([(g[None], p[None]) for g, p in zip(gts, poses)])
    from fs_nerf_amd.render import rendering as R
    est = R.StratifiedEstimator(NEAR, FAR, 64, 128)
    out = metrics.evaluation(HWF, student, est, None, loader, 1 << 20, dev, white_bkgd=True)
    assert len(out) == 3 and out[2] is None
    val_psnr, val_ssim, _ = out
    assert isinstance(val_psnr, torch.Tensor) and val_psnr.dim() == 0 and val_psnr.dtype == torch.float32
    assert val_psnr.is_cuda and isinstance(val_ssim, float)
    frames = torch.stack([_render(student, p, dev) for p in poses])
    gt = torch.stack(gts).to(dev)
    assert torch.equal(val_psnr, metrics.psnr(frames, gt))
    assert val_ssim == float(metrics.ssim(frames, gt, channel_axis=-1, data_range=1.0, gaussian_weights=True))
    fx, gx = frames.cpu().numpy(), gt.cpu().numpy()
    ref = np.mean([MR.ssim(fx[n], gx[n], channel_axis=-1, data_range=1.0, gaussian_weights=True) for n in range(3)])
    assert abs(val_ssim - ref) <= MEAN_TOL
    assert abs(float(val_psnr) - MR.psnr(fx, gx)) <= 1e-5
    # the reference's positional call, render_step_size included
    again = metrics.evaluation(HWF, student, est, None, loader, 1 << 20, dev, 5e-3, white_bkgd=True)
    assert torch.equal(again[0], val_psnr) and again[1] == val_ssim


def test_ssim_kernel_keeps_inside_its_lds_arrays():
    """The debug library (every LDS index of k_ssim_tile range-checked) in a child process: the record stays empty."""
    rep = debug_lib.run_worker("metrics_debug_worker.py")
    assert rep["metrics"] == [0, 0, 0, 0], f"k_ssim_tile indexed outside an LDS array: {rep['metrics']} (count, line, index, extent)"
    debug_lib.assert_no_other_unit_recorded(rep)
