"""-m gpu: LPIPS-VGG on the device (fs_nerf_amd.core.metrics.LPIPS, csrc/lpips.hip) against the float64 and float32
restatements of tests/lpips_ref.py, its determinism and layout independence, evaluation() with it, and the debug
build's LDS index record of the convolution kernel."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import debug_lib  # noqa: E402
import lpips_ref as LR  # noqa: E402

import fs_nerf_amd  # noqa: E402,F401
from fs_nerf_amd.core import metrics  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = [((16, 16), 2), ((37, 53), 2), ((64, 64), 3)]  # ((H, W), N); 37 x 53: odd sizes through every pool
KINDS = ["uniform", "smooth", "near"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return LR.random_state_dict(seed=7)


@pytest.fixture(scope="module")
def net(sd, dev):
    m = metrics.LPIPS(net="vgg")
    m.load_state_dict(sd)
    return m.to(dev).eval()


def make_pair(kind, N, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 3, H, W, generator=g)
    if kind == "uniform":
        y = torch.rand(N, 3, H, W, generator=g)
    elif kind == "smooth":
        hh = torch.linspace(0, 1, H)[:, None]
        ww = torch.linspace(0, 1, W)[None, :]
        base = 0.5 + 0.3 * torch.sin(6.0 * hh + 1.0) * torch.cos(4.0 * ww)
        x = (base + 0.05 * x).clamp(0, 1)
        y = (base + 0.05 * torch.rand(N, 3, H, W, generator=g)).clamp(0, 1)
    else:  # near-identical: the squared difference cancels
        y = x + 1e-3 * torch.rand(N, 3, H, W, generator=g)
    return x.float(), y.float()


def check(net, sd, x, y, normalize, dev, what):
    val, per = net(x.to(dev), y.to(dev), retPerLayer=True, normalize=normalize)
    N = x.shape[0]
    assert val.shape == (N, 1, 1, 1) and val.dtype == torch.float32 and val.is_cuda
    assert len(per) == 5 and all(p.shape == (N, 1, 1, 1) for p in per)
    v64, p64 = LR.lpips(sd, x, y, normalize, torch.float64)
    v32, p32 = LR.lpips(sd, x, y, normalize, torch.float32)
    hip = torch.cat([p.reshape(1, N) for p in per]).double().cpu()
    got = val.reshape(N).double().cpu()
    for a, b, c, name in ((hip, p64, p32.double(), "layer"), (got[None], v64[None], v32.double()[None], "total")):
        bar = 4 * (c - b).abs() + 1e-6 * b.abs() + 1e-9
        err = (a - b).abs()
        assert bool((err <= bar).all()), f"{what} {name}: |hip - f64| {err.tolist()} over {bar.tolist()} (f64 {b.tolist()})"
    assert float(v64.min()) >= 0.0


@pytest.mark.parametrize("size,N", SMALL, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("normalize", [False, True])
def test_matches_the_restatement(net, sd, dev, size, N, kind, normalize):
    H, W = size
    x, y = make_pair(kind, N, H, W, seed=H * W + N)
    if not normalize:
        x, y = 2 * x - 1, 2 * y - 1
    check(net, sd, x, y, normalize, dev, f"{kind} {H}x{W} normalize={normalize}")


@pytest.mark.parametrize("size,kind,normalize", [((378, 504), "smooth", True), ((800, 800), "uniform", False)],
                         ids=["378x504", "800x800"])
def test_matches_the_restatement_at_frame_sizes(net, sd, dev, size, kind, normalize):
    H, W = size
    x, y = make_pair(kind, 1, H, W, seed=H + W)
    if not normalize:
        x, y = 2 * x - 1, 2 * y - 1
    check(net, sd, x, y, normalize, dev, f"{kind} {H}x{W}")


def test_determinism_layouts_and_batches(net, dev):
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.rand(3, 3, 48, 70, device=dev, generator=g)
    y = torch.rand(3, 3, 48, 70, device=dev, generator=g)
    a = net(x, y, normalize=True)
    assert torch.equal(a, net(x, y, normalize=True))
    # NHWC storage seen as NCHW, and a sliced view of a larger batch
    xh, yh = x.permute(0, 2, 3, 1).contiguous(), y.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(net(xh.permute(0, 3, 1, 2), yh.permute(0, 3, 1, 2), normalize=True), a)
    big_x = torch.zeros(6, 4, 48, 71, device=dev)
    big_y = torch.zeros(6, 4, 48, 71, device=dev)
    big_x[::2, 1:, :, 1:] = x
    big_y[::2, 1:, :, 1:] = y
    assert torch.equal(net(big_x[::2, 1:, :, 1:], big_y[::2, 1:, :, 1:], normalize=True), a)
    # a batch is its pairs one by one
    singles = torch.cat([net(x[n:n + 1], y[n:n + 1], normalize=True) for n in range(3)])
    assert torch.equal(singles, a)
    # identical inputs
    z, per = net(x, x, retPerLayer=True)
    assert torch.equal(z, torch.zeros_like(z)) and all(torch.equal(p, torch.zeros_like(p)) for p in per)


def test_weights_are_repacked_when_they_change(sd, dev):
    m = metrics.LPIPS().to(dev)
    m.load_state_dict(sd)
    x = torch.rand(1, 3, 32, 32, device=dev)
    y = torch.rand(1, 3, 32, 32, device=dev)
    a = m(x, y)
    with torch.no_grad():
        m.lin4.model[1].weight.zero_()
    _, per = m(x, y, retPerLayer=True)
    assert float(per[4]) == 0.0 and float(per[0]) > 0.0
    m.load_state_dict(sd)
    assert torch.equal(m(x, y), a)


# ---------------------------------------------------------------- evaluation() on rendered frames
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


def test_evaluation_with_lpips(net, sd, dev):
    teacher, student = _models(dev)
    poses = [_pose(phi) for phi in (10.0, 100.0, 250.0)]
    gts = [_render(teacher, p, dev).cpu() for p in poses]
    loader = _Loader([(g[None], p[None]) for g, p in zip(gts, poses)])
    from fs_nerf_amd.render import rendering as R
    est = R.StratifiedEstimator(NEAR, FAR, 64, 128)
    base = metrics.evaluation(HWF, student, est, None, loader, 1 << 20, dev, white_bkgd=True)
    assert base[2] is None
    out = metrics.evaluation(HWF, student, est, net, loader, 1 << 20, dev, white_bkgd=True)
    assert torch.equal(out[0], base[0]) and out[1] == base[1]
    val = out[2]
    assert isinstance(val, torch.Tensor) and val.dim() == 0 and val.dtype == torch.float32 and val.is_cuda
    frames = torch.stack([_render(student, p, dev) for p in poses]).permute(0, 3, 1, 2)
    gt = torch.stack(gts).to(dev).permute(0, 3, 1, 2)
    assert torch.equal(val, net(frames, gt).mean())
    v64, _ = LR.lpips(sd, frames.cpu(), gt.cpu())
    assert abs(float(val) - float(v64.mean())) <= 1e-5 * float(v64.mean()) + 1e-7


def test_conv_kernel_keeps_inside_its_lds_arrays():
    """The debug library (every LDS index of k_lpips_conv range-checked) in a child process: the record stays empty."""
    rep = debug_lib.run_worker("lpips_debug_worker.py")
    assert rep["lpips"] == [0, 0, 0, 0], f"k_lpips_conv indexed outside an LDS array: {rep['lpips']} (count, line, index, extent)"
    debug_lib.assert_no_other_unit_recorded(rep)
