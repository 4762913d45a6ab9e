"""-m gpu: LPIPS-VGG as a loss (core.loss.LPIPSLoss, metrics.LPIPS with grad inputs, ops.lpips_vgg_fwd_save /
lpips_vgg_bwd, csrc/lpips.hip).  The value is the evaluation metric's, bit for bit; the gradient is compared with the
float64 restatement of tests/lpips_grad_ref.py, with that restatement in float32 as the yardstick:
    E(a) = max|a - g64| / max|g64|  per tensor,        E(hip) <= 4 E(f32 restatement) + 1e-6
(the 4x margin over the float32 yardstick is the forward test's own).  The inputs are lpips_grad_ref.CASES, whose seeds
keep every ReLU unit and pool winner away from a flip (tests/test_lpips_grad_cpu.py asserts it).  Set
FSN_LPIPS_ACCURACY_OUT=<file> to have the E values written as JSON (profiles/lpips_grad_accuracy.json is such a run)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import debug_lib  # noqa: E402
import lpips_grad_ref as GR  # noqa: E402
import lpips_ref as LR  # noqa: E402

import fs_nerf_amd  # noqa: E402,F401
from fs_nerf_amd import ops  # noqa: E402
from fs_nerf_amd.core import metrics  # noqa: E402
from fs_nerf_amd.core.loss import LPIPSLoss  # noqa: E402

pytestmark = pytest.mark.gpu

_ACCURACY = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return LR.random_state_dict(seed=GR.SD_SEED)


@pytest.fixture(scope="module")
def net(sd, dev):
    m = metrics.LPIPS(net="vgg")
    m.load_state_dict(sd)
    return m.to(dev).eval()


def _weights(N):
    return torch.tensor([0.7, -1.3, 0.45, 1.1][:N], dtype=torch.float32)


_REF = {}


def reference(sd, name):
    """(x, y, normalize, up, (dx64, dy64), (dx32, dy32)) of a committed case, computed once."""
    if name not in _REF:
        x, y, normalize = GR.case_inputs(name)
        up = _weights(x.shape[0])
        _, _, dx64, dy64 = GR.value_and_grad(sd, x, y, up, normalize, torch.float64)
        _, _, dx32, dy32 = GR.value_and_grad(sd, x, y, up, normalize, torch.float32)
        _REF[name] = (x, y, normalize, up, (dx64, dy64), (dx32, dy32))
    return _REF[name]


def E(a, g64):
    return float((a.double() - g64).abs().max() / g64.abs().max())


# ---------------------------------------------------------------- value
@pytest.mark.parametrize("name", ["16x16", "37x53", "32x32x3"])
def test_value_with_grad_inputs_is_the_metric_bit_for_bit(net, sd, dev, name):
    x, y, normalize = GR.case_inputs(name)
    N = x.shape[0]
    xd, yd = x.to(dev), y.to(dev)
    with torch.no_grad():
        val0, per0 = net(xd, yd, retPerLayer=True, normalize=normalize)
    xg, yg = xd.clone().requires_grad_(), yd.clone().requires_grad_()
    val1, per1 = net(xg, yg, retPerLayer=True, normalize=normalize)
    assert val1.requires_grad and val1.shape == (N, 1, 1, 1)
    assert torch.equal(val1.detach(), val0)
    assert all(torch.equal(a, b) for a, b in zip(per1, per0)) and not any(p.requires_grad for p in per1)
    for want in ((True, True), (True, False), (False, True)):
        a = xd.clone().requires_grad_(want[0])
        b = yd.clone().requires_grad_(want[1])
        v = LPIPSLoss(net, normalize=normalize, channel_axis=1, reduction="none")(a, b)
        assert v.shape == (N,) and v.dtype == torch.float32 and v.requires_grad
        assert torch.equal(v.detach(), val0.reshape(N))
    m = LPIPSLoss(net, normalize=normalize, channel_axis=1)(xg, yg)
    assert m.dim() == 0 and m.dtype == torch.float32 and torch.equal(m.detach(), val0.mean())
    # no input needs a gradient: the evaluation path, and nothing to back-propagate
    v = LPIPSLoss(net, normalize=normalize, channel_axis=1, reduction="none")(xd, yd)
    assert not v.requires_grad and torch.equal(v, val0.reshape(N))


# ---------------------------------------------------------------- gradient
def _grads(net, x, y, normalize, up, dev, want=(True, True), **attrs):
    a = x.to(dev).requires_grad_(want[0])
    b = y.to(dev).requires_grad_(want[1])
    loss = LPIPSLoss(net, normalize=normalize, channel_axis=1, reduction="none")
    for k, v in attrs.items():
        setattr(loss, k, v)
    (loss(a, b) * up.to(dev)).sum().backward()
    return a.grad, b.grad


@pytest.mark.parametrize("name", ["16x16", "16x16n", "37x53", "32x32x3"])
def test_gradient_against_the_float64_restatement(net, sd, dev, name):
    x, y, normalize, up, g64, g32 = reference(sd, name)
    dx, dy = _grads(net, x, y, normalize, up, dev)
    assert dx.shape == x.shape and dy.shape == y.shape and dx.dtype == torch.float32
    rec = {}
    for what, hip, r64, r32 in (("dx", dx, g64[0], g32[0]), ("dy", dy, g64[1], g32[1])):
        assert bool(torch.isfinite(hip).all())
        e_hip, e_f32 = E(hip.cpu(), r64), E(r32, r64)
        rec[what] = {"E_hip": e_hip, "E_f32_restatement": e_f32}
        print(f"{name} {what}: E(hip) {e_hip:.3e}  E(f32 restatement) {e_f32:.3e}")
    _ACCURACY[name] = rec
    out = os.environ.get("FSN_LPIPS_ACCURACY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"measure": "E(a) = max|a - g64| / max|g64| per tensor; bar E(hip) <= 4 E(f32) + 1e-6",
                       "cases": _ACCURACY}, f, indent=1)
    for what, r in rec.items():
        assert r["E_hip"] <= 4 * r["E_f32_restatement"] + 1e-6, f"{name} {what}: {r}"
    # one-sided runs: the same bits, and no gradient for the other image
    ax, none = _grads(net, x, y, normalize, up, dev, want=(True, False))
    assert none is None and torch.equal(ax, dx)
    none, by = _grads(net, x, y, normalize, up, dev, want=(False, True))
    assert none is None and torch.equal(by, dy)


def test_chunks_of_one_pair_give_the_bits_of_one_pass(net, dev):
    g = torch.Generator().manual_seed(11)
    x, y = torch.rand(3, 3, 48, 40, generator=g), torch.rand(3, 3, 48, 40, generator=g)
    up = _weights(3)
    for normalize in (False, True):
        one = _grads(net, x, y, normalize, up, dev)
        for ppp in (1, 2):
            chunked = _grads(net, x, y, normalize, up, dev, pairs_per_pass=ppp)
            assert torch.equal(chunked[0], one[0]) and torch.equal(chunked[1], one[1])
        # the pairs one at a time, as separate calls
        for n in range(3):
            single = _grads(net, x[n:n + 1], y[n:n + 1], normalize, up[n:n + 1], dev)
            assert torch.equal(single[0][0], one[0][n]) and torch.equal(single[1][0], one[1][n])
    # the default comes from max_workspace_bytes: a bound below one pair's workspace still runs one pair per pass
    small = _grads(net, x, y, True, up, dev, max_workspace_bytes=1)
    assert torch.equal(small[0], one[0]) and torch.equal(small[1], one[1])


def test_layouts_and_determinism(net, dev):
    g = torch.Generator().manual_seed(5)
    N, H, W = 2, 24, 19
    xh, yh = torch.rand(N, H, W, 3, generator=g).to(dev), torch.rand(N, H, W, 3, generator=g).to(dev)
    up = _weights(N).to(dev)

    def run(a, b, channel_axis):
        a, b = a.requires_grad_(), b.requires_grad_()
        (LPIPSLoss(net, channel_axis=channel_axis, reduction="none")(a, b) * up).sum().backward()
        return a.grad, b.grad

    ga, gb = run(xh.clone(), yh.clone(), -1)
    assert ga.shape == (N, H, W, 3)
    again = run(xh.clone(), yh.clone(), -1)
    assert torch.equal(again[0], ga) and torch.equal(again[1], gb)
    # the NCHW copies
    ca, cb = run(xh.permute(0, 3, 1, 2).contiguous(), yh.permute(0, 3, 1, 2).contiguous(), 1)
    assert ca.shape == (N, 3, H, W)
    assert torch.equal(ca.permute(0, 2, 3, 1), ga) and torch.equal(cb.permute(0, 2, 3, 1), gb)
    # sliced views of larger leaves: the gradient lands in the view's elements, zero elsewhere
    big_x = torch.zeros(2 * N, H, W + 1, 4, device=dev)
    big_y = torch.zeros(2 * N, H, W + 1, 4, device=dev)
    big_x[::2, :, 1:, 1:] = xh
    big_y[::2, :, 1:, 1:] = yh
    big_x.requires_grad_()
    big_y.requires_grad_()
    (LPIPSLoss(net, reduction="none")(big_x[::2, :, 1:, 1:], big_y[::2, :, 1:, 1:]) * up).sum().backward()
    assert torch.equal(big_x.grad[::2, :, 1:, 1:], ga) and torch.equal(big_y.grad[::2, :, 1:, 1:], gb)
    rest = big_x.grad.clone()
    rest[::2, :, 1:, 1:] = 0
    assert float(rest.abs().max()) == 0.0


def test_ops_check_their_arguments(net, dev):
    x = torch.rand(1, 3, 16, 16, device=dev)
    with pytest.raises(ValueError):
        ops.lpips_vgg_fwd_save(net.packed(), x, x, True, want_dx=False, want_dy=False)
    with pytest.raises(TypeError):
        ops.lpips_vgg_fwd_save(net.packed(), x.double(), x.double(), True)
    _, _, ws = ops.lpips_vgg_fwd_save(net.packed(), x, x, True, want_dy=False)
    with pytest.raises(ValueError):  # a workspace of another selection
        ops.lpips_vgg_bwd(net.packed(), net.packed_grad(), ws, x.shape, True, torch.ones(1, device=dev))
    p = net.net.convs()[0].weight  # the weights are frozen: one that asks for a gradient is refused
    p.requires_grad_(True)
    try:
        with pytest.raises(RuntimeError):
            net(x.clone().requires_grad_(), x)
        with pytest.raises(RuntimeError):
            LPIPSLoss(net, channel_axis=1)(x.clone().requires_grad_(), x)
    finally:
        p.requires_grad_(False)


# ---------------------------------------------------------------- end to end
def test_lpips_loss_backward_through_render_rays_is_the_explicit_gradient(net, dev):
    from fs_nerf_amd.core.models import NeRF
    from fs_nerf_amd.nerfdata import PatchLoader, RayDataset
    from fs_nerf_amd.render import rendering as Rm
    P, B, hw = 16, 2, 20
    torch.manual_seed(42)
    m = NeRF(3, 3, 4, 128, (), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
    with torch.no_grad():
        m.sigma.weight.mul_(64.0)
        m.sigma.bias.add_(3.0)
    m = m.to(dev).train()
    est = Rm.StratifiedEstimator(2.0, 6.0, 8, 0).train()
    imgs = np.random.default_rng(0).integers(0, 256, size=(2, hw, hw, 3), dtype=np.uint8)
    poses = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    poses[:, 2, 3] = (4.0, 4.2)
    ds = RayDataset(imgs, poses, (hw, hw, 1.2 * hw), near=2.0, far=6.0, device=dev)
    rays_o, rays_d, gt = next(iter(PatchLoader(ds, P, B, seed=4)))
    u = torch.rand(B * P * P, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    target = gt.view(B, P, P, 3)

    def render():
        for p in m.parameters():
            p.grad = None
        (rgb, _, _, _), _, _ = Rm.render_rays(rays_o, rays_d, est, m, train=True, white_bkgd=True, device=dev, u=u)
        assert rgb.shape == (B * P * P, 3) and rgb.requires_grad
        return rgb

    rgb = render()
    loss = LPIPSLoss(net)(rgb.view(B, P, P, 3), target)
    assert 0.0 < loss.item() < 10.0
    loss.backward()
    through_loss = [p.grad.clone() for p in m.parameters()]
    assert all(g is not None for g in through_loss) and any(float(g.abs().max()) > 0 for g in through_loss)

    again = render()
    assert torch.equal(again, rgb)
    xn = again.detach().view(B, P, P, 3).permute(0, 3, 1, 2)
    _, _, ws = ops.lpips_vgg_fwd_save(net.packed(), xn, target.permute(0, 3, 1, 2), True, want_dy=False)
    up = torch.full((B,), 1.0 / B, dtype=torch.float32, device=dev)  # d mean_n lpips_n / d lpips_n, as torch's mean
    G, none = ops.lpips_vgg_bwd(net.packed(), net.packed_grad(), ws, xn.shape, True, up, want_dy=False)
    assert none is None
    again.backward(gradient=G.permute(0, 2, 3, 1).reshape(B * P * P, 3))
    for g0, p in zip(through_loss, m.parameters()):
        assert torch.equal(g0, p.grad)


# ---------------------------------------------------------------- debug build
def test_new_kernels_keep_inside_their_lds_arrays():
    """The debug library (every LDS index of k_lpips_conv and k_lpips_first_bwd range-checked) in a child process:
    forward-save and backward at 37 x 53 leave the record empty."""
    rep = debug_lib.run_worker("lpips_grad_debug_worker.py")
    assert rep["lpips"] == [0, 0, 0, 0], f"an LPIPS kernel indexed outside an LDS array: {rep['lpips']} (count, line, index, extent)"
    debug_lib.assert_no_other_unit_recorded(rep)
