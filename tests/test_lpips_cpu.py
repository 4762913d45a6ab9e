"""LPIPS-VGG without a GPU: the module's state-dict layout and loading rules (fs_nerf_amd.core.metrics.LPIPS), the
closed forms of the torch restatement (tests/lpips_ref.py), and the argument checks of the new C entry points."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_ref as LR  # noqa: E402

import fs_nerf_amd  # noqa: E402,F401
from fs_nerf_amd import _lib as L  # noqa: E402
from fs_nerf_amd.core import metrics  # noqa: E402

# the `lpips` package's LPIPS(net="vgg") state dict (its `lins.K` aliases aside), written out
PACKAGE_LAYOUT = {
    "scaling_layer.shift": (1, 3, 1, 1), "scaling_layer.scale": (1, 3, 1, 1),
    "net.slice1.0.weight": (64, 3, 3, 3), "net.slice1.0.bias": (64,),
    "net.slice1.2.weight": (64, 64, 3, 3), "net.slice1.2.bias": (64,),
    "net.slice2.5.weight": (128, 64, 3, 3), "net.slice2.5.bias": (128,),
    "net.slice2.7.weight": (128, 128, 3, 3), "net.slice2.7.bias": (128,),
    "net.slice3.10.weight": (256, 128, 3, 3), "net.slice3.10.bias": (256,),
    "net.slice3.12.weight": (256, 256, 3, 3), "net.slice3.12.bias": (256,),
    "net.slice3.14.weight": (256, 256, 3, 3), "net.slice3.14.bias": (256,),
    "net.slice4.17.weight": (512, 256, 3, 3), "net.slice4.17.bias": (512,),
    "net.slice4.19.weight": (512, 512, 3, 3), "net.slice4.19.bias": (512,),
    "net.slice4.21.weight": (512, 512, 3, 3), "net.slice4.21.bias": (512,),
    "net.slice5.24.weight": (512, 512, 3, 3), "net.slice5.24.bias": (512,),
    "net.slice5.26.weight": (512, 512, 3, 3), "net.slice5.26.bias": (512,),
    "net.slice5.28.weight": (512, 512, 3, 3), "net.slice5.28.bias": (512,),
    "lin0.model.1.weight": (1, 64, 1, 1), "lin1.model.1.weight": (1, 128, 1, 1), "lin2.model.1.weight": (1, 256, 1, 1),
    "lin3.model.1.weight": (1, 512, 1, 1), "lin4.model.1.weight": (1, 512, 1, 1),
}


@pytest.fixture(scope="module")
def sd():
    return LR.random_state_dict(seed=5)


# ---------------------------------------------------------------- the module
def test_state_dict_is_the_package_layout():
    m = metrics.LPIPS(net="vgg")
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == PACKAGE_LAYOUT
    assert LR.state_dict_shapes() == PACKAGE_LAYOUT
    assert not any(p.requires_grad for p in m.parameters())


def test_load_state_dict_round_trips(sd):
    m = metrics.LPIPS()
    m.load_state_dict(sd)
    out = m.state_dict()
    assert set(out) == set(sd)
    for k in sd:
        assert torch.equal(out[k], sd[k]), k
    m2 = metrics.LPIPS()
    m2.load_state_dict(out)
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), out.values()))


def test_missing_keys_raise_and_are_named(sd):
    bad = dict(sd)
    del bad["net.slice3.12.weight"]
    del bad["lin2.model.1.weight"]
    with pytest.raises(RuntimeError, match=r"net\.slice3\.12\.weight") as e:
        metrics.LPIPS().load_state_dict(bad)
    assert "lin2.model.1.weight" in str(e.value)
    m = metrics.LPIPS()
    m.load_state_dict(bad, strict=False)
    with pytest.raises(RuntimeError, match="no weights"):
        m(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16))


def test_package_aliases_and_default_scaling_load(sd):
    pkg = {k: v for k, v in sd.items() if not k.startswith("scaling_layer.")}
    for k in range(5):
        pkg[f"lins.{k}.model.1.weight"] = pkg[f"lin{k}.model.1.weight"]
    m = metrics.LPIPS()
    m.load_state_dict(pkg)
    assert torch.equal(m.lin3.model[1].weight, sd["lin3.model.1.weight"])
    assert torch.equal(m.scaling_layer.shift.reshape(-1), torch.tensor(LR.SHIFT))
    assert torch.equal(m.scaling_layer.scale.reshape(-1), torch.tensor(LR.SCALE))
    only_alias = {k: v for k, v in pkg.items() if not k.startswith("lin0.")}
    m2 = metrics.LPIPS()
    m2.load_state_dict(only_alias)
    assert torch.equal(m2.lin0.model[1].weight, sd["lin0.model.1.weight"])


def test_other_backbones_raise():
    for net in ("alex", "squeeze"):
        with pytest.raises(NotImplementedError):
            metrics.LPIPS(net=net)


def test_calls_without_weights_or_on_cpu_raise(sd):
    x = torch.rand(2, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no weights"):
        metrics.LPIPS()(x, x)
    m = metrics.LPIPS()
    m.load_state_dict(sd)
    m.eval()
    m.train()
    with pytest.raises(RuntimeError, match="GPU"):
        m(x, x)
    with pytest.raises(ValueError):
        m(x, x[:1])
    with pytest.raises(ValueError):
        m(x[:, :, :15], x[:, :, :15])
    with pytest.raises(ValueError):
        m(x[:, :2], x[:, :2])
    with pytest.raises(ValueError):
        m(x[0], x[0])


# ---------------------------------------------------------------- closed forms of the restatement
def _pair(N=2, H=20, W=27, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, 3, H, W, generator=g) * 2 - 1, torch.rand(N, 3, H, W, generator=g) * 2 - 1


def test_identical_images_give_zero(sd):
    x, _ = _pair()
    v, per = LR.lpips(sd, x, x)
    assert torch.equal(v, torch.zeros(2, dtype=torch.float64)) and torch.equal(per, torch.zeros(5, 2, dtype=torch.float64))


def test_zero_lin_weights_give_zero(sd):
    z = dict(sd)
    for k in range(5):
        z[f"lin{k}.model.1.weight"] = torch.zeros_like(sd[f"lin{k}.model.1.weight"])
    x, y = _pair()
    v, _ = LR.lpips(z, x, y)
    assert torch.equal(v, torch.zeros(2, dtype=torch.float64))


def test_per_layer_values_sum_to_the_total(sd):
    x, y = _pair(H=37, W=53)
    v, per = LR.lpips(sd, x, y)
    assert per.shape == (5, 2) and bool((per > 0).all())
    assert torch.allclose(per.sum(0), v, rtol=1e-15, atol=0)
    v32, per32 = LR.lpips(sd, x, y, dtype=torch.float32)
    assert v32.dtype == torch.float32 and torch.allclose(v32.double(), v, rtol=1e-4)


def test_normalize_is_two_x_minus_one(sd):
    x, y = _pair()
    x01, y01 = (x + 1) / 2, (y + 1) / 2
    a, _ = LR.lpips(sd, x01, y01, normalize=True)
    b, _ = LR.lpips(sd, 2 * x01 - 1, 2 * y01 - 1, normalize=False)
    assert torch.equal(a, b)


# ---------------------------------------------------------------- C entry points, no device needed
def test_lpips_entry_points_validate_without_gpu():
    lib = L.lib()
    fake = C.c_void_p(256)  # never dereferenced: every check below fails before a launch
    st = (C.c_int64 * 4)(3 * 64 * 64, 64 * 64, 64, 1)
    assert lib.fsn_lpips_pack_bytes() > 4 * 14_000_000
    ws = [lib.fsn_lpips_workspace_floats(h, w) for h, w in ((16, 16), (64, 64), (800, 800))]
    assert 0 < ws[0] < ws[1] < ws[2]
    assert ws[2] >= 2 * 2 * 64 * 800 * 800  # two ping-pong buffers of both images at 64 channels
    assert lib.fsn_lpips_workspace_floats(15, 64) < 0 and lib.fsn_lpips_workspace_floats(64, 15) < 0
    assert b"16" in lib.fsn_last_error()
    # N = 0: a no-op, no pointer needed
    assert lib.fsn_lpips_vgg(None, None, None, 0, 64, 64, None, None, 0, None, None, None, None) == 0
    # too small, null pointers
    assert lib.fsn_lpips_vgg(fake, fake, fake, 1, 15, 64, st, st, 0, fake, None, fake, None) == -1
    assert lib.fsn_lpips_vgg(None, fake, fake, 1, 64, 64, st, st, 0, fake, None, fake, None) == -1
    assert b"null" in lib.fsn_last_error()
    assert lib.fsn_lpips_vgg(fake, fake, fake, 1, 64, 64, st, st, 0, fake, None, None, None) == -1
    assert lib.fsn_lpips_vgg(fake, fake, fake, 1, 64, 64, None, st, 0, fake, None, fake, None) == -1
    assert lib.fsn_lpips_vgg(fake, fake, fake, -1, 64, 64, st, st, 0, fake, None, fake, None) == -1
    ptrs = (C.c_void_p * 13)()
    assert lib.fsn_lpips_pack(ptrs, ptrs, ptrs, fake, fake, fake, None) == -1
    assert lib.fsn_lpips_pack(None, None, None, None, None, None, None) == -1
    buf = (C.c_uint32 * 4)()
    assert lib.fsn_debug_report(b"lpips", buf) == -2
