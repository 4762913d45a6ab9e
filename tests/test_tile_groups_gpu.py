"""Lane layout of the network tile (csrc/mlp_dev.hpp, tile_slot / mlp_tile): a sample's output does not depend on where
in a tile it sits, on which of a wave's sample groups evaluates it, or on what fills the tail of the last tile.

A workgroup tile is 128 NG samples; wave w evaluates the NG groups of 16 consecutive samples NG w + q.  NG = 2 in the
single-pass modes (bf16, fp16) of 256-wide networks, 1 otherwise - so an 8x256 and a 4x128 network in the four modes
cover both group counts in single-pass arithmetic and one group in the x3 modes.  Every comparison is bit equality: the
same sample goes through the same arithmetic whichever lanes hold it, and nothing here has a tolerance to choose."""
import os

import numpy as np
import pytest
import torch

from oracle import fsnerf_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = 300
# prefix lengths: one sample; the ends of group 0 (group 1 entirely past the end) and of group 1; the 128- and the
# 256-sample tile boundaries, one short, exact, one over
PREFIXES = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257)
SHIFTS = (1, 16, 128)  # 16 moves every sample into the other group of its wave
PRECISIONS = ("bf16", "fp16", "bf16x3", "fp16x3")
NETS = ("8x256", "4x128")
N_RAYS = 7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def inputs(dev):
    gen = torch.Generator().manual_seed(20)
    x = torch.rand(N, 3, generator=gen) * 3 - 1.5
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)
    ro = torch.rand(N_RAYS, 3, generator=gen) - 0.5
    rd = torch.nn.functional.normalize(torch.randn(N_RAYS, 3, generator=gen), dim=-1)
    ri = (torch.arange(N) * N_RAYS) // N  # 300 samples over 7 rays, packed ray by ray
    t0 = 0.5 + torch.rand(N, generator=gen) * 2.0
    t1 = t0 + 0.01 + torch.rand(N, generator=gen) * 0.05
    return {k: v.to(dev) for k, v in dict(x=x, d=d, ro=ro, rd=rd, ri=ri, t0=t0, t1=t1).items()}


def state_dict(net):
    if net == "8x256":
        g4 = np.load(os.path.join(GOLDEN, "g4_nerf_8x256.npz"))
        return 8, 256, (4,), {k[3:]: torch.from_numpy(g4[k]) for k in g4.files if k.startswith("sd.")}
    return 4, 128, (2,), O.init_nerf_state_dict(4, 128, [2], 10, 4, seed=7)


@pytest.fixture(scope="module")
def models(dev, inputs):
    """(network, precision) -> the model, its outputs on all 300 samples (point form and ray form, full and density
    only) and its range_events, computed once per module and released with it.  The first launch also calibrates the
    scaled fp16x3 network - on the whole input."""
    cache = {}

    def get(net, prec):
        if (net, prec) not in cache:
            from fs_nerf_amd.core.models import NeRF
            L, D, skip, sd = state_dict(net)
            m = NeRF(3, 3, L, D, skip, precision=prec, pos_fn={"n_freqs": 10, "log_space": True},
                     dir_fn={"n_freqs": 4, "log_space": True})
            m.load_state_dict(sd)
            m = m.to(dev).eval()
            i = inputs
            with torch.no_grad():
                ref = {("point", True): m(i["x"], i["d"]), ("point", False): m(i["x"]),
                       ("rays", True): m.forward_rays(i["ro"], i["rd"], i["ri"], i["t0"], i["t1"], True),
                       ("rays", False): m.forward_rays(i["ro"], i["rd"], i["ri"], i["t0"], i["t1"], False)}
            assert m.precision == prec, f"{net} {prec}: the model left its precision on the reference launch"
            for k, v in ref.items():
                assert v.shape == (N, 4 if k[1] else 1) and bool(torch.isfinite(v).all()), (net, prec, k)
            cache[(net, prec)] = (m, ref, m.range_events)
        return cache[(net, prec)]

    yield get
    cache.clear()


def point(m, i, full, sl):
    with torch.no_grad():
        return m(i["x"][sl], i["d"][sl]) if full else m(i["x"][sl])


def rays(m, i, full, sl):
    with torch.no_grad():
        return m.forward_rays(i["ro"], i["rd"], i["ri"][sl], i["t0"][sl], i["t1"][sl], full)


def first_difference(a, b):
    bad = (a != b).any(dim=-1).nonzero()
    return f"{int(bad.numel())} samples differ, first at {int(bad[0])}" if bad.numel() else "shapes differ"


@pytest.mark.parametrize("full", [True, False], ids=["full", "density"])
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("net", NETS)
def test_prefix_of_the_samples_gives_the_prefix_of_the_outputs(models, inputs, net, prec, full):
    m, ref, events = models(net, prec)
    for n in PREFIXES:
        y = point(m, inputs, full, slice(0, n))
        assert torch.equal(y, ref[("point", full)][:n]), f"{net} {prec} n={n}: {first_difference(y, ref[('point', full)][:n])}"
    assert m.range_events == events and m.precision == prec


@pytest.mark.parametrize("full", [True, False], ids=["full", "density"])
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("net", NETS)
def test_shifted_samples_give_the_shifted_outputs(models, inputs, net, prec, full):
    m, ref, events = models(net, prec)
    for k in SHIFTS:
        y = point(m, inputs, full, slice(k, N))
        assert torch.equal(y, ref[("point", full)][k:]), f"{net} {prec} k={k}: {first_difference(y, ref[('point', full)][k:])}"
    assert m.range_events == events and m.precision == prec


@pytest.mark.parametrize("full", [True, False], ids=["full", "density"])
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("net", NETS)
def test_ray_form_prefix_gives_the_prefix_of_the_outputs(models, inputs, net, prec, full):
    m, ref, events = models(net, prec)
    for n in PREFIXES:
        y = rays(m, inputs, full, slice(0, n))
        assert torch.equal(y, ref[("rays", full)][:n]), f"{net} {prec} n={n}: {first_difference(y, ref[('rays', full)][:n])}"
    assert m.range_events == events and m.precision == prec
