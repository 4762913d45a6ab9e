"""Encoding reuse in the fused render (csrc/render.hip, x3 / x2 modes): the direction fragments are encoded once per ray
into an LDS table, and the position fragments of layer 0 are parked in LDS for the skip layers.  Both are the same
function of the same inputs, evaluated less often, so nothing may move by a bit.

Yardstick: k_mlp_fwd (ops.mlp_fwd_rays), which encodes per sample and per use.  ops.render_fused(want_extras=True)
returns the per-sample sigmas, rgbs and the interval edges of the fine pass; the standalone forward of the fine
network on those same edges must return the same sigmas and rgbs, torch.equal ("same blob, same unit order, same
arithmetic per sample").  On top of that the four launch shapes (group by group / two phases with the hand-over
buffer, rays from tensors / from the camera) must agree with one another in every output.

Shapes: the smallest at which the table or the stash can go wrong - a fine tile that spans rays with different
directions, a last group that is partly empty, ragged tiles that end in padding, networks with no reachable skip
(the stash is never written), with one and with two skips (read once / twice), the 3-phase stream, masks with zeros
and non-unit entries, both x3 arithmetics and the two-pass fp16x2 (prec_is_x3 holds for it: the same table and stash
path, its own kernel instantiations and k-loop texts), more ray groups than workgroups (a workgroup refills the table).
"""
import functools

import pytest
import torch

from oracle import fsnerf_oracle as O

pytestmark = pytest.mark.gpu

#        layers, width, skip, position bands, direction bands
NETS = {"8x256": (8, 256, (4,), 10, 4),
        "4x128": (4, 128, (4,), 10, 4),       # the skip index is never reached: no wide layer
        "8x128-two-skips": (8, 128, (2, 5), 10, 4),
        "2x128": (2, 128, (), 10, 4)}         # the shortest stream
NEAR, FAR = 2.0, 6.0
FOCAL = 3.0  # a very wide pinhole: neighbouring pixels look in clearly different directions


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def state(net, seed):
    L, D, skip, nf, nfd = NETS[net]
    sd = O.init_nerf_state_dict(L, D, list(skip), nf, nfd, seed=seed)
    sd["sigma.weight"] = sd["sigma.weight"] * 64.0  # a medium the rays hit: the resampled edges bunch up
    sd["sigma.bias"] = sd["sigma.bias"] + 3.0
    return sd


@pytest.fixture(scope="module")
def models(dev):
    """(network, precision) -> (coarse, fine) packed once per module."""
    from fs_nerf_amd.core.models import NeRF
    cache = {}

    def get(net, prec):
        if (net, prec) not in cache:
            L, D, skip, nf, nfd = NETS[net]
            pair = []
            for seed in (42, 43):
                m = NeRF(3, 3, L, D, skip, precision=prec, pos_fn={"n_freqs": nf, "log_space": True},
                         dir_fn={"n_freqs": nfd, "log_space": True})
                m.load_state_dict(state(net, seed))
                pair.append(m.to(dev).eval())
            cache[(net, prec)] = (pair[0], pair[1], pair[0].packed(), pair[1].packed())
        return cache[(net, prec)]

    yield get
    cache.clear()


def camera(H, W, phi, dev):
    return (O.pose_from_spherical(4.0311289, 50.0, phi), H, W, FOCAL, 0, H, dev)


def jitter(R, NI, dev, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(R, generator=gen).to(dev), torch.rand(R, NI, generator=gen).to(dev)


def flat(out):
    col, op, dep, ex = out
    return {"colors": col, "opacity": op, "depth": dep, **ex}


def render_four_ways(pc, pf, cam, S, NI, dev, pos_mask=None, dir_mask=None):
    """The launch from ray tensors and from the camera, group by group and in two phases (want_extras hands the launch
    its edges tensor as the hand-over buffer, whatever R is) -> the rays and the four results' tensors by name."""
    from fs_nerf_amd import ops
    pose, H, W, focal = cam[:4]
    o, d = ops.get_rays(pose, H, W, focal, dev)
    R = H * W
    u, uf = jitter(R, NI, dev)
    kw = dict(near=NEAR, far=FAR, n_samples=S, n_importance=NI, u=u, u_fine=uf, bkgd=(1.0, 1.0, 1.0), pos_mask=pos_mask,
              dir_mask=dir_mask, want_extras=True)
    outs = {}
    for two_phase in (False, True):
        outs[("rays", two_phase)] = flat(ops.render_fused(pc, pf, o, d, two_phase=two_phase, **kw))
        outs[("camera", two_phase)] = flat(ops.render_fused(pc, pf, None, None, camera=cam, two_phase=two_phase, **kw))
    return o, d, outs


def assert_matches_standalone_forward(pf, o, d, out, S, NI, pos_mask=None, dir_mask=None, what=""):
    """The launch's per-sample sigmas / rgbs == k_mlp_fwd of the fine network on the launch's own edges, bit for bit."""
    from fs_nerf_amd import ops
    R, So = o.shape[0], S + NI
    edges = out["edges"]
    assert edges.shape == (R, So + 1) and out["sigmas"].shape == (R, So) and out["rgbs"].shape == (R, So, 3)
    ri = torch.arange(R, device=o.device).repeat_interleave(So)
    y = ops.mlp_fwd_rays(pf, o, d, ri, edges[:, :-1].reshape(-1), edges[:, 1:].reshape(-1), True, pos_mask, dir_mask)
    sig, rgb = y[:, 3].reshape(R, So), y[:, :3].reshape(R, So, 3)
    n_sig, n_rgb = int((sig != out["sigmas"]).sum()), int((rgb != out["rgbs"]).sum())
    print(f"{what}: {R} rays x {So} samples; sigma differs in {n_sig} entries (max "
          f"{float((sig - out['sigmas']).abs().max()):.3e}), rgb in {n_rgb} (max {float((rgb - out['rgbs']).abs().max()):.3e})")
    assert bool(torch.isfinite(y).all()) and float(out["opacity"].max()) > 0.5, "finite outputs, and the rays hit a medium"
    assert torch.equal(sig, out["sigmas"]), f"{what}: {n_sig} sigmas differ from the standalone forward"
    assert torch.equal(rgb, out["rgbs"]), f"{what}: {n_rgb} rgb entries differ from the standalone forward"


def assert_all_equal(outs, what):
    base_key = ("rays", False)
    for key, out in outs.items():
        assert set(out) == set(outs[base_key])
        for name, t in out.items():
            assert torch.equal(t, outs[base_key][name]), f"{what}: {name} of {key} differs from {base_key}"


#        id: network, precision, S, NI, image (H, W), masks
CASES = {
    # a 128-sample fine tile spans two rays; groups of four rays and of one
    "rays5-8x256": ("8x256", "fp16x3", 64, 128, (1, 5), False),
    # a tile holds pieces of three rays and the last tile is mostly padding
    "ragged7-8x256": ("8x256", "fp16x3", 40, 24, (1, 7), False),
    "pixels2x3-8x256": ("8x256", "fp16x3", 64, 128, (2, 3), False),
    "ragged7-4x128": ("4x128", "fp16x3", 40, 24, (1, 7), False),
    "rays5-4x128": ("4x128", "fp16x3", 64, 128, (1, 5), False),
    "rays5-two-skips": ("8x128-two-skips", "fp16x3", 64, 128, (1, 5), False),
    "ragged7-two-skips": ("8x128-two-skips", "fp16x3", 40, 24, (1, 7), False),
    "rays5-2x128": ("2x128", "fp16x3", 64, 128, (1, 5), False),
    "ragged7-2x128": ("2x128", "fp16x3", 40, 24, (1, 7), False),
    "masks-8x256": ("8x256", "fp16x3", 64, 128, (1, 5), True),
    "masks-ragged-two-skips": ("8x128-two-skips", "fp16x3", 40, 24, (1, 7), True),
    "bf16x3-8x256": ("8x256", "bf16x3", 64, 128, (1, 5), False),
    "bf16x3-4x128": ("4x128", "bf16x3", 40, 24, (1, 7), False),
    "bf16x3-masks-two-skips": ("8x128-two-skips", "bf16x3", 64, 128, (2, 3), True),
    "fp16x2-8x256": ("8x256", "fp16x2", 64, 128, (1, 5), False),
    "fp16x2-ragged-4x128": ("4x128", "fp16x2", 40, 24, (1, 7), False),
    "fp16x2-masks-two-skips": ("8x128-two-skips", "fp16x2", 64, 128, (2, 3), True),
    # three groups, every ray its own direction
    "rays9-8x256": ("8x256", "fp16x3", 64, 128, (3, 3), False),
    # 259 groups of four rays: more than the part has compute units, so workgroups take a second group and refill
    "groups259-two-skips": ("8x128-two-skips", "fp16x3", 64, 128, (3, 345), False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_fused_samples_are_the_standalone_forward(dev, models, case):
    net, prec, S, NI, (H, W), masked = CASES[case]
    _, mf, pc, pf = models(net, prec)
    # (the C2 configuration's coarse mask: ones, a fraction, zeros)
    pm = O.freq_mask(3, 10, 0.45).to(dev) if masked else None
    dm = O.freq_mask(3, 4, 0.6).to(dev) if masked else None
    if masked:
        for mask in (pm, dm):
            assert 0.0 in mask.tolist() and any(0.0 < v < 1.0 for v in mask.tolist())
    o, d, outs = render_four_ways(pc, pf, camera(H, W, 123.0, dev), S, NI, dev, pm, dm)
    assert len({tuple(r) for r in d.tolist()}) == H * W, "every ray its own direction"
    assert_all_equal(outs, case)
    assert_matches_standalone_forward(pf, o, d, outs[("rays", False)], S, NI, pm, dm, what=case)
    assert mf.precision == prec, "the model stayed in its arithmetic"


def test_second_launch_with_other_directions(dev, models):
    """Same origins, other directions in the next launch: a table left over from the launch before is not used."""
    from fs_nerf_amd import ops
    _, _, pc, pf = models("8x256", "fp16x3")
    S, NI, R = 64, 128, 5
    o, d = ops.get_rays(O.pose_from_spherical(4.0311289, 50.0, 123.0), 1, R, FOCAL, dev)
    d2 = d.flip(0).contiguous() * torch.tensor([1.0, -1.0, 1.0], device=dev)
    assert not bool((d2 == d).all(dim=1).any())
    u, uf = jitter(R, NI, dev)
    kw = dict(near=NEAR, far=FAR, n_samples=S, n_importance=NI, u=u, u_fine=uf, bkgd=(1.0, 1.0, 1.0), want_extras=True)
    for two_phase in (False, True):
        first = flat(ops.render_fused(pc, pf, o, d, two_phase=two_phase, **kw))
        second = flat(ops.render_fused(pc, pf, o, d2, two_phase=two_phase, **kw))
        assert not torch.equal(first["rgbs"], second["rgbs"])
        assert_matches_standalone_forward(pf, o, d, first, S, NI, what=f"first launch, two_phase={two_phase}")
        assert_matches_standalone_forward(pf, o, d2, second, S, NI, what=f"second launch, two_phase={two_phase}")


@pytest.mark.parametrize("prec", ["fp16x3", "fp16x2"])
@pytest.mark.parametrize("net,S,NI", [("8x256", 64, 128), ("8x128-two-skips", 40, 24)])
def test_sampler_only_launch_returns_the_full_launch_edges(dev, models, net, S, NI, prec):
    """ops.sample_fused (two_phase == 2: coarse passes only, stash in use, table never filled) on 5 rays."""
    from fs_nerf_amd import ops
    _, _, pc, pf = models(net, prec)
    R = 5
    o, d = ops.get_rays(O.pose_from_spherical(4.0311289, 50.0, 123.0), 1, R, FOCAL, dev)
    u, uf = jitter(R, NI, dev)
    kw = dict(near=NEAR, far=FAR, n_samples=S, n_importance=NI, u=u, u_fine=uf)
    edges, wc = ops.sample_fused(pc, o, d, want_weights=True, **kw)
    full = flat(ops.render_fused(pc, pf, o, d, bkgd=(1.0, 1.0, 1.0), want_extras=True, **kw))
    assert torch.equal(edges, full["edges"]) and torch.equal(wc, full["weights_coarse"])
    assert float((edges[:, 1:] - edges[:, :-1]).min()) >= 0.0
