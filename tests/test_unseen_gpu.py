"""-m gpu: fsn_unseen_poses / fsn_unseen_patch_batch against the float32 NumPy restatement of tests/unseen_ref.py, bit for
bit (a: poses, anchors and rays, both modes, world and NDC rays); against fsn_ray_patch_batch over the reported poses
and anchors (b) and fsn_unseen_poses over the same draws (c); UnseenPatchLoader's reproducibility, resume and rank
slices (d); and one served batch through render_rays(full_grad=True) and PatchDepthSmoothnessLoss (e).

Shapes: 12 x 20 intrinsics (H != W); (B, P, dilation, patches_per_pose) = (3, 5, 1, 1): 75 rows, less than a block;
(12, 5, 2, 4): 300 rows, more than one 256-thread block, four patches per pose; (4, 1, 1, 2): single-pixel patches;
(2, 4, 4, 1) on 13 x 13: ext == H == W, a single anchor."""
import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import ops
from fs_nerf_amd.nerfdata import UnseenPatchLoader, UnseenViewSampler

import unseen_ref as UR

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB  # a 64-bit seed: the key's high bits count
GEOMETRIES = [((12, 20, 11.0), 3, 5, 1, 1), ((12, 20, 11.0), 12, 5, 2, 4), ((12, 20, 11.0), 4, 1, 1, 2),
              ((13, 13, 9.5), 2, 4, 4, 1)]
FIRST = 8  # a multiple of every patches_per_pose above: the launch starts at a pose's first patch


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def sampler(name, dev):
    if name == "shell":      # an orbit around the focus with a tilted up axis, cameras from below to well above it
        return UnseenViewSampler("shell", focus=(0.3, -0.2, 0.5), up=(0.2, -0.1, 1.0), jitter=0.25, r=(3.5, 4.5),
                                 z=(-0.3, 0.85), device=dev)
    if name == "shell-down":  # cameras above the focus looking down: every ray has d_z < 0, as the NDC map needs
        return UnseenViewSampler("shell", focus=(0.3, -0.2, -4.0), up=(0.05, -0.02, 1.0), jitter=0.2, r=(3.5, 4.5),
                                 z=(0.9, 0.97), device=dev)
    return UnseenViewSampler("box", focus=(0.1, 0.2, -5.0), up=(0.05, 1.0, 0.02), jitter=0.3, lo=(-0.6, -0.4, -0.1),
                             hi=(0.7, 0.3, 0.2), device=dev)


CASES = [("shell", False), ("shell-down", True), ("box", False), ("box", True)]


def same(got, want):
    got = got.cpu()
    want = torch.from_numpy(np.ascontiguousarray(want))
    return got.dtype == want.dtype and got.shape == want.shape and bool(torch.isfinite(got.double()).all()) \
        and torch.equal(got, want)


@pytest.mark.parametrize("hwf,B,P,dil,per_pose", GEOMETRIES)
@pytest.mark.parametrize("name,ndc", CASES)
def test_patch_batch_is_the_restatement_and_the_explicit_patch_route(dev, name, ndc, hwf, B, P, dil, per_pose):
    s = sampler(name, dev)
    H, W, focal = hwf
    o, d, poses, anchors = ops.unseen_patch_batch(s.dist, H, W, focal, P, dil, device=dev, first_patch=FIRST, count=B,
                                                  patches_per_pose=per_pose, seed=SEED, ndc=ndc, near=1.0, want_poses=True,
                                                  want_anchors=True)
    # (a) bit for bit the NumPy restatement
    wo, wd, wposes, wanchors = UR.patch_batch(UR.dist_of(s.dist), SEED, FIRST, B, per_pose, H, W, focal, P, dil, ndc)
    assert same(poses, wposes) and same(anchors, wanchors)
    assert same(o, wo) and same(d, wd)
    assert o.shape == (B * P * P, 3)
    ext = (P - 1) * dil + 1
    AH, AW = H - ext + 1, W - ext + 1
    assert int(anchors.min()) >= 0 and int(anchors.max()) < AH * AW
    # (b) the same pinhole_ray: fsn_ray_patch_batch over the reported poses, the reported anchors as the explicit list
    explicit = torch.arange(B, device=dev) * (AH * AW) + anchors
    po, pd, _, _ = ops.ray_patch_batch(poses, None, H, W, focal, P, dil, ndc=ndc, near=1.0, order="explicit",
                                       anchors=explicit, want_rgb=False)
    assert torch.equal(o, po) and torch.equal(d, pd)
    # (c) fsn_unseen_poses over the draws the patches map to
    g0, n = FIRST // per_pose, B // per_pose
    assert torch.equal(ops.unseen_poses(s.dist, n, dev, seed=SEED, first=g0), poses[::per_pose])
    assert all(torch.equal(poses[k::per_pose], poses[::per_pose]) for k in range(per_pose))
    # outputs not asked for are not made, and the others do not change
    o2, d2, p2, a2 = ops.unseen_patch_batch(s.dist, H, W, focal, P, dil, device=dev, first_patch=FIRST, count=B,
                                            patches_per_pose=per_pose, seed=SEED, ndc=ndc)
    assert p2 is None and a2 is None and torch.equal(o2, o) and torch.equal(d2, d)


@pytest.mark.parametrize("name", ["shell", "box"])
def test_poses_are_the_restatement(dev, name):
    s = sampler(name, dev)
    first, count = 1000, 300  # more than one block
    got = s.poses12(count, seed=SEED, first=first)
    assert same(got, UR.poses(UR.dist_of(s.dist), SEED, np.arange(first, first + count)))
    full = s.poses(count, seed=SEED, first=first)
    assert full.shape == (count, 4, 4) and torch.equal(full[:, :3].reshape(count, 12), got)
    assert torch.equal(full[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev).expand(count, 4))
    assert torch.equal(s.poses12(5, seed=SEED, first=first + 7), got[7:12])   # any draw on its own
    assert not torch.equal(s.poses12(5, seed=SEED + 1, first=first), got[:5])
    assert s.poses12(0, seed=SEED).shape == (0, 12)


def test_loader_is_reproducible_resumable_and_rank_sliced(dev):
    s = sampler("shell", dev)
    hwf, P, dil, B, per_pose = (12, 20, 11.0), 5, 2, 4, 2
    mk = lambda **kw: UnseenPatchLoader(s, hwf, P, B, dilation=dil, patches_per_pose=per_pose, seed=SEED, **kw)
    a, b = mk(with_poses=True), mk(with_poses=True)
    batches = [next(a) for _ in range(5)]
    assert all(all(torch.equal(x, y) for x, y in zip(batch, next(b))) for batch in batches)
    assert all(o.shape == d.shape == (B * P * P, 3) and p.shape == (B, 12) for o, d, p in batches)
    assert not torch.equal(batches[0][1], batches[1][1])  # fresh poses every step
    # resumed at step 3: step 3's batch
    c = mk(with_poses=True)
    for _ in range(3):
        next(c)
    state = c.state_dict()
    r = UnseenPatchLoader(s, hwf, P, B, dilation=dil, patches_per_pose=per_pose, seed=1, with_poses=True)
    r.load_state_dict(state)
    assert all(torch.equal(x, y) for x, y in zip(next(r), batches[3]))
    assert all(torch.equal(x, y) for x, y in zip(next(r), batches[4]))
    # ranks 0..2 of world = 3 together serve the rows of the world = 1 loader over the same global patches
    world = 3
    whole = UnseenPatchLoader(s, hwf, P, B * world, dilation=dil, patches_per_pose=per_pose, seed=SEED, with_poses=True)
    ranks = [mk(rank=k, world=world, with_poses=True) for k in range(world)]
    for _ in range(2):
        o, d, p = next(whole)
        parts = [next(x) for x in ranks]
        assert torch.equal(torch.cat([x[0] for x in parts]), o) and torch.equal(torch.cat([x[1] for x in parts]), d)
        assert torch.equal(torch.cat([x[2] for x in parts]), p)
    assert len(next(mk())) == 2


def test_a_served_batch_trains_through_the_depth_smoothness_loss(dev):
    """The path the loader exists for: 2 patches of 4 x 4 rays of unseen poses -> render_rays(full_grad=True) through a
    2 x 128 network -> PatchDepthSmoothnessLoss -> backward: finite gradients on every parameter, not all zero."""
    from fs_nerf_amd.core.loss import PatchDepthSmoothnessLoss
    from fs_nerf_amd.core.models import NeRF
    from fs_nerf_amd.render import rendering as Rm
    from oracle import fsnerf_oracle as O
    sd = O.init_nerf_state_dict(2, 128, [], 10, 4, seed=6)
    sd["sigma.weight"] *= 16.0
    sd["sigma.bias"] += 1.0
    m = NeRF(3, 3, 2, 128, (), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
    m.load_state_dict(sd)
    m = m.to(dev).train()
    poses = torch.stack([O.pose_from_spherical(4.0, 50.0, phi) for phi in (0.0, 120.0, 240.0)])
    s = UnseenViewSampler.from_poses(poses, "shell", device=dev)
    o, d = next(UnseenPatchLoader(s, (16, 16, 20.0), 4, 2, dilation=2, seed=3))
    est = Rm.StratifiedEstimator(2.0, 6.0, 16, 8).train()
    gen = torch.Generator().manual_seed(1)
    (rgb, opacity, depth, _), _, _ = Rm.render_rays(o, d, est, m, train=True, white_bkgd=True, device=dev, full_grad=True,
                                                    u=torch.rand(32, generator=gen).to(dev),
                                                    u_fine=torch.rand(32, 8, generator=gen).to(dev))
    assert depth.requires_grad and depth.numel() == 32
    loss = PatchDepthSmoothnessLoss()(depth.view(2, 4, 4))
    loss.backward()
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert any(float(p.grad.abs().max()) > 0 for p in m.parameters())
