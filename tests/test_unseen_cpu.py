"""CPU: the unseen-view distribution without a device - properties of the NumPy restatement (tests/unseen_ref.py, which
tests/test_unseen_gpu.py holds the kernels to bit for bit), the host fit UnseenViewSampler.from_poses, UnseenPatchLoader's
bookkeeping with the launch replaced by a recorder, and argument validation of the two entry points and the classes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L
from fs_nerf_amd import ops
from fs_nerf_amd.nerfdata import UnseenPatchLoader, UnseenViewSampler

import unseen_ref as UR

N = 4096
EPS = float(np.finfo(np.float32).eps)


def shell_sampler(**kw):
    # heights up to 0.85: |up x zc| >= 0.5, so the look-at's cross product is far from its fallback and the frame's
    # error stays a few float32 roundings of unit-scale values (it grows as 1 / |up x zc|)
    args = dict(focus=(0.3, -0.2, 0.5), up=(0.2, -0.1, 1.0), jitter=0.25, r=(3.5, 4.5), z=(-0.3, 0.85), device="cpu")
    args.update(kw)
    return UnseenViewSampler("shell", **args)


def box_sampler(**kw):
    args = dict(focus=(0.1, 0.2, -5.0), up=(0.05, 1.0, 0.02), jitter=0.3, lo=(-0.6, -0.4, -0.1), hi=(0.7, 0.3, 0.2), device="cpu")
    args.update(kw)
    return UnseenViewSampler("box", **args)


def draws(sampler, seed=11, first=5):
    d = UR.dist_of(sampler.dist)
    m, info = UR.poses(d, seed, np.arange(first, first + N), details=True)
    return d, m.astype(np.float64).reshape(N, 3, 4), info


def test_random_numbers_are_a_pure_function_of_seed_draw_and_slot():
    b = UR.base(7, np.arange(N))
    u0, u1 = UR.u(b, 0), UR.u(b, 1)
    assert u0.dtype == np.float32 and u0.min() >= 0.0 and u0.max() < 1.0
    assert np.array_equal(u0, UR.u(UR.base(7, np.arange(N)), 0))          # no state
    assert not np.array_equal(u0, u1) and not np.array_equal(u0, UR.u(UR.base(8, np.arange(N)), 0))
    assert np.array_equal(UR.u(UR.base(7, [123]), 4), UR.u(UR.base(7, np.arange(200)), 4)[123:124])  # any draw on its own
    # 24 bits: every value is a multiple of 2^-24; the mean and variance of a uniform (4 sigma of N draws)
    assert np.all(u0.astype(np.float64) * 2 ** 24 % 1 == 0)
    assert abs(u0.mean() - 0.5) < 4 * math.sqrt(1 / 12 / N) and abs(u0.var() - 1 / 12) < 4 * math.sqrt(1 / 180 / N)
    # the 64-bit key: a seed's high bits count
    assert not np.array_equal(u0, UR.u(UR.base(7 + (1 << 40), np.arange(N)), 0))


def test_box_origins_lie_inside_the_box():
    d, m, _ = draws(box_sampler())
    origin = m[:, :, 3]
    assert np.all(origin >= d["lo"].astype(np.float64)) and np.all(origin <= d["hi"].astype(np.float64))
    # ... and fill it: every octant of the box is reached
    mid = 0.5 * (d["lo"] + d["hi"]).astype(np.float64)
    assert len({tuple(row) for row in (origin > mid).tolist()}) == 8
    # a box without extent along an axis is a plane of origins
    d2, m2, _ = draws(box_sampler(lo=(-0.6, -0.4, 0.2), hi=(0.7, 0.3, 0.2)))
    assert np.all(m2[:, 2, 3] == np.float64(d2["lo"][2]))


def test_shell_origins_keep_their_height_and_radius():
    d, m, info = draws(shell_sampler())
    assert np.all(info["z"] >= d["z_lo"]) and np.all(info["z"] <= d["z_hi"])
    assert np.all(info["r"] >= d["r_lo"]) and np.all(info["r"] <= d["r_hi"])
    # measured on the origins: the direction is a unit vector up to a handful of float32 roundings (c, s, h and the sum
    # of three products), the final sum centre + r * dir rounds once more at the scale of |centre| + r
    off = m[:, :, 3] - d["centre"].astype(np.float64)
    radius = np.linalg.norm(off, axis=1)
    tol = 8 * EPS * (float(np.abs(d["centre"]).max()) + float(d["r_hi"]))
    assert np.all(radius >= d["r_lo"] - tol) and np.all(radius <= d["r_hi"] + tol)
    height = off @ d["up"].astype(np.float64) / radius
    assert np.all(height >= d["z_lo"] - 8 * EPS) and np.all(height <= d["z_hi"] + 8 * EPS)
    # both ranges are used to their ends, the azimuth is uniform: every quadrant within 4 sigma of N / 4
    assert info["z"].min() < d["z_lo"] + 0.01 and info["z"].max() > d["z_hi"] - 0.01
    assert radius.min() < 3.51 and radius.max() > 4.49
    a, b = off @ d["e1"].astype(np.float64), off @ d["e2"].astype(np.float64)
    quadrants = np.bincount((a > 0) * 2 + (b > 0), minlength=4)
    assert np.all(np.abs(quadrants - N / 4) < 4 * math.sqrt(N * 3 / 16)), quadrants
    # the disc rejection: 4 / pi tries on average, capped at 16; no draw of these fell back to (1, 0)
    assert info["tries"].min() == 1 and info["tries"].max() <= UR.TRIES and not info["fallback"].any()
    assert abs(info["tries"].mean() - 4 / math.pi) < 4 * math.sqrt((1 - math.pi / 4) / (math.pi / 4) ** 2 / N)
    # a degenerate shell is a circle of origins
    _, m1, i1 = draws(shell_sampler(r=(4.0, 4.0), z=(0.5, 0.5)))
    assert np.all(i1["z"] == np.float32(0.5)) and np.all(i1["r"] == np.float32(4.0))


@pytest.mark.parametrize("make", [shell_sampler, box_sampler])
def test_poses_are_orthonormal_and_look_at_the_focus(make):
    d, m, info = draws(make())
    R = m[:, :, :3]
    # about a dozen float32 roundings of unit-scale values
    assert np.abs(np.einsum("nki,nkj->nij", R, R) - np.eye(3)).max() <= 1e-6
    assert np.all(np.linalg.det(R) > 0.999)  # right-handed: yc = zc x xc
    # y up: the camera's y axis has a positive component along `up`
    assert np.all(R[:, :, 1] @ d["up"].astype(np.float64) > 0)
    # the optical axis (origin, -zc) passes within jitter * sqrt(3) of the focus: it goes through the target, which lies
    # in the cube focus +- jitter (plus the rounding of the unit vector at the camera's distance)
    origin, axis = m[:, :, 3], -R[:, :, 2]
    to_focus = d["focus"].astype(np.float64) - origin
    along = np.einsum("nk,nk->n", to_focus, axis)
    miss = np.linalg.norm(to_focus - along[:, None] * axis, axis=1)
    assert np.all(along > 0)  # the focus is in front of the camera
    assert np.all(miss <= float(d["jitter"]) * math.sqrt(3) + 8 * EPS * np.linalg.norm(to_focus, axis=1))
    assert miss.max() > 0.5 * float(d["jitter"])  # the jitter is there
    assert np.abs(info["target"] - d["focus"]).max() <= d["jitter"] + 8 * EPS * (np.abs(d["focus"]).max() + d["jitter"])
    # without jitter every axis goes through the focus
    d0, m0, _ = draws(make(jitter=0.0))
    to0 = d0["focus"].astype(np.float64) - m0[:, :, 3]
    miss0 = np.linalg.norm(np.cross(to0, -m0[:, :, 2]), axis=1)
    assert np.all(miss0 <= 8 * EPS * np.linalg.norm(to0, axis=1))


def test_look_at_fallbacks_are_the_stated_rules():
    # a camera straight above the focus (box of one point on the up axis): up x zc = 0, e1 takes up's place
    s = box_sampler(focus=(0, 0, 0), up=(0, 0, 1), jitter=0.0, lo=(0, 0, 2), hi=(0, 0, 2))
    d = UR.dist_of(s.dist)
    m = UR.poses(d, 1, [0]).reshape(3, 4)
    assert np.array_equal(m[:, 2], [0, 0, 1]) and np.array_equal(m[:, 3], [0, 0, 2])
    x = np.cross(d["e1"], [0, 0, 1])
    assert np.array_equal(m[:, 0], (x / np.linalg.norm(x)).astype(np.float32)) and np.isfinite(m).all()
    # a camera on its target: zc = up
    s = box_sampler(focus=(1, 2, 3), up=(0, 1, 0), jitter=0.0, lo=(1, 2, 3), hi=(1, 2, 3))
    m = UR.poses(UR.dist_of(s.dist), 1, [0]).reshape(3, 4)
    assert np.array_equal(m[:, 2], [0, 1, 0]) and np.isfinite(m).all()
    assert abs(np.linalg.det(m[:, :3].astype(np.float64)) - 1) < 1e-6


def test_anchor_draw_covers_the_lattice_and_stays_inside():
    H, W, P, dil = 4, 6, 2, 1  # ext = 2: a 3 x 5 lattice
    row0, col0 = UR.anchors(3, np.arange(N), H, W, P, dil)
    assert row0.min() == 0 and row0.max() == 2 and col0.min() == 0 and col0.max() == 4
    counts = np.bincount(row0 * 5 + col0, minlength=15)
    assert counts.shape == (15,) and np.all(counts > 0)
    assert np.all(np.abs(counts - N / 15) < 4 * math.sqrt(N * 14 / 225)), counts
    # ext == H: a single anchor row; the anchor is keyed by the patch, the pose by patch // patches_per_pose
    r1, c1 = UR.anchors(3, np.arange(64), 13, 13, 4, 4)
    assert np.all(r1 == 0) and np.all(c1 == 0)
    d = UR.dist_of(shell_sampler().dist)
    o, dd, m, a = UR.patch_batch(d, 5, 8, 12, 4, 12, 20, 9.0, 5, 2, False)
    assert o.shape == dd.shape == (12 * 25, 3) and m.shape == (12, 12) and a.shape == (12,)
    assert np.array_equal(m[0], m[3]) and np.array_equal(m[4], m[7]) and not np.array_equal(m[3], m[4])
    assert np.array_equal(m[::4], UR.poses(d, 5, [2, 3, 4])) and len(set(a.tolist())) > 1
    assert a.min() >= 0 and a.max() < (12 - 9 + 1) * (20 - 9 + 1)
    assert np.array_equal(o.reshape(12, 25, 3)[:, 0], m.reshape(12, 3, 4)[:, :, 3])  # every row starts at its pose's origin


# ---------------------------------------------------------------- the host fit
def look_at(origin, target, up):
    zc = (origin - target) / np.linalg.norm(origin - target)
    xc = np.cross(up, zc)
    xc /= np.linalg.norm(xc)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = xc, np.cross(zc, xc), zc, origin
    return P


def test_from_poses_recovers_a_ring_of_cameras():
    centre, up = np.array([0.3, -0.2, 0.5]), np.array([0.2, -0.1, 1.0])
    up /= np.linalg.norm(up)
    e1 = np.cross(up, [1.0, 0.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(up, e1)
    radius, height = 4.0, 0.5  # height = sin(elevation)
    ring = [centre + radius * (math.sqrt(1 - height ** 2) * (math.cos(t) * e1 + math.sin(t) * e2) + height * up)
            for t in np.linspace(0, 2 * math.pi, 8, endpoint=False)]
    poses = np.stack([look_at(o, centre, up) for o in ring])
    s = UnseenViewSampler.from_poses(poses, "shell", margin=0.0, jitter=0.1, device="cpu")
    d = UR.dist_of(s.dist)
    assert np.allclose(d["focus"], centre, atol=1e-6) and np.allclose(d["centre"], centre, atol=1e-6)
    assert np.allclose(d["up"], up, atol=1e-6)
    assert np.allclose([d["r_lo"], d["r_hi"]], radius, rtol=1e-6) and np.allclose([d["z_lo"], d["z_hi"]], height, atol=1e-6)
    assert np.isclose(d["jitter"], 0.1 * radius, rtol=1e-6)
    frame = np.stack([d["e1"], d["e2"], d["up"]]).astype(np.float64)
    assert np.abs(frame @ frame.T - np.eye(3)).max() < 1e-6 and np.linalg.det(frame) > 0
    # the margin widens the ranges; the heights stay inside (-1, 1); torch poses [n,3,4] are taken too
    w = UR.dist_of(UnseenViewSampler.from_poses(torch.from_numpy(poses[:, :3]), "shell", margin=0.25, device="cpu").dist)
    assert np.isclose(w["r_lo"], 3.0) and np.isclose(w["r_hi"], 5.0) and np.isclose(w["z_lo"], 0.25) and np.isclose(w["z_hi"], 0.75)
    w = UR.dist_of(UnseenViewSampler.from_poses(poses, "shell", margin=0.9, device="cpu").dist)
    assert np.isclose(w["z_hi"], 0.999) and w["z_hi"] < 1.0 and np.isclose(w["z_lo"], -0.4)
    # the draws of the fitted distribution are cameras of that ring
    m = UR.poses(d, 0, np.arange(64)).astype(np.float64).reshape(-1, 3, 4)
    assert np.allclose(np.linalg.norm(m[:, :, 3] - centre, axis=1), radius, rtol=1e-5)


def test_from_poses_recovers_a_forward_facing_rig():
    target, up = np.array([0.0, 0.0, -5.0]), np.array([0.0, 1.0, 0.0])
    grid = [np.array([0.5 * i, 0.3 * j, 0.05 * i * j]) for i in (-1, 0, 1) for j in (-1, 0, 1)]
    poses = np.stack([look_at(o, target, up) for o in grid])
    d = UR.dist_of(UnseenViewSampler.from_poses(poses, "box", margin=0.0, device="cpu").dist)
    assert d["mode"] == UR.BOX
    assert np.allclose(d["lo"], [-0.5, -0.3, -0.05], atol=1e-6) and np.allclose(d["hi"], [0.5, 0.3, 0.05], atol=1e-6)
    assert np.allclose(d["focus"], target, atol=1e-5) and np.allclose(d["up"], up, atol=1e-2)
    w = UR.dist_of(UnseenViewSampler.from_poses(poses, "box", margin=0.1, device="cpu").dist)
    assert np.allclose(w["lo"], [-0.6, -0.36, -0.06], atol=1e-6) and np.allclose(w["hi"], [0.6, 0.36, 0.06], atol=1e-6)
    # parallel optical axes have no closest point: the caller names the focus
    parallel = np.stack([look_at(o, o + [0.0, 0.0, -1.0], up) for o in grid])
    with pytest.raises(ValueError, match="parallel"):
        UnseenViewSampler.from_poses(parallel, "box", device="cpu")
    f = UR.dist_of(UnseenViewSampler.from_poses(parallel, "box", focus=target, device="cpu").dist)
    assert np.allclose(f["focus"], target) and np.allclose(f["up"], up)
    with pytest.raises(ValueError):
        UnseenViewSampler.from_poses(poses[0], "box", device="cpu")  # not [n, 3|4, 4]


# ---------------------------------------------------------------- loader bookkeeping
@pytest.fixture
def launches(monkeypatch):
    """ops.unseen_patch_batch replaced by a recorder: every call is one launch; it returns (first_patch, count, the
    keywords, a pose tensor or None) in the four output slots."""
    calls = []

    def unseen_patch_batch(dist, H, W, focal, patch, dilation=1, **kw):
        assert isinstance(dist, L.UnseenDist)
        calls.append(dict(kw, hwf=(H, W, focal), patch=patch, dilation=dilation))
        return kw["first_patch"], kw["count"], (torch.zeros(kw["count"], 12) if kw["want_poses"] else None), None
    monkeypatch.setattr(ops, "unseen_patch_batch", unseen_patch_batch)
    return calls


def test_loader_rank_slices_and_resume(launches):
    B, world, steps = 8, 3, 5
    loaders = [UnseenPatchLoader(shell_sampler(), (12, 20, 9.0), 5, B, dilation=2, patches_per_pose=4, seed=3, rank=r,
                                 world=world) for r in range(world)]
    for s in range(steps):
        served = [next(ld) for ld in loaders]
        assert all(len(b) == 2 and b[1] == B for b in served)
        # three ranks cover [s * 3B, (s + 1) * 3B) disjointly
        assert sorted(p for b in served for p in range(b[0], b[0] + b[1])) == list(range(s * world * B, (s + 1) * world * B))
    assert len(launches) == world * steps  # one launch per next()
    assert all(c["seed"] == 3 and c["patches_per_pose"] == 4 and (c["patch"], c["dilation"]) == (5, 2)
               and c["hwf"] == (12, 20, 9.0) and not c["ndc"] and not c["want_poses"] for c in launches)
    # state_dict round-trips: another loader continues with the very same batches
    ld = loaders[1]
    state = ld.state_dict()
    assert state == {"seed": 3, "step": steps}
    other = UnseenPatchLoader(shell_sampler(), (12, 20, 9.0), 5, B, dilation=2, patches_per_pose=4, seed=99, rank=1, world=world)
    other.load_state_dict(state)
    assert [next(other)[0] for _ in range(3)] == [next(ld)[0] for _ in range(3)] == [((steps + k) * world + 1) * B for k in range(3)]
    assert other.state_dict() == {"seed": 3, "step": steps + 3}
    # an endless iterator: iter() is the loader itself and does not rewind; with_poses adds the third output
    wp = UnseenPatchLoader(box_sampler(), (12, 20, 9.0), 1, 4, ndc=True, seed=1, with_poses=True)
    assert iter(wp) is wp and [b[0] for _, b in zip(range(3), wp)] == [0, 4, 8]
    got = wp.next()
    assert len(got) == 3 and got[2].shape == (4, 12) and launches[-1]["ndc"] and launches[-1]["near"] == 1.0
    # seed=None: torch's initial seed, as the other loaders
    assert UnseenPatchLoader(box_sampler(), (12, 20, 9.0), 1, 4).seed == torch.initial_seed() & 0xFFFFFFFFFFFFFFFF


def test_value_errors():
    s = shell_sampler()
    for patch, dil in ((13, 1), (5, 3), (0, 1), (2, 0)):  # 5 pixels 3 apart span 13 > H = 12
        with pytest.raises(ValueError):
            UnseenPatchLoader(s, (12, 20, 9.0), patch, 4, dilation=dil)
    with pytest.raises(ValueError, match="multiple of patches_per_pose"):
        UnseenPatchLoader(s, (12, 20, 9.0), 2, 6, patches_per_pose=4)
    with pytest.raises(ValueError):
        UnseenPatchLoader(s, (12, 20, 9.0), 2, 4, patches_per_pose=0)
    with pytest.raises(ValueError):
        UnseenPatchLoader(s, (12, 20, 9.0), 2, 0)
    with pytest.raises(ValueError):
        UnseenPatchLoader(s, (12, 20, 9.0), 2, 4, rank=3, world=3)
    for z in ((-0.3, 1.0), (-0.3, 1.5), (-1.0, 0.5), (0.6, 0.5), (-0.3, 1.0 - 1e-9)):  # (1 - 1e-9 is 1 in float32)
        with pytest.raises(ValueError, match="height range"):
            shell_sampler(z=z)
    for r in ((-1.0, 2.0), (3.0, 2.0), (1.0, float("inf"))):
        with pytest.raises(ValueError, match="radius range"):
            shell_sampler(r=r)
    with pytest.raises(ValueError):
        box_sampler(lo=(0, 0, 0), hi=(1, -1, 1))
    with pytest.raises(ValueError):
        box_sampler(jitter=-0.1)
    with pytest.raises(ValueError):
        box_sampler(up=(0, 0, 0))
    with pytest.raises(ValueError):
        UnseenViewSampler("orbit", focus=(0, 0, 0), up=(0, 0, 1))
    with pytest.raises(ValueError):
        UnseenViewSampler("shell", focus=(0, 0, 0), up=(0, 0, 1))  # no ranges


def test_a_cpu_device_is_refused():
    s = shell_sampler()
    with pytest.raises(RuntimeError, match="GPU"):
        s.poses(4, seed=0)
    with pytest.raises(RuntimeError, match="GPU"):
        next(UnseenPatchLoader(s, (12, 20, 9.0), 2, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.unseen_poses(s.dist, 4, "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        ops.unseen_patch_batch(s.dist, 12, 20, 9.0, 2, device=torch.device("cpu"), count=4)


# ---------------------------------------------------------------- the two entry points
def test_entry_points_are_exported_and_validate_without_gpu():
    lib = L.lib()
    assert {"fsn_unseen_poses", "fsn_unseen_patch_batch"} <= set(L.SIGNATURES)
    assert L.FSN_UNSEEN_SHELL == 0 and L.FSN_UNSEEN_BOX == 1
    one = C.c_void_p(1)  # never dereferenced: every call below fails its checks before a launch
    good = shell_sampler().dist

    def changed(**kw):
        d = L.UnseenDist.from_buffer_copy(bytes(good))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def poses(d=good, first=0, count=4, out=one):
        return lib.fsn_unseen_poses(C.byref(d) if d is not None else None, 0, first, count, out, None)

    def patches(d=good, first=0, count=4, per_pose=1, H=12, W=20, focal=9.0, P=5, dil=2, o=one, dd=one, po=None, an=None):
        return lib.fsn_unseen_patch_batch(C.byref(d) if d is not None else None, 0, first, count, per_pose, H, W, focal, P, dil,
                                          0, 1.0, o, dd, po, an, None)
    for call, who in ((poses, b"fsn_unseen_poses"), (patches, b"fsn_unseen_patch_batch")):
        assert call(d=None) == -1 and who + b": null distribution" in lib.fsn_last_error()
        assert call(d=changed(mode=2)) == -1 and b"unknown mode" in lib.fsn_last_error()
        assert call(d=changed(z_hi=1.0)) == -1 and b"height range" in lib.fsn_last_error()
        assert call(d=changed(z_lo=-1.0)) == -1 and b"height range" in lib.fsn_last_error()
        assert call(d=changed(r_lo=5.0)) == -1 and b"radius range" in lib.fsn_last_error()
        assert call(d=changed(jitter=-1.0)) == -1 and b"jitter" in lib.fsn_last_error()
        assert call(d=changed(jitter=float("nan"))) == -1 and b"jitter" in lib.fsn_last_error()
        assert call(first=-1) == -1 and b"bad first" in lib.fsn_last_error()
        assert call(count=-1) == -1 and b"bad first" in lib.fsn_last_error()
        assert call(count=0) == 0  # an empty call is not an error
    box = box_sampler().dist
    bad_box = L.UnseenDist.from_buffer_copy(bytes(box))
    bad_box.lo[1] = 1.0
    assert poses(d=bad_box) == -1 and b"bad box" in lib.fsn_last_error()
    assert poses(d=box, count=0) == 0 and poses(d=changed(mode=1, z_hi=2.0), count=0) == 0  # a box reads no shell field
    assert poses(out=None) == -1 and b"null pointer" in lib.fsn_last_error()
    assert patches(P=0) == -1 and b"bad patch" in lib.fsn_last_error()
    assert patches(dil=0) == -1 and b"bad patch" in lib.fsn_last_error()
    assert patches(P=5, dil=3) == -1 and b"does not fit" in lib.fsn_last_error()   # ext = 13 > H
    assert patches(P=21, dil=1, H=30) == -1 and b"does not fit" in lib.fsn_last_error()  # ext = 21 > W
    assert patches(H=0) == -1 and b"geometry" in lib.fsn_last_error()
    assert patches(focal=0.0) == -1 and b"geometry" in lib.fsn_last_error()
    assert patches(per_pose=0) == -1 and b"patches_per_pose" in lib.fsn_last_error()
    assert patches(o=None, dd=None) == -1 and b"null pointer for every output" in lib.fsn_last_error()
    assert patches(count=(1 << 38) // 25 + 1) == -2 and b"2^38 rows" in lib.fsn_last_error()
