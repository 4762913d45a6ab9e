"""CPU: the visibility rule of OccGridEstimator.mark_invisible_cells (include/fsnerf_hip.h at fsn_occgrid_visibility) as
tests/occ_invisible_ref.py restates it.  The float64 form is conservative - no point on any pixel ray lies in a removed
cell - and the float32 form (the kernel's arithmetic, bit for bit: tests/test_occ_invisible_gpu.py) agrees with it
wherever float32 can decide."""
import math

import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401
from oracle import fsnerf_oracle as O

import occ_invisible_ref as VR

AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
AABB_NDC = [-1.2, -1.2, -1.0, 1.2, 1.2, 1.0]
HWF = (12, 12, 14.0)
RES, LEVELS = 16, 2


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """A `get_rays` pose [4,4]: x right, y up, looking down -z."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return torch.from_numpy(m).float()


def world_poses():
    """One camera outside the +-1.5 box looking in, one inside it, one looking past it (none on a lattice plane)."""
    return torch.stack([O.pose_from_spherical(4.0311289, 50.0, 33.0),
                        look_at((0.3137, -0.4211, 0.1719), (1.1, 0.9, -0.35)),
                        look_at((2.6173, 2.2391, 0.7713), (2.9, -3.1, 0.4))])


def ndc_poses():
    """The identity pose plus two tilted ones (forward-facing: they look down -z)."""
    def tilt(ax, ay, t):
        cx, sx, cy, sy = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay)
        rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = ry @ rx, t
        return torch.from_numpy(m).float()
    return torch.stack([torch.eye(4), tilt(0.11, -0.17, (0.23, -0.12, 0.05)), tilt(-0.08, 0.21, (-0.31, 0.17, -0.04))])


def ray_points(poses, hwf, ndc, per_ray, seed):
    """Random points on every pixel ray of every camera: world space (t up to 9 scene units), or the NDC space of to_ndc
    with near = 1 (t in [0, 1): z' runs from -1 to 1)."""
    gen = torch.Generator().manual_seed(seed)
    pts = []
    for p in poses:
        o, d = O.get_rays(p, hwf)
        o, d = o.reshape(-1, 3), d.reshape(-1, 3)
        if ndc:
            o, d = O.to_ndc(o, d, hwf, 1.0)
        t = torch.rand(o.shape[0], per_ray, generator=gen) * (1.0 if ndc else 9.0)
        pts.append((o[:, None, :] + d[:, None, :] * t[..., None]).reshape(-1, 3))
    pts = torch.cat(pts).numpy()
    return pts[pts[:, 2] < 1.0 - 1e-6] if ndc else pts


@pytest.mark.parametrize("ndc", [False, True])
def test_float64_rule_is_conservative(ndc):
    """near_plane 0, min_views 1: every ray point that falls in a grid cell falls in a visible one, at every level whose
    box holds it.  None may fail."""
    poses, aabb = (ndc_poses(), AABB_NDC) if ndc else (world_poses(), AABB)
    cams = VR.cams_from_views(poses, HWF)
    vis = VR.visibility(aabb, RES, LEVELS, cams, HWF[1], HWF[0], 0.0, 1, ndc=VR.ndc_args(HWF) if ndc else None, dtype=np.float64)
    pts = ray_points(poses, HWF, ndc, 40, 3)
    inside, value = VR.cell_is(vis, pts, aabb, RES, LEVELS)
    assert int(inside.sum()) > 10000, int(inside.sum())
    assert int((inside & ~value).sum()) == 0, f"{int((inside & ~value).sum())} of {int(inside.sum())} points lie in removed cells"
    # ... and the rule does remove cells, more of them when two views are asked for
    vis2 = VR.visibility(aabb, RES, LEVELS, cams, HWF[1], HWF[0], 0.0, 2, ndc=VR.ndc_args(HWF) if ndc else None, dtype=np.float64)
    assert 0.05 < vis[1].mean() < 0.95 and vis2.sum() < vis.sum() and not (vis2 & ~vis).any()


@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("near_plane,min_views", [(0.0, 1), (0.5, 2)])
def test_float32_restatement_agrees_with_float64(ndc, near_plane, min_views):
    """... except at cells where a float64 margin lies within 1e-5 * max(|its terms|) of zero: at most 1 % of the grid."""
    poses, aabb = (ndc_poses(), AABB_NDC) if ndc else (world_poses(), AABB)
    cams = VR.cams_from_views(poses, HWF)
    nd = VR.ndc_args(HWF) if ndc else None
    v64, unc = VR.visibility(aabb, RES, LEVELS, cams, HWF[1], HWF[0], near_plane, min_views, ndc=nd, dtype=np.float64, tol=1e-5)
    v32 = VR.visibility(aabb, RES, LEVELS, cams, HWF[1], HWF[0], near_plane, min_views, ndc=nd, dtype=np.float32)
    print(f"uncertain cells: {int(unc.sum())} of {unc.size}; float32 != float64 at {int((v32 != v64).sum())}")
    assert unc.mean() <= 0.01, unc.mean()
    assert np.array_equal(v32[~unc], v64[~unc]), int((v32 != v64)[~unc].sum())
    assert 0 < v32.sum() < v32.size


def test_near_plane_and_min_views_only_remove():
    cams = VR.cams_from_views(world_poses(), HWF)
    base = VR.visibility(AABB, RES, LEVELS, cams, 12, 12, 0.0, 1)
    near = VR.visibility(AABB, RES, LEVELS, cams, 12, 12, 0.5, 1)
    assert not (near & ~base).any() and near.sum() < base.sum()
    # what the near plane removes lies in front of a camera, nearer than near_plane along its axis: within
    # near_plane * |d_corner| of its centre, |d_corner|^2 = 1 + 2 (6.5 / 14)^2 for these images
    eyes = world_poses()[:, :3, 3].double().numpy()  # (the first one is outside the roi but inside level 1's box)
    for l in range(LEVELS):
        ax = (np.arange(RES) + 0.5) / RES * 3.0 * 2 ** l - 1.5 * 2 ** l
        c = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1)[base[l] & ~near[l]]
        assert len(c) > 0
        dist = np.linalg.norm(c[:, None, :] - eyes[None], axis=-1).min(1)
        assert dist.max() <= 0.5 * math.sqrt(1.0 + 2.0 * (6.5 / 14.0) ** 2) + 1e-6, dist.max()


def test_both_conventions_describe_the_same_cameras():
    """`get_rays` poses with the half-pixel principal point = OpenCV poses (y and z flipped) with that K."""
    poses = world_poses()
    K = torch.tensor([[14.0, 0.0, 6.5], [0.0, 14.0, 6.5], [0.0, 0.0, 1.0]])
    c2w = poses.clone()
    c2w[:, :3, 1:3] *= -1.0
    assert np.array_equal(VR.cams_from_views(poses, HWF), VR.cams_opencv(K, c2w))
    # a pixel ray's points project to its own pixel: u' = u + 1/2
    cam = VR.cams_from_views(poses[:1], HWF)[0].astype(np.float64)
    o, d = O.get_rays(poses[0], HWF)
    p = (o[3, 7] + 2.5 * d[3, 7]).double().numpy()
    X, Y, D = (cam[r:r + 3] @ p + cam[r + 3] for r in (0, 4, 8))
    assert abs(cam[12] * X / D + cam[14] - 7.5) < 1e-4 and abs(cam[13] * Y / D + cam[15] - 3.5) < 1e-4 and D > 0


def test_pack_bits_layout():
    m = np.zeros(64, bool)
    m[[0, 33, 63]] = True
    assert VR.pack_bits(m).tolist() == [1, np.array([(1 << 1) | (1 << 31)], np.uint32).view(np.int32)[0]]
