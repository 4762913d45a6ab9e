"""GPU: OccGridEstimator.mark_invisible_cells / mark_invisible_from_views (csrc/occ_invisible.hip).  The mask equals the
float32 restatement of the rule (tests/occ_invisible_ref.py) in every bit; an update on a marked estimator keeps the
invisible cells at occs == -1 and off, takes its threshold from the visible cells, and leaves the visible cells' occs
what an unmarked twin computes; every render route samples visible cells only; the mask travels in the state_dict."""
import math

import numpy as np
import pytest
import torch

from oracle import fsnerf_oracle as O

import occ_cone_ref as CR
import occ_invisible_ref as VR
from test_occ_invisible_cpu import AABB, AABB_NDC, HWF, look_at, ndc_poses, world_poses

pytestmark = pytest.mark.gpu
STEP = 2e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import fs_nerf_amd  # noqa: F401
    return torch.device("cuda:0")


def make_est(dev, res, levels, aabb=AABB, seed=5):
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    est = OccGridEstimator(aabb, res, levels).to(dev).train()
    est.generator = torch.Generator().manual_seed(seed)
    return est


def many_world_poses(n, seed=11):
    """The three cameras of the CPU tests, then random ones: eyes in a shell of radius 0.4 .. 4.2, looking at random
    points of the roi."""
    rng = np.random.default_rng(seed)
    poses = list(world_poses())
    while len(poses) < n:
        eye = rng.normal(size=3)
        eye *= rng.uniform(0.4, 4.2) / np.linalg.norm(eye)
        poses.append(look_at(eye, rng.uniform(-1.0, 1.0, size=3), up=(0.0, 0.3, 1.0)))
    return torch.stack(poses[:n])


def many_ndc_poses(n, seed=12):
    rng = np.random.default_rng(seed)
    poses = list(ndc_poses())
    while len(poses) < n:
        ax, ay = rng.uniform(-0.2, 0.2, size=2)
        rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
        ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = ry @ rx, rng.uniform(-0.4, 0.4, size=3) * (1.0, 1.0, 0.2)
        poses.append(torch.from_numpy(m).float())
    return torch.stack(poses[:n])


def opencv_form(poses, hwf):
    """`get_rays` poses -> (K, c2w) of mark_invisible_cells: y and z flipped, principal point at W/2 + 1/2, H/2 + 1/2."""
    H, W, f = hwf
    c2w = poses.clone()
    c2w[:, :3, 1:3] *= -1.0
    return torch.tensor([[f, 0.0, W / 2.0 + 0.5], [0.0, f, H / 2.0 + 0.5], [0.0, 0.0, 1.0]]), c2w


# ---------------------------------------------------------------- 1. the kernel against the float32 restatement
@pytest.mark.parametrize("res,levels", [(8, 1), (8, 3), (12, 1), (12, 3), (16, 1), (16, 3)])
def test_mask_equals_the_float32_restatement(dev, res, levels):
    """Every bit, through mark_invisible_from_views: 1, 3 and 70 cameras (more than a wave's worth), near_plane 0 and
    0.5, min_views 1 and 2.  12^3 cells are 27 waves: the last block is partial."""
    est = make_est(dev, res, levels)
    poses = many_world_poses(70)
    seen = set()
    for n in (1, 3, 70):
        cams = VR.cams_from_views(poses[:n], HWF)
        for near_plane in (0.0, 0.5):
            for min_views in (1, 2):
                est.mark_invisible_from_views(poses[:n], HWF, near_plane, min_views=min_views)
                want = VR.visibility(AABB, res, levels, cams, HWF[1], HWF[0], near_plane, min_views)
                got = est.visible.cpu().numpy()
                assert got.shape == want.shape and np.array_equal(got, want), (n, near_plane, min_views, int((got != want).sum()))
                assert np.array_equal(est.vis_bits.cpu().numpy(), VR.pack_bits(want))
                seen.add(int(want.sum()))
    assert len(seen) >= 4 and 0 in seen, "the cases differ; one camera never gives two views"


@pytest.mark.parametrize("n", [3, 70])
def test_ndc_mask_equals_the_float32_restatement(dev, n):
    """The LLFF path: the grid lives in NDC space; 2 levels, so that cells with z' >= 1 exist (all invisible)."""
    res, levels = 16, 2
    est = make_est(dev, res, levels, AABB_NDC)
    poses = many_ndc_poses(n)
    cams = VR.cams_from_views(poses, HWF)
    for near_plane, min_views in ((0.0, 1), (0.5, 1), (0.0, 2), (0.5, 2)):
        est.mark_invisible_from_views(poses, HWF, near_plane, ndc=True, min_views=min_views)
        want = VR.visibility(AABB_NDC, res, levels, cams, HWF[1], HWF[0], near_plane, min_views, ndc=VR.ndc_args(HWF))
        got = est.visible.cpu().numpy()
        assert np.array_equal(got, want), (near_plane, min_views, int((got != want).sum()))
        assert 0 < want.sum() < want.size and not want[1, :, :, 12:].any(), "level 1, z' >= 1: no real point"


def test_both_entry_points_agree(dev):
    """The same cameras in the two conventions; K holds cx = W/2 + 1/2, cy = H/2 + 1/2.  K per camera or shared, poses
    [N,3,4] or [N,4,4], host or device tensors; `chunk` is accepted."""
    poses = many_world_poses(5)
    K, c2w = opencv_form(poses, HWF)
    a, b = make_est(dev, 16, 2), make_est(dev, 16, 2)
    a.mark_invisible_from_views(poses, HWF, 0.3, min_views=2)
    b.mark_invisible_cells(K, c2w, HWF[1], HWF[0], 0.3, min_views=2)
    assert torch.equal(a.vis_bits, b.vis_bits) and 0 < int(a.visible.sum()) < a.visible.numel()
    b.mark_invisible_cells(K[None].expand(5, 3, 3).to(dev), c2w[:, :3, :].to(dev), HWF[1], HWF[0], near_plane=0.3, chunk=7, min_views=2)
    assert torch.equal(a.vis_bits, b.vis_bits)
    # a second call replaces the mask (masks are not intersected): one view asks less than two
    before = a.visible.clone()
    a.mark_invisible_from_views(poses, HWF, 0.3, min_views=1)
    assert bool((a.visible | ~before).all()) and int(a.visible.sum()) > int(before.sum())


def test_marking_sets_occs_and_bits(dev):
    """After a call: occs == -1 exactly at the invisible cells, 0 at cells that were -1 and are visible now, untouched
    elsewhere; bits &= visible."""
    est = make_est(dev, 16, 2)
    assert not est.marked and bool(est.visible.all())
    bins = torch.rand(2, 16, 16, 16, generator=torch.Generator().manual_seed(3)) < 0.5
    est.set_binaries(bins)
    poses = world_poses()
    est.mark_invisible_from_views(poses, HWF, min_views=2)
    vis2 = est.visible.cpu()
    assert est.marked and torch.equal(est.binaries.cpu(), bins & vis2)
    assert torch.equal(est.occs.cpu().reshape(vis2.shape), torch.where(vis2, bins.float(), torch.tensor(-1.0)))
    est.mark_invisible_from_views(poses, HWF, min_views=1)
    vis1 = est.visible.cpu()
    assert int((vis1 & ~vis2).sum()) > 0
    want = torch.where(vis1, torch.where(vis2, bins.float(), torch.tensor(0.0)), torch.tensor(-1.0))
    assert torch.equal(est.occs.cpu().reshape(vis1.shape), want) and torch.equal(est.binaries.cpu(), bins & vis2 & vis1)


# ---------------------------------------------------------------- 2. updates on a marked estimator
LO, HI = 0.004, 0.02


def two_constants(x):
    return torch.where(x[:, 0] < 0, torch.full_like(x[:, 0], HI), torch.full_like(x[:, 0], LO))


def assert_masked_state(est, thre, what, constants=True):
    """binaries & ~visible is empty, occs == -1 exactly on ~visible, binaries = (occs > min(mean over the visible cells,
    thre)) & visible with the threshold formed by torch in float64 from the final occs.  constants: occs come from a few
    constants, none within 1e-3 (relative) of the threshold.  Otherwise (a network's densities) the cells within 1e-6 of
    it are left out: the kernel's mean differs from torch's by the order of a float64 sum, and rounding it to float32
    moves the threshold by at most 6e-8 (relative)."""
    vis, occs = est.visible.reshape(-1), est.occs
    assert not bool((est.binaries.reshape(-1) & ~vis).any()), what
    assert torch.equal(occs == -1.0, ~vis), what
    o64 = occs.double()
    thr = min(float(o64[vis].mean()), thre)
    far = ((o64 - thr).abs() / abs(thr) > (1e-3 if constants else 1e-6)) | ~vis
    assert not constants or bool(far.all()), (what, "a cell sits on the threshold")
    assert int((~far).sum()) <= 2 and torch.equal(est.binaries.reshape(-1)[far], ((o64 > thr) & vis)[far]), what
    return thr


def make_nerf(dev):
    from fs_nerf_amd.core.models import NeRF
    sd = O.init_nerf_state_dict(4, 128, [], 10, 4, seed=4)
    sd["sigma.weight"] *= 64.0
    sd["sigma.bias"] += 3.0
    m = NeRF(3, 3, 4, 128, (), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
    m.load_state_dict(sd)
    return m.to(dev).eval()


def test_callable_updates_on_a_marked_estimator(dev):
    """During and after warm-up.  The threshold comes from the visible cells: their mean lies between the two constants
    (occ_thre = 1 leaves it to the mean), while the mean over all cells - the invisible ones hold -1 - lies below the
    lower constant and would switch every visible cell on.  During warm-up every cell is re-evaluated at a point that
    depends on (seed, cell) only, so an unmarked twin's occs are the marked one's on the visible cells, bit for bit.
    (Past warm-up half of the draws come from `bits`, which the mask changes on purpose: the twins part there.)  The
    updates themselves make no host synchronisation."""
    est, twin = make_est(dev, 16, 2), make_est(dev, 16, 2)
    est.mark_invisible_from_views(world_poses(), HWF, min_views=1)
    vis = est.visible.reshape(-1)
    assert 0.05 < float(vis.float().mean()) < 0.95
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for step in (0, 16):
            est.update_every_n_steps(step, two_constants, occ_thre=1.0)
            twin.update_every_n_steps(step, two_constants, occ_thre=1.0)
        est_warm, twin_warm = est.occs.clone(), twin.occs.clone()
        for step in (256, 272):
            est.update_every_n_steps(step, two_constants, occ_thre=1.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(est_warm[vis], twin_warm[vis]) and not bool((twin_warm == -1.0).any())
    thr = assert_masked_state(est, 1.0, "callable")
    all_mean = float(est.occs.double().mean())
    assert LO * 1.05 < thr < HI * 0.95 and all_mean < LO, (thr, all_mean)
    on = est.binaries.reshape(-1)
    assert torch.equal(on, vis & (est.occs == HI)) and 0 < int(on.sum()) < int(vis.sum())
    # the usual threshold: occ_thre below the mean decides
    est.update_every_n_steps(288, two_constants, occ_thre=1e-2)
    assert assert_masked_state(est, 1e-2, "occ_thre") == 1e-2
    assert est._updates == 5 and twin._updates == 2


def test_fused_refresh_on_a_marked_estimator(dev):
    """NeRF.occ_eval_fn(step, "fp16") in the slot: the one-launch refresh, then the masked end."""
    m = make_nerf(dev)
    fn = m.occ_eval_fn(STEP, "fp16")
    est, twin = make_est(dev, 16, 2), make_est(dev, 16, 2)
    est.mark_invisible_from_views(world_poses(), HWF, min_views=1)
    vis = est.visible.reshape(-1)
    for step in (0, 16):
        est.update_every_n_steps(step, fn)
        twin.update_every_n_steps(step, fn)
        assert_masked_state(est, 1e-2, ("fused warm-up", step), constants=False)
        assert torch.equal(est.occs[vis], twin.occs[vis])
    for step in (256, 272):
        est.update_every_n_steps(step, fn)
        assert_masked_state(est, 1e-2, ("fused", step), constants=False)
    assert 0 < int(est.binaries.sum()) < int(vis.sum())


def test_set_binaries_on_a_marked_estimator(dev):
    est = make_est(dev, 16, 2)
    est.mark_invisible_from_views(world_poses(), HWF, min_views=1)
    est.set_binaries(torch.ones(2, 16, 16, 16, dtype=torch.bool))
    assert torch.equal(est.binaries, est.visible)
    assert_masked_state(est, 0.5, "set_binaries")
    assert torch.equal(est.occs.reshape(est.visible.shape), torch.where(est.visible, 1.0, -1.0))
    est.update_every_n_steps(0, two_constants, occ_thre=0.5)  # ... and the next refresh does not bring them back
    assert_masked_state(est, 0.5, "refresh after set_binaries")
    assert torch.equal(est.binaries, est.visible)  # (occs = max(1 * 0.95, constant) at every visible cell)


# ---------------------------------------------------------------- 3. rendering reads only `bits`
def test_every_render_route_samples_visible_cells_only(dev):
    """A marked, fully refreshed grid; 64 rays of a camera that was not marked with; the multi-launch route and the
    one-launch route (+ its gather) return samples whose cell (the march's float32 lookup) is visible."""
    from fs_nerf_amd.render import rendering as Rm
    from test_occ_fused import unfused
    m = make_nerf(dev)
    res, levels = 16, 2
    est = make_est(dev, res, levels)
    est.mark_invisible_from_views(world_poses(), HWF, min_views=1)
    est.update_every_n_steps(0, lambda x: torch.full_like(x[:, 0], 1.0))  # everything that may be on is on
    assert torch.equal(est.binaries, est.visible)
    est.eval()
    o, d = O.get_rays(O.pose_from_spherical(4.0311289, 20.0, 200.0), (8, 8, 9.0))
    o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
    vis = est.visible.cpu().numpy().reshape(levels, -1)
    c, h = np.zeros(3, np.float32), np.full(3, 1.5, np.float32)
    with torch.no_grad():
        multi = unfused(lambda: Rm.render_rays(o, d, est, m, white_bkgd=True, render_step_size=STEP, device=dev, want_extras=True))
        one = Rm.render_rays(o, d, est, m, white_bkgd=True, render_step_size=STEP, device=dev, want_extras=True)
        (rgb_f, _, _, _), ri_f, _ = Rm.render_rays(o, d, est, m, white_bkgd=True, render_step_size=STEP, device=dev, want_extras=False)
    assert ri_f is None and float((rgb_f - one[0][0]).abs().max()) < 1e-3 and float((one[0][0] - multi[0][0]).abs().max()) < 1e-3
    for (_, ri, tv), what in ((multi, "multi-launch"), (one, "one launch + gather")):
        ri, tv = ri.cpu().numpy(), tv.cpu().numpy().astype(np.float32)
        assert len(ri) > 100, what
        p = o.numpy()[ri] + d.numpy()[ri] * tv[:, None]
        assert CR._occupied(p, c, h, res, levels, vis).all(), what
    # the same rays through a full, unmarked grid do enter cells the mask removed: the check above can fail
    full = make_est(dev, res, levels)
    full.set_binaries(torch.ones(levels, res, res, res, dtype=torch.bool))
    ri, t0, t1 = full.eval().sampling(o.to(dev), d.to(dev), render_step_size=STEP)
    tm = ((t0 + t1) / 2).cpu().numpy()
    p = o.numpy()[ri.cpu().numpy()] + d.numpy()[ri.cpu().numpy()] * tm[:, None]
    assert not CR._occupied(p, c, h, res, levels, vis).all()


# ---------------------------------------------------------------- 4. persistence
def test_state_dict_round_trip_gives_the_same_mask_and_next_update(dev):
    est = make_est(dev, 16, 2, seed=9)
    est.mark_invisible_from_views(world_poses(), HWF, min_views=2)

    def occ_eval_fn(x):
        return STEP * 40.0 * torch.relu(1.0 - x.norm(dim=-1))

    for step in (0, 256, 272):
        est.update_every_n_steps(step=step, occ_eval_fn=occ_eval_fn)
    sd = {k: v.clone() for k, v in est.state_dict().items()}
    assert set(sd) == {"occs", "bits", "vis_bits", "_extra_state"}
    resumed = make_est(dev, 16, 2, seed=9)  # never marked: loading registers the mask
    resumed.load_state_dict(sd, strict=True)
    assert resumed.marked and torch.equal(resumed.vis_bits, est.vis_bits) and resumed._updates == 3
    est.update_every_n_steps(step=288, occ_eval_fn=occ_eval_fn)
    resumed.update_every_n_steps(step=288, occ_eval_fn=occ_eval_fn)
    assert torch.equal(resumed.occs, est.occs) and torch.equal(resumed.bits, est.bits)
    assert torch.equal(resumed.occs == -1.0, ~resumed.visible.reshape(-1))


def test_unmarked_state_dict_is_unchanged_and_old_ones_load(dev):
    est = make_est(dev, 16, 2)
    assert set(est.state_dict().keys()) == {"occs", "bits", "_extra_state"}
    est.update_every_n_steps(0, two_constants)
    old = {k: v.clone() for k, v in est.state_dict().items()}
    fresh = make_est(dev, 16, 2)
    fresh.load_state_dict(old, strict=True)
    assert not fresh.marked and bool(fresh.visible.all()) and torch.equal(fresh.bits, est.bits)
    # ... into a marked estimator as well: a state without the mask is all-visible
    marked = make_est(dev, 16, 2)
    marked.mark_invisible_from_views(world_poses(), HWF)
    marked.load_state_dict(old, strict=True)
    assert not marked.marked and set(marked.state_dict().keys()) == {"occs", "bits", "_extra_state"}
    assert torch.equal(marked.occs, est.occs)


# ---------------------------------------------------------------- 5. errors
def test_bad_arguments_raise_and_leave_the_estimator_alone(dev):
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    est = make_est(dev, 16, 1)
    poses = world_poses()
    K, c2w = opencv_form(poses, HWF)
    with pytest.raises(ValueError):
        est.mark_invisible_from_views(poses, HWF, min_views=0)
    with pytest.raises(ValueError):
        est.mark_invisible_cells(K, c2w, 12, 12, near_plane=-0.1)
    with pytest.raises(ValueError):
        est.mark_invisible_cells(K[None].expand(2, 3, 3), c2w, 12, 12)  # two K for three poses
    with pytest.raises(ValueError):
        est.mark_invisible_cells(K, c2w, 0, 12)
    with pytest.raises(ValueError):
        est.mark_invisible_cells(K, c2w[:0], 12, 12)
    assert not est.marked and set(est.state_dict().keys()) == {"occs", "bits", "_extra_state"}
    cpu = OccGridEstimator(AABB, 16, 1)  # an estimator whose buffers are CPU tensors: there is no CPU path
    with pytest.raises(RuntimeError):
        cpu.mark_invisible_from_views(poses, HWF)
    with pytest.raises(RuntimeError):
        cpu.mark_invisible_cells(K, c2w, 12, 12)
    assert not cpu.marked
    # the entry point checks its own arguments too (FSN_E_INVALID = -1), before any launch
    import ctypes as C
    from fs_nerf_amd import _lib as L
    lib, ab = L.lib(), (C.c_float * 6)(*AABB)
    cams, vis = torch.zeros(1, 16, device=dev), torch.zeros(16 ** 3 // 32, dtype=torch.int32, device=dev)
    call = lambda cp, n, w, h, near, mv, vp: lib.fsn_occgrid_visibility(ab, 16, 1, cp, n, w, h, near, mv, 0, 0.0, 0.0, 0.0, vp, None)
    cp, vp = C.c_void_p(cams.data_ptr()), C.c_void_p(vis.data_ptr())
    assert call(None, 1, 12, 12, 0.0, 1, vp) == -1 and call(cp, 1, 12, 12, 0.0, 1, None) == -1
    assert call(cp, 0, 12, 12, 0.0, 1, vp) == -1 and call(cp, 1, 12, 12, 0.0, 0, vp) == -1
    assert call(cp, 1, 12, 12, -1.0, 1, vp) == -1 and call(cp, 1, 0, 12, 0.0, 1, vp) == -1 and call(cp, 1, 12, -3, 0.0, 1, vp) == -1
    assert lib.fsn_occgrid_update_masked(None, 64, None, 0.5, 0, None, None, None) == -1
    assert not bool(vis.any())
