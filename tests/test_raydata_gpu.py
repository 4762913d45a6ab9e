"""-m gpu: the device-resident data layer (fs_nerf_amd.nerfdata, csrc/raydata.hip): rays bit for bit U.build_rays' rows,
colours bit for bit the reference's byte arithmetic (tests/raydata_ref.py), the reference's own LLFFDataset tables
(tests/golden/g8_raydata.npz), shuffled epochs, resume, rank slices, residency, and the two consumers: evaluation() and
the training loop body."""
import math
import os

import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import ops
from fs_nerf_amd.core import metrics
from fs_nerf_amd.nerfdata import FrameLoader, RayDataset, RayLoader
from fs_nerf_amd.utils import utilities as U

import debug_lib
import raydata_ref as RR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def forward_poses(n, seed=0):
    """[n,4,4] forward-facing cameras: rotations a few degrees off identity, small translations (NDC rays stay far from
    the singular set d_z = 0, tests/test_gpu_parity.py)."""
    rng = np.random.default_rng(seed)
    out = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    for k in range(n):
        ax, ay, az = np.radians(rng.uniform(-5, 5, size=3))
        Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
        Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
        Rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
        out[k, :3, :3] = (Rz @ Ry @ Rx).astype(np.float32)
        out[k, :3, 3] = rng.uniform(-0.15, 0.15, size=3)
    return out


def byte_images(n, H, W, C, seed=0):
    """uint8 [n,H,W,C] with all 256 byte values in the colour channels and a spread of alphas (0 and 255 among them)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(n, H, W, C), dtype=np.uint8)
    flat = img.reshape(-1, C)
    flat[:256, 0] = rng.permutation(256)
    if C == 4:
        flat[:256, 3] = np.arange(256)
        assert len(np.unique(img[..., 3])) >= 128 and img[..., 3].min() == 0 and img[..., 3].max() == 255
    assert len(np.unique(img[..., :3])) == 256
    return img


CASES = [(C, white, ndc) for C, white in ((3, False), (4, True), (4, False)) for ndc in (False, True)]


@pytest.mark.parametrize("hw", [(12, 16), (7, 9)])
@pytest.mark.parametrize("C,white,ndc", CASES)
def test_identity_order_is_the_ray_tables_and_the_reference_colours(dev, hw, C, white, ndc):
    H, W = hw
    hwf = (H, W, 0.9 * W)
    imgs, poses = byte_images(5, H, W, C, seed=H + C), forward_poses(5, seed=W)
    ds = RayDataset(imgs, poses, hwf, near=0.0, far=1.0, ndc=ndc, white_bkgd=white, device=dev)
    assert len(ds) == 5 * H * W
    o, d, rgb, index = ds.batch("identity", start=0, count=len(ds), want_index=True)
    ro, rd, aabb = U.build_rays(poses, hwf, dev, ndc)
    assert torch.equal(o, ro) and torch.equal(d, rd)
    assert torch.equal(ds.aabb, aabb)
    assert torch.equal(rgb.cpu(), RR.colours(imgs, white).reshape(-1, 3))
    assert torch.equal(index.cpu(), torch.arange(len(ds)))
    # the loader without shuffle, the item interface and a window in the middle say the same
    got = list(RayLoader(ds, 100, shuffle=False))
    assert torch.equal(torch.cat([g[0] for g in got]), ro) and torch.equal(torch.cat([g[2] for g in got]), rgb)
    i = len(ds) - 3
    io, id_, ic = ds[i]
    assert io.shape == (3,) and torch.equal(io, ro[i]) and torch.equal(id_, rd[i]) and torch.equal(ic, rgb[i])
    wo, wd, wc, _ = ds.batch("identity", start=37, count=130)
    assert torch.equal(wo, ro[37:167]) and torch.equal(wd, rd[37:167]) and torch.equal(wc, rgb[37:167])
    # outputs not asked for are not made
    assert ds.batch("identity", start=0, count=4, want_rays=False)[:2] == (None, None)
    assert ds.batch("identity", start=0, count=4, want_rgb=False)[2] is None


def test_every_byte_against_every_alpha(dev):
    """One 256 x 256 RGBA image: colour byte = row, alpha = column - all 65,536 pairs of the white-background
    composition (a fused multiply-add would change about a tenth of them)."""
    v = np.arange(256, dtype=np.uint8)
    img = np.zeros((1, 256, 256, 4), np.uint8)
    img[0, :, :, 0] = v[:, None]
    img[0, :, :, 1] = v[::-1, None]
    img[0, :, :, 2] = (v[:, None] * 7 + 3) & 255
    img[0, :, :, 3] = v[None, :]
    poses = forward_poses(1)
    for white in (True, False):
        ds = RayDataset.blender(img, poses, (256, 256, 300.0), white, dev)
        rgb = ds.batch("identity", start=0, count=len(ds), want_rays=False)[2]
        assert torch.equal(rgb.cpu(), RR.colours(img, white).reshape(-1, 3)), white
    assert (ds.near, ds.far, ds.ndc) == (2.0, 6.0, False) and ds.aabb.tolist() == [-1.5] * 3 + [1.5] * 3


@pytest.mark.parametrize("ndc", [True, False])
def test_against_the_reference_dataset(dev, golden_dir, ndc):
    g = np.load(os.path.join(golden_dir, "g8_raydata.npz"))
    H, W, focal = int(g["hwf"][0]), int(g["hwf"][1]), float(g["hwf"][2])
    ds = RayDataset.llff(g["imgs"], g["poses"], float(g["min_bound"]), float(g["max_bound"]), (H, W, focal), ndc, dev)
    t = f"ndc{int(ndc)}_"
    o, d, rgb = ds[torch.arange(len(ds))]
    np.testing.assert_allclose(o.cpu().numpy(), g[t + "rays_o"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(d.cpu().numpy(), g[t + "rays_d"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(ds.aabb.cpu().numpy(), g[t + "aabb"], rtol=1e-4, atol=1e-5)
    assert np.array_equal(rgb.cpu().numpy(), g[t + "rgb"])
    assert ds.near == float(g[t + "near"]) and ds.far == float(g[t + "far"]) and ds.ndc == ndc
    assert ds.hwf == (H, W, focal) and torch.equal(ds.poses, torch.from_numpy(g["poses"]))


def small_dataset(dev, ndc=False):
    H, W = 7, 9
    return RayDataset(byte_images(5, H, W, 4, seed=1), forward_poses(5, seed=2), (H, W, 8.0), near=0.0, far=1.0, ndc=ndc,
                      white_bkgd=True, device=dev)


def test_shuffled_epochs_resume_and_rank_slices(dev):
    ds = small_dataset(dev, ndc=True)
    N, B, seed = len(ds), 64, 2024
    assert N == 315
    ld = RayLoader(ds, B, shuffle=True, seed=seed, with_index=True)
    assert len(ld) == 5
    epochs = []
    for epoch in range(2):
        it = iter(ld)
        batches = []
        while True:
            try:
                batches.append(next(it))
            except StopIteration:
                break
        assert [b[0].shape[0] for b in batches] == [64, 64, 64, 64, 59]
        idx = torch.cat([b[3] for b in batches])
        assert np.array_equal(idx.cpu().numpy(), RR.perm(N, seed, epoch))
        assert torch.equal(idx.sort().values.cpu(), torch.arange(N))  # every ray once
        for o, d, rgb, index in batches:
            eo, ed, ec = ds[index]  # the explicit-index order
            assert torch.equal(o, eo) and torch.equal(d, ed) and torch.equal(rgb, ec)
            assert o.is_cuda and o.dtype == torch.float32 and index.dtype == torch.int64
        epochs.append(batches)
    assert not torch.equal(epochs[0][0][3], epochs[1][0][3])
    # resume from a mid-epoch state
    a = RayLoader(ds, B, seed=seed, with_index=True)
    it = iter(a)
    next(it), next(it)
    state = a.state_dict()
    rest = list(it)
    b = RayLoader(ds, B, seed=1, with_index=True)
    b.load_state_dict(state)
    again = list(iter(b))
    assert len(again) == len(rest) == 3
    for x, y in zip(rest, again):
        assert all(torch.equal(p, q) for p, q in zip(x, y))
    # ranks 0 and 1 of world 2 serve the world-1 loader's batches of 2B, slice by slice
    whole = list(iter(RayLoader(ds, 2 * B, seed=seed, with_index=True)))
    ranks = [list(iter(RayLoader(ds, B, seed=seed, rank=r, world=2, with_index=True))) for r in (0, 1)]
    assert len(ranks[0]) == len(ranks[1]) == N // (2 * B) == 2
    for g in range(2):
        for r in (0, 1):
            for full, part in zip(whole[g], ranks[r][g]):
                assert torch.equal(full[r * B:(r + 1) * B], part)


class _Recorder:
    """ops.ray_batch replaced: counts the launches, passes them on."""

    def __init__(self, monkeypatch):
        self.calls, self.real = 0, ops.ray_batch
        monkeypatch.setattr(ops, "ray_batch", self)

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.real(*a, **kw)


def test_one_launch_per_batch_and_bad_indices_raise_before_any_launch(dev, monkeypatch):
    ds = small_dataset(dev)
    rec = _Recorder(monkeypatch)
    n = sum(1 for _ in RayLoader(ds, 64))
    assert n == 5 and rec.calls == 5
    rec.calls = 0
    for bad in (torch.tensor([len(ds)]), torch.tensor([-1]), torch.tensor([0, 5, len(ds)], device=dev), len(ds), -1):
        with pytest.raises(IndexError):
            ds[bad]
    with pytest.raises(TypeError):
        ds[torch.tensor([0.5])]
    assert rec.calls == 0, "an out-of-range index reached a launch"
    o, d, rgb = ds[torch.tensor([0, len(ds) - 1], dtype=torch.int32)]
    assert rec.calls == 1 and o.shape == (2, 3)


def test_only_the_bytes_stay_resident(dev):
    n, H, W, C = 8, 96, 128, 4
    imgs, poses = byte_images(n, H, W, C, seed=3), forward_poses(n, seed=4)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    ds = RayDataset(imgs, poses, (H, W, 100.0), near=0.0, far=1.0, ndc=True, device=dev)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated(dev) - before
    assert grown <= n * H * W * C + 64 * 1024, grown  # (float tables: 36 bytes per pixel)
    assert len(ds) == n * H * W and bool(torch.isfinite(ds.aabb).all())


# ---------------------------------------------------------------- consumers
def make_nerf(L, D, seed, dev):
    from fs_nerf_amd.core.models import NeRF
    torch.manual_seed(seed)
    m = NeRF(3, 3, L, D, (4,) if L > 4 else (), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
    with torch.no_grad():
        m.sigma.weight.mul_(64.0)
        m.sigma.bias.add_(3.0)
    return m.to(dev)


def orbit_pose(phi_deg, theta_deg=50.0, radius=4.0311289):
    th, ph = math.radians(theta_deg), math.radians(phi_deg)
    tr = torch.tensor([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, radius], [0, 0, 0, 1.0]])
    rt = torch.tensor([[1, 0, 0, 0], [0, math.cos(th), -math.sin(th), 0], [0, math.sin(th), math.cos(th), 0], [0, 0, 0, 1.0]])
    rp = torch.tensor([[math.cos(ph), -math.sin(ph), 0, 0], [math.sin(ph), math.cos(ph), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    return rp @ (rt @ tr)


class _HandLoader:
    """The minimal loader evaluation() accepts (tests/test_metrics_gpu.py): an iterable with a `.dataset`."""

    class _DS:
        near, far, ndc = 2.0, 6.0, False

    def __init__(self, items):
        self.items, self.dataset = items, self._DS()

    def __iter__(self):
        return iter(self.items)


def test_evaluation_fed_by_a_frame_loader(dev):
    from fs_nerf_amd.render import rendering as R
    HW = 32
    hwf = (HW, HW, 0.5 * HW / math.tan(0.5 * 0.6911112))
    poses = torch.stack([orbit_pose(phi) for phi in (10.0, 100.0, 250.0)])
    imgs = byte_images(3, HW, HW, 4, seed=6)
    ds = RayDataset.blender(imgs, poses, hwf, True, dev)
    floats = RR.colours(imgs, True)
    hand = _HandLoader([(floats[v][None], poses[v][None]) for v in range(3)])
    frames = list(FrameLoader(ds))
    assert len(frames) == 3
    for v, (rgb_gt, pose) in enumerate(frames):
        assert rgb_gt.is_cuda and rgb_gt.dtype == torch.float32 and rgb_gt.shape == (1, HW, HW, 3) and pose.shape == (1, 4, 4)
        assert torch.equal(rgb_gt.cpu(), floats[v][None]) and torch.equal(pose, poses[v][None])
    model = make_nerf(8, 256, 2, dev).eval()
    est = R.StratifiedEstimator(2.0, 6.0, 64, 128)
    want = metrics.evaluation(hwf, model, est, None, hand, 1 << 20, dev, white_bkgd=True)
    got = metrics.evaluation(hwf, model, est, None, FrameLoader(ds), 1 << 20, dev, white_bkgd=True)
    assert torch.equal(got[0], want[0]) and got[1] == want[1] and got[2] is None and want[2] is None
    # shuffled: the same views in the permutation's order
    sh = FrameLoader(ds, shuffle=True, seed=5)
    order = RR.perm(3, 5, 0).tolist()
    for v, (rgb_gt, pose) in zip(order, sh):
        assert torch.equal(rgb_gt.cpu(), floats[v][None]) and torch.equal(pose, poses[v][None])


def _four_steps(dev, feed):
    """The loop body of examples/train_synthetic.py on a 4x128 network, four steps; feed(k) -> (rays_o, rays_d, rgb)."""
    from fs_nerf_amd.core.loss import WeightNormRegularizer
    from fs_nerf_amd.core.optim import FusedAdam
    from fs_nerf_amd.core.scheduler import ExponentialDecay
    from fs_nerf_amd.render import rendering as R
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    iters, step = 4, 2e-2
    model = make_nerf(4, 128, 2, dev).train()
    torch.manual_seed(17)
    est = OccGridEstimator(roi_aabb=torch.tensor([-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]), resolution=32, levels=1).to(dev)
    est.train()
    est.generator = torch.Generator(device=dev).manual_seed(11)
    opt = FusedAdam(model.parameters(), lr=5e-4)
    wnorm = WeightNormRegularizer(model.named_parameters(), reg="l2", reg_ratio=0.5, Td=iters)
    sched = ExponentialDecay(opt, iters, 5e-4, r=0.1)
    losses = []
    for k in range(iters):
        ro, rd, gt = feed(k)
        (rgb, _, _, _), _, _ = R.render_rays(ro, rd, est, model, train=True, white_bkgd=True, render_step_size=step, device=dev)
        loss = torch.nn.functional.mse_loss(rgb, gt)
        if wnorm.active(k):
            loss = loss + 1e-5 * wnorm()
        loss.backward()
        opt.step()
        sched.step()
        opt.zero_grad()
        est.update_every_n_steps(step=k, occ_eval_fn=lambda x: model(x) * step, occ_thre=1e-2)
        losses.append(loss.detach().clone())
    return torch.stack(losses)


def test_training_steps_fed_by_a_ray_loader(dev):
    HW = 24
    hwf = (HW, HW, 0.5 * HW / math.tan(0.5 * 0.6911112))
    poses = torch.stack([orbit_pose(phi) for phi in range(0, 360, 90)])
    imgs = byte_images(4, HW, HW, 4, seed=9)
    ds = RayDataset.blender(imgs, poses, hwf, True, dev)
    loader = RayLoader(ds, 512, seed=31, with_index=True)
    served = []

    def from_loader(k, it=[None]):
        if it[0] is None:
            it[0] = iter(loader)
        try:
            batch = next(it[0])
        except StopIteration:  # (run-nerf.py:236-240)
            it[0] = iter(loader)
            batch = next(it[0])
        served.append(batch[3])
        return batch[:3]

    a = _four_steps(dev, from_loader)
    assert len(served) == 4 and not torch.equal(served[0], served[1])
    assert loader.epoch == 0 and loader.position == 4  # 2304 rays: 4 full batches and a short one left
    ro, rd, _ = U.build_rays(poses, hwf, dev, False)
    gt = RR.colours(imgs, True).reshape(-1, 3).to(dev)
    b = _four_steps(dev, lambda k: (ro[served[k]], rd[served[k]], gt[served[k]]))
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (a.tolist(), b.tolist())


# ---------------------------------------------------------------- debug build
def test_ray_batch_kernel_reports_no_out_of_range_index():
    """The debug library in a child process: the smallest identity case and one shuffled epoch of it, all inputs valid."""
    rep = debug_lib.run_worker("raydata_debug_worker.py")
    assert rep["raydata"] == [0, 0, 0, 0], f"k_ray_batch met an index outside the dataset: {rep['raydata']} (count, line, index, N)"
    debug_lib.assert_no_other_unit_recorded(rep)
