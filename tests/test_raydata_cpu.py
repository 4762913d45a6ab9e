"""CPU: the data layer without a device - the epoch permutation (the library's own host build of csrc/ray_perm.hpp against
the NumPy restatement in tests/raydata_ref.py, bijectivity, windows), the loaders' bookkeeping with the launch replaced
by a recorder, and argument validation of fsn_ray_batch / RayDataset."""
import ctypes as C

import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L
from fs_nerf_amd import ops
from fs_nerf_amd.nerfdata import FrameLoader, RayDataset, RayLoader

import raydata_ref as RR

LLFF_N = 8 * 378 * 504
SIZES = [1, 2, 3, 5, 63, 64, 65, 1000, 4097, 2 ** 16 + 1, LLFF_N]
BIG = 2 ** 33 + 7
SEEDS = (0, 67280421310721)
EPOCHS = (0, 1, 2 ** 31)


def host_perm(n, seed, epoch, start=0, count=None):
    return ops.ray_perm_host(n, seed, epoch, start, count).numpy()


@pytest.mark.parametrize("n", SIZES)
def test_host_permutation_is_the_numpy_restatement(n):
    for seed in SEEDS:
        for epoch in EPOCHS:
            assert np.array_equal(host_perm(n, seed, epoch), RR.perm(n, seed, epoch)), (n, seed, epoch)


def test_host_permutation_window_of_a_large_index_set():
    """N = 2^33 + 7 does not fit in memory: windows of positions at the beginning, in the middle and at the very end."""
    for seed in SEEDS:
        for epoch in EPOCHS:
            for start, count in ((0, 4096), (2 ** 32 + 12345, 4096), (BIG - 1000, 1000)):
                got = host_perm(BIG, seed, epoch, start, count)
                assert np.array_equal(got, RR.perm(BIG, seed, epoch, start, count)), (seed, epoch, start)
                assert got.min() >= 0 and got.max() < BIG and len(np.unique(got)) == count
    p40 = host_perm(2 ** 40, 3, 1, 2 ** 40 - 512, 512)  # the width the loaders must support at least
    assert np.array_equal(p40, RR.perm(2 ** 40, 3, 1, 2 ** 40 - 512, 512)) and p40.max() < 2 ** 40 and len(np.unique(p40)) == 512


@pytest.mark.parametrize("n", SIZES)
def test_an_epoch_is_a_permutation_and_epochs_and_seeds_differ(n):
    orders = {}
    for seed in SEEDS:
        for epoch in (0, 1):
            p = host_perm(n, seed, epoch)
            assert np.array_equal(np.sort(p), np.arange(n)), (n, seed, epoch)
            orders[seed, epoch] = p
    if n >= 64:
        assert not np.array_equal(orders[SEEDS[0], 0], orders[SEEDS[0], 1])
        assert not np.array_equal(orders[SEEDS[0], 0], orders[SEEDS[1], 0])
        assert not np.array_equal(orders[SEEDS[0], 0], np.arange(n))
    # served in arbitrary windows, the concatenation is the whole
    rng = np.random.default_rng(n)
    cuts = np.unique(np.concatenate([[0, n], rng.integers(0, n + 1, size=7)]))
    parts = [host_perm(n, SEEDS[1], 1, int(a), int(b - a)) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts), orders[SEEDS[1], 1])


def test_host_permutation_validates_its_window():
    lib = L.lib()
    assert lib.fsn_ray_perm_host(10, 0, 0, 8, 3, None) == -1 and b"fsn_ray_perm_host" in lib.fsn_last_error()
    assert lib.fsn_ray_perm_host(10, 0, 0, 0, 10, None) == -1 and b"null" in lib.fsn_last_error()
    assert lib.fsn_ray_perm_host(0, 0, 0, 0, 0, None) == 0


# ---------------------------------------------------------------- loader bookkeeping
@pytest.fixture
def launches(monkeypatch):
    """ops.ray_batch replaced by a recorder (the way tests/test_render_routes_cpu.py replaces launches): every call is
    one launch; it returns (start, count, a colour tensor of that many rows, (seed, epoch)) in the four output slots."""
    calls = []

    def ray_batch(poses12, images, H, W, focal, **kw):
        assert images.dtype == torch.uint8 and tuple(images.shape[1:3]) == (H, W) and poses12.shape == (images.shape[0], 12)
        calls.append(kw)
        return kw["start"], kw["count"], torch.zeros(kw["count"], 3), (kw["seed"], kw["epoch"])
    monkeypatch.setattr(ops, "ray_batch", ray_batch)
    return calls


def _dataset(n_rays=3 * 5 * 7):
    """A RayDataset around host tensors (its constructor needs a GPU; the recorder never looks at the data):
    n_rays = views * 5 * 7."""
    n = n_rays // 35
    assert n * 35 == n_rays
    ds = RayDataset.__new__(RayDataset)
    ds.imgs, ds.poses = torch.zeros(n, 5, 7, 3, dtype=torch.uint8), torch.eye(4).repeat(n, 1, 1)
    ds.poses12, ds.hwf = ds.poses[:, :3, :4].reshape(n, 12), (5, 7, 10.0)
    ds.near, ds.far, ds.ndc, ds.white_bkgd, ds.device = 2.0, 6.0, False, False, torch.device("cpu")
    return ds


def test_loader_batches_epochs_and_stop(launches):
    ds = _dataset(105)
    ld = RayLoader(ds, 32, shuffle=True, seed=5, with_index=True)
    assert len(ld) == 4 and ld.dataset is ds
    it = iter(ld)
    got = [next(it) for _ in range(4)]
    assert [(g[0], g[1]) for g in got] == [(0, 32), (32, 32), (64, 32), (96, 9)]  # N not a multiple of B: a short last batch
    assert all(g[3] == (5, 0) for g in got) and all(c["order"] == "permuted" and c["want_index"] for c in launches)
    with pytest.raises(StopIteration):
        next(it)
    assert len(launches) == 4  # one launch per next, none for the StopIteration
    it = iter(ld)  # the next epoch ...
    assert next(it)[3] == (5, 1)
    it = iter(ld)  # ... and an abandoned iterator counts as one
    assert next(it)[3] == (5, 2) and ld.state_dict() == {"seed": 5, "epoch": 2, "position": 1}
    assert sum(1 for _ in it) == 3
    # for-loop shape, three-tuples by default, identity order without shuffle
    del launches[:]
    plain = RayLoader(_dataset(70), 32, shuffle=False, seed=1)
    assert [len(b) for b in plain] == [3, 3, 3] and [c["order"] for c in launches] == ["identity"] * 3
    assert not any(c["want_index"] for c in launches)
    with pytest.raises(ValueError):
        RayLoader(ds, 0)
    with pytest.raises(ValueError):
        RayLoader(ds, 8, rank=2, world=2)


def test_loader_seed_defaults_to_the_initial_seed():
    torch.manual_seed(1234)
    assert RayLoader(_dataset(), 8).seed == 1234 and FrameLoader(_dataset()).seed == 1234


def _plain(batches):
    return [(b[0], b[1], b[3]) for b in batches]


def test_loader_state_dict_round_trip_mid_epoch(launches):
    ds = _dataset(105)
    ld = RayLoader(ds, 16, seed=9, with_index=True)
    for _ in iter(ld):  # epoch 0 in full
        pass
    it = iter(ld)
    head = [next(it) for _ in range(3)]
    state = ld.state_dict()
    assert state == {"seed": 9, "epoch": 1, "position": 3}
    rest = list(it)
    other = RayLoader(_dataset(105), 16, seed=77, with_index=True)
    other.load_state_dict(state)
    assert _plain(iter(other)) == _plain(rest) and len(head) + len(rest) == len(ld)
    assert next(iter(other))[3] == (9, 2)  # and then goes on to the next epoch
    # a state taken at the end of an epoch: nothing is left of it
    done = RayLoader(_dataset(105), 16, seed=1)
    done.load_state_dict(ld.state_dict())
    assert list(iter(done)) == []
    # a state taken before the first iter(): the restored loader starts epoch 0
    fresh = RayLoader(_dataset(105), 16, seed=1, with_index=True)
    fresh.load_state_dict(RayLoader(_dataset(105), 16, seed=4).state_dict())
    assert next(iter(fresh))[3] == (4, 0)


@pytest.mark.parametrize("world", [2, 8])
def test_loader_rank_slices(launches, world):
    n, B = 1015, 16
    loaders = [RayLoader(_dataset(n), B, seed=3, rank=r, world=world, with_index=True) for r in range(world)]
    steps = n // (B * world)
    assert all(len(ld) == steps for ld in loaders) and steps > 0 and n % (B * world) != 0
    per_rank = [list(iter(ld)) for ld in loaders]
    assert len(launches) == steps * world  # one launch per next
    covered = []
    for g in range(steps):
        slices = [per_rank[r][g] for r in range(world)]
        assert all(s[1] == B and s[3] == (3, 0) for s in slices)  # the same permutation on every rank
        pos = [set(range(s[0], s[0] + s[1])) for s in slices]
        assert sum(len(p) for p in pos) == len(set().union(*pos)) == B * world  # disjoint
        assert set().union(*pos) == set(range(g * B * world, (g + 1) * B * world))
        covered += sorted(set().union(*pos))
    assert covered == list(range(steps * B * world))  # the tail shorter than B * world is dropped


def test_frame_loader_bookkeeping(launches):
    ds = _dataset()
    fl = FrameLoader(ds)
    assert len(fl) == 3 and fl.dataset is ds
    items = list(fl)
    assert [tuple(g.shape) for g, _ in items] == [(1, 5, 7, 3)] * 3 and all(p.shape == (1, 4, 4) for _, p in items)
    assert [(c["order"], c["start"], c["count"], c["want_rays"]) for c in launches] == [("identity", 35 * v, 35, False) for v in range(3)]
    del launches[:]
    sh = FrameLoader(ds, shuffle=True, seed=11)
    for epoch in (0, 1):
        list(sh)
        assert [c["start"] // 35 for c in launches] == RR.perm(3, 11, epoch).tolist()
        del launches[:]


def test_item_interface_checks_the_range_before_any_launch(launches):
    ds = _dataset()
    for bad in (torch.tensor([len(ds)]), torch.tensor([-1]), torch.tensor([0, 5, len(ds)]), len(ds), -1):
        with pytest.raises(IndexError):
            ds[bad]
    assert launches == []


# ---------------------------------------------------------------- validation
def test_ray_batch_argument_validation_without_gpu():
    lib = L.lib()
    one = C.c_void_p(1)  # never dereferenced: every call below fails its checks before a launch

    def call(images=one, C_=3, white=0, order=0, start=0, count=4, poses=one, n=2, H=3, W=4):
        return lib.fsn_ray_batch(poses, n, images, H, W, C_, 5.0, 0, 1.0, white, order, 0, 0, None, start, count, one, one, one,
                                 None, None)
    assert call(C_=5) == -1 and b"channels" in lib.fsn_last_error()
    assert call(C_=3, white=1) == -1 and b"white_bkgd" in lib.fsn_last_error()
    assert call(start=21, count=4) == -1 and b"start + count > N" in lib.fsn_last_error()
    assert call(order=1, start=0, count=25) == -1 and b"start + count > N" in lib.fsn_last_error()
    assert call(images=None) == -1 and b"null" in lib.fsn_last_error()
    assert call(poses=None) == -1 and b"null" in lib.fsn_last_error()
    assert call(order=7) == -1 and b"order" in lib.fsn_last_error()
    assert call(H=0) == -1 and b"geometry" in lib.fsn_last_error()
    assert call(order=2, count=4) == -1 and b"null index list" in lib.fsn_last_error()
    assert call(count=0) == 0  # an empty batch is not an error


def test_dataset_refuses_float_images_and_cpu_devices():
    poses = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    u8 = np.zeros((2, 3, 4, 3), np.uint8)
    with pytest.raises(TypeError, match="bytes"):
        RayDataset(u8.astype(np.float32) / 255.0, poses, (3, 4, 5.0), near=2.0, far=6.0)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        RayDataset(u8, poses, (3, 4, 5.0), near=2.0, far=6.0, device="cpu")
    with pytest.raises(RuntimeError):
        RayDataset.blender(np.zeros((2, 3, 4, 4), np.uint8), poses, (3, 4, 5.0), True, torch.device("cpu"))
    with pytest.raises(RuntimeError):
        RayDataset.llff(u8, poses, 1.0, 9.0, (3, 4, 5.0), True, torch.device("cpu"))
    with pytest.raises(RuntimeError):
        ops.ray_batch(torch.zeros(2, 12), torch.zeros(2, 3, 4, 3, dtype=torch.uint8), 3, 4, 5.0, count=4)
