"""GPU: learnable intrinsics behind the loaders (csrc/pose_refine.hip, csrc/raydata.hip, nerfdata/intrinsics_refine.py;
DESIGN 6.3) against the restatements of tests/intrinsics_ref.py.  Rays are compared bit for bit (the NumPy float32 rows);
accuracy is measured as in tests/test_pose_refine_gpu.py, with its bar unchanged:
    E = max |a - g64| per block relative to the block's largest |g64|,   E_kernel <= 4 E_f32 + 16 * 2^-24
with g64 float64 autograd through the restatement and E_f32 the same restatement in float32 on the CPU; the blocks are
(focal, principal point) of K(phi) and (omega, tau, focal, principal point) of the gradient.  Every pair of the gradient
tests goes to profiles/intrinsics_accuracy.json (FSN_INTRINSICS_ACCURACY_OUT names another file)."""
import json
import os

import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import ops
from fs_nerf_amd.nerfdata import CameraRefiner, IntrinsicsRefiner, PatchLoader, RayDataset, RayLoader

import debug_lib
import intrinsics_ref as IR
import pose_refine_ref as PR
import test_intrinsics_cpu as TI
import test_pose_refine_cpu as TC
import test_pose_refine_gpu as TP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLACK, H, W, FOCAL = TP.SLACK, TP.H, TP.W, TP.FOCAL  # 5 x 7 images at focal 10
BLOCKS = ("omega", "tau", "focal", "principal point")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def set_phi(intr, phi):
    with torch.no_grad():
        intr.phi.copy_(phi)


# ---------------------------------------------------------------- the rays
@pytest.mark.parametrize("ndc", [False, True])
def test_zero_parameter_serves_the_stored_intrinsics_bit_for_bit(dev, ndc):
    ds = TP.dataset(dev, 3, H, W, FOCAL, ndc)
    for per_view in (False, True):
        intr = IntrinsicsRefiner(ds, per_view=per_view)
        assert intr.phi.shape == (3 if per_view else 1, 4) and intr.phi.dtype == torch.float32
        assert isinstance(intr.phi, torch.nn.Parameter) and intr.phi.device == ds.device and not bool(intr.phi.any())
        assert intr.K().tolist() == [[FOCAL, FOCAL, W * 0.5, H * 0.5]] * intr.phi.shape[0]
        assert intr.K() is intr.K()  # composed once per change of phi
        for cam in (None, CameraRefiner(ds)):
            plain = list(RayLoader(ds, 40, shuffle=True, seed=3, with_index=True))
            refined = list(RayLoader(ds, 40, shuffle=True, seed=3, with_index=True, cameras=cam, intrinsics=intr))
            assert len(plain) == len(refined) == 3
            for a, b in zip(plain, refined):
                assert all(torch.equal(x, y) for x, y in zip(a, b))
                assert b[0].requires_grad and b[1].requires_grad and not b[2].requires_grad  # (NDC origins depend on K)
            assert len(next(iter(RayLoader(ds, 40, seed=3, cameras=cam, intrinsics=intr)))) == 3
            a = next(iter(PatchLoader(ds, 3, 2, shuffle=True, seed=5)))
            b = next(iter(PatchLoader(ds, 3, 2, shuffle=True, seed=5, cameras=cam, intrinsics=intr)))
            assert len(a) == len(b) == 3 and b[0].shape == (18, 3) and all(torch.equal(x, y) for x, y in zip(a, b))
    assert IntrinsicsRefiner(ds).hwf() == (H, W, FOCAL)
    # a change of phi is seen by the next batch; the state dict round-trips
    set_phi(intr, IR.random_phi(3, np.random.default_rng(0)))
    assert not torch.equal(intr.K(), IntrinsicsRefiner(ds, per_view=True).K())
    other = IntrinsicsRefiner((H, W, FOCAL), 3, per_view=True, device=dev)
    other.load_state_dict(intr.state_dict())
    assert torch.equal(other.phi, intr.phi) and torch.equal(other.K(), intr.K())
    with pytest.raises(ValueError, match="frame_rays"):
        intr.hwf()
    with pytest.raises(ValueError, match="frame_rays"):
        IntrinsicsRefiner(ds, tie_focal=False).hwf()
    moved = IntrinsicsRefiner(ds)
    set_phi(moved, torch.tensor([[0.1, 0.0, 0.01, 0.0]]))
    with pytest.raises(ValueError, match="frame_rays"):
        moved.hwf()
    set_phi(moved, torch.tensor([[0.1, 0.0, 0.0, 0.0]]))
    assert moved.hwf() == (H, W, float(moved.K()[0, 0])) and abs(moved.hwf()[2] - FOCAL * np.exp(0.1)) <= 1e-5
    with pytest.raises(ValueError):
        RayLoader(ds, 40, intrinsics=IntrinsicsRefiner((H, W, FOCAL), 2, per_view=True, device=dev))
    with pytest.raises(ValueError):
        PatchLoader(ds, 3, 2, intrinsics=IntrinsicsRefiner((H, W + 1, FOCAL), device=dev))


@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("per_view", [False, True])
@pytest.mark.parametrize("tie_focal", [False, True])
def test_rows_equal_the_float32_restatement_bit_for_bit(dev, ndc, per_view, tie_focal):
    n = 8  # 280 rays
    ds = TP.dataset(dev, n, H, W, FOCAL, ndc, seed=1)
    intr = IntrinsicsRefiner(ds, per_view=per_view, tie_focal=tie_focal)
    set_phi(intr, IR.random_phi(intr.phi.shape[0], np.random.default_rng(4)))
    cam = CameraRefiner(ds)
    with torch.no_grad():
        cam.xi.copy_(PR.random_xi(n, 0.05, np.random.default_rng(1), tau=0.02))
    K = intr.K().cpu()
    if tie_focal:
        assert torch.equal(K[:, 0], K[:, 1])
    for cameras in (None, cam):
        P = (ds.poses12 if cameras is None else cameras.poses12()).cpu()
        # every ray of the dataset in two batches (more than one block, a short last one)
        for o, d, _, index in RayLoader(ds, 270, shuffle=True, seed=2, with_index=True, cameras=cameras, intrinsics=intr):
            wo, wd = IR.rows_f32(P, K, index.cpu(), H, W, FOCAL, ndc)
            assert torch.equal(o.detach().cpu(), torch.from_numpy(wo)) and torch.equal(d.detach().cpu(), torch.from_numpy(wd))
        for o, d, _, index in PatchLoader(ds, 3, 50, dilation=1, shuffle=True, seed=2, with_index=True, cameras=cameras,
                                          intrinsics=intr):
            wo, wd = IR.rows_f32(P, K, index.cpu(), H, W, FOCAL, ndc)
            assert torch.equal(o.detach().cpu(), torch.from_numpy(wo)) and torch.equal(d.detach().cpu(), torch.from_numpy(wd))
    # frame_rays: the batch rows of that view, in one launch
    for view in range(n):
        o, d = intr.frame_rays(ds.poses[view], view=view, ndc=ndc)
        bo, bd, _, _ = ds.batch("identity", start=view * H * W, count=H * W, K=intr.K())
        assert o.shape == (H * W, 3) and torch.equal(o, bo) and torch.equal(d, bd)
    if per_view:
        with pytest.raises(ValueError):
            intr.frame_rays(ds.poses[0], view=n)


@pytest.mark.parametrize("tie_focal", [False, True])
def test_table_accuracy(dev, tie_focal):
    rng = np.random.default_rng(3)
    phi = IR.random_phi(64, rng, focal=0.5, centre=0.2)
    phi[0] = 0.0
    got = ops.intrinsics_compose(phi.to(dev), H, W, FOCAL, tie_focal).cpu()
    want = IR.table(phi.double(), H, W, FOCAL, tie_focal)
    e_kernel = IR.block_error(got, want, IR.FOCAL_PP)
    e_f32 = IR.block_error(IR.table(phi, H, W, FOCAL, tie_focal), want, IR.FOCAL_PP)
    print(f"K(phi) tie={tie_focal}: E_kernel {e_kernel}  E_f32 {e_f32}")
    assert all(k <= 4 * f + SLACK for k, f in zip(e_kernel, e_f32)), (e_kernel, e_f32)
    assert got[0].tolist() == [FOCAL, FOCAL, W * 0.5, H * 0.5]
    if tie_focal:
        assert torch.equal(got[:, 0], got[:, 1])


# ---------------------------------------------------------------- the gradient
_ACCURACY = {}


def _write_accuracy():
    out = os.environ.get("FSN_INTRINSICS_ACCURACY_OUT", os.path.join(ROOT, "profiles", "intrinsics_accuracy.json"))
    try:
        with open(out, "w") as f:
            json.dump({"measure": "E = max |a - g64| per block (omega, tau, focal, principal point) relative to the block's "
                                  "largest |g64|; bar E_kernel <= 4 E_f32 + 16 * 2^-24; images 5 x 7, focal 10",
                       "cases": _ACCURACY}, f, indent=1)
    except OSError:  # (a read-only checkout: the figures stay in the test's output)
        pass


def grad_case(n_views, count, ndc, theta, per_view, seed):
    """test_pose_refine_gpu's case and a random phi [1 or n, 4]."""
    P0, xi, index, go, gd = TP.grad_case(n_views, count, ndc, theta, seed)
    return P0, xi, IR.random_phi(n_views if per_view else 1, np.random.default_rng(seed + 1)), index, go, gd


def kernel_grad(dev, P0, xi, phi, index, go, gd, ndc, tie_focal, want_xi_grad=None):
    """-> (grad_xi or None, grad_phi, grad_K_views) of the two launches."""
    opt = lambda t: None if t is None else t.to(dev)
    phi = phi.to(dev)
    K = ops.intrinsics_compose(phi, H, W, FOCAL, tie_focal)
    g_xi, g_K = ops.ray_camera_grad(P0.to(dev), opt(xi), H, W, FOCAL, K, index.to(dev), opt(go), opt(gd), ndc=ndc,
                                    want_xi_grad=want_xi_grad)
    return g_xi, ops.intrinsics_grad(phi, g_K, H, W, FOCAL, tie_focal), g_K


def check_grad(dev, tag, P0, xi, phi, index, go, gd, ndc, tie_focal):
    g_xi, g_phi, g_K = kernel_grad(dev, P0, xi, phi, index, go, gd, ndc, tie_focal)
    got = torch.cat([g_xi.cpu(), g_phi.cpu().expand(P0.shape[0], 4) if phi.shape[0] == 1 else g_phi.cpu()], 1)
    cat = lambda pair: torch.cat([pair[0], pair[1].expand(P0.shape[0], 4) if phi.shape[0] == 1 else pair[1]], 1)
    want = cat(IR.camera_grad(P0.double(), xi.double(), phi.double(), index, H, W, FOCAL, ndc, tie_focal, go, gd))
    f32 = cat(IR.camera_grad(P0, xi, phi, index, H, W, FOCAL, ndc, tie_focal, go, gd))
    blocks = (slice(0, 3), slice(3, 6), slice(6, 8), slice(8, 10))
    e_kernel, e_f32 = IR.block_error(got, want, blocks), IR.block_error(f32, want, blocks)
    _ACCURACY[tag] = {"E_kernel": e_kernel, "E_f32": e_f32}
    print(f"{tag}: E_kernel " + " ".join(f"{e:.3e}" for e in e_kernel) + "  E_f32 " + " ".join(f"{e:.3e}" for e in e_f32))
    absent = torch.bincount(index // (H * W), minlength=P0.shape[0]) == 0
    assert not bool(g_xi.cpu()[absent].any()) and not bool(g_K.cpu()[absent].any()), "a view without a ray has a gradient"
    if phi.shape[0] > 1:
        assert not bool(g_phi.cpu()[absent].any())
    if tie_focal:
        assert not bool(g_phi[:, 1].any())  # exactly 0
    assert bool(torch.isfinite(got).all())
    return [(tag, block, k, f) for block, k, f in zip(BLOCKS, e_kernel, e_f32) if k > 4 * f + SLACK]


@pytest.mark.parametrize("ndc", [False, True])
@pytest.mark.parametrize("n_views", [1, 3, 65])
def test_gradient_accuracy(dev, n_views, ndc):
    missed, k = [], 0
    for count in (1, 63, 64, 65, 257, 1025, 4097):  # (1025: one entry past the workgroup's first stride)
        for per_view in (False, True):
            for tie_focal in (True, False):
                for theta in (0.0, 0.3):
                    k += 1
                    tag = (f"{'ndc' if ndc else 'world'} views={n_views} count={count} {'per-view' if per_view else 'shared'} "
                           f"{'tied' if tie_focal else 'untied'} theta={theta:g}")
                    case = grad_case(n_views, count, ndc, theta, per_view, seed=1000 * count + 2 * k)
                    missed += check_grad(dev, tag, *case, ndc, tie_focal)
    _write_accuracy()
    assert not missed, missed


@pytest.mark.parametrize("ndc", [False, True])
def test_gradient_structure(dev, ndc):
    P0, xi, phi, index, go, gd = grad_case(3, 192, ndc, 0.3, True, seed=7)
    tag = "ndc" if ndc else "world"
    missed = check_grad(dev, f"{tag} 192 rays null grad_o", P0, xi, phi, index, None, gd, ndc, False)
    missed += check_grad(dev, f"{tag} 192 rays null grad_d", P0, xi, phi, index, go, None, ndc, False)
    # every ray in view 1: the other two get exactly 0 (check_grad asserts it)
    missed += check_grad(dev, f"{tag} one view of three", P0, xi, phi, index % (H * W) + H * W, go, gd, ndc, False)
    _write_accuracy()
    assert not missed, missed
    full = kernel_grad(dev, P0, xi, phi, index, go, gd, ndc, False)
    for out in kernel_grad(dev, P0, xi, phi, index, None, None, ndc, False):
        assert not bool(out.any())
    for out in kernel_grad(dev, P0, xi, phi, index[:0], go[:0], gd[:0], ndc, False):  # count = 0: every row written, 0
        assert not bool(out.any())
    # no correction: a null xi is a zero xi (and grad_xi may be left out)
    zero = kernel_grad(dev, P0, torch.zeros_like(xi), phi, index, go, gd, ndc, False)
    null = kernel_grad(dev, P0, None, phi, index, go, gd, ndc, False, want_xi_grad=True)
    assert all(torch.equal(a, b) for a, b in zip(zero, null)) and float(null[0].abs().max()) > 0
    none = kernel_grad(dev, P0, None, phi, index, go, gd, ndc, False)
    assert none[0] is None and torch.equal(none[1], null[1]) and torch.equal(none[2], null[2])
    # an index outside the dataset contributes nothing (here: at the end, so that no other entry moves)
    bad = torch.cat([index, torch.tensor([3 * H * W, -1])])
    pad = torch.ones(2, 3)
    padded = kernel_grad(dev, P0, xi, phi, bad, torch.cat([go, pad]), torch.cat([gd, pad]), ndc, False)
    assert all(torch.equal(a, b) for a, b in zip(padded, full))
    # with the stored intrinsics in K, grad_xi is ops.ray_pose_grad's: the same sums in the same order
    for rows in (1, 3):
        g_xi, _, g_K = kernel_grad(dev, P0, xi, torch.zeros(rows, 4), index, go, gd, ndc, True)
        assert torch.equal(g_xi, TP.kernel_grad(dev, P0, xi, index, go, gd, ndc)) and float(g_K.abs().max()) > 0


def test_two_calls_give_the_same_bits(dev):
    for ndc in (False, True):
        for per_view in (False, True):
            case = grad_case(65, 4097, ndc, 0.3, per_view, seed=5)
            a, b = kernel_grad(dev, *case, ndc, False), kernel_grad(dev, *case, ndc, False)
            assert all(torch.equal(x, y) and float(x.abs().max()) > 0 for x, y in zip(a, b))


# ---------------------------------------------------------------- autograd wiring
@pytest.mark.parametrize("loader_kind", ["rays", "patches"])
def test_backward_through_render_rays_is_the_direct_calls(dev, loader_kind):
    from fs_nerf_amd.render import rendering as Rm
    ds = TP.dataset(dev, 3, 16, 16, 22.0, False, seed=4)
    coarse, fine = TP.small_net(dev, 6), TP.small_net(dev, 7)
    est = Rm.StratifiedEstimator(2.0, 6.0, 16, 8).train()

    def step(cam, intr):
        if loader_kind == "rays":
            loader = RayLoader(ds, 256, shuffle=True, seed=1, with_index=True, cameras=cam, intrinsics=intr)
        else:
            loader = PatchLoader(ds, 4, 2, shuffle=True, seed=1, with_index=True, cameras=cam, intrinsics=intr)
        o, d, rgb_gt, index = next(iter(loader))
        assert o.shape[0] == (256 if loader_kind == "rays" else 32)
        seen = {}
        o.register_hook(lambda g: seen.__setitem__("o", g.clone()))
        d.register_hook(lambda g: seen.__setitem__("d", g.clone()))
        gen = torch.Generator().manual_seed(3)
        u, u_fine = torch.rand(o.shape[0], generator=gen).to(dev), torch.rand(o.shape[0], 8, generator=gen).to(dev)
        intr.phi.grad = None
        if cam is not None:
            cam.xi.grad = None
        (rgb, _, _, _), _, _ = Rm.render_rays(o, d, est, coarse, model_fine=fine, train=True, white_bkgd=True, device=dev,
                                              u=u, u_fine=u_fine)
        torch.nn.functional.mse_loss(rgb, rgb_gt).backward()
        return index, seen

    def direct(cam, intr, index, seen):
        g_xi, g_K = ops.ray_camera_grad(ds.poses12, None if cam is None else cam.xi.detach(), 16, 16, 22.0, intr.K(), index,
                                        seen["o"], seen["d"])
        return g_xi, ops.intrinsics_grad(intr.phi.detach(), g_K, 16, 16, 22.0, intr.tie_focal)

    cam = CameraRefiner(ds)
    with torch.no_grad():
        cam.xi.copy_(PR.random_xi(3, 0.05, np.random.default_rng(0), tau=0.02))
    phi0 = IR.random_phi(3, np.random.default_rng(1), focal=0.05, centre=0.01)
    both = IntrinsicsRefiner(ds, per_view=True, tie_focal=False, learn_principal_point=True)
    set_phi(both, phi0)
    step(cam, both)  # (the first backward of a model in an fp16 mode calibrates its per-stage factors)
    index, seen = step(cam, both)
    g_xi, g_phi = direct(cam, both, index, seen)
    assert torch.equal(cam.xi.grad, g_xi) and torch.equal(both.phi.grad, g_phi)
    assert all(float(g.abs().max()) > 0 for g in (g_xi[:, :3], g_xi[:, 3:], g_phi[:, :2], g_phi[:, 2:]))
    assert bool(torch.isfinite(g_xi).all()) and bool(torch.isfinite(g_phi).all())
    # intrinsics alone, shared and tied (the defaults): phi.grad[:, 1] and the principal point's half are exactly 0
    alone = IntrinsicsRefiner(ds)
    set_phi(alone, phi0[:1])
    index, seen = step(None, alone)
    _, g_phi = direct(None, alone, index, seen)
    assert alone.phi.grad.shape == (1, 4) and torch.equal(alone.phi.grad[:, 0], g_phi[:, 0]) and float(g_phi[:, 0].abs()) > 0
    assert not bool(alone.phi.grad[:, 1:].any()) and not bool(g_phi[:, 1].any()) and float(g_phi[:, 2:].abs().max()) > 0
    # the focal fixed, the principal point free
    pp = IntrinsicsRefiner(ds, per_view=True, tie_focal=False, learn_focal=False, learn_principal_point=True)
    set_phi(pp, phi0)
    index, seen = step(cam, pp)
    g_xi, g_phi = direct(cam, pp, index, seen)
    assert torch.equal(cam.xi.grad, g_xi) and not bool(pp.phi.grad[:, :2].any()) and float(g_phi[:, :2].abs().max()) > 0
    assert torch.equal(pp.phi.grad[:, 2:], g_phi[:, 2:])


# ---------------------------------------------------------------- recovery
def recovery_dataset(dev, poses, ndc):
    imgs = np.zeros((TC.REC_VIEWS, TC.REC_H, TC.REC_W, 3), np.uint8)
    return RayDataset(imgs, poses, (TC.REC_H, TC.REC_W, TC.REC_FOCAL), near=0.0, far=1.0, ndc=ndc, device=dev)


def run_adam(loader, params, to, td):
    opt = torch.optim.Adam(params, lr=1e-2)
    for _ in range(TC.REC_STEPS):
        o, d, _, idx = next(iter(loader))
        opt.zero_grad()
        TC.ray_loss(o, d, to[idx], td[idx]).backward()
        opt.step()


@pytest.mark.parametrize("per_view", [False, True])
@pytest.mark.parametrize("ndc", [False, True])
def test_adam_through_the_loader_recovers_the_intrinsics(dev, ndc, per_view):
    """No network: the loss is the summed squared error of o and d between the loader's rays and the rays of phi*, every
    column free.  tests/test_intrinsics_cpu.py holds the float64 reference to the same bound (it reaches ~1e-7 x)."""
    poses, phi_star, index = TI.intrinsics_case(ndc, per_view)
    H_, W_, f0 = TC.REC_H, TC.REC_W, TC.REC_FOCAL
    to, td = (t.float().to(dev) for t in IR.rays(PR.poses12(poses).double(), IR.table(phi_star, H_, W_, f0, False), index,
                                                 H_, W_, f0, ndc))
    ds = recovery_dataset(dev, poses, ndc)
    intr = IntrinsicsRefiner(ds, per_view=per_view, tie_focal=False, learn_principal_point=True)
    run_adam(RayLoader(ds, len(ds), shuffle=True, seed=2, with_index=True, intrinsics=intr), [intr.phi], to, td)
    ratio = TI.relative_error(intr.phi, phi_star)
    print(f"ndc={ndc} per_view={per_view}: max |phi - phi*| = {ratio:.2e} x the largest target entry")
    assert ratio <= TC.REC_BOUND, ratio


@pytest.mark.parametrize("ndc", [False, True])
def test_adam_through_the_loader_recovers_pose_and_focal_jointly(dev, ndc):
    """xi* ~ 0.1 N with a shared tied focal off by exp(-0.15), the principal point fixed (the defaults)."""
    poses, xi_star, phi_star, index = TI.joint_case(ndc)
    H_, W_, f0 = TC.REC_H, TC.REC_W, TC.REC_FOCAL
    to, td = (t.float().to(dev) for t in IR.rays(PR.compose(PR.poses12(poses).double(), xi_star),
                                                 IR.table(phi_star, H_, W_, f0), index, H_, W_, f0, ndc))
    ds = recovery_dataset(dev, poses, ndc)
    cam, intr = CameraRefiner(ds), IntrinsicsRefiner(ds)
    run_adam(RayLoader(ds, len(ds), shuffle=True, seed=2, with_index=True, cameras=cam, intrinsics=intr),
             [cam.xi, intr.phi], to, td)
    r_xi, r_phi = TI.relative_error(cam.xi, xi_star), TI.relative_error(intr.phi[:, :1], phi_star[:, :1])
    print(f"joint, ndc={ndc}: xi {r_xi:.2e}, focal {r_phi:.2e} x the largest target entry after {TC.REC_STEPS} steps")
    assert not bool(intr.phi.detach()[:, 1:].any())
    assert r_xi <= TC.REC_BOUND and r_phi <= TC.REC_BOUND, (r_xi, r_phi)


# ---------------------------------------------------------------- debug build
def test_debug_build_reports_an_index_outside_the_dataset():
    rep = debug_lib.run_worker("intrinsics_debug_worker.py")
    assert rep["valid"] == [0, 0, 0, 0], f"valid indices were recorded: {rep['valid']} (count, line, index, N)"
    count, line, index, extent = rep["bad"]
    assert count == 2 and line > 0 and extent == rep["n_rays"] and index == rep["first_bad"], rep["bad"]
    assert rep["equal_without_the_entries"]
    debug_lib.assert_no_other_unit_recorded(rep)
