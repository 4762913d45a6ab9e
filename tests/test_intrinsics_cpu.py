"""CPU: the learnable-intrinsics layer's C-ABI (declared, bound, exported; argument validation without a device), the
documented errors of IntrinsicsRefiner and the loaders, and the float64 restatement of tests/intrinsics_ref.py recovering
known intrinsics - alone, and jointly with a pose correction - by the recipe of tests/test_pose_refine_cpu.py (the bound
the GPU test holds the loaders to)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L

import intrinsics_ref as IR
import pose_refine_ref as PR
import test_pose_refine_cpu as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("fsn_intrinsics_compose", "fsn_ray_batch_k", "fsn_ray_patch_batch_k", "fsn_ray_camera_grad",
           "fsn_intrinsics_grad")


def test_the_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "fsnerf_hip.h")).read()
    lib = L.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in L.SIGNATURES, name
        assert hasattr(lib, name), name
    from fs_nerf_amd import nerfdata, ops
    assert all(callable(f) for f in (ops.intrinsics_compose, ops.ray_camera_grad, ops.intrinsics_grad))
    assert nerfdata.IntrinsicsRefiner is not None


def test_argument_validation_without_gpu():
    lib = L.lib()
    p = C.c_void_p(64)  # never dereferenced: every call below is refused (or is empty) before any HIP call

    def compose(phi=p, m=3, H=8, W=8, focal0=10.0, out=p):
        return lib.fsn_intrinsics_compose(phi, m, H, W, focal0, 1, out, None)

    assert compose(phi=None) == -1 and b"fsn_intrinsics_compose" in lib.fsn_last_error()
    assert compose(out=None) == -1 and compose(m=-1) == -1 and compose(H=0) == -1 and compose(W=-2) == -1
    assert compose(focal0=0.0) == -1 and compose(focal0=-1.0) == -1
    assert compose(m=0) == 0  # no row: nothing to do

    def grad(poses0=p, xi=p, n=3, H=8, W=8, focal0=10.0, K=p, k_rows=1, index=p, count=5, grad_xi=p, grad_K=p):
        return lib.fsn_ray_camera_grad(poses0, xi, n, H, W, focal0, K, k_rows, 0, 1.0, index, p, p, count, grad_xi, grad_K,
                                       None)

    assert grad(poses0=None) == -1 and b"fsn_ray_camera_grad" in lib.fsn_last_error()
    assert grad(K=None) == -1 and grad(grad_K=None) == -1 and grad(index=None) == -1
    assert grad(n=-1) == -1 and grad(count=-1) == -1
    assert grad(H=0) == -1 and grad(W=0) == -1 and grad(focal0=0.0) == -1 and grad(focal0=-3.0) == -1
    assert grad(k_rows=2) == -1 and b"camera table" in lib.fsn_last_error()
    assert grad(k_rows=0) == -1 and grad(k_rows=-1) == -1 and grad(k_rows=4) == -1
    assert grad(H=1 << 16, W=1 << 16) == -2  # a view of 2^32 pixels: refused by name
    assert grad(n=0, k_rows=1) == 0 and grad(n=0, k_rows=0) == 0  # no view: nothing to write

    def chain(phi=p, gK=p, n=3, m=1, H=8, W=8, focal0=10.0, out=p):
        return lib.fsn_intrinsics_grad(phi, gK, n, m, H, W, focal0, 1, out, None)

    assert chain(phi=None) == -1 and b"fsn_intrinsics_grad" in lib.fsn_last_error()
    assert chain(gK=None) == -1 and chain(out=None) == -1
    assert chain(n=-1) == -1 and chain(m=2) == -1 and chain(m=0) == -1 and chain(m=-1) == -1
    assert chain(H=0) == -1 and chain(W=0) == -1 and chain(focal0=0.0) == -1
    assert chain(n=0, m=0) == 0  # per view, no view: nothing to write

    def batch(fn=lib.fsn_ray_batch_k, K=p, k_rows=1, n=3, focal=5.0, count=4, tail=()):
        return fn(p, n, p, 8, 8, 3, focal, K, k_rows, 0, 1.0, 0, 0, 0, 0, None, 0, count, *tail, p, p, p, None, None)

    for fn, tail, name in ((lib.fsn_ray_batch_k, (), b"fsn_ray_batch_k"), (lib.fsn_ray_patch_batch_k, (2, 1), b"fsn_ray_patch_batch_k")):
        assert batch(fn, K=None, tail=tail) == -1 and name in lib.fsn_last_error()
        assert batch(fn, k_rows=2, tail=tail) == -1 and b"camera table" in lib.fsn_last_error()
        assert batch(fn, k_rows=0, tail=tail) == -1 and batch(fn, k_rows=-3, tail=tail) == -1
        assert batch(fn, focal=0.0, tail=tail) == -1 and batch(fn, n=-1, k_rows=1, tail=tail) == -1
        assert batch(fn, count=-1, tail=tail) == -1 and name in lib.fsn_last_error()
        assert batch(fn, count=0, tail=tail) == 0 and batch(fn, count=0, k_rows=3, tail=tail) == 0  # empty: nothing to do


def test_the_host_layer_raises_the_documented_errors():
    from fs_nerf_amd import ops
    from fs_nerf_amd.nerfdata import IntrinsicsRefiner, PatchLoader, RayLoader
    z = torch.zeros(1, 4)
    with pytest.raises(RuntimeError):
        ops.intrinsics_compose(z, 8, 8, 10.0)
    with pytest.raises(RuntimeError):
        ops.intrinsics_grad(z, torch.zeros(3, 4), 8, 8, 10.0)
    with pytest.raises(RuntimeError):
        ops.ray_camera_grad(torch.zeros(3, 12), None, 8, 8, 10.0, z, torch.zeros(5, dtype=torch.int64), None, None)
    with pytest.raises(RuntimeError):
        ops.ray_camera_grad(torch.zeros(3, 12), torch.zeros(3, 6), 8, 8, 10.0, z, torch.zeros(5, dtype=torch.int64), None, None)
    with pytest.raises(RuntimeError):
        IntrinsicsRefiner((8, 8, 10.0), device="cpu")
    with pytest.raises(ValueError, match="per_view"):
        IntrinsicsRefiner((8, 8, 10.0), per_view=True)
    for hwf in ((8, 8), (0, 8, 10.0), (8, 8, 0.0), (8, -1, 10.0)):
        with pytest.raises(ValueError, match="hwf"):
            IntrinsicsRefiner(hwf)
    # the loaders refuse intrinsics of another view count, image size or device - before they touch the dataset
    cpu = torch.device("cpu")
    ds = types.SimpleNamespace(n_views=3, device=cpu, hwf=(8, 8, 10.0), n_anchors=lambda patch, dilation: 3 * 49)
    for bad in (types.SimpleNamespace(n_views=2, device=cpu, hwf0=(8, 8, 10.0)),
                types.SimpleNamespace(n_views=3, device=cpu, hwf0=(8, 9, 10.0)),
                types.SimpleNamespace(n_views=None, device=cpu, hwf0=(8, 8, 11.0)),
                types.SimpleNamespace(n_views=None, device=torch.device("meta"), hwf0=(8, 8, 10.0))):
        with pytest.raises(ValueError, match="intrinsics"):
            RayLoader(ds, 16, intrinsics=bad)
        with pytest.raises(ValueError, match="intrinsics"):
            PatchLoader(ds, 2, 4, intrinsics=bad)
    ok = types.SimpleNamespace(n_views=None, device=cpu, hwf0=(8, 8, 10.0))
    assert RayLoader(ds, 16, intrinsics=ok).intrinsics is ok and PatchLoader(ds, 2, 4, intrinsics=ok).intrinsics is ok


def test_zero_parameter_is_the_stored_intrinsics_and_the_restatements_agree():
    H, W, f0 = 5, 7, 10.0
    K0 = IR.table(torch.zeros(1, 4, dtype=torch.float32), H, W, f0)
    assert K0.tolist() == [[f0, f0, W * 0.5, H * 0.5]]
    rng = np.random.default_rng(0)
    P = PR.poses12(PR.forward_poses(3, seed=1))
    index = torch.arange(3 * H * W)
    for ndc in (False, True):
        # K = the stored intrinsics: the rays of pose_refine_ref, exactly
        a, b = IR.rays(P.double(), K0.double(), index, H, W, f0, ndc), PR.rays(P.double(), index, H, W, f0, ndc)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        # the NumPy float32 rows against the float64 torch restatement, shared and per-view tables
        for m in (1, 3):
            K = IR.table(IR.random_phi(m, rng), H, W, f0, tie_focal=False)
            o32, d32 = IR.rows_f32(P, K, index, H, W, f0, ndc)
            o64, d64 = IR.rays(P.double(), K.double(), index, H, W, f0, ndc)
            assert float(np.abs(o32 - o64.numpy()).max()) <= 1e-5 and float(np.abs(d32 - d64.numpy()).max()) <= 1e-5


# ---------------------------------------------------------------- recovery: the geometry of the GPU test
def intrinsics_case(ndc, per_view):
    """(stored poses [3,4,4] float32, phi* [m,4] float64: log focal factors ~ N(0, 0.1^2), principal-point offsets ~
    N(0, 0.03^2), all ray indices)."""
    rng = np.random.default_rng((21 if ndc else 22) + (2 if per_view else 0))
    poses = PR.forward_poses(TC.REC_VIEWS, seed=5) if ndc else PR.world_poses(TC.REC_VIEWS, seed=5)
    m = TC.REC_VIEWS if per_view else 1
    phi_star = torch.from_numpy(np.concatenate([rng.standard_normal((m, 2)) * 0.1, rng.standard_normal((m, 2)) * 0.03], 1))
    return poses, phi_star, torch.arange(TC.REC_VIEWS * TC.REC_H * TC.REC_W)


JOINT_PHI = -0.15


def joint_case(ndc):
    """test_pose_refine_cpu's case (xi* ~ 0.1 N) with a shared tied focal off by exp(-0.15), principal point fixed."""
    poses, xi_star, index = TC.recovery_case(ndc)
    return poses, xi_star, torch.tensor([[JOINT_PHI, 0.0, 0.0, 0.0]], dtype=torch.float64), index


def relative_error(got, want):
    return float((got.detach().cpu().double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("per_view", [False, True])
@pytest.mark.parametrize("ndc", [False, True])
def test_the_float64_reference_recovers_the_intrinsics(ndc, per_view):
    poses, phi_star, index = intrinsics_case(ndc, per_view)
    P0 = PR.poses12(poses).double()
    H, W, f0 = TC.REC_H, TC.REC_W, TC.REC_FOCAL
    to, td = IR.rays(P0, IR.table(phi_star, H, W, f0, False), index, H, W, f0, ndc)
    phi, = IR.recover(lambda x: TC.ray_loss(*IR.rays(P0, IR.table(x, H, W, f0, False), index, H, W, f0, ndc), to, td),
                      [torch.zeros_like(phi_star)], TC.REC_STEPS)
    ratio = relative_error(phi, phi_star)
    print(f"float64 reference, ndc={ndc} per_view={per_view}: max |phi - phi*| = {ratio:.2e} x the largest target entry")
    assert ratio <= TC.REC_BOUND, ratio


@pytest.mark.parametrize("ndc", [False, True])
def test_the_float64_reference_recovers_pose_and_focal_jointly(ndc):
    poses, xi_star, phi_star, index = joint_case(ndc)
    P0 = PR.poses12(poses).double()
    H, W, f0 = TC.REC_H, TC.REC_W, TC.REC_FOCAL
    to, td = IR.rays(PR.compose(P0, xi_star), IR.table(phi_star, H, W, f0), index, H, W, f0, ndc)

    def step(xi, phi):  # (the principal point is fixed: its columns stay out of the table)
        free = torch.cat([phi[:, :1], torch.zeros(1, 3, dtype=phi.dtype)], 1)
        return TC.ray_loss(*IR.rays(PR.compose(P0, xi), IR.table(free, H, W, f0), index, H, W, f0, ndc), to, td)

    xi, phi = IR.recover(step, [torch.zeros_like(xi_star), torch.zeros_like(phi_star)], TC.REC_STEPS)
    r_xi, r_phi = relative_error(xi, xi_star), relative_error(phi[:, :1], phi_star[:, :1])
    print(f"float64 reference, joint, ndc={ndc}: xi {r_xi:.2e}, focal {r_phi:.2e} x the largest target entry")
    assert r_xi <= TC.REC_BOUND and r_phi <= TC.REC_BOUND, (r_xi, r_phi)
