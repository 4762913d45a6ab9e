"""CPU: the depth-warp operator's restatements (tests/warp_ref.py) against an independent spelling through
F.grid_sample, the float32 restatement against the float64 one, the invalid rows, the argument checks of the two entry
points (no launch is made), WarpSource's host side, and the float64 depth-recovery run whose figure bounds the GPU's."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L
from fs_nerf_amd.core.loss import WarpConsistencyLoss
from fs_nerf_amd.nerfdata import WarpSource

import warp_ref as R

CASES = R.CASES


def rel(a, b):
    """tests/test_train_step._rel: the largest difference relative to the reference tensor's largest entry."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if a.size else 0.0


def grid_sample_spelling(case, g):
    """The spelling a user writes today, in float64: float image tables, projection with matrix products,
    F.grid_sample(mode="bilinear", align_corners=True), autograd -> (colour, d_depth, d_rays_o, d_rays_d) on the rows
    that are valid (the validity itself is warp_f64's)."""
    o, d, t = (torch.as_tensor(case[k]).double().requires_grad_() for k in ("o", "d", "t"))
    s = torch.as_tensor(case["s"])
    V, H, W, _ = case["images"].shape
    tab = R._tables_f64(case["images"], case["white_bkgd"]).permute(0, 3, 1, 2)  # [V,3,H,W]
    with torch.no_grad():
        _, valid, _ = R.warp_f64(o, d, t, s, case["poses"], case["images"], case["K"], case["white_bkgd"], 1e-3,
                                 case["border"])
    c2w = torch.as_tensor(case["poses"]).double().view(V, 3, 4)
    K = torch.as_tensor(case["K"]).double()
    colour = torch.zeros(len(s), 3, dtype=torch.float64)
    for view in range(V):
        rows = torch.nonzero(valid & (s == view)).reshape(-1)
        if rows.numel() == 0:
            continue
        X = o[rows] + t[rows, None] * d[rows]
        cam = (X - c2w[view, :, 3]) @ c2w[view, :, :3]  # world -> camera
        fx, fy, cx, cy = K[view if K.shape[0] > 1 else 0]
        px = cx + fx * cam[:, 0] / -cam[:, 2]
        py = cy - fy * cam[:, 1] / -cam[:, 2]
        grid = torch.stack([2.0 * px / (W - 1) - 1.0, 2.0 * py / (H - 1) - 1.0], -1).view(1, 1, -1, 2)
        out = F.grid_sample(tab[view:view + 1], grid, mode="bilinear", padding_mode="border", align_corners=True)
        colour = colour.index_put((rows,), out[0, :, 0, :].T)
    go, gd, gt = torch.autograd.grad(colour, (o, d, t), torch.as_tensor(g).double())
    return colour.detach(), torch.nan_to_num(gt), torch.nan_to_num(go), torch.nan_to_num(gd)


@pytest.mark.parametrize("shape", CASES)
def test_f64_restatement_is_the_grid_sample_spelling(shape):
    case = R.make_case(*shape, seed=11)
    g = np.random.default_rng(3).standard_normal((shape[0], 3))
    ref = R.grads_f64(case, g)
    colour, gt, go, gd = grid_sample_spelling(case, g)
    for name, a, b in (("colour", ref["colour"], colour), ("d_depth", ref["d_depth"], gt), ("d_rays_o", ref["d_rays_o"], go),
                       ("d_rays_d", ref["d_rays_d"], gd)):
        err = float((a - b).abs().max())
        assert err <= 1e-10 * max(1.0, float(b.abs().max())), (name, err)


@pytest.mark.parametrize("shape", CASES)
def test_f32_restatement_against_f64(shape):
    """The float32 restatement's own error: colour within 1e-5 (absolute; colours are in [0, 1]), gradients within the
    project's bar for this family, 2e-4 of the tensor's largest entry.  The printed figures are what the GPU tests
    quote next to the kernel's."""
    case = R.make_case(*shape, seed=11)
    g = np.random.default_rng(3).standard_normal((shape[0], 3)).astype(np.float32)
    r32 = R.warp_f32(case["o"], case["d"], case["t"], case["s"], case["poses"], case["images"], case["K"],
                     case["white_bkgd"], 1e-3, case["border"], g=g)
    ref = R.grads_f64(case, g)
    assert np.array_equal(r32["valid"], ref["valid"].numpy())
    err_c = float(np.abs(r32["colour"] - ref["colour"].numpy()).max())
    figs = {k: rel(r32[k], ref[k].numpy()) for k in ("d_depth", "d_rays_o", "d_rays_d")}
    print(f"warp f32 restatement vs f64 {shape}: colour {err_c:.2e} " + " ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    assert err_c <= 1e-5
    assert all(v <= 2e-4 for v in figs.values()), figs


def test_invalid_rows_give_zeros():
    case = R.make_case(65, 3, 5, 7, 4, True, True, 0.5, seed=5)
    g = np.ones((65, 3), dtype=np.float32)
    r32 = R.warp_f32(case["o"], case["d"], case["t"], case["s"], case["poses"], case["images"], case["K"], True, 1e-3, 0.5, g=g)
    ref = R.grads_f64(case, g)
    bad = np.array([k != "valid" for k in case["kind"]])
    assert bad.sum() == R.N_INVALID and not r32["valid"][bad].any() and r32["valid"][~bad].all()
    for k in ("colour", "d_depth", "d_rays_o", "d_rays_d"):
        assert not r32[k][bad].view(np.int32).any(), k          # bits all zero
        assert not ref[k].numpy()[bad].any(), k
        assert np.isfinite(r32[k]).all(), k
    # uvz: zeros where the view is out of range, the projection (a NaN for a NaN depth) elsewhere
    out_of_range = np.array([k in ("s=-1", "s=V") for k in case["kind"]])
    assert not r32["uvz"][out_of_range].view(np.int32).any()
    nan_row = case["kind"].index("t=nan")
    assert (r32["uvz"][nan_row].view(np.int32) == 0x7FC00000).all()


def _stub_dataset(V, ndc=False, centres=None):
    H, W = 4, 6
    poses = torch.eye(4).repeat(V, 1, 1)
    if centres is not None:
        poses[:, :3, 3] = torch.as_tensor(centres, dtype=torch.float32)
    return types.SimpleNamespace(ndc=ndc, imgs=torch.zeros(V, H, W, 3, dtype=torch.uint8), white_bkgd=False,
                                 hwf=(H, W, 5.0), device=torch.device("cpu"), poses=poses,
                                 poses12=poses[:, :3, :4].reshape(-1, 12).contiguous())


def test_warp_source_refuses_ndc():
    with pytest.raises(ValueError, match="metric depth"):
        WarpSource(_stub_dataset(3, ndc=True))


def test_other_views_exclude_the_view_itself():
    centres = [[0, 0, 0], [1, 0, 0], [3, 0, 0], [3.5, 0, 0]]
    src = WarpSource(_stub_dataset(4, centres=centres))
    assert src.other_views(1).reshape(-1).tolist() == [1, 0, 3, 2]
    two = src.other_views(2)
    assert two.tolist() == [[1, 2], [0, 2], [3, 1], [2, 1]] and two.dtype == torch.int64
    assert all(v not in row for v, row in enumerate(src.other_views(3).tolist()))
    assert src.other_views(5)[:, 3:].eq(-1).all() and src.other_views(5)[:, :3].ge(0).all()
    assert WarpSource(_stub_dataset(1)).other_views(2).tolist() == [[-1, -1]]
    assert src.other_views(1) is src.other_views(1)  # computed once
    # nearest_views: the nearest CURRENT centre for any query pose; the stored K is the ray batch's
    q = torch.eye(4)[:3].reshape(1, 12).repeat(2, 1)
    q[0, 3], q[1, 3] = 2.9, 0.4
    assert src.nearest_views(q).tolist() == [2, 0]
    assert src.K().tolist() == [[5.0, 5.0, 3.0, 2.0]] and src.poses12() is src.dataset.poses12
    with pytest.raises(ValueError):
        src.other_views(0)


def test_loss_refuses_what_it_cannot_do():
    with pytest.raises(ValueError, match="l1"):
        WarpConsistencyLoss(kind="huber")
    loss = WarpConsistencyLoss(threshold=0.5)
    with pytest.raises(ValueError, match="opacity"):
        loss(torch.zeros(2, 3), torch.ones(2), torch.zeros(2, 3), torch.ones(2, 3), torch.zeros(2, dtype=torch.int64), None)


def test_entry_points_validate_without_gpu():
    """FSN_E_INVALID with a message, before any device work; n = 0 is not an error."""
    lib = L.lib()
    assert {"fsn_warp_sample_fwd", "fsn_warp_sample_bwd"} <= set(L.FUNCTIONS)
    assert [p.name for p in L.FUNCTIONS["fsn_warp_sample_fwd"][1]][-4:] == ["colour", "valid", "uvz", "stream"]
    assert L.FUNCTIONS["fsn_warp_sample_fwd"][1][-3].pointee == "uint8_t"
    p = C.c_void_p(256)  # never dereferenced: every call below is refused, or has nothing to do

    def fwd(n=4, V=2, H=4, W=4, Cn=4, white=0, m=1, z_min=1e-3, border=0.0, ptr=p, out=p):
        return lib.fsn_warp_sample_fwd(ptr, ptr, ptr, ptr, n, ptr, V, ptr, H, W, Cn, white, ptr, m, z_min, border, out, out,
                                       None, None)

    def bwd(n=4, V=2, H=4, W=4, Cn=4, white=0, m=1, z_min=1e-3, border=0.0, ptr=p, g=p):
        return lib.fsn_warp_sample_bwd(ptr, ptr, ptr, ptr, n, ptr, V, ptr, H, W, Cn, white, ptr, m, z_min, border, g, None,
                                       None, None, None)

    for call in (fwd, bwd):
        for kw, text in ((dict(Cn=5), b"channels"), (dict(Cn=3, white=1), b"white_bkgd"), (dict(H=1), b"H, W >= 2"),
                         (dict(W=1), b"H, W >= 2"), (dict(m=3), b"camera table"), (dict(z_min=0.0), b"z_min"),
                         (dict(z_min=float("nan")), b"z_min"), (dict(border=-0.5), b"border"), (dict(ptr=None), b"null"),
                         (dict(n=-1), b"negative")):
            assert call(**kw) == L.FSN_E_INVALID, kw
            assert text in lib.fsn_last_error(), (kw, lib.fsn_last_error())
        assert call(n=0, ptr=None) == 0
    assert fwd(out=None) == L.FSN_E_INVALID and b"null colour" in lib.fsn_last_error()
    assert bwd(g=None) == L.FSN_E_INVALID and b"null d_colour" in lib.fsn_last_error()
    assert bwd() == 0  # no gradient wanted: nothing is launched
    assert lib.fsn_warp_sample_fwd(p, p, p, p, 4, p, 2, C.c_void_p(258), 4, 4, 4, 0, p, 1, 1e-3, 0.0, p, p, None,
                                   None) == L.FSN_E_INVALID and b"aligned" in lib.fsn_last_error()


def test_depth_recovery_f64():
    """The end-to-end scene on the float64 restatement: the figure E2E_F64_ERR next to the GPU test's bound."""
    scene = R.plane_scene()
    assert scene["interior"].sum() >= 300
    t, t0 = scene["t"].astype(np.float64), scene["t0"].astype(np.float64)
    start = float((np.abs(t0 - t) / t)[scene["interior"]].max())
    err = R.recover_f64(scene)
    print(f"warp depth recovery, float64: start {start:.3e} -> {err:.3e} after {R.E2E_STEPS} steps "
          f"(recorded {R.E2E_F64_ERR:.3e}, GPU bound {R.E2E_BOUND:.3e})")
    assert 0.099 < start < 0.101
    assert err <= R.E2E_F64_ERR, (err, R.E2E_F64_ERR)
    assert R.E2E_BOUND == 2.0 * R.E2E_F64_ERR and R.E2E_BOUND < 0.05  # well inside the start's 0.1: the depth is recovered
