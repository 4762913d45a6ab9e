"""GPU: depth-warp sampling (csrc/warp.hip: fsn_warp_sample_fwd / _bwd) through ops.warp_sample, nerfdata.WarpSource
and core.loss.WarpConsistencyLoss, against the restatements of tests/warp_ref.py.

Forward: colour, valid and uvz are the float32 NumPy restatement's bit for bit (uvz stores a NaN as the canonical quiet
NaN, so that holds for the rows with a NaN or infinite depth too).  Gradients: within 2e-4 of the float64 reference,
relative to the tensor's largest entry (test_train_step._rel, the project's gradient bar for this family); the tests
print the kernel's figure and the float32 restatement's beside it.  Shapes: warp_ref.CASES.

Measured on the MI355X (the tests print the figures; DESIGN.md 6.1, "Depth-warp consistency"): forward bit for bit on
every shape; d_depth <= 2.0e-6, d_rays_o <= 6.3e-6, d_rays_d <= 4.5e-6, each equal to the float32 restatement's figure
to the digits printed; loss values within 5.7e-8, loss gradients within 4.1e-6; depth recovery 1.722e-2 (float64
1.722e-2, bound 3.46e-2)."""
import functools

import numpy as np
import pytest
import torch

import fs_nerf_amd  # noqa: F401

import debug_lib
import warp_ref as R
from test_train_step import _rel

TOL_GRAD, TOL_LOSS = 2e-4, 1e-5
GRADS = ("d_depth", "d_rays_o", "d_rays_d")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _bits_zero(t):
    return bool((_bits(t) == 0).all())


@functools.lru_cache(maxsize=None)
def _setup(shape):
    """the case, its cotangent and both restatements: built once per shape, never modified"""
    case = R.make_case(*shape, seed=11)
    g = np.random.default_rng(3).standard_normal((shape[0], 3)).astype(np.float32)
    r32 = R.warp_f32(case["o"], case["d"], case["t"], case["s"], case["poses"], case["images"], case["K"],
                     case["white_bkgd"], 1e-3, case["border"], g=g)
    return case, g, r32, R.grads_f64(case, g)


def _run(case, g, need=(True, True, True), want_uvz=True):
    """ops.warp_sample on the case, backward under g -> (colour, valid, uvz, {gradient name: tensor or None})"""
    from fs_nerf_amd import ops
    dev = torch.device("cuda:0")
    o, d, t, s, poses, images, K = R.case_tensors(case, dev)
    for x, flag in zip((t, o, d), need):
        x.requires_grad_(flag)
    colour, valid, uvz = ops.warp_sample(o, d, t, s, poses, images, K, white_bkgd=case["white_bkgd"], border=case["border"],
                                         want_uvz=want_uvz)
    if any(need):
        colour.backward(torch.as_tensor(g).to(dev))
    return colour, valid, uvz, dict(zip(GRADS, (t.grad, o.grad, d.grad)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.CASES)
def test_forward_bits_gradients_and_determinism(shape):
    """Measured on the MI355X: see the module docstring's pointer; figures are printed per shape."""
    case, g, r32, r64 = _setup(shape)
    colour, valid, uvz, grads = _run(case, g)
    assert valid.dtype == torch.bool and not valid.requires_grad and not uvz.requires_grad
    assert np.array_equal(valid.cpu().numpy(), r32["valid"])
    assert np.array_equal(_bits(colour).numpy(), r32["colour"].view(np.int32)), "colour is not the restatement's bit for bit"
    assert np.array_equal(_bits(uvz).numpy(), r32["uvz"].view(np.int32)), "uvz is not the restatement's bit for bit"
    bad = torch.as_tensor(~r32["valid"])
    for name in GRADS:
        got = grads[name].cpu()
        fig, fig32 = _rel(got, r64[name]), _rel(torch.as_tensor(r32[name]), r64[name])
        print(f"warp {shape} {name}: kernel {fig:.2e}, float32 restatement {fig32:.2e} (bar {TOL_GRAD:.0e})")
        assert fig <= TOL_GRAD, (name, fig)
        assert _bits_zero(got[bad]), f"{name}: an invalid row's gradient is not exactly 0"
        assert torch.isfinite(got).all()
    assert _bits_zero(colour.cpu()[bad])
    # two calls are equal bit for bit
    colour2, valid2, uvz2, grads2 = _run(case, g)
    assert torch.equal(_bits(colour), _bits(colour2)) and torch.equal(valid, valid2) and torch.equal(_bits(uvz), _bits(uvz2))
    assert all(torch.equal(_bits(grads[k]), _bits(grads2[k])) for k in GRADS)
    # only the depth asks for a gradient: the other pointers are NULL, the depth's bits are the same; no uvz: None
    colour3, _, uvz3, grads3 = _run(case, g, need=(True, False, False), want_uvz=False)
    assert uvz3 is None and grads3["d_rays_o"] is None and grads3["d_rays_d"] is None
    assert torch.equal(_bits(grads3["d_depth"]), _bits(grads["d_depth"])) and torch.equal(_bits(colour3), _bits(colour))
    _, _, _, grads4 = _run(case, g, need=(False, True, True))
    assert grads4["d_depth"] is None and all(torch.equal(_bits(grads4[k]), _bits(grads[k])) for k in GRADS[1:])


@pytest.mark.gpu
def test_cotangent_on_green_leaves_a_pure_red_image_alone():
    """Images whose green and blue bytes are 0 (the red ones vary): a cotangent on colour[:, 1] alone gives d_depth = 0
    exactly - no channel leaks into another's slope."""
    case, _, _, _ = _setup(R.CASES[2])
    red = dict(case)
    red["images"] = case["images"].copy()
    red["images"][..., 1:3] = 0
    g = np.zeros((len(case["t"]), 3), dtype=np.float32)
    g[:, 1] = 1.0
    colour, valid, _, grads = _run(red, g)
    colour = colour.detach()
    assert valid.any() and float(colour[:, 0].abs().max()) > 0 and float(colour[:, 1:].abs().max()) == 0.0
    assert all(bool((grads[k] == 0).all()) for k in GRADS)
    g[:, 0] = 1.0  # ... and the red channel does move the depth
    assert float(_run(red, g)[3]["d_depth"].abs().max()) > 0


@pytest.mark.gpu
def test_integer_coordinates_return_the_pixel_itself():
    """An axis-aligned camera at the origin (R = I, fx = fy = 4, cx = 4, cy = 2 on 4 x 8 images) and points (x, y, -2)
    with x, y multiples of 0.5: u = 4 + 2x and v = 2 - 2y are exact in float32.  u on an integer (fu = 0) returns pixel
    (v, u) bit for bit; u = W - 1 exactly takes the cell x0 = W - 2 with fu = 1 and returns pixel W - 1, and v = H - 1
    likewise.  The bytes are drawn from [128, 255]: c00 + 1 * (c10 - c00) is c10 bit for bit when the difference is
    exact, which it is for two floats within a factor of two of each other (Sterbenz)."""
    from fs_nerf_amd import ops
    dev = torch.device("cuda:0")
    H, W = 4, 8
    images = torch.as_tensor(np.random.default_rng(2).integers(128, 256, (1, H, W, 3), dtype=np.uint8))
    us, vs = np.meshgrid(np.arange(W), np.arange(H))
    us, vs = us.reshape(-1), vs.reshape(-1)
    n = us.size
    o = torch.tensor(np.stack([(us - 4) / 2.0, (2 - vs) / 2.0, np.zeros(n)], 1), dtype=torch.float32)
    d = torch.tensor([[0.0, 0.0, -1.0]]).repeat(n, 1)
    t = torch.full((n,), 2.0)
    poses = torch.eye(4)[:3].reshape(1, 12).contiguous()
    K = torch.tensor([[4.0, 4.0, 4.0, 2.0]])
    colour, valid, uvz = ops.warp_sample(o.to(dev), d.to(dev), t.to(dev), torch.zeros(n, dtype=torch.int64, device=dev),
                                         poses.to(dev), images.to(dev), K.to(dev), border=0.0, want_uvz=True)
    assert valid.all()
    assert torch.equal(uvz.cpu(), torch.tensor(np.stack([us, vs, np.full(n, 2.0)], 1), dtype=torch.float32))
    want = images[0, vs, us].to(torch.float32) / 255.0
    assert torch.equal(_bits(colour), _bits(want))
    # half a pixel further out the row is invalid under border = 0
    out = ops.warp_sample((o + torch.tensor([0.25, 0.0, 0.0])).to(dev), d.to(dev), t.to(dev),
                          torch.zeros(n, dtype=torch.int64, device=dev), poses.to(dev), images.to(dev), K.to(dev))
    assert out[2] is None and out[1].cpu().tolist() == (us + 0.5 <= W - 1).tolist()


@pytest.mark.gpu
def test_no_rows_and_argument_errors():
    from fs_nerf_amd import ops
    dev = torch.device("cuda:0")
    case = _setup(R.CASES[1])[0]
    o, d, t, s, poses, images, K = R.case_tensors(case, dev)
    e3, e1 = torch.empty(0, 3, device=dev, requires_grad=True), torch.empty(0, device=dev, requires_grad=True)
    colour, valid, uvz = ops.warp_sample(e3, e3, e1, s[:0], poses, images, K, white_bkgd=True, want_uvz=True)
    assert colour.shape == (0, 3) and valid.shape == (0,) and valid.dtype == torch.bool and uvz.shape == (0, 3)
    colour.sum().backward()
    assert e1.grad.shape == (0,) and e3.grad.shape == (0, 3)
    with pytest.raises(TypeError, match="rays_o"):
        ops.warp_sample(o.double(), d, t, s, poses, images, K)
    with pytest.raises(ValueError, match="rays_o and rays_d"):
        ops.warp_sample(o[:-1], d, t, s, poses, images, K)
    with pytest.raises(ValueError, match="src_view"):
        ops.warp_sample(o, d, t, s[:-1], poses, images, K)
    with pytest.raises(TypeError, match="src_view"):
        ops.warp_sample(o, d, t, s.float(), poses, images, K)
    with pytest.raises(TypeError, match="images"):
        ops.warp_sample(o, d, t, s, poses, images.float(), K)
    with pytest.raises(ValueError, match="camera table"):
        ops.warp_sample(o, d, t, s, poses, images, K[:2])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.warp_sample(o.cpu(), d, t, s, poses, images, K)
    with pytest.raises(RuntimeError, match="border"):
        ops.warp_sample(o, d, t, s, poses, images, K, border=-1.0)
    with pytest.raises(RuntimeError, match="white_bkgd"):
        ops.warp_sample(o, d, t, s, poses, images[..., :3].contiguous(), K, white_bkgd=True)


def _source(case, dev):
    """nerfdata.WarpSource over a RayDataset of the case's images and poses (the case's K through a stand-in refiner)."""
    from fs_nerf_amd.nerfdata import RayDataset, WarpSource
    V, H, W, _ = case["images"].shape
    ds = RayDataset(case["images"], case["poses"].reshape(V, 3, 4), (H, W, float(case["K"][0, 0])), near=1.0, far=8.0,
                    white_bkgd=case["white_bkgd"], device=dev)
    table = torch.as_tensor(case["K"]).to(dev)

    class Table:
        def K(self):
            return table
    return WarpSource(ds, intrinsics=Table())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["l1", "l2"])
@pytest.mark.parametrize("threshold", [None, 0.5])
def test_consistency_loss_against_float64(kind, threshold):
    """Value within 1e-5 and gradients (rgb, depth, rays_o, rays_d) within 2e-4 of the float64 restatement; a row that is
    invalid, or masked by the opacity threshold, has gradient bits all zero."""
    from fs_nerf_amd.core.loss import WarpConsistencyLoss
    dev = torch.device("cuda:0")
    case = _setup(R.CASES[4])[0]
    n = len(case["t"])
    gen = torch.Generator().manual_seed(17)
    rgb, opacity = torch.rand(n, 3, generator=gen), torch.rand(n, generator=gen)
    o, d, t, s, _, _, _ = R.case_tensors(case, dev)
    leaves = [x.requires_grad_() for x in (rgb.to(dev), t, o, d)]
    loss = WarpConsistencyLoss(kind, threshold=threshold, border=case["border"])
    val = loss(leaves[0], t, o, d, s, _source(case, dev), opacity=opacity.to(dev) if threshold is not None else None)
    val.backward()
    ref_leaves = [torch.as_tensor(x).double().requires_grad_() for x in (rgb, case["t"], case["o"], case["d"])]
    ref = R.loss_f64(*ref_leaves, case["s"], case["poses"], case["images"], case["K"], case["white_bkgd"], kind=kind,
                     threshold=threshold, border=case["border"], opacity=opacity.double())
    ref.backward()
    dead = torch.as_tensor([k != "valid" for k in case["kind"]])
    if threshold is not None:
        dead = dead | ~(opacity > threshold)
    assert 0 < int(dead.sum()) < n
    val, ref = val.detach(), ref.detach()
    fig =abs(float(val) - float(ref)) / abs(float(ref))
    print(f"warp loss {kind} threshold {threshold}: value {float(val):.6f} (float64 {float(ref):.6f}, off by {fig:.2e})")
    assert val.dim() == 0 and fig <= TOL_LOSS
    for name, x, x64 in zip(("rgb", "depth", "rays_o", "rays_d"), leaves, ref_leaves):
        fig = _rel(x.grad, x64.grad)
        print(f"warp loss {kind} threshold {threshold} d_{name}: {fig:.2e} (bar {TOL_GRAD:.0e})")
        assert fig <= TOL_GRAD, (name, fig)
        assert _bits_zero(x.grad.cpu()[dead]), name


@pytest.mark.gpu
def test_consistency_loss_of_an_all_invalid_batch():
    from fs_nerf_amd.core.loss import WarpConsistencyLoss
    dev = torch.device("cuda:0")
    case = _setup(R.CASES[3])[0]
    o, d, t, s, _, _, _ = R.case_tensors(case, dev)
    leaves = [x.requires_grad_() for x in (torch.rand(len(case["t"]), 3, device=dev), t, o, d)]
    val = WarpConsistencyLoss("l1")(leaves[0], t, o, d, torch.full_like(s, -1), _source(case, dev))
    val.backward()
    assert float(val) == 0.0 and all(_bits_zero(x.grad) for x in leaves)


@pytest.mark.gpu
def test_depth_recovery_end_to_end():
    """warp_ref.plane_scene through RayDataset, WarpSource.other_views and WarpConsistencyLoss("l2"): Adam on a per-ray
    depth recovers the plane to within warp_ref.E2E_BOUND = 2 x the float64 restatement's figure for the same schedule
    (1.73e-2 after 150 steps from 0.1; tests/test_warp_cpu.py::test_depth_recovery_f64)."""
    from fs_nerf_amd.core.loss import WarpConsistencyLoss
    from fs_nerf_amd.nerfdata import RayDataset, WarpSource
    dev = torch.device("cuda:0")
    scene = R.plane_scene()
    ds = RayDataset(scene["images"], scene["poses"], scene["hwf"], near=2.0, far=6.0, device=dev)
    src = WarpSource(ds)
    H, W, _ = scene["hwf"]
    o, d, rgb, index = ds.batch("identity", start=0, count=H * W, want_index=True)  # view 0's rays and its photograph
    assert torch.equal(o.cpu(), torch.as_tensor(scene["o"])) and float((d.cpu() - torch.as_tensor(scene["d"])).abs().max()) < 1e-6
    view = torch.div(index, H * W, rounding_mode="floor")
    src_view = src.other_views(1)[view, 0]
    assert torch.equal(src_view.cpu(), torch.as_tensor(scene["src"]))
    depth = torch.as_tensor(scene["t0"]).to(dev).requires_grad_()
    opt = torch.optim.Adam([depth], lr=R.E2E_LR)
    loss = WarpConsistencyLoss("l2", border=0.5)
    for _ in range(R.E2E_STEPS):
        opt.zero_grad()
        loss(rgb, depth, o, d, src_view, src).backward()
        opt.step()
    t = torch.as_tensor(scene["t"]).double()
    err = float(((depth.detach().cpu().double() - t).abs() / t)[torch.as_tensor(scene["interior"])].max())
    print(f"warp depth recovery on the GPU: 1.0e-01 -> {err:.3e} after {R.E2E_STEPS} steps (float64 {R.E2E_F64_ERR:.3e}, "
          f"bound {R.E2E_BOUND:.3e})")
    assert err <= R.E2E_BOUND


@pytest.mark.gpu
def test_debug_build_records_a_bad_source_view_and_nothing_else():
    rep = debug_lib.run_worker("warp_debug_worker.py")
    assert rep["valid"] == [0, 0, 0, 0], f"the warp kernels noted something on valid rows: {rep['valid']}"
    count, _line, first, extent = rep["bad"]
    assert (count, first, extent) == (2, rep["first_bad"], rep["n_views"]), rep["bad"]
    assert rep["bad_rows_zero"] and rep["good_rows_equal"]  # an invalid row's outputs are zeros; it reads no image byte
    debug_lib.assert_no_other_unit_recorded(rep)
