"""The rules every wrapper of fs_nerf_amd.ops obeys, checked through its public surface:
1. a launch goes to the CURRENT stream of the tensors' device (the handle is read inside that device's guard);
2. a tensor a conversion made (a float64 mask cast to float32, a non-contiguous `u` copied) stays alive until the call is
   enqueued - the outputs are allocated after it, and the caching allocator hands a dropped block to the next
   torch.empty of its size class;
3. a tensor goes through the door as it is and is checked there against the header's declaration of the parameter.
And the two measurement hooks (`ops.launch_timer`, `ops.clock_buffer`) that bench.py assigns from outside.

Shapes: a 4 x 128 network, 40 rays, 8 + 8 samples, a 16^3 all-occupied grid with step 0.1.  Forty rays on purpose:
colors is 480 bytes, opacity / depth 160 each - the allocator's 512-byte class, that of the 63-float pos_mask and the
40-float u, so a dropped temporary's block is the very next one handed out."""
import ctypes as C

import pytest
import torch

import test_occ_fused as TF

pytestmark = pytest.mark.gpu
R, S, NI, STEP = 40, 8, 8, 0.1
# symbols whose last pointer argument is an output, not a stream (include/fsnerf_hip.h)
NO_STREAM = {"fsn_debug_report", "fsn_ray_perm_host", "fsn_mlp_pack_host", "fsn_mlp_pack_scaled_host",
             "fsn_weight_stream_pack_host", "fsn_weight_norm_workspace_floats"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import fs_nerf_amd  # noqa: F401
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def scene(dev):
    """Model, packed blob, all-occupied grid and seeded inputs, made once (read-only for the tests)."""
    from fs_nerf_amd.render.occgrid import OccGridEstimator
    m = TF.make_model(4, 128, 4, dev, gain=2.0, shift=1.0)  # thin medium: the cull keeps samples on every ray
    est = OccGridEstimator(roi_aabb=torch.tensor(TF.AABB), resolution=16, levels=1).to(dev)
    est.set_binaries(torch.ones(1, 16, 16, 16, dtype=torch.bool))
    est.eval()
    o, d = TF.orbit_rays(R, 5)
    gen = torch.Generator().manual_seed(11)
    s = dict(m=m, pm=m.packed(), est=est, o=o.to(dev), d=d.to(dev), u=torch.rand(R, generator=gen).to(dev),
             u_fine=torch.rand(R, NI, generator=gen).to(dev), x=(torch.rand(R * S, 3, generator=gen) * 2 - 1).to(dev),
             dirs=torch.nn.functional.normalize(torch.randn(R * S, 3, generator=gen), dim=-1).to(dev),
             sig=torch.rand(R, S, generator=gen).to(dev), rgb=torch.rand(R, S, 3, generator=gen).to(dev),
             g4=torch.randn(R * S, 4, generator=gen).to(dev))
    s["occ"] = dict(aabb=est.aabb, res=est.resolution, levels=est.levels, bits=est.bits, near_plane=0.0, far_plane=1e10,
                    step=STEP, max_steps=est.max_steps(STEP))
    torch.cuda.synchronize()
    return s


class Recorder:
    """Stands in for the loaded library: forwards every fsn_* call and records (symbol, arguments)."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("fsn_"):
            return fn

        def rec(*args):
            self.calls.append((name, args))
            return fn(*args)
        return rec


def takes_stream(name):
    from fs_nerf_amd import _lib
    args = _lib.SIGNATURES[name][1]
    return bool(args) and args[-1] is C.c_void_p and name not in NO_STREAM


def recorded(monkeypatch):
    from fs_nerf_amd import _lib
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    return rec


def check_streams(rec, stream, expect):
    assert stream.cuda_stream != 0
    launches = [(n, a) for n, a in rec.calls if takes_stream(n)]
    assert expect <= {n for n, _ in launches}, f"not launched: {sorted(expect - {n for n, _ in launches})}"
    wrong = [n for n, a in launches if a[-1] != stream.cuda_stream]
    assert not wrong, f"launched on another stream than the current one: {wrong}"


def test_every_launch_goes_to_the_current_stream(dev, scene, monkeypatch):
    from fs_nerf_amd import ops
    from oracle import fsnerf_oracle as O
    s = scene
    m, pm, o, d, u, occ = s["m"], s["pm"], s["o"], s["d"], s["u"], s["occ"]
    desc = ops.make_desc(m.n_layers, m.d_hidden, m.skip, m.pos_encoder.freqs, m.dir_encoder.freqs)
    weights, biases = ops.sd_tensor_lists({k: v.detach() for k, v in m.state_dict().items()}, m.n_layers)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    occs, bits = torch.rand(16 ** 3, device=dev), occ["bits"].clone()
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    rec = recorded(monkeypatch)
    with torch.cuda.stream(side), torch.no_grad():
        # rays, sampling, compositing
        ops.get_rays(O.pose_from_spherical(4.0311289, 50.0, 10.0), 8, 5, 11.0, dev)
        edges = ops.stratified_edges(2.0, 6.0, S, R, u, dev)
        ops.composite(s["sig"], s["rgb"], edges[:, :-1], edges[:, 1:])
        ri, t0, t1 = ops.edges_to_packed(edges)
        sig, rgb = s["sig"].reshape(-1), s["rgb"].reshape(-1, 3)
        col, op, dep, ex = ops.composite_packed(sig, rgb, t0, t1, ri, R)
        ops.composite_packed_bwd(sig, rgb, t0, t1, ri, R, None, torch.ones_like(col), torch.ones_like(op))
        ops.composite_packed_bwd_full(sig, rgb, t0, t1, ri, R, None, torch.ones_like(col), None, opacity=op, depth=dep,
                                      d_depth=torch.ones_like(dep), d_weights=torch.ones_like(sig))
        # network: inference, one-launch render and sampler, training step
        ops.mlp_fwd(pm, s["x"], s["dirs"])
        kw = dict(near=2.0, far=6.0, n_samples=S, n_importance=NI, u=u, u_fine=s["u_fine"])
        ops.render_fused(None, pm, o, d, **kw)
        ops.sample_fused(pm, o, d, **kw)
        out, work = ops.nerf_train_fwd(desc, m.train_prec(), weights, biases, s["x"], s["dirs"], None, None, status=word)
        ops.nerf_train_bwd(desc, m.train_prec(), weights, work, out, s["g4"], status=word)
        # occupancy grid
        ops.occgrid_march(o, d, occ["aabb"], occ["res"], occ["levels"], occ["bits"], 0.0, 1e10, STEP, u, occ["max_steps"])
        ops.occ_sample_fused(pm, o, d, u=u, **occ)
        ops.render_occ_fused(pm, o, d, u=u, want_extras=True, **occ)
        ops.occgrid_update(occs, bits, torch.arange(0, 64, 2, device=dev), torch.rand(32, device=dev), 0.95,
                           torch.full((1,), 0.5, device=dev))
        # packed primitives, proposal sampler, metrics
        spans = ops.RaySpans(R * S, R, ray_indices=ri)
        ops.packed_scan_fwd(sig, spans, False, True)
        ops.accumulate_fwd(ex["weights"], None, spans)
        cdfs = torch.linspace(0.0, 1.0, S + 1, device=dev).repeat(R, 1)
        ops.importance_sample(cdfs.clone(), cdfs, NI, u)
        img = s["rgb"].reshape(1, 3, R, S)
        ops.psnr_nchw(img, img.flip(-1))
        ops.to8b(s["sig"])
    side.synchronize()
    check_streams(rec, side, {
        "fsn_get_rays", "fsn_stratified_edges", "fsn_composite_fwd", "fsn_edges_to_packed", "fsn_composite_packed_fwd",
        "fsn_composite_packed_bwd", "fsn_composite_packed_bwd_full", "fsn_mlp_fwd", "fsn_render_rays_fused",
        "fsn_nerf_train_fwd", "fsn_nerf_train_bwd", "fsn_occgrid_march_ex", "fsn_render_rays_occgrid_ex",
        "fsn_occ_gather_ex", "fsn_occgrid_update", "fsn_packed_scan_fwd", "fsn_accumulate_fwd", "fsn_importance_sample",
        "fsn_psnr", "fsn_to8b"})
    assert sum(n == "fsn_render_rays_fused" for n, _ in rec.calls) == 2  # render_fused and sample_fused
    assert sum(n == "fsn_render_rays_occgrid_ex" for n, _ in rec.calls) == 2  # the sampler and the extras mode
    assert sum(n == "fsn_occ_gather_ex" for n, _ in rec.calls) == 2, "every ray keeps samples: both gathers ran"


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second GPU")
def test_launch_goes_to_the_stream_of_the_tensors_device(monkeypatch):
    """Tensors on cuda:1 while cuda:0 is the current device: the handle must be cuda:1's current stream."""
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd import ops
    from oracle import fsnerf_oracle as O
    d1 = torch.device("cuda:1")
    gen = torch.Generator().manual_seed(3)
    sig, rgb, u = (torch.rand(*sh, generator=gen).to(d1) for sh in ((R, S), (R, S, 3), (R,)))
    side = torch.cuda.Stream(device=d1)
    torch.cuda.synchronize(d1)
    torch.cuda.set_device(0)
    rec = recorded(monkeypatch)
    with torch.cuda.stream(side):
        assert torch.cuda.current_device() == 0
        ops.get_rays(O.pose_from_spherical(4.0311289, 50.0, 10.0), 8, 5, 11.0, d1)
        edges = ops.stratified_edges(2.0, 6.0, S, R, u, d1)
        ops.composite(sig, rgb, edges[:, :-1], edges[:, 1:])
        ri, _, _ = ops.edges_to_packed(edges)
        ops.packed_scan_fwd(sig.reshape(-1), ops.RaySpans(R * S, R, ray_indices=ri), False, True)
        ops.psnr_nchw(rgb.reshape(1, 3, R, S), rgb.reshape(1, 3, R, S).flip(-1))
        ops.to8b(sig)
    side.synchronize()
    check_streams(rec, side, {"fsn_get_rays", "fsn_stratified_edges", "fsn_composite_fwd", "fsn_edges_to_packed",
                              "fsn_packed_scan_fwd", "fsn_psnr", "fsn_to8b"})


def tensors_of(ret):
    if isinstance(ret, torch.Tensor):
        return [ret]
    if isinstance(ret, dict):
        return [t for k in sorted(ret) for t in tensors_of(ret[k])]
    if isinstance(ret, (tuple, list)):
        return [t for r in ret for t in tensors_of(r)]
    return []


def strided(t):
    """The values of `t` as a non-contiguous float32 view (every second element of a longer buffer)."""
    buf = torch.zeros(t.numel() * 2, device=t.device, dtype=torch.float32)
    buf[::2] = t.reshape(-1)
    v = buf[::2]
    assert not v.is_contiguous()
    return v


@pytest.mark.parametrize("fn", ["render_fused", "sample_fused", "occ_sample_fused", "render_occ_fused", "render_occ_fused-extras"])
def test_converted_arguments_outlive_the_launch(dev, scene, fn):
    """Masks, jitter and bounds handed in as float64 or as non-contiguous views (the wrapper converts: a temporary) give
    the tensors of a call with ready contiguous float32 arguments, bit for bit."""
    from fs_nerf_amd import ops
    s = scene
    pm, o, d, occ = s["pm"], s["o"], s["d"], s["occ"]
    ready = dict(pos_mask=(torch.arange(63, device=dev) < 45).float(), dir_mask=(torch.arange(27, device=dev) < 15).float(),
                 u=s["u"])
    if fn in ("render_fused", "sample_fused"):
        ready["u_fine"] = s["u_fine"]
        call = lambda kw: getattr(ops, fn)(*((None,) if fn == "render_fused" else ()), pm, o, d, near=2.0, far=6.0,
                                           n_samples=S, n_importance=NI, **kw)
    else:
        ready["t_min"] = torch.full((R,), 2.5, device=dev)
        ready["t_max"] = torch.linspace(4.0, 6.0, R, device=dev)
        extra = dict(want_extras=True) if fn.endswith("extras") else {}
        call = lambda kw: getattr(ops, fn.split("-")[0])(pm, o, d, **occ, **extra, **kw)
    raw = {k: (strided(v) if k in ("u", "t_max") else v.double()) for k, v in ready.items()}
    assert all(v.dtype == torch.float64 or not v.is_contiguous() for v in raw.values())
    with torch.no_grad():
        got = tensors_of(call(raw))
        want = tensors_of(call(ready))
    torch.cuda.synchronize()
    assert len(got) == len(want) >= 1
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), f"{fn}: returned tensor {i} differs"
    assert any(t.numel() > 0 and bool((t != 0).any()) for t in want), "the call rendered something"


def test_the_door_checks_tensors_against_the_header(dev, scene, monkeypatch):
    """3. a tensor handed to `_launch` where include/fsnerf_hip.h has a device pointer is checked against the pointee
    before the C function is called: dtype (width and kind), contiguity, device.  None still arrives as NULL."""
    from fs_nerf_amd import _lib, ops
    rec = recorded(monkeypatch)
    sig = scene["sig"].reshape(-1)
    info = torch.empty(R, 2, dtype=torch.int64, device=dev)
    out8 = torch.empty(R * S, dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError, match="fsn_pack_info: ray_indices: expected torch.int64"):  # const int64_t* ray_indices
        ops._launch("fsn_pack_info", dev, torch.zeros(R * S, dtype=torch.int32, device=dev), R * S, R, info)
    with pytest.raises(TypeError, match="fsn_to8b: out: expected torch.uint8"):               # uint8_t* out
        ops._launch("fsn_to8b", dev, sig, R * S, torch.empty(R * S, dtype=torch.int8, device=dev))
    with pytest.raises(ValueError, match="fsn_to8b: x: expected a contiguous tensor"):
        ops._launch("fsn_to8b", dev, strided(sig), R * S, out8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops._launch("fsn_to8b", dev, sig.cpu(), R * S, out8)
    with pytest.raises(TypeError, match="takes 3 arguments"):
        ops._launch("fsn_to8b", dev, sig, R * S)
    h = ops._Held(_lib.RenderArgs())
    with pytest.raises(TypeError, match="fsn_render_args: u: expected torch.float32"):          # const float* u
        h.set("u", scene["u"].double())
    with pytest.raises(ValueError, match="fsn_render_args: u: expected a contiguous tensor"):
        h.set("u", strided(scene["u"]))
    assert h.a.u is None and rec.calls == [], "every refusal comes before the call"
    edges = torch.empty(R, S + 1, device=dev)
    ops._launch("fsn_stratified_edges", dev, 2.0, 6.0, S, R, None, 0, edges)  # u = NULL: the deterministic edges
    ops._launch("fsn_to8b", dev, sig, R * S, out8)
    h.set("u", scene["u"])
    torch.cuda.synchronize()
    (n0, a0), (n1, a1) = rec.calls
    assert n0 == "fsn_stratified_edges" and a0[4] is None and a0[6] == edges.data_ptr() and a0[:4] == (2.0, 6.0, S, R)
    assert n1 == "fsn_to8b" and a1[:3] == (sig.data_ptr(), R * S, out8.data_ptr())
    assert h.a.u == scene["u"].data_ptr()
    assert torch.equal(edges[:, 0], torch.full((R,), 2.0, device=dev)) and torch.equal(out8, ops.to8b(sig))


def test_measurement_hooks(dev, scene):
    from fs_nerf_amd import ops
    s = scene
    pm, o, d = s["pm"], s["o"], s["d"]
    kw = dict(near=2.0, far=6.0, n_samples=S, n_importance=NI, u=s["u"], u_fine=s["u_fine"])
    edges = ops.stratified_edges(2.0, 6.0, S, R, s["u"], dev)
    clock = torch.zeros(2, dtype=torch.int64, device=dev)
    try:
        timer = ops.launch_timer = []
        with torch.no_grad():
            ops.render_fused(None, pm, o, d, **kw)
            assert len(timer) == 1 and len(timer[0]) == 2, "one event pair per render_fused launch"
            ops.sample_fused(pm, o, d, **kw)
            ops.mlp_fwd(pm, s["x"], s["dirs"])
            ops.composite(s["sig"], s["rgb"], edges[:, :-1], edges[:, 1:])
            assert len(timer) == 1, "only the render launches are bracketed"
            torch.cuda.synchronize()
            assert timer[0][0].elapsed_time(timer[0][1]) > 0.0
            ops.launch_timer = None
            ops.clock_buffer = clock
            ops.render_fused(None, pm, o, d, **kw)
        torch.cuda.synchronize()
        assert bool((clock != 0).any()), "the launch adds its clock differences to ops.clock_buffer"
    finally:
        ops.launch_timer = None
        ops.clock_buffer = None
