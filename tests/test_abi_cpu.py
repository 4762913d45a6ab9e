"""CPU: the C-ABI library loads and exports every symbol declared in include/fsnerf_hip.h; argument
validation works without a GPU (no compute call is made); the host layer refuses CPU tensors."""
import ctypes as C
import os
import re

import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L
from fs_nerf_amd import ops

import debug_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_symbol_is_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fsnerf_hip.h")).read()
    declared = set(re.findall(r"\b(fsn_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"fsn_stream_t"}
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)
    lib = L.lib()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.fsn_version() >= 100
    # the #define constants of the header and their Python mirrors
    for name, val in re.findall(r"#define\s+(FSN_(?:STATUS|PREC)_[A-Z0-9_]+)\s+(\d+)u?", hdr):
        assert getattr(L, name) == int(val), name


def test_debug_records_register_themselves_and_are_reported_by_name():
    """The debug library's registry (csrc/common.hip) without a GPU call: every FSN_DEBUG_DEFINE_RECORD(unit) of the
    sources is reportable by its name, an unknown unit and null arguments are refused before any HIP call."""
    dbg = C.CDLL(debug_lib.build_debug_library())
    dbg.fsn_debug_units.restype = dbg.fsn_last_error.restype = C.c_char_p
    dbg.fsn_debug_report.argtypes = [C.c_char_p, C.c_void_p]
    csrc = os.path.join(ROOT, "fs-nerf_amd", "csrc")
    defined = [u for f in sorted(os.listdir(csrc)) if f.endswith(".hip")
               for u in re.findall(r"^FSN_DEBUG_DEFINE_RECORD\((\w+)\)", open(os.path.join(csrc, f)).read(), re.M)]
    assert len(defined) >= 6 and len(set(defined)) == len(defined), defined
    assert dbg.fsn_debug_units() == ",".join(sorted(defined)).encode()
    buf = (C.c_uint32 * 4)()
    assert dbg.fsn_debug_report(b"nosuch", buf) == -1 and dbg.fsn_debug_units() in dbg.fsn_last_error()
    assert dbg.fsn_debug_report(None, buf) == -1
    assert dbg.fsn_debug_report(b"render", None) == -1
    assert L.lib().fsn_debug_units() == b""


def test_argument_validation_without_gpu():
    lib = L.lib()
    assert lib.fsn_get_rays(None, 4, 4, 2.0, 0, 4, None, None, None) == -1
    assert b"null" in lib.fsn_last_error()
    pose = (C.c_float * 12)()
    assert lib.fsn_get_rays(pose, 4, 4, 2.0, 3, 4, 1, 1, None) == -1          # rows out of range
    assert lib.fsn_stratified_edges(2.0, 6.0, 0, 10, None, 0, None, None) == -1  # S = 0
    assert lib.fsn_composite_fwd(None, None, None, None, 0, 64, None, None, None, None, None, None, None, None) == 0
    desc = ops.make_desc(8, 256, [4], [1.0] * 10, [1.0] * 4)
    assert lib.fsn_mlp_blob_bytes(C.byref(desc), 0) == lib.fsn_mlp_blob_bytes(C.byref(desc), 2) > 2_000_000
    assert lib.fsn_mlp_blob_bytes(C.byref(desc), 1) < lib.fsn_mlp_blob_bytes(C.byref(desc), 0)
    assert lib.fsn_mlp_blob_bytes(C.byref(desc), 7) == -1
    a = L.RenderArgs()
    a.R, a.S, a.n_imp = 0, 64, 128
    assert lib.fsn_render_rays_fused(C.byref(desc), 2, None, None, C.byref(a), None) == 0  # zero rays: no-op
    a.R, a.S = 10, 600
    assert lib.fsn_render_rays_fused(C.byref(desc), 2, None, None, C.byref(a), None) < 0


def test_training_and_occgrid_entry_points_validate_without_gpu():
    lib = L.lib()
    from fs_nerf_amd import ops
    d = ops.make_desc(8, 256, (4,), [2.0 ** i for i in range(10)], [2.0 ** i for i in range(4)])
    # workspace sizing needs no device: saved activations + gradients = 20 KB per sample on the MFMA path
    n = 128 * 64
    w_mfma = lib.fsn_nerf_train_workspace_floats(C.byref(d), L.FSN_PREC_FP16X3, n)
    assert w_mfma > 0
    # the plain-fp32 (library GEMM) formulation is a test helper, not a mode of the product library
    assert lib.fsn_nerf_train_workspace_floats(C.byref(d), 4, n) < 0  # (4 was the test-only fp32 formulation's code: not a mode of the library)
    assert 4.5e3 * n < w_mfma < 7e3 * n + 5e7 and w_mfma % 1024 == 0
    assert lib.fsn_nerf_train_workspace_floats(C.byref(d), 9, n) < 0 and b"precision" in lib.fsn_last_error()
    assert lib.fsn_nerf_train_workspace_floats(C.byref(d), L.FSN_PREC_FP16X3, -1) < 0
    assert lib.fsn_nerf_train_fwd(C.byref(d), 7, None, None, None, None, None, None, 4, None, None, None, None) != 0
    assert lib.fsn_nerf_train_bwd(C.byref(d), L.FSN_PREC_FP16X3, None, 0, None, None, None, None, None, None, 0, None, None, None, None) != 0
    assert lib.fsn_grad_scale(None, 5, None, None) != 0 and b"fsn_grad_scale" in lib.fsn_last_error()
    # the two-pass mode is inference only
    assert lib.fsn_nerf_train_fwd(C.byref(d), L.FSN_PREC_FP16X2, None, None, None, None, None, None, 4, None, None, None, None) != 0
    aabb = (C.c_float * 6)(0, 0, 0, 1, 1, 1)
    assert lib.fsn_occgrid_march(None, None, 5, aabb, 0, 1, None, 0.0, 1.0, 0.1, None, 8, None, None, None, None, None, None) != 0
    assert b"resolution" in lib.fsn_last_error()
    bad = (C.c_float * 6)(0, 0, 0, 1, -1, 1)
    assert lib.fsn_occgrid_march(None, None, 5, bad, 16, 1, None, 0.0, 1.0, 0.1, None, 8, None, None, None, None, None, None) != 0
    assert lib.fsn_occgrid_update(None, 64, None, None, 0, 0.95, None, None, None) != 0
    assert lib.fsn_packed_visibility(None, None, None, None, 0, 0, 1e-4, 0.0, None, None) == 0  # empty: nothing to do
    # modes an entry point has no kernel for are refused by name, in front of the launch dispatch (FSN_E_UNSUPPORTED = -2)
    o = L.OccRenderArgs()
    o.R, o.step, o.max_steps = 0, 0.1, 8
    assert lib.fsn_render_rays_occgrid(C.byref(d), L.FSN_PREC_FP16X2, None, C.byref(o), None) == -2
    assert b"fsn_render_rays_occgrid: precision mode 6" in lib.fsn_last_error()
    assert lib.fsn_mlp_layer_maxima(C.byref(d), L.FSN_PREC_FP16, None, None, None, None, None, 0, None, None) == -2
    assert b"fsn_mlp_layer_maxima: precision mode 3" in lib.fsn_last_error()
    for x3 in (L.FSN_PREC_BF16X3, L.FSN_PREC_FP16X3, L.FSN_PREC_FP16X3U, L.FSN_PREC_FP16X2):
        assert lib.fsn_occgrid_refresh(C.byref(d), x3, None, None, None, 16, 1, aabb, 0, 0, 0, None, 0.1, None, None, None, None) == -2
        assert b"fsn_occgrid_refresh: precision mode" in lib.fsn_last_error()


def test_host_layer_has_no_cpu_fallback():
    from fs_nerf_amd.core.models import NeRF, PositionalEncoder
    from fs_nerf_amd.utils import utilities as U
    with pytest.raises(RuntimeError):
        PositionalEncoder(3, 4, True)(torch.zeros(5, 3))
    with pytest.raises(RuntimeError):
        U.get_rays(torch.eye(4), (4, 4, 2.0), torch.device("cpu"))
    m = NeRF(3, 3, 4, 128, (4,), pos_fn={"n_freqs": 10, "log_space": True}, dir_fn={"n_freqs": 4, "log_space": True})
    assert set(m.state_dict()) == {f"layers.{i}.{p}" for i in range(4) for p in ("weight", "bias")} | {
        f"{n}.{p}" for n in ("sigma", "connection", "branch", "rgb") for p in ("weight", "bias")}
    assert m.layers[1].weight.shape == (128, 128) and m.branch.weight.shape == (64, 128 + 27)
    with pytest.raises(ValueError):
        NeRF(3, 3, 8, 256, (7,), pos_fn={"n_freqs": 10, "log_space": True},
             dir_fn={"n_freqs": 4, "log_space": True}).eval().packed()
    assert U.get_chunks(torch.zeros(10, 3), 4)[-1].shape == (2, 3)


def test_generated_asm_blocks_declare_the_scc_clobber():
    """The k-loop blocks (csrc/kloop_gen.hpp) compare in their phase openings; the asm statements that carry them must
    tell the compiler so (tools/scan_asm_scc.py checks the compiled code for the consequence)."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fs-nerf_amd", "csrc")
    gen = open(os.path.join(csrc, "kloop_gen.hpp")).read()
    assert "s_cmp_ge_u32" in gen
    dev = open(os.path.join(csrc, "mlp_dev.hpp")).read()
    emit = dev[dev.index("#define FSN_KLOOP_EMIT"):dev.index("#define FSN_KLOOP_CASE")]
    stmts = re.findall(r"asm volatile\(TXT\([^;]*;", emit)
    assert len(stmts) == 2 and all('"scc"' in st and '"memory"' in st for st in stmts), stmts
