"""CPU: the C-ABI library loads and exports every symbol declared in include/fsnerf_hip.h; the binding derived from the
header (fs_nerf_amd._lib.parse_header) has the compiler's struct layouts and refuses what it does not know; argument
validation works without a GPU (no compute call is made); the host layer refuses CPU tensors."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L
from fs_nerf_amd import ops

import debug_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_symbol_is_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "fsnerf_hip.h")).read()
    declared = set(re.findall(r"\b(fsn_[a-z0-9_]+)\s*\(", hdr))  # (a second reading of the header: the parser dropped nothing)
    declared -= {"fsn_stream_t"}
    assert declared == set(L.SIGNATURES) == set(L.FUNCTIONS), declared ^ set(L.SIGNATURES)
    assert len(declared) >= 101
    lib, dbg = L.lib(), C.CDLL(debug_lib.build_debug_library())
    for name in L.SIGNATURES:
        assert hasattr(lib, name), name
        assert hasattr(dbg, name), f"debug library: {name}"
    assert lib.fsn_version() >= 100
    # every integer #define of the header's FSN_ namespace and its Python mirror
    consts = re.findall(r"#define\s+(FSN_[A-Z0-9_]+)\s+\(?(-?\d+)u?\)?", hdr)
    assert len(consts) >= 24 and {n for n, _ in consts} == set(L.DEFINES)
    for name, val in consts:
        assert getattr(L, name) == int(val), name
    assert L.FSN_E_INVALID == -1 and L.FSN_STATUS_GRAD_RANGE == 4 and L.FSN_PROP_MAX_ROW == 1024


def test_struct_layouts_are_the_compilers(tmp_path):
    """sizeof, and every field's offsetof and sizeof, of the three argument structs as g++ lays them out from the header
    (a stand-alone program) against the ctypes structures derived from it."""
    rows = []
    for name, st in L.STRUCTS.items():
        rows.append(f'  printf("{name} %zu 0\\n", sizeof({name}));')
        rows += [f'  printf("{name}.{f.name} %zu %zu\\n", offsetof({name}, {f.name}), sizeof((({name}*)0)->{f.name}));'
                 for f in st.fields]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "fsnerf_hip.h"\nint main() {\n' + "\n".join(rows)
                   + "\n  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["g++", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = {k: (int(a), int(b)) for k, a, b in (ln.split() for ln in subprocess.run([exe], check=True, capture_output=True,
                                                                                  text=True).stdout.splitlines())}
    want = {}
    for name, st in L.STRUCTS.items():
        want[name] = (C.sizeof(st), 0)
        want.update({f"{name}.{f.name}": (getattr(st, f.name).offset, getattr(st, f.name).size) for f in st.fields})
    assert [len(st.fields) for st in (L.MlpDesc, L.RenderArgs, L.OccRenderArgs)] == [7, 31, 36]
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


SYNTHETIC = """
/* a header of the real one's shape: one declaration per entry of the type map */
#ifndef FSN_SYN_H
#define FSN_SYN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* fsn_stream_t; /* a handle */
#define FSN_A 3
#define FSN_B (-2)   /* negative */
#define FSN_C 4u
#define FSN_F 1.5f
typedef struct fsn_s {
  int32_t a, b, c; /* three in one declaration */
  double d;
  float v[3];
  const float* p;
  uint64_t* q;
} fsn_s;
int fsn_f0(void);
const char* fsn_f1(const char* s, fsn_stream_t stream);
int64_t fsn_f2(int a, int32_t b, uint32_t c, int64_t d, uint64_t e, uint8_t f, float g, double h);
int fsn_f3(const float* a, double* b, const int32_t* c, uint32_t* d, const int64_t* e, uint64_t* f, const uint8_t* g,
           void* h, const void* i);
int fsn_f4(const fsn_s* args_host, const float* const* w_host_of_dev, float* const* dw, fsn_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_every_entry_of_its_type_map():
    fns, structs, defines = L.parse_header(SYNTHETIC)
    vp = C.c_void_p
    assert list(fns) == ["fsn_f0", "fsn_f1", "fsn_f2", "fsn_f3", "fsn_f4"]
    sig = lambda n: (fns[n][0].ctype, [(p.name, p.ctype, p.pointee) for p in fns[n][1]])
    assert sig("fsn_f0") == (C.c_int, [])
    assert sig("fsn_f1") == (C.c_char_p, [("s", C.c_char_p, "char"), ("stream", vp, None)])
    assert sig("fsn_f2") == (C.c_int64, [("a", C.c_int, None), ("b", C.c_int32, None), ("c", C.c_uint32, None),
                                         ("d", C.c_int64, None), ("e", C.c_uint64, None), ("f", C.c_uint8, None),
                                         ("g", C.c_float, None), ("h", C.c_double, None)])
    assert sig("fsn_f3") == (C.c_int, [("a", vp, "float"), ("b", vp, "double"), ("c", vp, "int32_t"), ("d", vp, "uint32_t"),
                                       ("e", vp, "int64_t"), ("f", vp, "uint64_t"), ("g", vp, "uint8_t"), ("h", vp, "void"),
                                       ("i", vp, "void")])
    S = structs["fsn_s"]
    assert sig("fsn_f4") == (C.c_int, [("args_host", C.POINTER(S), "fsn_s"), ("w_host_of_dev", vp, "float*"),
                                       ("dw", vp, "float*"), ("stream", vp, None)])
    assert [(f.name, f.pointee) for f in S.fields] == [("a", None), ("b", None), ("c", None), ("d", None), ("v", None),
                                                       ("p", "float"), ("q", "uint64_t")]
    assert [t for _, t in S._fields_[:4]] == [C.c_int32] * 3 + [C.c_double] and S._fields_[5][1] is vp
    assert S.d.offset == 16 and S.v.offset == 24 and S.v.size == 12 and S.p.offset == 40 and C.sizeof(S) == 56
    assert [L.define_int(defines, n) for n in ("FSN_A", "FSN_B", "FSN_C")] == [3, -2, 4] and "FSN_SYN_H" not in defines
    with pytest.raises(ValueError, match="FSN_F.*1.5f"):
        L.define_int(defines, "FSN_F")


@pytest.mark.parametrize("bad, quoted", [
    ("int fsn_g(size_t n);", "size_t n"),                        # a type outside the map
    ("int fsn_g(unsigned int n);", "unsigned int n"),            # two-word types are outside the grammar
    ("int fsn_g(const double* const* rows);\nvoid fsn_h(int a);", "void"),  # no void results
    ("int fsn_g(int a)\nint fsn_h(int b);", "int fsn_g"),        # a missing ;
    ("int fsn_g(int a);\nint fsn_h(int b)", "fsn_h"),            # ... at the end
    ("int fsn_g(int);", "fsn_g"),                                # a parameter without a name
    ("int fsn_g(int a);\nint64_t fsn_g(int a);", "fsn_g"),       # a duplicate symbol
    ("typedef struct fsn_t { float* p, q; } fsn_t;", "float\\* p, q"),
    ("typedef struct fsn_t { fsn_stream_t* s; } fsn_t;", "fsn_stream_t\\* s"),
    ("int fsn_g(float v[3]);", "v\\[3\\]"),                      # arrays are struct fields only
])
def test_parser_refuses_what_it_does_not_know(bad, quoted):
    head = "typedef void* fsn_stream_t;\n"
    L.parse_header(head + "int fsn_ok(const double* const* rows, fsn_stream_t stream);")
    with pytest.raises(ValueError, match=quoted):
        L.parse_header(head + bad)


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
