"""CPU (no GPU): the two weight streams of the training backward - the dgrad chain's transposed weights and the
input gradient's weight slices (fs-nerf_amd/csrc/mlp_layout.hpp: stream_table_bwd, stream_table_input_grad; one piece
function, csrc/mlp_pack.hpp pack_piece) - packed by `fsn_weight_stream_pack_host` and replayed unit by unit through the
v_mfma_f32_16x16x32 lane maps (test_pack_layout.Emu.mfma), the way k_train_bwd and k_input_grad consume them.

What a replay must give is stated from the source weights alone: W^ = the weight rounded by the mode's own rule
(hi = rne16(w), lo = rne16((w - hi) * lo_scale), decoded back), times a small-integer B operand.  Products of a 22-bit
weight and a small integer are exact in float64, so the only error is float64 summation: |err| <= n_terms 2^-52
sum |w^| |d| (twice the textbook (n-1) u bound; derived, not measured).  A wrong element map or rounding is off by the
size of a weight, twelve orders of magnitude above that."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fs_nerf_amd  # noqa: F401
from fs_nerf_amd import _lib as L
from fs_nerf_amd import ops
from test_pack_layout import Emu
from wstream_ref import CORNERS, K_MAX_LAYERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fs-nerf_amd", "csrc")
NETS = dict(CORNERS, **{"6x128": (6, 128, (1, 3), 10, 4)})
TRAIN_PRECS = [L.FSN_PREC_BF16X3, L.FSN_PREC_BF16, L.FSN_PREC_FP16X3, L.FSN_PREC_FP16]
BWD, IG = L.FSN_WSTREAM_BWD, L.FSN_WSTREAM_INPUT_GRAD
FLAGS = [(1, 0), (0, 1), (1, 1)]
PHASE = 16384


def is_x3(prec):
    return prec in (L.FSN_PREC_BF16X3, L.FSN_PREC_FP16X3)


def unit_bytes(prec):
    return 2048 if is_x3(prec) else 1024


def enc_width(nf):
    return 3 * (1 + 2 * nf)


def make_desc(net):
    n_layers, d_hidden, skip, nf, nfd = net
    return ops.make_desc(n_layers, d_hidden, list(skip), [2.0 ** i for i in range(nf)], [2.0 ** i for i in range(nfd)])


def make_weights(net, seed=5):
    """Seeded weights in state_dict order (layers.0 .., sigma, connection, branch, rgb), float32, row-major [out, in]."""
    n_layers, D, skip, nf, nfd = net
    rng = np.random.default_rng(seed)
    shapes = [(D, enc_width(nf))] + [(D, D + (enc_width(nf) if l - 1 in skip else 0)) for l in range(1, n_layers)]
    shapes += [(1, D), (D, D), (D // 2, D + enc_width(nfd)), (3, D // 2)]
    # magnitudes spread over a few binades, so that low parts are exercised at several exponents
    return [(rng.standard_normal(s) * 2.0 ** rng.integers(-6, 1, size=s)).astype(np.float32) for s in shapes]


def ptrs(ws):
    return (C.c_void_p * len(ws))(*[w.ctypes.data for w in ws])


def stream_bytes(desc, prec, kind, wx=0, wd=0):
    return L.lib().fsn_weight_stream_bytes(C.byref(desc), prec, kind, wx, wd)


def pack_host(net, ws, prec, kind, wx=0, wd=0):
    desc = make_desc(net)
    nb = stream_bytes(desc, prec, kind, wx, wd)
    assert nb > 0 and nb % unit_bytes(prec) == 0
    buf = np.full(nb + 64, 0xAB, dtype=np.uint8)  # a guard behind the stream: the packer writes `nb` bytes, no more
    L.check(L.lib().fsn_weight_stream_pack_host(C.byref(desc), prec, kind, wx, wd, ptrs(ws), buf.ctypes.data),
            "fsn_weight_stream_pack_host")
    assert (buf[nb:] == 0xAB).all()
    return buf[:nb]


# ------------------------------------------------------------------------------------------------ the mode's rounding
def rne16(w, prec):
    """float32 -> the mode's 16-bit format and back (round to nearest even), float32."""
    w = np.asarray(w, dtype=np.float32)
    if prec >= L.FSN_PREC_FP16X3:
        return w.astype(np.float16).astype(np.float32)
    u = w.view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def rounded(w, prec):
    """W^ as float64: what the stream holds of w."""
    hi = rne16(w, prec)
    if not is_x3(prec):
        return hi.astype(np.float64)
    scale = np.float32(2048.0 if prec == L.FSN_PREC_FP16X3 else 1.0)
    lo = rne16((w - hi) * scale, prec)
    return hi.astype(np.float64) + lo.astype(np.float64) / float(scale)


def a_frag(stream, prec, unit):
    """A operand of `unit` as float64 [lane, j] (hi + lo / lo_scale), as Emu.a_frag reads the forward blob's."""
    ub = unit_bytes(prec)
    base = unit * ub
    if prec >= L.FSN_PREC_FP16X3:
        dec = lambda b: b.view(np.float16).astype(np.float64)
    else:
        dec = lambda b: (b.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    v = dec(stream[base:base + 1024]).reshape(64, 8)
    if is_x3(prec):
        v = v + dec(stream[base + 1024:base + 2048]).reshape(64, 8) / (2048.0 if prec == L.FSN_PREC_FP16X3 else 1.0)
    return v


def small_ints(rng, rows):
    return rng.integers(-4, 5, size=(rows, 16)).astype(np.float64)


def tol(w_hat_abs_t, d, n_terms):
    return n_terms * 2.0 ** -52 * (w_hat_abs_t @ np.abs(d))


# ------------------------------------------------------------------------------------------------ backward stream
def b_acc_order(d, ks):
    """B operand of k-step ks when d [features, 16 samples] sits in accumulators: element j of lane (c, g) is register
    j&3 of output tile 2 ks + (j>>2), i.e. feature 32 ks + 16 (j>>2) + 4 g + (j&3)."""
    b = np.zeros((64, 8))
    for lane in range(64):
        c, g = lane & 15, lane >> 4
        for j in range(8):
            b[lane, j] = d[32 * ks + 16 * (j >> 2) + 4 * g + (j & 3), c]
    return b


@pytest.mark.parametrize("prec", TRAIN_PRECS)
@pytest.mark.parametrize("name", list(NETS))
def test_backward_stream_replays_to_transposed_weights(name, prec):
    net = NETS[name]
    n_layers, D, skip, nf, nfd = net
    NT = D // 32
    ws = make_weights(net)
    stream = pack_host(net, ws, prec, BWD)
    rng = np.random.default_rng(11)
    # the chain's GEMMs in the order k_train_bwd runs them: (weight, contraction length = its output features)
    chain = [(ws[n_layers + 2], D // 2), (ws[n_layers + 1], D)] + [(ws[l], D) for l in range(n_layers - 1, 0, -1)]
    unit = 0
    for w, k_len in chain:
        d = small_ints(rng, k_len)
        bfr = [b_acc_order(d, ks) for ks in range(k_len // 32)]
        got = np.zeros((D, 16))
        for tp in range(NT):
            acc = [np.zeros((4, 64)), np.zeros((4, 64))]
            for ks in range(k_len // 32):
                for sub in range(2):
                    acc[sub] = Emu.mfma(a_frag(stream, prec, unit), bfr[ks], acc[sub])
                    unit += 1
            for sub in range(2):
                for lane in range(64):
                    got[32 * tp + 16 * sub + 4 * (lane >> 4):32 * tp + 16 * sub + 4 * (lane >> 4) + 4, lane & 15] = acc[sub][:, lane]
        wt = rounded(w, prec)[:, :D].T  # [input feature, output]
        want = wt @ d
        assert (np.abs(got - want) <= tol(np.abs(wt), d, k_len)).all(), (name, prec, float(np.abs(got - want).max()))
    # the unit count of the closed formula, and nothing but zero padding behind it
    assert unit == NT * NT * (2 * n_layers + 1)
    assert stream[unit * unit_bytes(prec) - 1024:unit * unit_bytes(prec)].any() and not stream[unit * unit_bytes(prec):].any()


# ------------------------------------------------------------------------------------------------ input-gradient slices
def enc_slot_feature(q, g, n_freqs, slots):
    """Feature of slot q of lane group g in the PositionalEncoder's order [x, sin f0 x, cos f0 x, ...] (Emu.encode's
    layout read backwards): pair p = 3 band + coord = 4 (q >> 1) + g at slots (2i, 2i+1) = (sin, cos); x, y in group 2's
    last two slots, z in group 3's second to last; None = unused."""
    p = 4 * (q >> 1) + g
    if p < 3 * n_freqs:
        band, coord = divmod(p, 3)
        return 3 + band * 6 + (q & 1) * 3 + coord
    if g == 2 and q >= slots - 2:
        return q - (slots - 2)
    if g == 3 and q == slots - 2:
        return 2
    return None


def test_slot_map_is_a_bijection_onto_the_features():
    for nf, slots in [(10, 16), (0, 16), (4, 8), (0, 8), (7, 16), (3, 8)]:
        fs = [enc_slot_feature(q, g, nf, slots) for g in range(4) for q in range(slots)]
        assert sorted(f for f in fs if f is not None) == list(range(enc_width(nf)))


@pytest.mark.parametrize("wx,wd", FLAGS)
@pytest.mark.parametrize("prec", TRAIN_PRECS)
@pytest.mark.parametrize("name", list(NETS))
def test_input_grad_slices_replay_to_encoding_columns(name, prec, wx, wd):
    net = NETS[name]
    n_layers, D, skip, nf, nfd = net
    NT = D // 32
    ws = make_weights(net)
    stream = pack_host(net, ws, prec, IG, wx, wd)
    rng = np.random.default_rng(13)
    # (weight, first encoding column, n_freqs, 16-row output tiles, contraction length)
    jobs = []
    if wx:
        jobs += [(ws[0], 0, nf, 4, D)] + [(ws[l], D, nf, 4, D) for l in range(1, n_layers) if l - 1 in skip]
    if wd:
        jobs += [(ws[n_layers + 2], D, nfd, 2, D // 2)]
    unit = 0
    for w, col0, n_freqs, mt, k_len in jobs:
        d = small_ints(rng, k_len)
        acc = [np.zeros((4, 64)) for _ in range(mt)]
        for ks in range(k_len // 32):
            b = np.zeros((64, 8))  # linear k order: element j of lane (c, gk) is feature 32 ks + 8 gk + j
            for lane in range(64):
                b[lane] = d[32 * ks + 8 * (lane >> 4):32 * ks + 8 * (lane >> 4) + 8, lane & 15]
            for t in range(mt):
                acc[t] = Emu.mfma(a_frag(stream, prec, unit), b, acc[t])
                unit += 1
        wh = rounded(w, prec)
        used = 0
        for t in range(mt):
            for gs in range(4):
                for reg in range(4):
                    got = acc[t][reg, 16 * gs:16 * gs + 16]  # row 4 gs + reg of tile t, the 16 samples
                    f = enc_slot_feature(4 * t + reg, gs, n_freqs, 4 * mt)
                    if f is None:
                        assert (got == 0.0).all(), (name, prec, t, gs, reg)
                        continue
                    used += 1
                    col = wh[:, col0 + f]
                    assert (np.abs(got - col @ d) <= tol(np.abs(col), d, k_len)).all(), (name, prec, t, gs, reg)
        assert used == enc_width(n_freqs)
    assert unit * unit_bytes(prec) == stream.size  # no padding


# ------------------------------------------------------------------------------------------------ geometry
def test_stream_sizes_are_the_closed_formulas():
    """Every admitted (n_layers, d_hidden, number of skips), both unit sizes: the backward stream has the parent's
    NT^2 + 2 NT^2 + (L-1) 2 NT^2 units in whole phases, the slices NT (4 jobs + 1) units, never more than the stream."""
    for D in (128, 256):
        NT = D // 32
        for n_layers in range(2, K_MAX_LAYERS + 1):
            for k in range(n_layers):
                desc = ops.make_desc(n_layers, D, list(range(k)), [1.0] * 10, [1.0] * 4)
                for prec in (L.FSN_PREC_BF16X3, L.FSN_PREC_FP16):
                    ub = unit_bytes(prec)
                    units = NT * NT + 2 * NT * NT + (n_layers - 1) * 2 * NT * NT
                    nph = (units + PHASE // ub - 1) // (PHASE // ub)
                    bwd = stream_bytes(desc, prec, BWD)
                    assert bwd == nph * PHASE, (n_layers, D, k, prec)
                    both = stream_bytes(desc, prec, IG, 1, 1)
                    assert both == ((1 + k) * 4 * NT + 2 * (NT // 2)) * ub
                    assert stream_bytes(desc, prec, IG, 1, 0) + stream_bytes(desc, prec, IG, 0, 1) == both <= bwd


# fsn_nerf_train_workspace_floats of the commit before the streams shared a table, at n = (300, 4096): [x3, single pass]
WORKSPACE_FLOATS = {
    "min": [[644608, 5940224], [599552, 5895168]],
    "bare": [[677376, 6214656], [628224, 6165504]],
    "deep": [[3715584, 26696704], [3379712, 26360832]],
    "wide-skips": [[5280256, 44193792], [4657664, 43571200]],
    "wide-min": [[1645056, 14151680], [1473024, 13979648]],
    "6x128": [[1446400, 13060096], [1327616, 12941312]],
}


@pytest.mark.parametrize("name", list(NETS))
def test_training_workspace_is_unchanged(name):
    desc = make_desc(NETS[name])
    for prec in TRAIN_PRECS:
        got = [L.lib().fsn_nerf_train_workspace_floats(C.byref(desc), prec, n) for n in (300, 4096)]
        assert got == WORKSPACE_FLOATS[name][0 if is_x3(prec) else 1], (name, prec)


# ------------------------------------------------------------------------------------------------ errors
def test_entry_points_refuse_bad_arguments():
    lib = L.lib()
    net = NETS["min"]
    desc, ws = make_desc(net), make_weights(net)
    W = ptrs(ws)
    buf = np.zeros(stream_bytes(desc, 0, BWD), dtype=np.uint8)
    dst = buf.ctypes.data
    for prec in (L.FSN_PREC_FP16X3U, L.FSN_PREC_FP16X2, 5, 9, -1):  # not a training mode
        assert stream_bytes(desc, prec, BWD) == L.FSN_E_UNSUPPORTED and b"fsn_weight_stream_bytes" in lib.fsn_last_error()
        assert lib.fsn_weight_stream_pack_host(C.byref(desc), prec, BWD, 0, 0, W, dst) == L.FSN_E_UNSUPPORTED
    for kind in (0, 3, -1):
        assert stream_bytes(desc, 0, kind, 1, 1) == L.FSN_E_INVALID and b"kind" in lib.fsn_last_error()
        assert lib.fsn_weight_stream_pack_host(C.byref(desc), 0, kind, 1, 1, W, dst) == L.FSN_E_INVALID
    assert stream_bytes(desc, 0, IG, 0, 0) == L.FSN_E_INVALID
    assert lib.fsn_weight_stream_pack_host(C.byref(desc), 0, IG, 0, 0, W, dst) == L.FSN_E_INVALID
    assert stream_bytes(desc, 0, BWD, 0, 0) > 0  # (the backward stream does not read the flags)
    assert lib.fsn_weight_stream_bytes(None, 0, BWD, 0, 0) == L.FSN_E_INVALID
    assert lib.fsn_weight_stream_pack_host(None, 0, BWD, 0, 0, W, dst) == L.FSN_E_INVALID
    assert lib.fsn_weight_stream_pack_host(C.byref(desc), 0, BWD, 0, 0, None, dst) == L.FSN_E_INVALID
    assert lib.fsn_weight_stream_pack_host(C.byref(desc), 0, BWD, 0, 0, W, None) == L.FSN_E_INVALID
    assert b"fsn_weight_stream_pack_host: null pointer" in lib.fsn_last_error()
    hole = ptrs(ws)
    hole[net[0] + 1] = None  # the connection: read by the backward stream, not by the slices
    assert lib.fsn_weight_stream_pack_host(C.byref(desc), 0, BWD, 0, 0, hole, dst) == L.FSN_E_INVALID
    assert lib.fsn_weight_stream_pack_host(C.byref(desc), 0, IG, 1, 1, hole, dst) == 0
    bad = ops.make_desc(2, 192, [], [1.0] * 10, [1.0] * 4)  # a descriptor the blob's size query refuses
    assert stream_bytes(bad, 0, BWD) == lib.fsn_mlp_blob_bytes(C.byref(bad), 0) == L.FSN_E_UNSUPPORTED
    # the device packer checks the same things before any HIP call
    assert lib.fsn_weight_stream_pack(C.byref(desc), L.FSN_PREC_FP16X2, BWD, 0, 0, W, dst, None) == L.FSN_E_UNSUPPORTED
    assert lib.fsn_weight_stream_pack(C.byref(desc), 0, IG, 0, 0, W, dst, None) == L.FSN_E_INVALID
    assert lib.fsn_weight_stream_pack(C.byref(desc), 0, BWD, 0, 0, W, None, None) == L.FSN_E_INVALID


# ------------------------------------------------------------------------------------------------ sanitizer program
def test_host_packers_under_asan_ubsan_standalone():
    """csrc/stream_pack_main.cpp: all three streams of the six networks in the four training modes through the host
    functions, compiled with -fsanitize=address,undefined - an executable of its own, run as a child process."""
    r = subprocess.run(["make", "-C", CSRC, "sanitize-streams"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([os.path.join(CSRC, "pack_streams_san")], capture_output=True, text=True, env=env, timeout=600)
    tail = out.stdout[-2000:] + out.stderr[-3000:]
    assert out.returncode == 0 and "packed " in out.stdout, tail
    assert "AddressSanitizer" not in tail and "runtime error" not in tail, tail
