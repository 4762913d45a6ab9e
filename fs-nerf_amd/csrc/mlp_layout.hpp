// mlp_layout.hpp — the packed-weights blob: geometry shared by the host packer, the device
// packer and the MFMA kernels.  (DESIGN.md "weight blob" describes this in prose.)
//
// The NeRF MLP (src/core/models.py:96-143) is evaluated TRANSPOSED on the matrix cores:
//   H_out^T [features x samples] = W [out x in] . H_in^T [in x samples]
// with v_mfma_f32_16x16x32_{f16,bf16}: A = a 16(out) x 32(in) weight fragment, B = a 32(in) x 16
// (samples) activation fragment, D = a 16(out) x 16(samples) fp32 accumulator tile with
// column = lane&15 = sample and row = 4(lane>>4) + reg = out feature.  Two such tiles (32 features)
// hold, lane for lane, exactly the 8 elements a lane needs as B operand of one k-step of the next
// layer, so activations never leave registers.
//
// A "unit" is the A operand of one (layer, 32-feature output pair tp, k-step ks, half sub): one
// 1-KiB fragment of the 16-bit (bf16 or fp16) high parts and, in the x3 modes, one 1-KiB fragment
// of the low parts, lane-linear (lane l owns bytes [16 l, 16 l + 16)).  Units are stored in the
// order the kernel consumes them (layer, pair, k-step, half) and streamed through LDS in 16-KiB
// "phases".
#pragma once
#include <cstdint>

#include "fsnerf_hip.h"

#if defined(__HIPCC__)
#define FSN_HD __host__ __device__ __forceinline__
#else
#define FSN_HD inline
#endif

namespace fsn {

constexpr uint32_t kBlobMagic = 0x4e53460au;  // "\nFSN"
constexpr int kPhaseBytes = 16384;
constexpr int kKsPos = 2;  // k-steps (of 32) reserved for the positional encoding: 64 slots
constexpr int kKsDir = 1;  // k-steps reserved for the direction encoding: 32 slots
constexpr int kMaxLayers = 16;

// Properties of an arithmetic mode (FSN_PREC_*), for host and device, run time and compile time.  The numbering
// carries two of them: the odd modes are the single-pass ones, and every fp16 mode is numbered from FSN_PREC_FP16X3 up.
constexpr int kPrecSinglePassBit = 1;
FSN_HD constexpr bool prec_is_x3(int prec) { return (prec & kPrecSinglePassBit) == 0; }  // high / low parts (x3 and x2)
FSN_HD constexpr bool prec_is_f16(int prec) { return prec >= FSN_PREC_FP16X3; }
// the weights' low parts are read (FSN_PREC_FP16X2 streams the x3 blob and drops them)
FSN_HD constexpr bool prec_reads_w_lo(int prec) { return prec_is_x3(prec) && prec != FSN_PREC_FP16X2; }
// Low parts of the split fp16 modes (weights in the blob, activations in registers and in the training workspace) are
// stored SCALED: low = fp16((v - high) * 2^11).  The unscaled remainder of a value below ~0.1 is an fp16 subnormal
// (fixed 2^-24 resolution: an activation of 1e-3 kept ~15 bits, a sigma error of 4e-4); scaled it is a normal fp16
// number down to |v| ~ 6e-5 (and still carries 2^-36 absolute below that).  The two correction products al.wh, ah.wl
// are summed in their own accumulator and folded in as 2^-11 * corr by the epilogue.  bf16 has float32's exponent
// range: scale 1.
constexpr float kLoScaleF16 = 2048.0f;
// FSN_PREC_FP16X3U (round 4): low parts UNSCALED, all three products of a unit in one accumulator - float32-grade because
// per-layer power-of-two scales folded into the packed weights (mlp_pack.hpp, PackArgs::sc_*) keep every layer's
// activations at 2^4 .. 2^10, where an activation's unscaled low part is a normal fp16 number or negligible against the
// layer's scale.
FSN_HD constexpr bool prec_lo_scaled(int prec) { return prec == FSN_PREC_FP16X3 || prec == FSN_PREC_FP16X2; }
FSN_HD float lo_scale(int prec) { return prec_lo_scaled(prec) ? kLoScaleF16 : 1.0f; }
FSN_HD constexpr int enc_width(int n_freqs) { return 3 * (1 + 2 * n_freqs); }  // features of a PositionalEncoder
FSN_HD int unit_bytes(int prec) { return prec_is_x3(prec) ? 2048 : 1024; }
FSN_HD int units_per_phase(int prec) { return kPhaseBytes / unit_bytes(prec); }

// The list of arithmetic modes an entry point admits, stated once per entry point: prec_in is its argument check,
// dispatch_net / dispatch_prec (mlp_dev.hpp) instantiate exactly the same list.
template <int... MODES>
struct PrecModes {};
template <int... MODES>
constexpr bool prec_in(PrecModes<MODES...>, int prec) { return ((prec == MODES) || ...); }
using PrecInference = PrecModes<FSN_PREC_BF16X3, FSN_PREC_BF16, FSN_PREC_FP16X3, FSN_PREC_FP16, FSN_PREC_FP16X3U, FSN_PREC_FP16X2>;
using PrecTraining = PrecModes<FSN_PREC_BF16X3, FSN_PREC_BF16, FSN_PREC_FP16X3, FSN_PREC_FP16>;

// One GEMM of the network as the kernel sees it.
struct LayerGeom {
  int32_t nt_out;      // 32-feature output pairs (two 16-row MFMA tiles each)
  int32_t ks_act;      // k-steps (of 32) fed by the previous layer's activations
  int32_t ks_enc;      // k-steps fed by an encoding (kKsPos / kKsDir) or 0
  int32_t enc_is_dir;  // which encoding
  int32_t n_freqs;     // of that encoding
  int32_t d_act;       // input columns coming from activations (0 for layer 0)
  int32_t ld;          // row stride of the source weight matrix (= in_features)
  int32_t unit0;       // first unit of this layer in the stream
};

struct NetGeom {
  int32_t n_gemm;  // n_layers + 2 (connection, branch)
  LayerGeom g[kMaxLayers + 2];
  int32_t units_hidden;  // units of layers 0..n_layers-1 (density-only pass stops here)
  int32_t units_total;
  int32_t nph_density, nph_full;  // phases per pass
  // aux region (float32 offsets)
  int32_t aux_bias[kMaxLayers + 2];
  int32_t aux_wsigma, aux_wrgb, aux_misc, aux_floats;
  int64_t aux_off, stream_off, total_bytes;  // byte offsets in the blob
};

// Encoding slot -> feature index of the reference's PositionalEncoder layout
// (src/core/models.py:28,37-39: [x, sin f0 x, cos f0 x, sin f1 x, ...], blocks d_in=3 wide), or -1.
// The four lanes g = lane>>4 that share a sample own `slots` = 8 * k-steps slots each, q = 8*ks + j.
// Pair p = 3*band+coord goes to lane group p&3 at slots (2i, 2i+1) = (sin, cos), i = p>>2; the
// identity features x, y sit in group 2's last two slots and z in group 3's second to last.
FSN_HD int enc_slot_feature(int q, int g, int n_freqs, int slots) {
  const int P = 3 * n_freqs;
  const int np = P > g ? (P - g + 3) / 4 : 0;  // pairs owned by this lane group
  if (q < 2 * np) {
    const int p = 4 * (q >> 1) + g;
    const int band = p / 3, coord = p - 3 * band;
    return 3 + band * 6 + (q & 1) * 3 + coord;
  }
  if (g == 2 && q >= slots - 2) return q - (slots - 2);  // x, y
  if (g == 3 && q == slots - 2) return 2;                // z
  return -1;
}

FSN_HD uint16_t bf16_rne(float f) {
  union { float f; uint32_t u; } v;
  v.f = f;
  if ((v.u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((v.u >> 16) | 0x40);  // NaN stays NaN
  return (uint16_t)((v.u + 0x7fffu + ((v.u >> 16) & 1u)) >> 16);
}
FSN_HD float bf16_to_f32(uint16_t b) {
  union { float f; uint32_t u; } v;
  v.u = (uint32_t)b << 16;
  return v.f;
}

// IEEE binary16, round to nearest even, subnormals kept
FSN_HD uint16_t f16_rne(float f) {
  union { float f; uint32_t u; } v;
  v.f = f;
  const uint32_t sign = (v.u >> 16) & 0x8000u;
  uint32_t x = v.u & 0x7fffffffu;
  if (x > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
  if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // >= 65520 rounds to infinity
  if (x < 0x38800000u) {                                      // < 2^-14: subnormal half or zero
    v.u = x;
    const float a = v.f * 16777216.0f;  // * 2^24, exact
    float r = (float)(int)a;            // a < 1024: truncate, then round half to even by hand
    const float frac = a - r;
    if (frac > 0.5f || (frac == 0.5f && ((int)r & 1))) r += 1.0f;
    return (uint16_t)(sign | (uint32_t)(int)r);
  }
  x += 0xfffu + ((x >> 13) & 1u);
  return (uint16_t)(sign | ((x - 0x38000000u) >> 13));
}
FSN_HD float f16_to_f32(uint16_t h) {
  union { float f; uint32_t u; } v;
  const uint32_t sign = ((uint32_t)h & 0x8000u) << 16;
  const uint32_t e = (h >> 10) & 31u, m = h & 0x3ffu;
  if (e == 0) {
    v.f = (float)m * 5.9604644775390625e-08f;  // m * 2^-24
    v.u |= sign;
    return v.f;
  }
  v.u = sign | (e == 31 ? 0x7f800000u | (m << 13) : ((e + 112u) << 23) | (m << 13));
  return v.f;
}
FSN_HD uint16_t half_rne(float f, bool f16) { return f16 ? f16_rne(f) : bf16_rne(f); }
FSN_HD float half_to_f32(uint16_t h, bool f16) { return f16 ? f16_to_f32(h) : bf16_to_f32(h); }

// Fills `G` from the descriptor; returns 0 or an FSN_E_* code (message via set_error on host).
// What is accepted here is what can be PACKED: n_layers 2..16 at either width.  The kernels keep the aux area in LDS
// (kAuxCapFloats = 3456 floats, mlp_dev.hpp) and refuse a geometry whose aux_floats = (n_layers + 5) d_hidden + 36,
// rounded up to 64, does not fit ("network too deep"): 128-wide networks run up to 16 layers, 256-wide ones up to 8
// (8x256 needs 3392, 9x256 3648).  The shortest pass - 2 layers x 128, no skip, single-pass units - has 3 phases.
inline int build_geom(const fsn_mlp_desc& d, int prec, NetGeom& G, const char** why) {
  *why = "";
  if (prec < 0 || (prec > FSN_PREC_FP16X3U && prec != FSN_PREC_FP16X2)) { *why = "unknown precision mode"; return FSN_E_INVALID; }
  if (d.d_hidden != 256 && d.d_hidden != 128) { *why = "d_hidden must be 128 or 256"; return FSN_E_UNSUPPORTED; }
  if (d.n_layers < 2 || d.n_layers > kMaxLayers) { *why = "n_layers must be in [2,16]"; return FSN_E_UNSUPPORTED; }
  if (d.n_freqs_pos < 0 || d.n_freqs_pos > 10) { *why = "n_freqs (position) must be <= 10"; return FSN_E_UNSUPPORTED; }
  if (d.n_freqs_dir < 0 || d.n_freqs_dir > 4) { *why = "n_freqs (direction) must be <= 4"; return FSN_E_UNSUPPORTED; }
  if (d.skip_mask >> (d.n_layers - 1)) { *why = "skip index >= n_layers-1 (the reference model cannot run it either)"; return FSN_E_INVALID; }
  const int D = d.d_hidden, NT = D / 32, L = d.n_layers;
  const int d_pe = enc_width(d.n_freqs_pos), d_de = enc_width(d.n_freqs_dir);
  int u = 0;
  for (int l = 0; l < L; ++l) {
    LayerGeom& g = G.g[l];
    const bool wide = l > 0 && ((d.skip_mask >> (l - 1)) & 1u);
    g.nt_out = NT;
    g.ks_act = l == 0 ? 0 : NT;
    g.ks_enc = (l == 0 || wide) ? kKsPos : 0;
    g.enc_is_dir = 0;
    g.n_freqs = d.n_freqs_pos;
    g.d_act = l == 0 ? 0 : D;
    g.ld = g.d_act + (g.ks_enc ? d_pe : 0);
    g.unit0 = u;
    u += 2 * g.nt_out * (g.ks_act + g.ks_enc);
  }
  G.units_hidden = u;
  LayerGeom& c = G.g[L];  // connection
  c = LayerGeom{NT, NT, 0, 0, 0, D, D, u};
  u += 2 * NT * NT;
  LayerGeom& b = G.g[L + 1];  // branch
  b = LayerGeom{NT / 2, NT, kKsDir, 1, d.n_freqs_dir, D, D + d_de, u};
  u += 2 * (NT / 2) * (NT + kKsDir);
  G.n_gemm = L + 2;
  G.units_total = u;
  const int upp = units_per_phase(prec);
  if (G.units_hidden % upp) { *why = "internal: hidden units not phase aligned"; return FSN_E_UNSUPPORTED; }
  G.nph_density = G.units_hidden / upp;
  G.nph_full = (G.units_total + upp - 1) / upp;
  int a = 0;
  for (int l = 0; l < L + 2; ++l) { G.aux_bias[l] = a; a += D; }
  G.aux_wsigma = a; a += D;
  G.aux_wrgb = a; a += 2 * D;  // [3][D/2]
  G.aux_misc = a; a += 4 + 32;  // b_sigma, b_rgb[3], freqs_pos[16], freqs_dir[16]
  G.aux_floats = (a + 63) / 64 * 64;
  G.aux_off = 256;
  G.stream_off = (G.aux_off + (int64_t)G.aux_floats * 4 + 4095) / 4096 * 4096;
  G.total_bytes = G.stream_off + (int64_t)G.nph_full * kPhaseBytes;
  return FSN_OK;
}

// ------------------------------------------------------------------ weight streams
// Three streams feed the MFMA kernels in ONE format - a run of units (1 KiB of 16-bit high parts, in the x3 modes 1 KiB
// of low parts behind them, lane-linear: lane l owns bytes [16 l, 16 l + 16) of a part) - and differ only in which
// weight element a fragment element is.  A StreamTable says, GEMM by GEMM, where the units come from; pack_piece
// (mlp_pack.hpp) is the one function that turns (table, weights, piece) into 16 bytes, on the host and on the device.
//   kStreamFwd        the forward blob's stream: A[row][k] = W[row][source column of k] x the layer's power of two
//   kStreamBwd        the dgrad chain's stream (train_fused.hip): the same GEMMs transposed, A[row i][k = o] = W[o][i]
//   kStreamInputGrad  the encoding columns of the layers that read an encoding (input_grad.hip), transposed, rows in
//                     the encoder's slot order
// The forward and backward streams are consumed through WStream in 16-KiB phases and padded with zeros to a whole
// phase; the slices are copied to LDS as they are and end with their last unit.
enum StreamKind : int32_t { kStreamFwd = 0, kStreamBwd = FSN_WSTREAM_BWD, kStreamInputGrad = FSN_WSTREAM_INPUT_GRAD };

struct StreamGemm {
  int32_t w;        // source weight: index in state_dict order (layers.0 .., sigma, connection, branch, rgb)
  int32_t ld;       // its row stride (= in_features)
  int32_t col0;     // first column read: 0 (backward), the first encoding column (forward, input gradient)
  int32_t nt_out;   // output tiles: 32-row pairs of two units each (forward, backward), 16-row tiles (input gradient)
  int32_t ks;       // k-steps (of 32)
  int32_t unit0;    // first unit in the stream
  int32_t ks_act;   // forward: the first ks_act k-steps read activations, the others the encoding
  int32_t n_freqs;  // forward, input gradient: of the encoding read
  float sc_act, sc_enc;  // forward: power-of-two factors on the activation / encoding columns (fsn_mlp_pack_scaled)
};

struct StreamTable {
  int32_t kind, prec, n_gemm, units_total;
  StreamGemm g[kMaxLayers + 2];
};

FSN_HD int stream_phases(const StreamTable& T) { return (T.units_total + units_per_phase(T.prec) - 1) / units_per_phase(T.prec); }
FSN_HD int64_t stream_bytes(const StreamTable& T) {
  return T.kind == kStreamInputGrad ? (int64_t)T.units_total * unit_bytes(T.prec) : (int64_t)stream_phases(T) * kPhaseBytes;
}

inline void stream_begin(StreamTable& T, int kind, int prec) { T = StreamTable{}; T.kind = kind; T.prec = prec; }
inline void stream_add(StreamTable& T, StreamGemm g) {
  g.unit0 = T.units_total;
  T.units_total += (T.kind == kStreamInputGrad ? 1 : 2) * g.nt_out * g.ks;
  T.g[T.n_gemm++] = g;
}

// weight index (state_dict order) of GEMM g (kernel order: hidden 0..L-1, connection, branch)
FSN_HD int gemm_to_sd(int g, int L) { return g < L ? g : g + 1; }  // skips "sigma" at index L

// Forward: the GEMMs of `G` in kernel order.  sc_act / sc_enc: per-GEMM factors, or null = 1.
inline void stream_table_fwd(const NetGeom& G, int prec, const float* sc_act, const float* sc_enc, StreamTable& T) {
  stream_begin(T, kStreamFwd, prec);
  const int L = G.n_gemm - 2;
  for (int g = 0; g < G.n_gemm; ++g) {
    const LayerGeom& l = G.g[g];
    stream_add(T, StreamGemm{gemm_to_sd(g, L), l.ld, l.d_act, l.nt_out, l.ks_act + l.ks_enc, 0, l.ks_act, l.n_freqs,
                             sc_act ? sc_act[g] : 1.0f, sc_enc ? sc_enc[g] : 1.0f});
  }
}

// Backward: branch^T restricted to the first D input columns (D/2 outputs = NT/2 k-steps), connection^T, then layers
// L-1 down to 1, each restricted to its D activation columns.  This IS the order k_train_bwd (train_fused.hip) consumes:
// its gemm_layer calls are d feat, d h_{L-1}, then dPre_{l-1} for l = L-1 .. 1.  NT^2 (2 L + 1) units.
inline void stream_table_bwd(const fsn_mlp_desc& d, int prec, StreamTable& T) {
  stream_begin(T, kStreamBwd, prec);
  const int L = d.n_layers, D = d.d_hidden, NT = D / 32;
  stream_add(T, StreamGemm{L + 2, D + enc_width(d.n_freqs_dir), 0, NT, NT / 2, 0, 0, 0, 1.0f, 1.0f});
  stream_add(T, StreamGemm{L + 1, D, 0, NT, NT, 0, 0, 0, 1.0f, 1.0f});
  for (int l = L - 1; l >= 1; --l) {
    const bool wide = (d.skip_mask >> (l - 1)) & 1u;
    stream_add(T, StreamGemm{l, D + (wide ? enc_width(d.n_freqs_pos) : 0), 0, NT, NT, 0, 0, 0, 1.0f, 1.0f});
  }
}

// Input-gradient slices: the position jobs - layer 0 and every skip-fed layer, in layer order - when d_x is wanted, then
// the direction job (the branch) when d_dirs is.  A lane group owns 8 slots per k-step of the encoding, a 16-row output
// tile takes 4 of them from each group (slot q = 4 t + reg of lane group gs is row 4 gs + reg of tile t): 2 kKsPos = 4
// tiles for a position job, 2 kKsDir = 2 for the direction job.  The contraction runs over the layer's outputs; the
// units are ordered (job, k-step, tile).  At most NT (4 L + 1) units: never more than the backward stream.
inline void stream_table_input_grad(const fsn_mlp_desc& d, int prec, bool want_x, bool want_dirs, StreamTable& T) {
  stream_begin(T, kStreamInputGrad, prec);
  const int L = d.n_layers, D = d.d_hidden, NT = D / 32, d_pe = enc_width(d.n_freqs_pos);
  if (want_x) {
    stream_add(T, StreamGemm{0, d_pe, 0, 2 * kKsPos, NT, 0, 0, d.n_freqs_pos, 1.0f, 1.0f});
    for (int l = 1; l < L; ++l)
      if ((d.skip_mask >> (l - 1)) & 1u) stream_add(T, StreamGemm{l, D + d_pe, D, 2 * kKsPos, NT, 0, 0, d.n_freqs_pos, 1.0f, 1.0f});
  }
  if (want_dirs) stream_add(T, StreamGemm{L + 2, D + enc_width(d.n_freqs_dir), D, 2 * kKsDir, NT / 2, 0, 0, d.n_freqs_dir, 1.0f, 1.0f});
}

}  // namespace fsn
