// input_grad.hip — gradients of the training step with respect to the network's INPUTS: sample positions and
// directions (point form) or rays_o / rays_d (ray form).  DESIGN.md 6, "Input gradient".
//
//   weight slices     : the encoding columns of the weights that read an encoding - W_0[:, :d_pe], W_l[:, D:D+d_pe] of the
//                       skip-fed layers, W_branch[:, D:D+d_de] - transposed, as lane-linear MFMA A fragments: the
//                       kStreamInputGrad weight stream of mlp_layout.hpp (stream_table_input_grad), packed by the one
//                       device packer (mlp.hip, pack_stream_device).  The jobs below are that table's GEMMs.
//   k_input_grad      : per 128-sample tile, g_enc^T [encoding slots x samples] = sum over those layers of
//                       W_enc^T [slots x D] . dPre_l [D x samples] / (grad_scale bs[l]) on v_mfma_f32_16x16x32, the
//                       gradient tiles read from the packed T-layout the dgrad chain stored them in (train_fused.hip),
//                       then the positional encoder's backward on the sample's own lanes.
//   k_ray_grad        : the ray form's segmented sum of the per-sample results.
//
// Lane layout = the chain's: wave w owns samples 16 w .. 16 w + 15 of the tile, the four lanes g = lane >> 4 of a sample
// share its encoding slots exactly as encode<> lays them out (enc_slot_feature: lane group g owns slots q = 0 .. 8 NKS - 1).
// An output tile t of the MFMA (16 rows x 16 samples, row 4 g + reg in lane group g) is therefore packed so that its row
// 4 g + reg IS slot q = 4 t + reg of group g: after the GEMMs every lane holds the gradients of its own slots and the
// encoder backward needs no exchange but the final sum over the four lanes.
// k index of a k-step: (lane group gk, element j) = feature 32 ks + 8 gk + j - the four pair-rows 16 ks + 4 gk .. + 3 of
// the T-layout, i.e. four dwords (dword pairs in the x3 modes) per lane and k-step, no unzip.
//
// Precision: the call's training mode.  x3: hi.hi + (hi.lo + lo.hi) on the stored parts (fp16: both low parts carry
// 2^11, their products go to an accumulator of their own); single-pass modes: one product.  sin / cos are recomputed
// from the sample position with sincos_f32 in every mode (arguments reach 512 x 1.5 rad).
#include "mlp_dev.hpp"
#include "mlp_layout.hpp"
#include "mlp_pack.hpp"
#include "ray_dev.hpp"
#include "train_internal.hpp"

namespace fsn {

constexpr int kIgMaxJobs = kMaxLayers + 1;   // position jobs (layer 0, skip-fed layers), then the direction job
constexpr int kIgLdsBytes = 144 * 1024;      // weight slices: all of them resident when they fit, else one job at a time
constexpr int kIgPosTiles = 4 * kKsPos / 2;  // 16-row output tiles of a position job (64 slots) ...
constexpr int kIgDirTiles = 4 * kKsDir / 2;  // ... and of the direction job (32 slots)
static_assert(kIgPosTiles == 4 && kIgDirTiles == 2, "slot q = 4 t + reg of lane group g");
static_assert(kIgMaxJobs <= kMaxLayers + 2, "the slices' table (StreamTable) holds every job");

// ------------------------------------------------------------------ the kernel
struct InputGradArgs {
  const uint32_t* ws;             // the training workspace
  const char* blob;               // packed weight slices
  int64_t src[kIgMaxJobs];        // dword offset of the job's gradient tensor in the workspace
  int32_t stage[kIgMaxJobs];      // its index in the per-stage factors
  int32_t unit0[kIgMaxJobs + 1];  // first unit of the job in the blob
  int32_t n_pos, has_dir, resident;
  const float *scale, *bscale;    // grad_scale (or null = 1), per-stage factors of THIS call's chain (fp16 modes) or null
  const uint32_t* status;         // fp16 modes: this call's range-guard word, or null
  const float *x, *dirs, *rays_o, *rays_d, *t0, *t1;
  const int64_t* ri;
  const float *pos_mask, *dir_mask;
  float freqs_pos[16], freqs_dir[16];
  int32_t n_freqs_pos, n_freqs_dir;
  int64_t n;
  float *d_x, *d_dirs;
};

// One job: gout[4 t + reg] += (W_enc^T . dPre)[slot 4 t + reg of this lane's group][this lane's sample] * inv.
// A: this lane's 16 bytes of the job's first unit (LDS); src: this lane's sample at pair-row 4 g of the gradient's tile.
template <int MT, int KS, int PREC>
__device__ __forceinline__ void ig_job(const char* A, const uint32_t* __restrict__ src, float inv, float* gout) {
  constexpr bool F16 = prec_is_f16(PREC), X3 = prec_is_x3(PREC);
  constexpr int NPL = X3 ? 2 : 1, UB = X3 ? 2048 : 1024;
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
  typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
  f32x4 acc[MT], cor[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    cor[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll 2
  for (int ks = 0; ks < KS; ++ks) {
    u32x4 h, l = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t* p = src + (16 * ks + i) * kTRow * NPL;
      if constexpr (X3) {
        const u32x2 v = *reinterpret_cast<const u32x2*>(p);
        h[i] = v[0];
        l[i] = v[1];
      } else {
        h[i] = *p;
      }
    }
    const s16x8 bh = __builtin_bit_cast(s16x8, h), bl = __builtin_bit_cast(s16x8, l);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const char* u = A + (ks * MT + t) * UB;
      const s16x8 ah = *reinterpret_cast<const s16x8*>(u);
      acc[t] = mfma16<F16>(ah, bh, acc[t]);
      if constexpr (X3) {
        const s16x8 al = *reinterpret_cast<const s16x8*>(u + 1024);
        cor[t] = mfma16<F16>(al, bh, cor[t]);
        cor[t] = mfma16<F16>(ah, bl, cor[t]);
      }
    }
  }
  constexpr float IK = (F16 && X3) ? 1.0f / kLoScaleF16 : 1.0f;  // (both low parts of the fp16 split carry 2^11)
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) gout[4 * t + r] += (acc[t][r] + cor[t][r] * IK) * inv;
}

// Backward of encode<> for this lane's SLOTS slots of one sample: partial d x (summed over the four lanes by the caller).
// feature order x, sin f0, cos f0, sin f1, ...: d x_c = m_c g_c + sum_k f_k (m^sin cos(f_k x_c) g^sin - m^cos sin(f_k x_c) g^cos)
template <int SLOTS>
__device__ __forceinline__ void enc_bwd(const float* gs, float x0, float x1, float x2, int n_freqs, const float* freqs,
                                        const float* mask, int g, float (&d)[3]) {
  const int P = 3 * n_freqs;
  d[0] = d[1] = d[2] = 0.f;
#pragma unroll
  for (int i = 0; i < SLOTS / 2; ++i) {
    const int p = 4 * i + g;
    if (p < P) {
      const int band = (p * 11) >> 5;  // p / 3 for p < 32
      const int coord = p - 3 * band;
      const float xc = coord == 0 ? x0 : (coord == 1 ? x1 : x2);
      const float f = freqs[band];
      float s, c;
      sincos_f32(xc * f, s, c);
      const float v = f * (mask[3 + band * 6 + coord] * c * gs[2 * i] - mask[3 + band * 6 + 3 + coord] * s * gs[2 * i + 1]);
      d[0] += coord == 0 ? v : 0.f;
      d[1] += coord == 1 ? v : 0.f;
      d[2] += coord == 2 ? v : 0.f;
    }
  }
  if (g == 2) {
    d[0] += mask[0] * gs[SLOTS - 2];
    d[1] += mask[1] * gs[SLOTS - 1];
  }
  if (g == 3) d[2] += mask[2] * gs[SLOTS - 2];
}

template <int NT, int PREC>
__global__ __launch_bounds__(kThreads) void k_input_grad(InputGradArgs a) {
  constexpr bool F16 = prec_is_f16(PREC), X3 = prec_is_x3(PREC);
  constexpr int NPL = X3 ? 2 : 1, UB = X3 ? 2048 : 1024, D = 32 * NT;
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
  __shared__ __attribute__((aligned(16))) char lds[kIgLdsBytes + 128 * 4];
  float* pm = reinterpret_cast<float*>(lds + kIgLdsBytes);  // position mask [64], direction mask [32], frequencies [16 + 16]
  float* dm = pm + 64;
  float* fq = dm + 32;
  {
    const int i = threadIdx.x;
    const int npe = 3 * (1 + 2 * a.n_freqs_pos), nde = 3 * (1 + 2 * a.n_freqs_dir);
    if (i < 64) pm[i] = (a.pos_mask && i < npe) ? a.pos_mask[i] : 1.0f;
    else if (i < 96) dm[i - 64] = (a.dir_mask && i - 64 < nde) ? a.dir_mask[i - 64] : 1.0f;
    else if (i < 112) fq[i - 96] = a.freqs_pos[i - 96];
    else if (i < 128) fq[i - 96] = a.freqs_dir[i - 112];
  }
  const int n_jobs = a.n_pos + a.has_dir;
  auto stage_in = [&](int j0, int j1) {  // units of jobs [j0, j1) -> LDS offset 0 (lane-linear fragments: a plain copy)
    const u32x4* g = reinterpret_cast<const u32x4*>(a.blob + (int64_t)a.unit0[j0] * UB);
    const int n16 = (a.unit0[j1] - a.unit0[j0]) * (UB / 16);
    for (int i = threadIdx.x; i < n16; i += kThreads) reinterpret_cast<u32x4*>(lds)[i] = g[i];
  };
  if (a.resident) stage_in(0, n_jobs);
  __syncthreads();
  // fp16 modes: this call's chain or forward left the range - the step is a skipped one, zeros like the weight gradients
  const bool skip = F16 && a.status && (a.status[0] & (FSN_STATUS_FP16_RANGE | FSN_STATUS_GRAD_RANGE));
  const float scale = a.scale ? a.scale[0] : 1.0f;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4;
  const int col = wave * 16 + (lane & 15);
  const int64_t ntiles = (a.n + kTileCols - 1) / kTileCols;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t s = tile * kTileCols + col;
    const bool valid = s < a.n;
    const int64_t sc = valid ? s : a.n - 1;
    float q[6];
    if (a.ri) {
      ray_sample(a.rays_o, a.rays_d, a.ri, a.t0, a.t1, sc, q, true);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        q[c] = a.x[3 * sc + c];
        q[3 + c] = a.dirs[3 * sc + c];
      }
    }
    float gpe[8 * kKsPos], gde[8 * kKsDir];
#pragma unroll
    for (int i = 0; i < 8 * kKsPos; ++i) gpe[i] = 0.f;
#pragma unroll
    for (int i = 0; i < 8 * kKsDir; ++i) gde[i] = 0.f;
    for (int j = 0; j < n_jobs; ++j) {
      if (!a.resident) {  // (workgroup-uniform: every wave walks the same tiles and jobs)
        __syncthreads();
        stage_in(j, j + 1);
        __syncthreads();
      }
      const char* A = lds + (a.resident ? a.unit0[j] * UB : 0) + lane * 16;
      const float bsj = (F16 && a.bscale) ? a.bscale[a.stage[j]] : 1.0f;
      const float inv = 1.0f / (scale * bsj);  // (powers of two)
      if (j < a.n_pos) {
        const uint32_t* src = a.ws + a.src[j] + tile * D * kTileCols + t_layout_off(NPL, D / 2, 4 * g, col);
        ig_job<kIgPosTiles, NT, PREC>(A, src, inv, gpe);
      } else {
        const uint32_t* src = a.ws + a.src[j] + tile * (D / 2) * kTileCols + t_layout_off(NPL, D / 4, 4 * g, col);
        ig_job<kIgDirTiles, NT / 2, PREC>(A, src, inv, gde);
      }
    }
    if (a.d_x) {
      float d[3];
      enc_bwd<8 * kKsPos>(gpe, q[0], q[1], q[2], a.n_freqs_pos, fq, pm, g, d);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        d[c] += __shfl_xor(d[c], 16, 64);
        d[c] += __shfl_xor(d[c], 32, 64);
        if (lane < 16 && valid) a.d_x[3 * s + c] = skip ? 0.f : d[c];
      }
    }
    if (a.d_dirs) {
      float d[3];
      enc_bwd<8 * kKsDir>(gde, q[3], q[4], q[5], a.n_freqs_dir, fq + 16, dm, g, d);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        d[c] += __shfl_xor(d[c], 16, 64);
        d[c] += __shfl_xor(d[c], 32, 64);
        if (lane < 16 && valid) a.d_dirs[3 * s + c] = skip ? 0.f : d[c];
      }
    }
  }
}

int input_grad_launch(const fsn_mlp_desc& d, int prec, const float* const* W, int64_t n, float* ws, const InputGradWs& o,
                      const float* grad_scale_dev, const float* bscale, const uint32_t* status, const InputGradReq& rq,
                      hipStream_t s) {
  if (!rq.d_x && !rq.d_dirs) return FSN_OK;
  const int L = d.n_layers, D = d.d_hidden, NT = D / 32;
  // the jobs are the GEMMs of the slices' table (mlp_layout.hpp): position jobs, then the direction job
  StreamTable tab;
  stream_table_input_grad(d, prec, rq.d_x != nullptr, rq.d_dirs != nullptr, tab);
  InputGradArgs a{};
  a.has_dir = rq.d_dirs ? 1 : 0;
  a.n_pos = tab.n_gemm - a.has_dir;
  for (int j = 0; j < tab.n_gemm; ++j) {
    const int w = tab.g[j].w;  // a hidden layer's index is its stage; the branch (L + 2) is stage L + 1 and reads dBo
    a.stage[j] = j < a.n_pos ? w : L + 1;
    a.src[j] = j < a.n_pos ? o.dp + w * o.h_stride : o.dbo;
    a.unit0[j] = tab.g[j].unit0;
  }
  a.unit0[tab.n_gemm] = tab.units_total;
  const int64_t bytes = stream_bytes(tab);
  FSN_REQUIRE((int64_t)NT * kIgPosTiles * unit_bytes(prec) <= kIgLdsBytes, FSN_E_HIP, "internal: input-gradient LDS budget");
  char* blob = reinterpret_cast<char*>(ws + o.blob);
  if (int rc = pack_stream_device(tab, W, blob, s)) return rc;
  a.ws = reinterpret_cast<const uint32_t*>(ws);
  a.blob = blob;
  a.resident = bytes <= kIgLdsBytes ? 1 : 0;
  a.scale = grad_scale_dev; a.bscale = bscale; a.status = status;
  a.x = rq.x; a.dirs = rq.dirs;
  if (rq.rays) { a.rays_o = rq.rays->rays_o; a.rays_d = rq.rays->rays_d; a.t0 = rq.rays->t0; a.t1 = rq.rays->t1; a.ri = rq.rays->ri; }
  a.pos_mask = rq.pos_mask; a.dir_mask = rq.dir_mask;
  for (int i = 0; i < 16; ++i) { a.freqs_pos[i] = d.freqs_pos[i]; a.freqs_dir[i] = d.freqs_dir[i]; }
  a.n_freqs_pos = d.n_freqs_pos; a.n_freqs_dir = d.n_freqs_dir;
  a.n = n; a.d_x = rq.d_x; a.d_dirs = rq.d_dirs;
  const int cus = fsn_device_cus();
  if (cus <= 0) return FSN_E_HIP;
  const int64_t T = (n + kTileCols - 1) / kTileCols;
  const unsigned grid = (unsigned)(T < cus ? T : cus);
  return dispatch_net(PrecTraining{}, D, prec, [&](auto NTc, auto PREC) {
    k_input_grad<NTc(), PREC()><<<grid, kThreads, 0, s>>>(a);
    FSN_LAUNCH_CHECK("k_input_grad");
    return FSN_OK;
  });
}

// ------------------------------------------------------------------ ray form: per-ray sums
// One wave per ray; lane l takes samples l, l + 64, ... of the ray, then a butterfly over the lanes: a fixed order.
__global__ void k_ray_grad(const float* __restrict__ d_x, const float* __restrict__ d_dirs, SpanArgs sp,
                           const float* __restrict__ t0, const float* __restrict__ t1, int64_t R,
                           float* __restrict__ d_o, float* __restrict__ d_d) {
  RayWork rw;
  ray_work(sp, R, rw);  // (a ray without samples goes on: it gets zeros)
  const int64_t r = rw.r, beg = rw.beg;
  const int S = rw.S, lane = rw.lane;
  if (r >= R) return;
  float so[3] = {0.f, 0.f, 0.f}, sd[3] = {0.f, 0.f, 0.f};
  for (int i = lane; i < S; i += 64) {
    const int64_t k = beg + i;
    const float m = (t0[k] + t1[k]) / 2.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float gx = d_x ? d_x[3 * k + c] : 0.f;
      so[c] += gx;
      sd[c] += m * gx + (d_dirs ? d_dirs[3 * k + c] : 0.f);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float vo = wave_sum(so[c]), vd = wave_sum(sd[c]);
    if (lane == 0) {
      if (d_o) d_o[3 * r + c] = vo;
      if (d_d) d_d[3 * r + c] = vd;
    }
  }
}

}  // namespace fsn

using namespace fsn;

extern "C" int fsn_nerf_train_bwd_inputs(const fsn_mlp_desc* desc, int prec, const float* const* W, int64_t n, float* ws,
                                         const float* out, const float* d_out, const float* grad_scale, float* const* dW,
                                         float* const* db, int accumulate, float* stage_scales, uint32_t* stage_amax,
                                         uint32_t* status, const float* x, const float* dirs, const float* rays_o,
                                         const float* rays_d, const int64_t* ray_indices, const float* t_starts,
                                         const float* t_ends, const float* pos_mask, const float* dir_mask, float* d_x,
                                         float* d_dirs, fsn_stream_t stream) {
  const bool ray_form = rays_o || rays_d || ray_indices || t_starts || t_ends;
  const TrainRays rays{rays_o, rays_d, t_starts, t_ends, ray_indices};
  const InputGradReq rq{x, dirs, ray_form ? &rays : nullptr, pos_mask, dir_mask, d_x, d_dirs};
  return train_bwd_checked("fsn_nerf_train_bwd_inputs", desc, prec, W, n, ws, out, d_out, grad_scale, dW, db, accumulate,
                           stage_scales, stage_amax, status, stream, &rq);
}

extern "C" int fsn_ray_grad_reduce(const float* d_x, const float* d_dirs, const int64_t* ray_indices, const float* t_starts,
                                   const float* t_ends, int64_t N, int64_t R, float* d_rays_o, float* d_rays_d,
                                   fsn_stream_t stream) {
  FSN_REQUIRE(N >= 0 && R >= 0, FSN_E_INVALID, "fsn_ray_grad_reduce: bad sizes");
  if (R == 0 || (!d_rays_o && !d_rays_d)) return FSN_OK;
  RayLaunch L;
  if (int rc = ray_launch("fsn_ray_grad_reduce", ray_indices, nullptr, N, R, 0, false, &L)) return rc;
  if (!L.launch) {  // N == 0, nothing to launch: every ray is an empty one
    if (d_rays_o) FSN_HIP(hipMemsetAsync(d_rays_o, 0, (size_t)R * 3 * sizeof(float), as_stream(stream)));
    if (d_rays_d) FSN_HIP(hipMemsetAsync(d_rays_d, 0, (size_t)R * 3 * sizeof(float), as_stream(stream)));
    return FSN_OK;
  }
  FSN_REQUIRE(t_starts && t_ends, FSN_E_INVALID, "fsn_ray_grad_reduce: null pointer");
  k_ray_grad<<<L.grid, 256, 0, as_stream(stream)>>>(d_x, d_dirs, L.sp, t_starts, t_ends, R, d_rays_o, d_rays_d);
  FSN_LAUNCH_CHECK("k_ray_grad");
  return FSN_OK;
}
