// depth_prior.hip — two patch losses that hold rendered depth against a monocular depth prior (DESIGN.md 6.1,
// "Monocular depth priors"): a scale-and-shift-invariant least-squares fit (the prior is known up to an affine map per
// image) and an ordinal ranking term over ALL pairs of a patch (only the prior's ordering is trusted).  The definitions
// are this package's own.  depth, prior and the optional weight are [B, P, Q] float32, P * Q <= kMaxPatch.
// A pixel is VALID iff prior and depth are finite and weight > 0 (no weight: 1); an invalid pixel contributes nothing and
// gets a gradient of exactly 0.  Each forward runs one wavefront per patch, each backward one thread per pixel in gather
// form; no LDS (the ranking kernels hand a patch's pixels round the wave through readlane), no atomics, every sum in a fixed order, every output entry written once: bitwise reproducible.
#include "common.hpp"
#include "ray_dev.hpp"

namespace fsn {

constexpr int kMaxPatch = 4096;  // pixels of a patch (64 x 64)

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the weight of pixel k of a patch: 0 for an invalid pixel
__device__ __forceinline__ float prior_weight(const float* __restrict__ d, const float* __restrict__ p,
                                              const float* __restrict__ w, int64_t k) {
  const float wk = w ? w[k] : 1.0f;
  return (isfinite(d[k]) && isfinite(p[k]) && wk > 0.f) ? wk : 0.f;
}

// ------------------------------------------------------------------ scale-and-shift-invariant fit
// x = depth, or 1 / max(depth, z_min) with `inverse`; every sum below in float64.
__device__ __forceinline__ double ssi_x(float depth, int inverse, float z_min) {
  return inverse ? 1.0 / (double)fmaxf(depth, z_min) : (double)depth;
}

// M = sum w, mx = sum w x / M, mp = sum w p / M; then, centred, vx = sum w (x - mx)^2 / M, cxp = sum w (x - mx)(p - mp) / M;
// s = cxp / vx, t = mp - s mx; L = sum w (s x + t - p)^2 / M.  Three passes of the wave over the patch, the lanes
// striding over the pixels.  Degenerate (fewer than two valid pixels, M <= 0, vx <= rel_eps mx^2): L = 0, flag 1.
// The fit (s, t, M, flag) goes out twice: as float32 for the caller and as float64 for the backward, whose residual
// s x + t - p cancels to nothing near a perfect fit - rounded to float32, (s, t) would leave it an error of 2^-24 |s x|.
__global__ void __launch_bounds__(256) k_ssi_depth_fwd(const float* __restrict__ depth, const float* __restrict__ prior,
                                                       const float* __restrict__ weight, int64_t B, int n, int inverse,
                                                       float z_min, float rel_eps, float* __restrict__ out,
                                                       float* __restrict__ fit, double* __restrict__ fit64) {
  const int lane = lane_id();
  const int64_t b = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t base = b * (int64_t)n;
  double M = 0.0, sx = 0.0, sp = 0.0;
  long long cnt = 0;
  for (int k = lane; k < n; k += 64) {
    const float w = prior_weight(depth, prior, weight, base + k);
    if (w > 0.f) {
      M += (double)w;
      sx += (double)w * ssi_x(depth[base + k], inverse, z_min);
      sp += (double)w * (double)prior[base + k];
      ++cnt;
    }
  }
  M = wave_sum_f64(M);
  sx = wave_sum_f64(sx);
  sp = wave_sum_f64(sp);
  cnt = wave_sum_i64(cnt);
  double s = 0.0, t = 0.0, L = 0.0;
  bool degenerate = cnt < 2 || !(M > 0.0);
  if (!degenerate) {
    const double mx = sx / M, mp = sp / M;
    double vx = 0.0, cxp = 0.0;
    for (int k = lane; k < n; k += 64) {
      const float w = prior_weight(depth, prior, weight, base + k);
      if (w > 0.f) {
        const double dx = ssi_x(depth[base + k], inverse, z_min) - mx;
        vx += (double)w * dx * dx;
        cxp += (double)w * dx * ((double)prior[base + k] - mp);
      }
    }
    vx = wave_sum_f64(vx) / M;
    cxp = wave_sum_f64(cxp) / M;
    degenerate = !(vx > (double)rel_eps * mx * mx);
    if (!degenerate) {
      s = cxp / vx;
      t = mp - s * mx;
      for (int k = lane; k < n; k += 64) {
        const float w = prior_weight(depth, prior, weight, base + k);
        if (w > 0.f) {
          const double r = s * ssi_x(depth[base + k], inverse, z_min) + t - (double)prior[base + k];
          L += (double)w * r * r;
        }
      }
      L = wave_sum_f64(L) / M;
    }
  }
  if (lane == 0) {
    out[b] = degenerate ? 0.f : (float)L;
    fit[4 * b + 0] = degenerate ? 0.f : (float)s;
    fit[4 * b + 1] = degenerate ? 0.f : (float)t;
    fit[4 * b + 2] = (float)M;
    fit[4 * b + 3] = degenerate ? 1.f : 0.f;
    fit64[4 * b + 0] = degenerate ? 0.0 : s;
    fit64[4 * b + 1] = degenerate ? 0.0 : t;
    fit64[4 * b + 2] = M;
    fit64[4 * b + 3] = degenerate ? 1.0 : 0.0;
  }
}

// (s, t) minimise the same weighted quadratic, so dL_b/dx_k is the partial at fixed (s, t): 2 w_k s (s x_k + t - p_k) / M,
// the residual formed again in float64 from the saved float64 fit; through x = 1 / max(depth, z_min): times -x^2, 0 below z_min.
__global__ void __launch_bounds__(256) k_ssi_depth_bwd(const float* __restrict__ depth, const float* __restrict__ prior,
                                                       const float* __restrict__ weight, const double* __restrict__ fit64,
                                                       int64_t n_pix, int n, int inverse, float z_min,
                                                       const float* __restrict__ d_out, float* __restrict__ d_depth) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_pix) return;
  const int64_t b = k / n;
  const float w = prior_weight(depth, prior, weight, k);
  float g = 0.f;
  if (w > 0.f && fit64[4 * b + 3] == 0.0) {
    const double s = fit64[4 * b], t = fit64[4 * b + 1], M = fit64[4 * b + 2];
    const float dk = depth[k];
    const double x = ssi_x(dk, inverse, z_min);
    double dx = 2.0 * (double)w * s * (s * x + t - (double)prior[k]) / M;
    if (inverse) dx = dk < z_min ? 0.0 : -dx * x * x;
    g = (float)((double)d_out[b] * dx);
  }
  d_depth[k] = g;
}

// ------------------------------------------------------------------ ordinal ranking over all pairs
// does the prior put a pixel with prior value pa nearer than one with pb?  (false when either is NaN)
template <bool kDisparity>
__device__ __forceinline__ bool prior_nearer(float pa, float pb, float gap) {
  return kDisparity ? pa > pb + gap : pa < pb - gap;
}
// the hinge of the ordered pair (near pixel, far pixel): positive iff the pair is active
__device__ __forceinline__ float rank_hinge(float d_near, float d_far, float margin) { return (d_near - d_far) + margin; }

// Pixel j of the patch at `base` as the pair loops read it: its depth, and its prior with NaN for an invalid pixel and
// for j >= n (nothing is read there) - a NaN prior is ranked against nobody, so the loops need no validity test.
__device__ __forceinline__ void rank_pixel(const float* __restrict__ depth, const float* __restrict__ prior,
                                           const float* __restrict__ weight, int64_t base, int j, int n, float& dj,
                                           float& pj) {
  dj = 0.f;
  pj = __builtin_nanf("");
  if (j < n && prior_weight(depth, prior, weight, base + j) > 0.f) {
    dj = depth[base + j];
    pj = prior[base + j];
  }
}
// lane t's value in every lane (t is the same in all lanes)
__device__ __forceinline__ float lane_bcast(float v, int t) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), t));
}

// out[b] = sum over the ordered pairs (i, j) of valid pixels the prior ranks (i nearer) of max(0, d_i - d_j + margin),
// pairs[b] = their number.  One wave per patch: the lanes stride over i, every lane walks all j - 64 at a time, each lane
// loading one of them and the wave reading them lane by lane.  Per i a float32 sum in ascending j, from +0 (a pair that
// is not ranked adds +0); the sums of the i's are added in float64.
template <bool kDisparity>
__global__ void __launch_bounds__(64) k_depth_rank_fwd(const float* __restrict__ depth, const float* __restrict__ prior,
                                                       const float* __restrict__ weight, int n, float margin, float gap,
                                                       float* __restrict__ out, long long* __restrict__ pairs) {
  const int lane = lane_id();
  const int64_t b = blockIdx.x, base = b * (int64_t)n;
  double acc = 0.0;
  long long cnt = 0;
  for (int ib = 0; ib < n; ib += 64) {
    float di, pi;
    rank_pixel(depth, prior, weight, base, ib + lane, n, di, pi);
    float row = 0.f;
    int row_cnt = 0;
    for (int jb = 0; jb < n; jb += 64) {
      float dj_lane, pj_lane;
      rank_pixel(depth, prior, weight, base, jb + lane, n, dj_lane, pj_lane);
#pragma unroll 16
      for (int t = 0; t < 64; ++t) {
        const float dj = lane_bcast(dj_lane, t), pj = lane_bcast(pj_lane, t);
        const bool ranked = prior_nearer<kDisparity>(pi, pj, gap);
        row += ranked ? fmaxf(rank_hinge(di, dj, margin), 0.f) : 0.f;
        row_cnt += ranked ? 1 : 0;
      }
    }
    acc += (double)row;
    cnt += row_cnt;
  }
  acc = wave_sum_f64(acc);
  cnt = wave_sum_i64(cnt);
  if (lane == 0) {
    out[b] = (float)acc;
    pairs[b] = cnt;
  }
}

// Gather form, one thread per pixel: wave c of patch b owns the pixels k = 64 c + lane and walks all partners j of the
// patch as the forward does; +1 for every active pair in which k is the nearer pixel, -1 for every active pair in which
// it is the farther one (an integer), times d_out[b].  Four waves per workgroup; `chunks` = ceil(n / 64) waves per patch.
template <bool kDisparity>
__global__ void __launch_bounds__(256) k_depth_rank_bwd(const float* __restrict__ depth, const float* __restrict__ prior,
                                                        const float* __restrict__ weight, int64_t n_waves, int chunks,
                                                        int n, float margin, float gap, const float* __restrict__ d_out,
                                                        float* __restrict__ d_depth) {
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wave >= n_waves) return;
  const int64_t b = wave / chunks, base = b * (int64_t)n;
  const int k = (int)(wave - b * chunks) * 64 + lane;
  float dk, pk;
  rank_pixel(depth, prior, weight, base, k, n, dk, pk);
  int net = 0;
  for (int jb = 0; jb < n; jb += 64) {
    float dj_lane, pj_lane;
    rank_pixel(depth, prior, weight, base, jb + lane, n, dj_lane, pj_lane);
#pragma unroll 16
    for (int t = 0; t < 64; ++t) {
      const float dj = lane_bcast(dj_lane, t), pj = lane_bcast(pj_lane, t);
      net += (prior_nearer<kDisparity>(pk, pj, gap) && rank_hinge(dk, dj, margin) > 0.f) ? 1 : 0;
      net -= (prior_nearer<kDisparity>(pj, pk, gap) && rank_hinge(dj, dk, margin) > 0.f) ? 1 : 0;
    }
  }
  if (k < n) d_depth[base + k] = pk == pk ? d_out[b] * (float)net : 0.f;  // (an invalid pixel: exactly 0)
}

}  // namespace fsn

using namespace fsn;

// sizes of the four entry points: B >= 0, P, Q >= 1, P * Q <= kMaxPatch, and a grid that fits
static int depth_prior_sizes(const char* who, int64_t B, int P, int Q) {
  FSN_REQUIRE(B >= 0 && P >= 1 && Q >= 1, FSN_E_INVALID, "%s: bad sizes B=%lld P=%d Q=%d", who, (long long)B, P, Q);
  FSN_REQUIRE((int64_t)P * Q <= kMaxPatch, FSN_E_UNSUPPORTED, "%s: a patch of %d x %d pixels (at most %d)", who, P, Q,
              kMaxPatch);
  // (the grids: B workgroups, ceil(B P Q / 256), and four waves of 64 pixels of one patch per workgroup)
  FSN_REQUIRE(B <= 0x7fffffff && (double)B * P * Q <= 256.0 * 0x7fffffff &&
                  (double)B * ((P * Q + 63) / 64) <= 4.0 * 0x7fffffff,
              FSN_E_INVALID, "%s: bad sizes (too many pixels)", who);
  return FSN_OK;
}

extern "C" int fsn_ssi_depth_fwd(const float* depth, const float* prior, const float* weight, int64_t B, int P, int Q,
                                 int inverse, float z_min, float rel_eps, float* out, float* fit, double* fit64,
                                 fsn_stream_t stream) {
  if (int rc = depth_prior_sizes("fsn_ssi_depth_fwd", B, P, Q)) return rc;
  FSN_REQUIRE(!inverse || z_min > 0.f, FSN_E_INVALID, "fsn_ssi_depth_fwd: z_min must be positive in disparity space");
  FSN_REQUIRE(rel_eps >= 0.f, FSN_E_INVALID, "fsn_ssi_depth_fwd: negative rel_eps");
  if (B == 0) return FSN_OK;
  FSN_REQUIRE(depth && prior && out && fit && fit64, FSN_E_INVALID, "fsn_ssi_depth_fwd: null pointer");
  k_ssi_depth_fwd<<<(unsigned)((B + 3) / 4), 256, 0, as_stream(stream)>>>(depth, prior, weight, B, P * Q, inverse ? 1 : 0,
                                                                          z_min, rel_eps, out, fit, fit64);
  FSN_LAUNCH_CHECK("k_ssi_depth_fwd");
  return FSN_OK;
}

extern "C" int fsn_ssi_depth_bwd(const float* depth, const float* prior, const float* weight, const double* fit64, int64_t B,
                                 int P, int Q, int inverse, float z_min, const float* d_out, float* d_depth,
                                 fsn_stream_t stream) {
  if (int rc = depth_prior_sizes("fsn_ssi_depth_bwd", B, P, Q)) return rc;
  FSN_REQUIRE(!inverse || z_min > 0.f, FSN_E_INVALID, "fsn_ssi_depth_bwd: z_min must be positive in disparity space");
  if (B == 0) return FSN_OK;
  FSN_REQUIRE(depth && prior && fit64 && d_out && d_depth, FSN_E_INVALID, "fsn_ssi_depth_bwd: null pointer");
  const int64_t n_pix = B * (int64_t)P * Q;
  k_ssi_depth_bwd<<<(unsigned)((n_pix + 255) / 256), 256, 0, as_stream(stream)>>>(depth, prior, weight, fit64, n_pix, P * Q,
                                                                                  inverse ? 1 : 0, z_min, d_out, d_depth);
  FSN_LAUNCH_CHECK("k_ssi_depth_bwd");
  return FSN_OK;
}

extern "C" int fsn_depth_rank_fwd(const float* depth, const float* prior, const float* weight, int64_t B, int P, int Q,
                                  float margin, float prior_gap, int prior_is_disparity, float* out, int64_t* pairs,
                                  fsn_stream_t stream) {
  if (int rc = depth_prior_sizes("fsn_depth_rank_fwd", B, P, Q)) return rc;
  FSN_REQUIRE(prior_gap >= 0.f, FSN_E_INVALID, "fsn_depth_rank_fwd: negative prior_gap");
  if (B == 0) return FSN_OK;
  FSN_REQUIRE(depth && prior && out && pairs, FSN_E_INVALID, "fsn_depth_rank_fwd: null pointer");
  if (prior_is_disparity)
    k_depth_rank_fwd<true><<<(unsigned)B, 64, 0, as_stream(stream)>>>(depth, prior, weight, P * Q, margin, prior_gap, out,
                                                                      reinterpret_cast<long long*>(pairs));
  else
    k_depth_rank_fwd<false><<<(unsigned)B, 64, 0, as_stream(stream)>>>(depth, prior, weight, P * Q, margin, prior_gap, out,
                                                                       reinterpret_cast<long long*>(pairs));
  FSN_LAUNCH_CHECK("k_depth_rank_fwd");
  return FSN_OK;
}

extern "C" int fsn_depth_rank_bwd(const float* depth, const float* prior, const float* weight, int64_t B, int P, int Q,
                                  float margin, float prior_gap, int prior_is_disparity, const float* d_out,
                                  float* d_depth, fsn_stream_t stream) {
  if (int rc = depth_prior_sizes("fsn_depth_rank_bwd", B, P, Q)) return rc;
  FSN_REQUIRE(prior_gap >= 0.f, FSN_E_INVALID, "fsn_depth_rank_bwd: negative prior_gap");
  if (B == 0) return FSN_OK;
  FSN_REQUIRE(depth && prior && d_out && d_depth, FSN_E_INVALID, "fsn_depth_rank_bwd: null pointer");
  const int chunks = (P * Q + 63) / 64;
  const int64_t n_waves = B * chunks;
  const unsigned grid = (unsigned)((n_waves + 3) / 4);
  if (prior_is_disparity)
    k_depth_rank_bwd<true><<<grid, 256, 0, as_stream(stream)>>>(depth, prior, weight, n_waves, chunks, P * Q, margin,
                                                                prior_gap, d_out, d_depth);
  else
    k_depth_rank_bwd<false><<<grid, 256, 0, as_stream(stream)>>>(depth, prior, weight, n_waves, chunks, P * Q, margin,
                                                                 prior_gap, d_out, d_depth);
  FSN_LAUNCH_CHECK("k_depth_rank_bwd");
  return FSN_OK;
}
