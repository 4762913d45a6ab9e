// ssim_dev.hpp — what the SSIM forward (metrics.hip) and its backward (ssim_grad.hip) share: the tile geometry, the
// strides and window parameters, the argument checks, and the windowed moments of one 32x32 tile.
// The moments index LDS through FSN_AT, so a translation unit defines FSN_DEBUG_RECORD (its own debug record) BEFORE it
// includes this header.
#pragma once
#include "common.hpp"

#include <cmath>

namespace fsn {

constexpr int kSsimTile = 32;
constexpr int kSsimThreads = 256;
constexpr int kSsimRowsPerThread = kSsimTile * kSsimTile / kSsimThreads;  // 4

struct Strides4 {
  int64_t n, c, h, w;
};

struct SsimParams {
  double taps[11];  // normalised window taps, 2r+1 used
  double cn;       // NP / (NP - 1) or 1
  double C1, C2;
};

// scipy.ndimage mode='reflect' (half-sample symmetric) for |overhang| <= r < n; indices outside that range only feed
// outputs that are not written and are clamped into the image so that every load stays in bounds.
__device__ __forceinline__ int reflect_idx(int i, int n) {
  i = i < 0 ? -i - 1 : i;
  i = i >= n ? 2 * n - 1 - i : i;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// The five windowed moments (x, y, x^2, y^2, xy) of the tile at (h0, w0) of one channel: thread t holds column
// t % 32, rows (t / 32) * 4 .. + 3 of the tile in m[moment][row].  Steps 1-3 of metrics.hip's header.
template <int R>
__device__ __forceinline__ void ssim_tile_moments(const float* __restrict__ xb, const float* __restrict__ yb, int H, int W,
                                                  const Strides4& sx, const Strides4& sy, const SsimParams& p, int h0, int w0,
                                                  float (&lx)[kSsimTile + 2 * R][kSsimTile + 2 * R + 1],
                                                  float (&ly)[kSsimTile + 2 * R][kSsimTile + 2 * R + 1],
                                                  double (&hm)[5][kSsimTile + 2 * R][kSsimTile + 1],
                                                  double (&m)[5][kSsimRowsPerThread]) {
  constexpr int T = kSsimTile, HB = T + 2 * R, K = 2 * R + 1;
  // 1. halo through reflect indexing
  for (int i = threadIdx.x; i < HB * HB; i += kSsimThreads) {
    const int r = i / HB, q = i - r * HB;
    const int hh = reflect_idx(h0 - R + r, H), ww = reflect_idx(w0 - R + q, W);
    FSN_AT(FSN_AT(lx, r), q) = xb[hh * sx.h + ww * sx.w];
    FSN_AT(FSN_AT(ly, r), q) = yb[hh * sy.h + ww * sy.w];
  }
  __syncthreads();

  // 2. horizontal pass
  for (int i = threadIdx.x; i < HB * T; i += kSsimThreads) {
    const int r = i / T, q = i - r * T;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
    for (int t = 0; t < K; ++t) {
      const double wt = p.taps[t];
      const double u = FSN_AT(FSN_AT(lx, r), q + t), v = FSN_AT(FSN_AT(ly, r), q + t);
      a0 = __builtin_fma(wt, u, a0);
      a1 = __builtin_fma(wt, v, a1);
      a2 = __builtin_fma(wt, u * u, a2);  // u * u, v * v, u * v: exact in float64 for float32 inputs
      a3 = __builtin_fma(wt, v * v, a3);
      a4 = __builtin_fma(wt, u * v, a4);
    }
    FSN_AT(FSN_AT(hm[0], r), q) = a0;
    FSN_AT(FSN_AT(hm[1], r), q) = a1;
    FSN_AT(FSN_AT(hm[2], r), q) = a2;
    FSN_AT(FSN_AT(hm[3], r), q) = a3;
    FSN_AT(FSN_AT(hm[4], r), q) = a4;
  }
  __syncthreads();

  // 3. vertical pass: column q, output rows r0 .. r0+3 of the tile
  constexpr int RT = kSsimRowsPerThread;
  const int q = threadIdx.x % T, r0 = (threadIdx.x / T) * RT;
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int j = 0; j < RT; ++j) m[k][j] = 0.0;
#pragma unroll
  for (int s = 0; s < K + RT - 1; ++s) {
    double v[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = FSN_AT(FSN_AT(hm[k], r0 + s), q);
#pragma unroll
    for (int j = 0; j < RT; ++j) {
      const int t = s - j;
      if (t >= 0 && t < K) {
#pragma unroll
        for (int k = 0; k < 5; ++k) m[k][j] = __builtin_fma(p.taps[t], v[k], m[k][j]);
      }
    }
  }
}

static int ssim_radius(int window) { return window == FSN_SSIM_GAUSSIAN ? 5 : 3; }

static int check_strides(const int64_t* s, const char* what) {
  FSN_REQUIRE(s, FSN_E_INVALID, "%s: null stride array", what);
  return FSN_OK;
}

static Strides4 strides4(const int64_t* s) { return Strides4{s[0], s[1], s[2], s[3]}; }

static int64_t ssim_tiles(int H, int W) {
  return (int64_t)((H + kSsimTile - 1) / kSsimTile) * ((W + kSsimTile - 1) / kSsimTile);
}

// the shape and window checks of fsn_ssim and fsn_ssim_grad (`who` names the entry point in the message)
static int ssim_check_shape(const char* who, int64_t N, int C, int H, int W, int window) {
  FSN_REQUIRE(N >= 0 && C >= 1 && H >= 1 && W >= 1, FSN_E_INVALID, "%s: bad shape (N=%lld C=%d H=%d W=%d)", who,
              (long long)N, C, H, W);
  FSN_REQUIRE(window == FSN_SSIM_GAUSSIAN || window == FSN_SSIM_UNIFORM, FSN_E_UNSUPPORTED, "%s: unknown window code %d",
              who, window);
  const int win = 2 * ssim_radius(window) + 1;
  FSN_REQUIRE(H >= win && W >= win, FSN_E_INVALID, "%s: image %dx%d is smaller than the %dx%d window", who, H, W, win,
              win);
  return FSN_OK;
}

static SsimParams ssim_params(int window, int use_sample_covariance, double data_range, double K1, double K2) {
  const int r = ssim_radius(window), win = 2 * r + 1;
  SsimParams p{};
  double taps[11], sum = 0.0;
  for (int t = 0; t < win; ++t) {
    const double d = t - r;
    taps[t] = window == FSN_SSIM_GAUSSIAN ? std::exp(-d * d / (2.0 * 1.5 * 1.5)) : 1.0;
    sum += taps[t];
  }
  for (int t = 0; t < win; ++t) p.taps[t] = taps[t] / sum;
  const double NP = (double)win * win;
  p.cn = use_sample_covariance ? NP / (NP - 1.0) : 1.0;
  p.C1 = (K1 * data_range) * (K1 * data_range);
  p.C2 = (K2 * data_range) * (K2 * data_range);
  return p;
}

}  // namespace fsn
