// metrics.hip — the two numbers the reference's evaluation() returns (src/run-nerf.py:108-191), on the device:
//   * SSIM: skimage.metrics.structural_similarity (scikit-image 0.22) of N image pairs, each channel on its own,
//     averaged over the interior (the map cropped by the window radius) and then over channels;
//   * PSNR: -10 log10(MSE), per image and over the whole stack (F.mse_loss over every element, :157-160).
// Inputs are float32 with four arbitrary element strides (n, c, h, w), so NHWC, NCHW and permuted views are read
// without a copy.  Every sum is taken in a fixed order (per-workgroup partials in a workspace, then one finishing
// workgroup): no atomics, the results are bitwise reproducible.
//
// SSIM tile kernel: one 256-thread workgroup per (image, channel, 32x32 output tile).
//   1. the (32+2r)^2 halo of x and y goes to LDS (float32, the input values) through scipy's mode='reflect' indexing
//      (d c b a | a b c d | d c b a);
//   2. horizontal pass of the separable window for the five moments x, y, x^2, y^2, xy into LDS, in float64;
//   3. vertical pass in registers, in float64, four consecutive output rows per thread (14 LDS rows feed 4 outputs);
//   4. S, the optional S map (float32), and the interior sum of S -> one float64 partial per workgroup.  k_ssim_finish
//      sums the partials of each image in a fixed order.
// Precision: the window sums are taken in float64 with float64 taps.  In float32, uxx - ux^2 cancels where the image
// is flat and S amplifies that error by up to 1/C2 ~ 1100; the float32 taps do not sum to exactly 1, which biases the
// variances of textured images.  Float64 removes both (DESIGN.md "Evaluation metrics"); the arithmetic is ~130 FMAs
// per pixel and channel, far below the launch cost at image sizes.
#include "common.hpp"

#include <cmath>

namespace fsn {

// debug build: the LDS indices of k_ssim_tile are range-checked (common.hpp), read by fsn_debug_report_metrics
FSN_DEBUG_DEFINE_RECORD(g_dbg_metrics)
#define FSN_DEBUG_RECORD g_dbg_metrics

constexpr int kSsimTile = 32;
constexpr int kSsimThreads = 256;
constexpr int kSsimRowsPerThread = kSsimTile * kSsimTile / kSsimThreads;  // 4
constexpr int kSqErrChunk = kSsimThreads * 16;                              // elements per squared-error workgroup

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

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// fixed-order sum over the 256 threads of the workgroup; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();  // red may still be read by an earlier call
  if (lane == 0) red[wid] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int k = 0; k < kSsimThreads / 64; ++k) s += red[k];
  return s;
}

template <int R>
__global__ void __launch_bounds__(kSsimThreads) k_ssim_tile(const float* __restrict__ x, const float* __restrict__ y,
                                                            int C, int H, int W, Strides4 sx, Strides4 sy, SsimParams p,
                                                            int tiles_w, int tiles, float* __restrict__ smap, Strides4 ss,
                                                            double* __restrict__ partials) {
  constexpr int T = kSsimTile, HB = T + 2 * R, K = 2 * R + 1;
  __shared__ float lx[HB][HB + 1];
  __shared__ float ly[HB][HB + 1];
  __shared__ double hm[5][HB][T + 1];  // horizontal pass: x, y, x^2, y^2, xy
  __shared__ double red[kSsimThreads / 64];

  const int64_t blk = blockIdx.x;
  const int tile = (int)(blk % tiles);
  const int64_t nc = blk / tiles;
  const int c = (int)(nc % C);
  const int64_t n = nc / C;
  const int h0 = (tile / tiles_w) * T, w0 = (tile % tiles_w) * T;
  const float* xb = x + n * sx.n + c * sx.c;
  const float* yb = y + n * sy.n + c * sy.c;

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
  double m[5][RT];
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

  // 4. S, map, interior sum
  const int ow = w0 + q;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < RT; ++j) {
    const int oh = h0 + r0 + j;
    if (oh < H && ow < W) {
      const double ux = m[0][j], uy = m[1][j];
      const double vx = p.cn * (m[2][j] - ux * ux);
      const double vy = p.cn * (m[3][j] - uy * uy);
      const double vxy = p.cn * (m[4][j] - ux * uy);
      const double S = ((2.0 * ux * uy + p.C1) * (2.0 * vxy + p.C2)) / ((ux * ux + uy * uy + p.C1) * (vx + vy + p.C2));
      if (smap) smap[n * ss.n + c * ss.c + oh * ss.h + ow * ss.w] = (float)S;
      if (oh >= R && oh < H - R && ow >= R && ow < W - R) acc += S;
    }
  }
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blk] = tot;
}

// per image: the mean of S over C channels x interior (every channel has the same interior), then the mean over images
__global__ void __launch_bounds__(kSsimThreads) k_ssim_finish(const double* __restrict__ partials, int64_t N, int64_t per_image,
                                                              double inv_count, double* __restrict__ out) {
  __shared__ double red[kSsimThreads / 64];
  double mean = 0.0;
  for (int64_t n = 0; n < N; ++n) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < per_image; i += kSsimThreads) s += partials[n * per_image + i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
      out[n] = s * inv_count;
      mean += out[n];
    }
  }
  if (threadIdx.x == 0) out[N] = mean / (double)N;
}

// squared error: one partial per (image, chunk of kSqErrChunk elements in (h, w, c) order)
__global__ void __launch_bounds__(kSsimThreads) k_sqerr_partial(const float* __restrict__ x, const float* __restrict__ y,
                                                                int C, int W, int64_t per_image, Strides4 sx, Strides4 sy,
                                                                int64_t chunks, double* __restrict__ partials) {
  __shared__ double red[kSsimThreads / 64];
  const int64_t blk = blockIdx.x;
  const int64_t n = blk / chunks, e0 = (blk % chunks) * kSqErrChunk;
  const int64_t e1 = min(e0 + (int64_t)kSqErrChunk, per_image);
  double acc = 0.0;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += kSsimThreads) {
    const int64_t hw = e / C;
    const int c = (int)(e - hw * C);
    const int64_t h = hw / W, w = hw - h * W;
    const double d = (double)x[n * sx.n + c * sx.c + h * sx.h + w * sx.w] - (double)y[n * sy.n + c * sy.c + h * sy.h + w * sy.w];
    acc += d * d;
  }
  const double tot = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blk] = tot;
}

__global__ void __launch_bounds__(kSsimThreads) k_psnr_finish(const double* __restrict__ partials, int64_t N, int64_t chunks,
                                                              int64_t per_image, float* __restrict__ out) {
  __shared__ double red[kSsimThreads / 64];
  double total = 0.0;
  for (int64_t n = 0; n < N; ++n) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < chunks; i += kSsimThreads) s += partials[n * chunks + i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
      out[n] = (float)(-10.0 * log10(s / (double)per_image));
      total += s;
    }
  }
  if (threadIdx.x == 0) out[N] = (float)(-10.0 * log10(total / ((double)per_image * (double)N)));
}

static int ssim_radius(int window) { return window == FSN_SSIM_GAUSSIAN ? 5 : 3; }

static int check_strides(const int64_t* s, const char* what) {
  FSN_REQUIRE(s, FSN_E_INVALID, "%s: null stride array", what);
  return FSN_OK;
}

static Strides4 strides4(const int64_t* s) { return Strides4{s[0], s[1], s[2], s[3]}; }

}  // namespace fsn

using namespace fsn;

static int64_t ssim_tiles(int H, int W) {
  return (int64_t)((H + kSsimTile - 1) / kSsimTile) * ((W + kSsimTile - 1) / kSsimTile);
}

extern "C" int64_t fsn_ssim_workspace_doubles(int64_t N, int C, int H, int W) {
  FSN_REQUIRE(N >= 0 && C >= 1 && H >= 1 && W >= 1, FSN_E_INVALID, "fsn_ssim_workspace_doubles: bad shape");
  return N * C * ssim_tiles(H, W);
}

extern "C" int fsn_ssim(const float* x, const float* y, int64_t N, int C, int H, int W, const int64_t* x_strides_host,
                        const int64_t* y_strides_host, int window, int use_sample_covariance, double data_range,
                        double K1, double K2, double* workspace, double* out, float* smap,
                        const int64_t* smap_strides_host, fsn_stream_t stream) {
  FSN_REQUIRE(N >= 0 && C >= 1 && H >= 1 && W >= 1, FSN_E_INVALID, "fsn_ssim: bad shape (N=%lld C=%d H=%d W=%d)",
              (long long)N, C, H, W);
  FSN_REQUIRE(window == FSN_SSIM_GAUSSIAN || window == FSN_SSIM_UNIFORM, FSN_E_UNSUPPORTED,
              "fsn_ssim: unknown window code %d", window);
  const int r = ssim_radius(window), win = 2 * r + 1;
  FSN_REQUIRE(H >= win && W >= win, FSN_E_INVALID, "fsn_ssim: image %dx%d is smaller than the %dx%d window", H, W,
              win, win);
  if (N == 0) return FSN_OK;
  FSN_REQUIRE(x && y && workspace && out, FSN_E_INVALID, "fsn_ssim: null pointer");
  int rc = check_strides(x_strides_host, "fsn_ssim");
  if (rc == FSN_OK) rc = check_strides(y_strides_host, "fsn_ssim");
  if (rc == FSN_OK && smap) rc = check_strides(smap_strides_host, "fsn_ssim");
  if (rc != FSN_OK) return rc;
  const int64_t tiles = ssim_tiles(H, W), blocks = N * C * tiles;
  FSN_REQUIRE(blocks < (int64_t(1) << 31), FSN_E_UNSUPPORTED, "fsn_ssim: %lld tiles in one call", (long long)blocks);

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

  const Strides4 sx = strides4(x_strides_host), sy = strides4(y_strides_host);
  const Strides4 ss = smap ? strides4(smap_strides_host) : Strides4{0, 0, 0, 0};
  const int tiles_w = (W + kSsimTile - 1) / kSsimTile;
  hipStream_t s = as_stream(stream);
  if (window == FSN_SSIM_GAUSSIAN)
    k_ssim_tile<5><<<(unsigned)blocks, kSsimThreads, 0, s>>>(x, y, C, H, W, sx, sy, p, tiles_w, (int)tiles, smap, ss,
                                                            workspace);
  else
    k_ssim_tile<3><<<(unsigned)blocks, kSsimThreads, 0, s>>>(x, y, C, H, W, sx, sy, p, tiles_w, (int)tiles, smap, ss,
                                                            workspace);
  FSN_LAUNCH_CHECK("k_ssim_tile");
  const double count = (double)C * (double)(H - 2 * r) * (double)(W - 2 * r);
  k_ssim_finish<<<1, kSsimThreads, 0, s>>>(workspace, N, C * tiles, 1.0 / count, out);
  FSN_LAUNCH_CHECK("k_ssim_finish");
  return FSN_OK;
}

extern "C" int64_t fsn_psnr_workspace_doubles(int64_t N, int C, int H, int W) {
  FSN_REQUIRE(N >= 0 && C >= 1 && H >= 1 && W >= 1, FSN_E_INVALID, "fsn_psnr_workspace_doubles: bad shape");
  const int64_t per_image = (int64_t)C * H * W;
  return N * ((per_image + kSqErrChunk - 1) / kSqErrChunk);
}

extern "C" int fsn_psnr(const float* x, const float* y, int64_t N, int C, int H, int W, const int64_t* x_strides_host,
                        const int64_t* y_strides_host, double* workspace, float* out, fsn_stream_t stream) {
  FSN_REQUIRE(N >= 0 && C >= 1 && H >= 1 && W >= 1, FSN_E_INVALID, "fsn_psnr: bad shape (N=%lld C=%d H=%d W=%d)",
              (long long)N, C, H, W);
  if (N == 0) return FSN_OK;
  FSN_REQUIRE(x && y && workspace && out, FSN_E_INVALID, "fsn_psnr: null pointer");
  int rc = check_strides(x_strides_host, "fsn_psnr");
  if (rc == FSN_OK) rc = check_strides(y_strides_host, "fsn_psnr");
  if (rc != FSN_OK) return rc;
  const int64_t per_image = (int64_t)C * H * W, chunks = (per_image + kSqErrChunk - 1) / kSqErrChunk;
  FSN_REQUIRE(N * chunks < (int64_t(1) << 31), FSN_E_UNSUPPORTED, "fsn_psnr: too many elements in one call");
  hipStream_t s = as_stream(stream);
  k_sqerr_partial<<<(unsigned)(N * chunks), kSsimThreads, 0, s>>>(x, y, C, W, per_image, strides4(x_strides_host),
                                                                  strides4(y_strides_host), chunks, workspace);
  FSN_LAUNCH_CHECK("k_sqerr_partial");
  k_psnr_finish<<<1, kSsimThreads, 0, s>>>(workspace, N, chunks, per_image, out);
  FSN_LAUNCH_CHECK("k_psnr_finish");
  return FSN_OK;
}

extern "C" int fsn_debug_report_metrics(uint32_t* out_host) {
  FSN_REQUIRE(out_host, FSN_E_INVALID, "fsn_debug_report_metrics: null pointer");
#ifdef FSN_DEBUG
  FSN_HIP(hipDeviceSynchronize());
  unsigned zero[4] = {0u, 0u, 0u, 0u};
  FSN_HIP(hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_dbg_metrics), sizeof(unsigned) * 4));
  FSN_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_dbg_metrics), zero, sizeof(zero)));
  return FSN_OK;
#else
  FSN_REQUIRE(false, FSN_E_UNSUPPORTED, "fsn_debug_report_metrics: not a debug build (make -C fs-nerf_amd/csrc debug)");
#endif
}
