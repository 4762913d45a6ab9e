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
// debug build: the LDS indices of k_ssim_tile are range-checked (common.hpp), read by fsn_debug_report("metrics")
FSN_DEBUG_DEFINE_RECORD(metrics)
}  // namespace fsn
#define FSN_DEBUG_RECORD g_dbg_metrics
#include "ssim_dev.hpp"  // tile geometry, window parameters and the moments of steps 1-3, shared with ssim_grad.hip

namespace fsn {

constexpr int kSqErrChunk = kSsimThreads * 16;  // elements per squared-error workgroup

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
  constexpr int T = kSsimTile, HB = T + 2 * R;
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

  // 1-3. the windowed moments (ssim_dev.hpp): column q, output rows r0 .. r0+3 of the tile
  constexpr int RT = kSsimRowsPerThread;
  const int q = threadIdx.x % T, r0 = (threadIdx.x / T) * RT;
  double m[5][RT];
  ssim_tile_moments<R>(xb, yb, H, W, sx, sy, p, h0, w0, lx, ly, hm, m);

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

}  // namespace fsn

using namespace fsn;

extern "C" int64_t fsn_ssim_workspace_doubles(int64_t N, int C, int H, int W) {
  FSN_REQUIRE(N >= 0 && C >= 1 && H >= 1 && W >= 1, FSN_E_INVALID, "fsn_ssim_workspace_doubles: bad shape");
  return N * C * ssim_tiles(H, W);
}

extern "C" int fsn_ssim(const float* x, const float* y, int64_t N, int C, int H, int W, const int64_t* x_strides_host,
                        const int64_t* y_strides_host, int window, int use_sample_covariance, double data_range,
                        double K1, double K2, double* workspace, double* out, float* smap,
                        const int64_t* smap_strides_host, fsn_stream_t stream) {
  int rc = ssim_check_shape("fsn_ssim", N, C, H, W, window);
  if (rc != FSN_OK) return rc;
  const int r = ssim_radius(window);
  if (N == 0) return FSN_OK;
  FSN_REQUIRE(x && y && workspace && out, FSN_E_INVALID, "fsn_ssim: null pointer");
  rc = check_strides(x_strides_host, "fsn_ssim");
  if (rc == FSN_OK) rc = check_strides(y_strides_host, "fsn_ssim");
  if (rc == FSN_OK && smap) rc = check_strides(smap_strides_host, "fsn_ssim");
  if (rc != FSN_OK) return rc;
  const int64_t tiles = ssim_tiles(H, W), blocks = N * C * tiles;
  FSN_REQUIRE(blocks < (int64_t(1) << 31), FSN_E_UNSUPPORTED, "fsn_ssim: %lld tiles in one call", (long long)blocks);

  const SsimParams p = ssim_params(window, use_sample_covariance, data_range, K1, K2);
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
