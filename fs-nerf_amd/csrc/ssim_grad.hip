// ssim_grad.hip — the backward of fsn_ssim's interior mean (metrics.hip): d(sum_n upstream[n] ssim_n) / dx and / dy,
// for the structural (D-SSIM) term of patch-mode training.  Per image n and channel, with metrics.hip's window taps w,
// radius r, cn, C1, C2 and moments ux, uy, uxx, uyy, uxy:
//   A1 = 2 ux uy + C1                      B1 = ux^2 + uy^2 + C1
//   A2 = 2 cn (uxy - ux uy) + C2           B2 = cn (uxx - ux^2 + uyy - uy^2) + C2          S = A1 A2 / (B1 B2)
// On the interior q in [r, H-r) x [r, W-r), with g = upstream[n] / (C (H-2r) (W-2r)), and zero elsewhere:
//   Suxy = 2 cn A1 / (B1 B2)
//   Suxx = Suyy = -S cn / B2
//   Sux  = (2 uy A2 - 2 cn uy A1) / (B1 B2) - 2 S ux / B1 + 2 S cn ux / B2          (Suy: x and y swapped)
//   dx(p) = F[g Sux](p) + 2 x(p) F[g Suxx](p) + y(p) F[g Suxy](p)                    (dy: x and y swapped)
// where F[m](p) = sum_q w(q - p) m(q).  The window of an interior pixel never leaves the image, so the adjoint of the
// filter is exact with zero extension and the reflect edges of the forward play no part.
// Two kernels on metrics.hip's tiling (one 256-thread workgroup per image, channel and 32x32 tile):
//   k_ssim_grad_maps    the moments of the tile (ssim_dev.hpp, the forward's own steps 1-3) -> the four masked
//                       coefficient maps g Sux, g Suy, g Suxx, g Suxy in the workspace, [N, C, 4, H, W] float64;
//   k_ssim_grad_filter  one map at a time: its (32+2r)^2 halo (zero outside the image) to LDS, horizontal pass to LDS,
//                       vertical pass in registers; then the combination with x and y, rounded ONCE to float32.
// Gather form: every output pixel sums over its own window in a fixed order - no atomics, bitwise reproducible, and an
// image's gradient does not depend on what else is in the batch.
// Precision: float64 throughout for the reason in metrics.hip's header.  Here it matters more: for a near-identical
// pair the terms of Sux are of size 2 cn ux / C2 ~ 2000 and cancel to ~0.
#include "common.hpp"

namespace fsn {
// debug build: the LDS indices of both kernels are range-checked (common.hpp), read by fsn_debug_report("ssim_grad")
FSN_DEBUG_DEFINE_RECORD(ssim_grad)
}  // namespace fsn
#define FSN_DEBUG_RECORD g_dbg_ssim_grad
#include "ssim_dev.hpp"

namespace fsn {

constexpr int kSsimGradMaps = 4;  // g Sux, g Suy, g Suxx, g Suxy

struct TileAt {
  int64_t n;
  int c, h0, w0;
};

__device__ __forceinline__ TileAt tile_at(int C, int tiles_w, int tiles) {
  const int64_t blk = blockIdx.x;
  const int tile = (int)(blk % tiles);
  const int64_t nc = blk / tiles;
  return TileAt{nc / C, (int)(nc % C), (tile / tiles_w) * kSsimTile, (tile % tiles_w) * kSsimTile};
}

template <int R>
__global__ void __launch_bounds__(kSsimThreads) k_ssim_grad_maps(const float* __restrict__ x, const float* __restrict__ y,
                                                                 int C, int H, int W, Strides4 sx, Strides4 sy, SsimParams p,
                                                                 int tiles_w, int tiles, const double* __restrict__ upstream,
                                                                 double count, double* __restrict__ maps) {
  constexpr int T = kSsimTile, HB = T + 2 * R, RT = kSsimRowsPerThread;
  __shared__ float lx[HB][HB + 1];
  __shared__ float ly[HB][HB + 1];
  __shared__ double hm[5][HB][T + 1];

  const TileAt t = tile_at(C, tiles_w, tiles);
  const int q = threadIdx.x % T, r0 = (threadIdx.x / T) * RT;
  double m[5][RT];
  ssim_tile_moments<R>(x + t.n * sx.n + t.c * sx.c, y + t.n * sy.n + t.c * sy.c, H, W, sx, sy, p, t.h0, t.w0, lx, ly, hm, m);

  const double g = upstream[t.n] / count;
  const int64_t plane = (int64_t)H * W;
  double* mb = maps + (t.n * C + t.c) * kSsimGradMaps * plane;
  const int ow = t.w0 + q;
#pragma unroll
  for (int j = 0; j < RT; ++j) {
    const int oh = t.h0 + r0 + j;
    if (oh >= H || ow >= W) continue;
    double cux = 0.0, cuy = 0.0, cuxx = 0.0, cuxy = 0.0;  // outside the interior the maps are zero
    if (oh >= R && oh < H - R && ow >= R && ow < W - R) {
      const double ux = m[0][j], uy = m[1][j];
      const double A1 = 2.0 * ux * uy + p.C1;
      const double A2 = 2.0 * p.cn * (m[4][j] - ux * uy) + p.C2;
      const double B1 = ux * ux + uy * uy + p.C1;
      const double B2 = p.cn * ((m[2][j] - ux * ux) + (m[3][j] - uy * uy)) + p.C2;
      const double D = B1 * B2;
      const double S = (A1 * A2) / D;
      cuxy = g * (2.0 * p.cn * A1 / D);
      cuxx = g * (-S * p.cn / B2);
      cux = g * ((2.0 * uy * A2 - 2.0 * p.cn * uy * A1) / D - 2.0 * S * ux / B1 + 2.0 * S * p.cn * ux / B2);
      cuy = g * ((2.0 * ux * A2 - 2.0 * p.cn * ux * A1) / D - 2.0 * S * uy / B1 + 2.0 * S * p.cn * uy / B2);
    }
    const int64_t at = (int64_t)oh * W + ow;
    mb[at] = cux;
    mb[plane + at] = cuy;
    mb[2 * plane + at] = cuxx;
    mb[3 * plane + at] = cuxy;
  }
}

template <int R>
__global__ void __launch_bounds__(kSsimThreads) k_ssim_grad_filter(const float* __restrict__ x, const float* __restrict__ y,
                                                                   int C, int H, int W, Strides4 sx, Strides4 sy, SsimParams p,
                                                                   int tiles_w, int tiles, const double* __restrict__ maps,
                                                                   float* __restrict__ dx, Strides4 sdx,
                                                                   float* __restrict__ dy, Strides4 sdy) {
  constexpr int T = kSsimTile, HB = T + 2 * R, K = 2 * R + 1, RT = kSsimRowsPerThread;
  __shared__ double lm[HB][HB + 1];  // one map's halo
  __shared__ double hm[HB][T + 1];   // its horizontal pass

  const TileAt t = tile_at(C, tiles_w, tiles);
  const int64_t plane = (int64_t)H * W;
  const double* mb = maps + (t.n * C + t.c) * kSsimGradMaps * plane;
  const int q = threadIdx.x % T, r0 = (threadIdx.x / T) * RT;
  double F[kSsimGradMaps][RT];
#pragma unroll
  for (int k = 0; k < kSsimGradMaps; ++k) {
#pragma unroll
    for (int j = 0; j < RT; ++j) F[k][j] = 0.0;
    if ((k == 0 && !dx) || (k == 1 && !dy)) continue;  // (uniform over the workgroup)
    // halo, zero outside the image.  lm was last read before the previous map's second barrier, hm before this one.
    for (int i = threadIdx.x; i < HB * HB; i += kSsimThreads) {
      const int r = i / HB, c = i - r * HB;
      const int hh = t.h0 - R + r, ww = t.w0 - R + c;
      const bool in = hh >= 0 && hh < H && ww >= 0 && ww < W;
      FSN_AT(FSN_AT(lm, r), c) = in ? mb[k * plane + (int64_t)hh * W + ww] : 0.0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < HB * T; i += kSsimThreads) {
      const int r = i / T, c = i - r * T;
      double a = 0.0;
#pragma unroll
      for (int s = 0; s < K; ++s) a = __builtin_fma(p.taps[s], FSN_AT(FSN_AT(lm, r), c + s), a);
      FSN_AT(FSN_AT(hm, r), c) = a;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < K + RT - 1; ++s) {
      const double v = FSN_AT(FSN_AT(hm, r0 + s), q);
#pragma unroll
      for (int j = 0; j < RT; ++j) {
        const int tap = s - j;
        if (tap >= 0 && tap < K) F[k][j] = __builtin_fma(p.taps[tap], v, F[k][j]);
      }
    }
  }

  const int ow = t.w0 + q;
#pragma unroll
  for (int j = 0; j < RT; ++j) {
    const int oh = t.h0 + r0 + j;
    if (oh >= H || ow >= W) continue;
    const double xv = x[t.n * sx.n + t.c * sx.c + oh * sx.h + ow * sx.w];
    const double yv = y[t.n * sy.n + t.c * sy.c + oh * sy.h + ow * sy.w];
    if (dx) dx[t.n * sdx.n + t.c * sdx.c + oh * sdx.h + ow * sdx.w] = (float)(F[0][j] + 2.0 * xv * F[2][j] + yv * F[3][j]);
    if (dy) dy[t.n * sdy.n + t.c * sdy.c + oh * sdy.h + ow * sdy.w] = (float)(F[1][j] + 2.0 * yv * F[2][j] + xv * F[3][j]);
  }
}

}  // namespace fsn

using namespace fsn;

extern "C" int64_t fsn_ssim_grad_workspace_doubles(int64_t N, int C, int H, int W) {
  FSN_REQUIRE(N >= 0 && C >= 1 && H >= 1 && W >= 1, FSN_E_INVALID, "fsn_ssim_grad_workspace_doubles: bad shape");
  FSN_REQUIRE(N <= ((int64_t)1 << 58) / ((int64_t)C * H * W), FSN_E_UNSUPPORTED,
              "fsn_ssim_grad_workspace_doubles: more than 2^60 doubles");
  return N * C * kSsimGradMaps * H * W;
}

extern "C" int fsn_ssim_grad(const float* x, const float* y, int64_t N, int C, int H, int W, const int64_t* x_strides_host,
                             const int64_t* y_strides_host, int window, int use_sample_covariance, double data_range,
                             double K1, double K2, const double* upstream, double* workspace, float* dx,
                             const int64_t* dx_strides_host, float* dy, const int64_t* dy_strides_host,
                             fsn_stream_t stream) {
  int rc = ssim_check_shape("fsn_ssim_grad", N, C, H, W, window);
  if (rc != FSN_OK) return rc;
  if (N == 0) return FSN_OK;
  FSN_REQUIRE(x && y && upstream && workspace, FSN_E_INVALID, "fsn_ssim_grad: null pointer");
  FSN_REQUIRE(dx || dy, FSN_E_INVALID, "fsn_ssim_grad: null pointer for both gradients (dx and dy)");
  rc = check_strides(x_strides_host, "fsn_ssim_grad");
  if (rc == FSN_OK) rc = check_strides(y_strides_host, "fsn_ssim_grad");
  if (rc == FSN_OK && dx) rc = check_strides(dx_strides_host, "fsn_ssim_grad");
  if (rc == FSN_OK && dy) rc = check_strides(dy_strides_host, "fsn_ssim_grad");
  if (rc != FSN_OK) return rc;
  const int64_t tiles = ssim_tiles(H, W), blocks = N * C * tiles;
  FSN_REQUIRE(blocks < (int64_t(1) << 31), FSN_E_UNSUPPORTED, "fsn_ssim_grad: %lld tiles in one call", (long long)blocks);

  const int r = ssim_radius(window);
  const SsimParams p = ssim_params(window, use_sample_covariance, data_range, K1, K2);
  const Strides4 sx = strides4(x_strides_host), sy = strides4(y_strides_host);
  const Strides4 sdx = dx ? strides4(dx_strides_host) : Strides4{0, 0, 0, 0};
  const Strides4 sdy = dy ? strides4(dy_strides_host) : Strides4{0, 0, 0, 0};
  const int tiles_w = (W + kSsimTile - 1) / kSsimTile;
  const double count = (double)C * (double)(H - 2 * r) * (double)(W - 2 * r);
  hipStream_t s = as_stream(stream);
  if (window == FSN_SSIM_GAUSSIAN) {
    k_ssim_grad_maps<5><<<(unsigned)blocks, kSsimThreads, 0, s>>>(x, y, C, H, W, sx, sy, p, tiles_w, (int)tiles, upstream,
                                                                 count, workspace);
    FSN_LAUNCH_CHECK("k_ssim_grad_maps");
    k_ssim_grad_filter<5><<<(unsigned)blocks, kSsimThreads, 0, s>>>(x, y, C, H, W, sx, sy, p, tiles_w, (int)tiles, workspace,
                                                                   dx, sdx, dy, sdy);
  } else {
    k_ssim_grad_maps<3><<<(unsigned)blocks, kSsimThreads, 0, s>>>(x, y, C, H, W, sx, sy, p, tiles_w, (int)tiles, upstream,
                                                                 count, workspace);
    FSN_LAUNCH_CHECK("k_ssim_grad_maps");
    k_ssim_grad_filter<3><<<(unsigned)blocks, kSsimThreads, 0, s>>>(x, y, C, H, W, sx, sy, p, tiles_w, (int)tiles, workspace,
                                                                   dx, sdx, dy, sdy);
  }
  FSN_LAUNCH_CHECK("k_ssim_grad_filter");
  return FSN_OK;
}
