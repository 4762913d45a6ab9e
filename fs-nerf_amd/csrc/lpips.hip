// lpips.hip — LPIPS v0.1 with the VGG16 backbone (the `lpips` package's LPIPS(net="vgg")), the third number of the
// reference's evaluation() (src/run-nerf.py:108-191), on the device.  Per image pair (x, y):
//   x <- 2x - 1 if normalize;  x <- (x - shift) / scale                              (k_lpips_input)
//   VGG16 features: 13 conv3x3 (padding 1, bias, ReLU), 2x2 stride-2 max-pools        (k_lpips_conv)
//   taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3: f / (sqrt(sum_c f^2) + 1e-10) per pixel, the squared
//   difference of the two images, the 1x1 `lin` weights (no bias), the spatial mean   (k_lpips_head, k_lpips_finish)
//   and the sum of the five values.
//
// Convolution = implicit GEMM on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32): M = pixels, N = Cout,
// K = 9 Cin in (tap, cin) order (the first layer's K = 27 zero-padded to 32).  One 256-thread workgroup computes a
// 128-pixel x BN-channel tile (BN = 64 for the 64-channel layers, else 128); the 128 pixels are an 8 x 16 patch ordered
// by 2x2 quads, so the four rows an MFMA accumulator register group holds are one quad.  K goes in chunks of 32: every
// chunk lies inside one tap (Cin is a multiple of 32 past the first layer), its A tile (128 pixels x 32 channels, the
// shifted source pixel, zero outside the image) and B tile (BN x 32 of the packed weights) are loaded as float4 into
// registers one chunk ahead and stored to LDS as [row][k] with a 36-float stride (ds_read_b128 without bank
// conflicts).  In a chunk, lane half h takes k = 16h + s at MFMA step s, for A and B alike, so each lane reads its
// fragments as four 16-byte LDS reads.  The epilogue adds the bias and applies ReLU.
// Max-pool: every pool of VGG16 follows a tap, whose full-resolution activations the head needs, so the pool is fused
// into the NEXT convolution's operand load (max of the four source pixels, floor on odd sizes) instead of its producer.
//
// Memory: the two images of a pair go through the network together (blockIdx.z) and the pairs one after another, so
// the workspace (two ping-pong activation buffers of 2 x 64 x H x W floats, the head partials) depends on H and W only.
// Sums: per-pixel head values in float64, one partial per workgroup, summed by one workgroup in a fixed order: no
// atomics, the results are bitwise reproducible and independent of the input layout and of the batch.
//
// As a loss (second half of the file): fsn_lpips_vgg_fwd_save runs B pairs at once (blockIdx.z over the x images, then
// the y images) through the same kernels and keeps every layer's post-ReLU activation of the images that need a
// gradient; fsn_lpips_vgg_bwd walks back: k_lpips_tap_bwd (head gradient in float64 + the gradient arriving through the
// max-pool, times the ReLU mask), the convolutions' data gradients through k_lpips_conv with Cin and Cout exchanged on
// weights packed [Cin][9 Cout] with the taps flipped, and k_lpips_first_bwd for conv1_1 and the scaling layer.
#include "common.hpp"

#include <cmath>

namespace fsn {

// debug build: the LDS indices of k_lpips_conv are range-checked (common.hpp), read by fsn_debug_report("lpips")
FSN_DEBUG_DEFINE_RECORD(lpips)
#define FSN_DEBUG_RECORD g_dbg_lpips

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kLayers = 13, kTaps = 5;
constexpr int kCin[kLayers] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int kCout[kLayers] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr bool kPoolIn[kLayers] = {false, false, true, false, true, false, false, true, false, false, true, false, false};
constexpr int kTapOf[kLayers] = {-1, 0, -1, 1, -1, -1, 2, -1, -1, 3, -1, -1, 4};  // the tap a layer's output is
constexpr int kTapC[kTaps] = {64, 128, 256, 512, 512};
constexpr int kFirstKp = 32;  // 27 padded

constexpr int kThreads = 256;
constexpr int kBM = 128, kBK = 32, kLds = 36;  // LDS row stride in floats: 16 lanes' b128 reads hit distinct banks
constexpr int kTileH = 8, kTileW = 16;         // the 128 pixels of a workgroup: 4 x 8 quads of 2 x 2
constexpr int kHeadPix = kThreads;             // pixels per head workgroup (one partial each)

static int kp_of(int l) { return l == 0 ? kFirstKp : 9 * kCin[l]; }

// float offsets of the packed blob: per layer W [Cout][Kp] then b [Cout]; lin weights of the five taps; shift[3];
// scale[3].  Every block starts on a multiple of four floats.
struct BlobLayout {
  int64_t w[kLayers], b[kLayers], lin[kTaps], shift, scale, total;
};

static BlobLayout blob_layout() {
  BlobLayout L{};
  int64_t o = 0;
  for (int l = 0; l < kLayers; ++l) {
    L.w[l] = o;
    o += (int64_t)kCout[l] * kp_of(l);
    L.b[l] = o;
    o += kCout[l];
  }
  for (int t = 0; t < kTaps; ++t) {
    L.lin[t] = o;
    o += kTapC[t];
  }
  L.shift = o;
  L.scale = o + 4;
  L.total = o + 8;
  return L;
}

struct Strides4 {
  int64_t n, c, h, w;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// fixed-order sum over the 256 threads of the workgroup; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int k = 0; k < kThreads / 64; ++k) s += red[k];
  return s;
}

// ---------------------------------------------------------------- weight pack
// [Cout][Cin][3][3] -> [Cout][Kp] with k = (ky * 3 + kx) * Cin + cin; k >= 9 Cin (first layer: 27..31) is zero
__global__ void __launch_bounds__(kThreads) k_lpips_pack_conv(const float* __restrict__ w, int Cin, int Cout, int Kp,
                                                              float* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)Cout * Kp) return;
  const int n = (int)(i / Kp), k = (int)(i - (int64_t)n * Kp);
  float v = 0.f;
  if (k < 9 * Cin) {
    const int tap = k / Cin, c = k - tap * Cin;
    v = w[((int64_t)n * Cin + c) * 9 + tap];
  }
  dst[i] = v;
}

__global__ void __launch_bounds__(kThreads) k_lpips_copy(const float* __restrict__ src, int n, float* __restrict__ dst) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// ---------------------------------------------------------------- input stage
// both images of pair n = n0 + blockIdx.y -> act [H][W][3] each: (v' - shift) / scale with v' = 2v - 1 under normalize
// (float32, the scaling layer's arithmetic).  The x image goes to slot blockIdx.y, the y image to slot y_slot0 +
// blockIdx.y (fsn_lpips_vgg: one pair, slots 0 and 1; the batched forward: the x group, then the y group)
__global__ void __launch_bounds__(kThreads) k_lpips_input(const float* __restrict__ x, const float* __restrict__ y,
                                                          Strides4 sx, Strides4 sy, int64_t n0, int H, int W,
                                                          int normalize, const float* __restrict__ shift_scale,
                                                          int64_t y_slot0, float* __restrict__ act) {
  const int64_t per = (int64_t)H * W * 3;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= 2 * per) return;
  const int img = (int)(i / per);
  const int64_t n = n0 + blockIdx.y;
  const int64_t e = i - img * per, p = e / 3;
  const int c = (int)(e - p * 3);
  const int h = (int)(p / W), w = (int)(p - (int64_t)h * W);
  const Strides4 s = img ? sy : sx;
  const float* src = img ? y : x;
  float v = src[n * s.n + c * s.c + h * s.h + w * s.w];
  if (normalize) v = 2.f * v - 1.f;
  act[((img ? y_slot0 : 0) + blockIdx.y) * per + e] = (v - shift_scale[c]) / shift_scale[4 + c];
}

// ---------------------------------------------------------------- convolution
struct ConvArgs {
  const float* in;   // source activations [split][Hs][Ws][Cin] of the images blockIdx.z < split
  const float* in2;  // ... and of the images blockIdx.z >= split (image blockIdx.z - split)
  float* out;        // [split][H][W][Cout]
  float* out2;
  int split;
  const float* mask;  // kEpiMask: the saved activation [images][H][W][Cout] whose sign gates the result
  const float* w;   // packed [Cout][Kp]
  const float* b;   // [Cout]
  int H, W;         // output (= input after the pool) size
  int Ws;           // source width (the pooled-input mode reads 2x2 windows of it)
  int Cin, Cout, Kp, tiles_w;
  int64_t in_img, out_img;  // floats per image
};

enum { kModeFirst = 0, kModePlain = 1, kModePool = 2 };
// epilogue: the forward's bias + ReLU; the data gradient as it is (its consumer is the tap kernel); the data gradient
// times the ReLU mask of the layer input's saved activation
enum { kEpiRelu = 0, kEpiRaw = 1, kEpiMask = 2 };

// pixel m (0..127) of a workgroup tile: quad m >> 2 in a 4 x 8 quad grid, position m & 3 inside the quad
__device__ __forceinline__ void tile_pixel(int m, int h0, int w0, int& h, int& w) {
  const int quad = m >> 2, r = m & 3;
  h = h0 + 2 * (quad >> 3) + (r >> 1);
  w = w0 + 2 * (quad & 7) + (r & 1);
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

__device__ __forceinline__ f32x4 max4(f32x4 a, f32x4 b) {
  f32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = a[j] > b[j] || a[j] != a[j] ? a[j] : b[j];  // NaN propagates, as max_pool2d's
  return r;
}

template <int BN, int MODE, int EPI>
__global__ void __launch_bounds__(kThreads) k_lpips_conv(ConvArgs a) {
  constexpr int TN = BN / 64;                   // 32 x 32 accumulator tiles per wave along N (the wave's M: 2 tiles)
  constexpr int BLD = BN * kBK / 4 / kThreads;  // float4 loads of B per thread and chunk
  __shared__ __attribute__((aligned(16))) float As[kBM][kLds];
  __shared__ __attribute__((aligned(16))) float Bs[BN][kLds];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1, li = lane & 31, lh = lane >> 5;
  const int tile = blockIdx.x, img = blockIdx.z, n0 = blockIdx.y * BN;
  const int h0 = (tile / a.tiles_w) * kTileH, w0 = (tile % a.tiles_w) * kTileW;
  const int simg = img < a.split ? img : img - a.split;
  const float* in = (img < a.split ? a.in : a.in2) + simg * a.in_img;
  const float* wp = a.w + (int64_t)n0 * a.Kp;
  const int H = a.H, W = a.W, Cin = a.Cin;

  f32x16 acc[2][TN];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

  // the A rows (pixels) and the k quad this thread loads: m = (tid >> 3) + 32 i, channels 4q .. 4q+3 of the chunk
  const int q = tid & 7;
  f32x4 ra[4], rb[BLD];
  auto load = [&](int kc) {
    const int k0 = kc * kBK, tap = k0 / Cin, c0 = k0 - tap * Cin + 4 * q;
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int h, w;
      tile_pixel((tid >> 3) + 32 * i, h0, w0, h, w);
      const int sh = h + dy, sw = w + dx;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (sh >= 0 && sh < H && sw >= 0 && sw < W) {
        if (MODE == kModePool) {
          const int64_t row = (int64_t)a.Ws * Cin;
          const float* p = in + ((int64_t)(2 * sh) * a.Ws + 2 * sw) * Cin + c0;
          v = max4(max4(ld4(p), ld4(p + Cin)), max4(ld4(p + row), ld4(p + row + Cin)));
        } else {
          v = ld4(in + ((int64_t)sh * W + sw) * Cin + c0);
        }
      }
      ra[i] = v;
    }
#pragma unroll
    for (int j = 0; j < BLD; ++j) {
      const int e = tid + kThreads * j, n = e >> 3;
      rb[j] = ld4(wp + (int64_t)n * a.Kp + k0 + 4 * (e & 7));
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<f32x4*>(FSN_SPAN(FSN_AT(As, (tid >> 3) + 32 * i), 4 * q, 4)) = ra[i];
#pragma unroll
    for (int j = 0; j < BLD; ++j) {
      const int e = tid + kThreads * j;
      *reinterpret_cast<f32x4*>(FSN_SPAN(FSN_AT(Bs, e >> 3), 4 * (e & 7), 4)) = rb[j];
    }
  };
  auto compute = [&]() {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 av[2], bv[TN];
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
        av[tm] = *reinterpret_cast<const f32x4*>(FSN_SPAN(FSN_AT(As, 64 * wm + 32 * tm + li), 16 * lh + 4 * j, 4));
#pragma unroll
      for (int tn = 0; tn < TN; ++tn)
        bv[tn] = *reinterpret_cast<const f32x4*>(FSN_SPAN(FSN_AT(Bs, (BN / 2) * wn + 32 * tn + li), 16 * lh + 4 * j, 4));
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
          for (int tn = 0; tn < TN; ++tn)
            acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm][s], bv[tn][s], acc[tm][tn], 0, 0, 0);
    }
  };

  if (MODE == kModeFirst) {
    // Cin = 3, K = 27 padded to 32: one chunk, element (m, k) with k = tap * 3 + c
    for (int e = tid; e < kBM * kBK; e += kThreads) {
      const int m = e >> 5, k = e & 31;
      float v = 0.f;
      if (k < 27) {
        const int tap = k / 3, c = k - 3 * tap;
        int h, w;
        tile_pixel(m, h0, w0, h, w);
        const int sh = h + tap / 3 - 1, sw = w + tap % 3 - 1;
        if (sh >= 0 && sh < H && sw >= 0 && sw < W) v = in[((int64_t)sh * W + sw) * 3 + c];
      }
      FSN_AT(FSN_AT(As, m), k) = v;
    }
#pragma unroll
    for (int j = 0; j < BLD; ++j) {
      const int e = tid + kThreads * j;
      rb[j] = ld4(wp + (int64_t)(e >> 3) * a.Kp + 4 * (e & 7));
      *reinterpret_cast<f32x4*>(FSN_SPAN(FSN_AT(Bs, e >> 3), 4 * (e & 7), 4)) = rb[j];
    }
    __syncthreads();
    compute();
  } else {
    const int nk = a.Kp / kBK;
    load(0);
    for (int kc = 0; kc < nk; ++kc) {
      store();
      __syncthreads();
      if (kc + 1 < nk) load(kc + 1);  // in flight while the MFMAs of this chunk run
      compute();
      __syncthreads();
    }
  }

  // epilogue: accumulator register r of lane (li, lh) is row (r & 3) + 8 (r >> 2) + 4 lh, column li of its tile
  float* out = (img < a.split ? a.out : a.out2) + simg * a.out_img;
  const float* mask = EPI == kEpiMask ? a.mask + img * a.out_img : nullptr;
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    const int n = n0 + (BN / 2) * wn + 32 * tn + li;
    const float bn = EPI == kEpiRelu ? a.b[n] : 0.f;
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int h, w;
        tile_pixel(64 * wm + 32 * tm + (r & 3) + 8 * (r >> 2) + 4 * lh, h0, w0, h, w);
        if (h < H && w < W) {
          const int64_t o = ((int64_t)h * W + w) * a.Cout + n;
          if (EPI == kEpiRelu) {
            const float v = acc[tm][tn][r] + bn;
            out[o] = v < 0.f ? 0.f : v;  // ReLU (a NaN stays a NaN)
          } else if (EPI == kEpiMask) {
            out[o] = mask[o] > 0.f ? acc[tm][tn][r] : 0.f;
          } else {
            out[o] = acc[tm][tn][r];
          }
        }
      }
  }
}

// ---------------------------------------------------------------- head
// per pixel p of a tap of pair blockIdx.y (ax, ay: the x and the y images [pairs][HW][C]):
// sum_c lin[c] (fx / (|fx| + 1e-10) - fy / (|fy| + 1e-10))^2 in float64; one partial (the workgroup's sum) per kHeadPix
// pixels of one pair, pair b's at partials + b * pair_stride
__global__ void __launch_bounds__(kThreads) k_lpips_head(const float* __restrict__ ax, const float* __restrict__ ay,
                                                         int64_t HW, int C, const float* __restrict__ lin,
                                                         double* __restrict__ partials, int64_t pair_stride) {
  __shared__ double red[kThreads / 64];
  const int64_t p = (int64_t)blockIdx.x * kHeadPix + threadIdx.x;
  double v = 0.0;
  if (p < HW) {
    const float* fx = ax + (blockIdx.y * HW + p) * C;
    const float* fy = ay + (blockIdx.y * HW + p) * C;
    double sxx = 0.0, syy = 0.0;
    for (int c = 0; c < C; c += 4) {
      const f32x4 u = ld4(fx + c), w = ld4(fy + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sxx += (double)u[j] * (double)u[j];
        syy += (double)w[j] * (double)w[j];
      }
    }
    const double ix = 1.0 / (sqrt(sxx) + 1e-10), iy = 1.0 / (sqrt(syy) + 1e-10);
    for (int c = 0; c < C; c += 4) {
      const f32x4 u = ld4(fx + c), w = ld4(fy + c), l = ld4(lin + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double d = (double)u[j] * ix - (double)w[j] * iy;
        v += (double)l[j] * d * d;
      }
    }
  }
  const double tot = block_sum(v, red);
  if (threadIdx.x == 0) partials[blockIdx.y * pair_stride + blockIdx.x] = tot;
}

struct FinishArgs {
  int64_t off[kTaps], count[kTaps];  // each tap's partials
  double inv_hw[kTaps];
};

// pair n = n0 + blockIdx.x (its partials at blockIdx.x * pair_stride): each tap's partials in a fixed order -> its
// spatial mean; out[n] = the sum over the taps
__global__ void __launch_bounds__(kThreads) k_lpips_finish(const double* __restrict__ partials, int64_t pair_stride,
                                                           FinishArgs f, int64_t n0, int64_t N, float* __restrict__ out,
                                                           float* __restrict__ per_layer) {
  __shared__ double red[kThreads / 64];
  const int64_t n = n0 + blockIdx.x;
  partials += blockIdx.x * pair_stride;
  double total = 0.0;
  for (int t = 0; t < kTaps; ++t) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < f.count[t]; i += kThreads) s += partials[f.off[t] + i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
      const double val = s * f.inv_hw[t];
      total += val;
      if (per_layer) per_layer[t * N + n] = (float)val;
    }
  }
  if (threadIdx.x == 0) out[n] = (float)total;
}

struct Dims {
  int H[kTaps], W[kTaps];  // the five stages' sizes
};

static Dims stage_dims(int H, int W) {
  Dims d{};
  for (int s = 0; s < kTaps; ++s) {
    d.H[s] = s == 0 ? H : d.H[s - 1] / 2;
    d.W[s] = s == 0 ? W : d.W[s - 1] / 2;
  }
  return d;
}

static int64_t head_blocks(int64_t hw) { return (hw + kHeadPix - 1) / kHeadPix; }

static int64_t act_floats(int H, int W) { return 2 * 64 * (int64_t)H * W; }  // one ping-pong buffer: stage 1 is largest

static int64_t partial_count(int H, int W) {
  const Dims d = stage_dims(H, W);
  int64_t p = 0;
  for (int t = 0; t < kTaps; ++t) p += head_blocks((int64_t)d.H[t] * d.W[t]);
  return p;
}

constexpr int kMaxSide = 1 << 14;

// ================================================================ the gradient with respect to the images
// ---------------------------------------------------------------- data-gradient weight pack
// dX = conv3x3(dY, W') with W'[ci][tap][co] = W[co][ci][8 - tap]: the forward's implicit GEMM with Cin and Cout
// exchanged.  [Cout][Cin][3][3] -> [Cin][9 Cout] with k = tap * Cout + co, the [N][Kp] layout k_lpips_conv reads.
__global__ void __launch_bounds__(kThreads) k_lpips_pack_dgrad(const float* __restrict__ w, int Cin, int Cout,
                                                               float* __restrict__ dst) {
  const int64_t K = 9 * (int64_t)Cout;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)Cin * K) return;
  const int ci = (int)(i / K), k = (int)(i - ci * K);
  const int tap = k / Cout, co = k - tap * Cout;
  dst[i] = w[((int64_t)co * Cin + ci) * 9 + (8 - tap)];
}

// the first layer's [64][3][3][3] -> [tap][ci][co] with the tap flipped (k_lpips_first_bwd)
__global__ void __launch_bounds__(kThreads) k_lpips_pack_dgrad_first(const float* __restrict__ w, float* __restrict__ dst) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= 27 * 64) return;
  const int tap = i / 192, ci = (i - tap * 192) / 64, co = i & 63;
  dst[i] = w[(co * 3 + ci) * 9 + (8 - tap)];
}

struct GradBlobLayout {
  int64_t w[kLayers], total;  // w[0]: the first layer's [9][3][64]; w[l]: [Cin][9 Cout]
};

static GradBlobLayout grad_blob_layout() {
  GradBlobLayout L{};
  int64_t o = 0;
  for (int l = 0; l < kLayers; ++l) {
    L.w[l] = o;
    o += l == 0 ? 27 * 64 : (int64_t)kCin[l] * 9 * kCout[l];
  }
  L.total = o;
  return L;
}

// ---------------------------------------------------------------- tap backward
// One tap of pair b = blockIdx.y, eight threads per pixel (thread j of a pixel takes the channel quads j, j + 8, ...),
// float64.  With s = |f|, u = f / (s + eps), g_c = 2 lin_c (ux_c - uy_c) up[b] / HW the head's gradient is
//   x image:  g_k / (sx + eps) - fx_k (g . fx) / (sx (sx + eps)^2),     y image: the same with -g and fy;
// a pixel whose tap vector is all zero gets 0 (autograd: NaN, 0 * inf from sqrt).  To it the kernel adds what arrives
// through the max-pool from the next stage (`pooled`: the raw data gradient of that stage's first convolution, at the
// pooled size Hp x Wp = floor(H / 2) x floor(W / 2)): a window's value goes to its FIRST maximum in row-major order
// (max_pool2d's rule); an odd last row or column lies in no window.  The sum, where f > 0 (the ReLU mask), is the
// gradient with respect to the tap layer's pre-activation, rounded once to float32.
struct TapBwdArgs {
  const float* fx;  // the tap's activations, x group and y group: [B][HW][C]
  const float* fy;
  const float* lin;
  const double* up;  // [B]
  const float* px;   // pooled gradients [B][Hp Wp][C] of the two groups, or null (relu5_3 starts the chain)
  const float* py;
  float* gx;  // out [B][HW][C]; null: that image has no gradient
  float* gy;
  int H, W, C, Hp, Wp;
};

constexpr int kTapSub = 8, kTapPix = kThreads / kTapSub;

__device__ __forceinline__ double sub_sum8(double v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}

__global__ void __launch_bounds__(kThreads) k_lpips_tap_bwd(TapBwdArgs a) {
  const int sub = threadIdx.x & (kTapSub - 1), C = a.C;
  const int64_t HW = (int64_t)a.H * a.W, b = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * kTapPix + (threadIdx.x >> 3);
  const bool ok = p < HW;  // (the threads past the end still take part in the shuffles)
  const float* fx = a.fx + (b * HW + (ok ? p : 0)) * C;
  const float* fy = a.fy + (b * HW + (ok ? p : 0)) * C;
  double sxx = 0.0, syy = 0.0;
  if (ok)
    for (int c = 4 * sub; c < C; c += 4 * kTapSub) {
      const f32x4 u = ld4(fx + c), w = ld4(fy + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sxx += (double)u[j] * (double)u[j];
        syy += (double)w[j] * (double)w[j];
      }
    }
  sxx = sub_sum8(sxx);
  syy = sub_sum8(syy);
  const double sx = sqrt(sxx), sy = sqrt(syy);
  const double ix = 1.0 / (sx + 1e-10), iy = 1.0 / (sy + 1e-10);
  double dfx = 0.0, dfy = 0.0;  // sum_c lin_c (ux_c - uy_c) f_c for the two images
  if (ok)
    for (int c = 4 * sub; c < C; c += 4 * kTapSub) {
      const f32x4 u = ld4(fx + c), w = ld4(fy + c), l = ld4(a.lin + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double ld = (double)l[j] * ((double)u[j] * ix - (double)w[j] * iy);
        dfx += ld * (double)u[j];
        dfy += ld * (double)w[j];
      }
    }
  dfx = sub_sum8(dfx);
  dfy = sub_sum8(dfy);
  if (!ok) return;
  const double k = 2.0 * a.up[b] / (double)HW;
  const double cx = sx > 0.0 ? k * dfx * ix * ix / sx : 0.0, cy = sy > 0.0 ? k * dfy * iy * iy / sy : 0.0;
  const double kx = sx > 0.0 ? k * ix : 0.0, ky = sy > 0.0 ? k * iy : 0.0;

  const int h = (int)(p / a.W), w = (int)(p - (int64_t)h * a.W);
  const bool pooled = a.px != nullptr && (h >> 1) < a.Hp && (w >> 1) < a.Wp;
  const int r = 2 * (h & 1) + (w & 1);  // this pixel's place in its window, row-major
  const int64_t win0 = (b * HW + (int64_t)(h & ~1) * a.W + (w & ~1)) * C;  // the window's first pixel
  const int64_t pin = pooled ? ((b * a.Hp + (h >> 1)) * a.Wp + (w >> 1)) * C : 0;
  // the pooled gradient of the channels c .. c + 3 where this pixel is its window's first maximum, else 0
  auto through_pool = [&](const float* act, const float* pg, int c) {
    f32x4 out = {0.f, 0.f, 0.f, 0.f};
    if (!pooled) return out;
    const float* q = act + win0 + c;
    const f32x4 v[4] = {ld4(q), ld4(q + C), ld4(q + (int64_t)a.W * C), ld4(q + (int64_t)a.W * C + C)};
    const f32x4 g = ld4(pg + pin + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float mine = r == 0 ? v[0][j] : r == 1 ? v[1][j] : r == 2 ? v[2][j] : v[3][j];
      bool win = true;
#pragma unroll
      for (int o = 0; o < 4; ++o) win = win && (o < r ? mine > v[o][j] : o > r ? mine >= v[o][j] : true);
      out[j] = win ? g[j] : 0.f;
    }
    return out;
  };
  for (int c = 4 * sub; c < C; c += 4 * kTapSub) {
    const f32x4 u = ld4(fx + c), v = ld4(fy + c), l = ld4(a.lin + c);
    double d[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = (double)l[j] * ((double)u[j] * ix - (double)v[j] * iy);
    if (a.gx) {
      const f32x4 in = through_pool(a.fx, a.px, c);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o[j] = u[j] > 0.f ? (float)(kx * d[j] - (double)u[j] * cx + (double)in[j]) : 0.f;
      *reinterpret_cast<f32x4*>(a.gx + (b * HW + p) * C + c) = o;
    }
    if (a.gy) {
      const f32x4 in = through_pool(a.fy, a.py, c);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o[j] = v[j] > 0.f ? (float)((double)v[j] * cy - ky * d[j] + (double)in[j]) : 0.f;
      *reinterpret_cast<f32x4*>(a.gy + (b * HW + p) * C + c) = o;
    }
  }
}

// ---------------------------------------------------------------- first layer and input stage, backward
// conv1_1's data gradient has three channels (a matrix-core tile would be 95 % padding): four threads per pixel, each
// 16 of the 64 channels of the nine neighbours (576 multiply-adds per colour), summed over the four in a fixed order;
// then the scaling layer (/ scale, and x 2 under normalize) and the store through the gradient tensor's own strides.
struct FirstBwdArgs {
  const float* g;      // gradient w.r.t. conv1_1's pre-activation [B][H][W][64]
  const float* w;      // [9][3][64], tap flipped
  const float* scale;  // 3 floats
  float* d;            // image gradient of pair blockIdx.y, element strides s
  Strides4 s;
  int H, W, normalize;
};

constexpr int kFirstSub = 4, kFirstPix = kThreads / kFirstSub;

__global__ void __launch_bounds__(kThreads) k_lpips_first_bwd(FirstBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float Wl[27 * 64];
  for (int e = threadIdx.x; e < 27 * 64; e += kThreads) FSN_AT(Wl, e) = a.w[e];
  __syncthreads();
  const int sub = threadIdx.x & (kFirstSub - 1), H = a.H, W = a.W;
  const int64_t HW = (int64_t)H * W, b = blockIdx.y;
  const int64_t p = (int64_t)blockIdx.x * kFirstPix + (threadIdx.x >> 2);
  const bool ok = p < HW;
  const int h = ok ? (int)(p / W) : 0, w = ok ? (int)(p - (int64_t)h * W) : 0;
  const float* g = a.g + b * HW * 64;
  float acc[3] = {0.f, 0.f, 0.f};
  if (ok)
    for (int tap = 0; tap < 9; ++tap) {
      const int sh = h + tap / 3 - 1, sw = w + tap % 3 - 1;
      if (sh < 0 || sh >= H || sw < 0 || sw >= W) continue;
      const float* src = g + ((int64_t)sh * W + sw) * 64;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * (sub + kFirstSub * j);
        const f32x4 v = ld4(src + c);
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(FSN_SPAN(Wl, (tap * 3 + ci) * 64 + c, 4));
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[ci] = __builtin_fmaf(v[e], wv[e], acc[ci]);
        }
      }
    }
#pragma unroll
  for (int ci = 0; ci < 3; ++ci) {
    acc[ci] += __shfl_xor(acc[ci], 1, 64);
    acc[ci] += __shfl_xor(acc[ci], 2, 64);
  }
  if (ok && sub < 3) {
    float v = (sub == 0 ? acc[0] : sub == 1 ? acc[1] : acc[2]) / a.scale[sub];
    if (a.normalize) v *= 2.f;
    a.d[b * a.s.n + sub * a.s.c + h * a.s.h + w * a.s.w] = v;
  }
}

// ---------------------------------------------------------------- training workspace
// floats: the normalised inputs [2B][HW][3]; every layer's post-ReLU activation - a tap's for all 2B images (x group,
// then y group: the head reads both), any other layer's for the back-propagated images only; two ping-pong buffers for
// the images without a gradient; two for the gradients; the head partials (doubles).
struct TrainLayout {
  int64_t in0, act[kLayers], pp[2], g[2], partials, pair_partials, total;
  int nb;  // back-propagated images: B (want_dx + want_dy)
};

static int64_t round4(int64_t v) { return (v + 3) & ~(int64_t)3; }

static TrainLayout train_layout(int64_t B, int H, int W, int want_dx, int want_dy) {
  TrainLayout T{};
  const Dims d = stage_dims(H, W);
  const int sides = (want_dx ? 1 : 0) + (want_dy ? 1 : 0);
  T.nb = (int)(B * sides);
  const int64_t HW = (int64_t)H * W;
  int64_t o = 0;
  T.in0 = o;
  o += round4(2 * B * HW * 3);
  int stage = 0;
  for (int l = 0; l < kLayers; ++l) {
    if (kPoolIn[l]) ++stage;
    T.act[l] = o;
    o += (kTapOf[l] >= 0 ? 2 * B : (int64_t)T.nb) * d.H[stage] * d.W[stage] * kCout[l];
  }
  for (int k = 0; k < 2; ++k) {
    T.pp[k] = o;
    o += sides == 2 ? 0 : B * HW * 64;
  }
  for (int k = 0; k < 2; ++k) {
    T.g[k] = o;
    o += (int64_t)T.nb * HW * 64;
  }
  T.partials = o;  // a multiple of four floats: the doubles are aligned
  T.pair_partials = partial_count(H, W);
  o += 2 * B * T.pair_partials;
  T.total = o;
  return T;
}

constexpr int64_t kMaxPairs = 32767;  // 2B images on blockIdx.z

static int check_train_shape(const char* who, int64_t B, int H, int W, int want_dx, int want_dy) {
  FSN_REQUIRE(B >= 1 && B <= kMaxPairs, FSN_E_INVALID, "%s: B = %lld pairs (1 .. %lld per pass)", who, (long long)B,
              (long long)kMaxPairs);
  FSN_REQUIRE(H >= 16 && W >= 16, FSN_E_INVALID, "%s: image %dx%d: LPIPS-VGG needs at least 16x16 (four pools)", who, H,
              W);
  FSN_REQUIRE(H <= kMaxSide && W <= kMaxSide, FSN_E_UNSUPPORTED, "%s: image %dx%d above %d", who, H, W, kMaxSide);
  FSN_REQUIRE(want_dx || want_dy, FSN_E_INVALID, "%s: neither dx nor dy is wanted", who);
  return FSN_OK;
}

template <int BN, int MODE, int EPI = kEpiRelu>
static void launch_conv(const ConvArgs& a, int tiles, int images, hipStream_t s) {
  k_lpips_conv<BN, MODE, EPI><<<dim3((unsigned)tiles, (unsigned)(a.Cout / BN), (unsigned)images), kThreads, 0, s>>>(a);
}

// layer l of the forward on `images` images (a.in .. a.out2, a.split set by the caller)
static void forward_layer(int l, ConvArgs& a, const float* blob, const BlobLayout& L, const Dims& d, int stage, int Hs,
                          int Ws, int images, hipStream_t s) {
  a.w = blob + L.w[l];
  a.b = blob + L.b[l];
  a.mask = nullptr;
  a.H = d.H[stage];
  a.W = d.W[stage];
  a.Ws = Ws;
  a.Cin = kCin[l];
  a.Cout = kCout[l];
  a.Kp = kp_of(l);
  a.tiles_w = (a.W + kTileW - 1) / kTileW;
  a.in_img = (int64_t)Hs * Ws * kCin[l];
  a.out_img = (int64_t)a.H * a.W * kCout[l];
  const int tiles = ((a.H + kTileH - 1) / kTileH) * a.tiles_w;
  if (l == 0)
    launch_conv<64, kModeFirst>(a, tiles, images, s);
  else if (kCout[l] == 64)
    launch_conv<64, kModePlain>(a, tiles, images, s);
  else if (kPoolIn[l])
    launch_conv<128, kModePool>(a, tiles, images, s);
  else
    launch_conv<128, kModePlain>(a, tiles, images, s);
}

}  // namespace fsn

using namespace fsn;

extern "C" int64_t fsn_lpips_pack_bytes(void) { return blob_layout().total * (int64_t)sizeof(float); }

extern "C" int fsn_lpips_pack(const float* const* conv_w_host, const float* const* conv_b_host,
                              const float* const* lin_w_host, const float* shift, const float* scale, void* packed,
                              fsn_stream_t stream) {
  FSN_REQUIRE(conv_w_host && conv_b_host && lin_w_host && shift && scale && packed, FSN_E_INVALID,
              "fsn_lpips_pack: null pointer");
  for (int l = 0; l < kLayers; ++l)
    FSN_REQUIRE(conv_w_host[l] && conv_b_host[l], FSN_E_INVALID, "fsn_lpips_pack: null pointer (layer %d)", l);
  for (int t = 0; t < kTaps; ++t) FSN_REQUIRE(lin_w_host[t], FSN_E_INVALID, "fsn_lpips_pack: null pointer (lin%d)", t);
  const BlobLayout L = blob_layout();
  float* dst = static_cast<float*>(packed);
  hipStream_t s = as_stream(stream);
  auto copy = [&](const float* src, int n, int64_t off) {
    k_lpips_copy<<<(n + kThreads - 1) / kThreads, kThreads, 0, s>>>(src, n, dst + off);
  };
  for (int l = 0; l < kLayers; ++l) {
    const int64_t n = (int64_t)kCout[l] * kp_of(l);
    k_lpips_pack_conv<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, s>>>(conv_w_host[l], kCin[l], kCout[l],
                                                                                     kp_of(l), dst + L.w[l]);
    copy(conv_b_host[l], kCout[l], L.b[l]);
  }
  for (int t = 0; t < kTaps; ++t) copy(lin_w_host[t], kTapC[t], L.lin[t]);
  copy(shift, 3, L.shift);
  copy(scale, 3, L.scale);
  FSN_LAUNCH_CHECK("fsn_lpips_pack");
  return FSN_OK;
}

extern "C" int64_t fsn_lpips_workspace_floats(int H, int W) {
  FSN_REQUIRE(H >= 16 && W >= 16, FSN_E_INVALID,
              "fsn_lpips_workspace_floats: image %dx%d: LPIPS-VGG needs at least 16x16 (four pools)", H, W);
  FSN_REQUIRE(H <= kMaxSide && W <= kMaxSide, FSN_E_UNSUPPORTED, "fsn_lpips_workspace_floats: image %dx%d above %d",
              H, W, kMaxSide);
  return 2 * act_floats(H, W) + 2 * partial_count(H, W);  // the partials are doubles
}

extern "C" int fsn_lpips_vgg(const void* packed, const float* x, const float* y, int64_t N, int H, int W,
                             const int64_t* x_strides_host, const int64_t* y_strides_host, int normalize, float* out,
                             float* per_layer, float* workspace, fsn_stream_t stream) {
  FSN_REQUIRE(N >= 0, FSN_E_INVALID, "fsn_lpips_vgg: N = %lld", (long long)N);
  FSN_REQUIRE(H >= 16 && W >= 16, FSN_E_INVALID, "fsn_lpips_vgg: image %dx%d: LPIPS-VGG needs at least 16x16", H, W);
  FSN_REQUIRE(H <= kMaxSide && W <= kMaxSide, FSN_E_UNSUPPORTED, "fsn_lpips_vgg: image %dx%d above %d", H, W,
              kMaxSide);
  if (N == 0) return FSN_OK;
  FSN_REQUIRE(packed && x && y && out && workspace, FSN_E_INVALID, "fsn_lpips_vgg: null pointer");
  FSN_REQUIRE(x_strides_host && y_strides_host, FSN_E_INVALID, "fsn_lpips_vgg: null stride array");

  const BlobLayout L = blob_layout();
  const float* blob = static_cast<const float*>(packed);
  const Dims d = stage_dims(H, W);
  const int64_t act = act_floats(H, W);
  float* buf[2] = {workspace, workspace + act};
  double* partials = reinterpret_cast<double*>(workspace + 2 * act);
  FinishArgs fin{};
  int64_t off = 0;
  for (int t = 0; t < kTaps; ++t) {
    const int64_t hw = (int64_t)d.H[t] * d.W[t];
    fin.off[t] = off;
    fin.count[t] = head_blocks(hw);
    fin.inv_hw[t] = 1.0 / (double)hw;
    off += fin.count[t];
  }
  const Strides4 sx{x_strides_host[0], x_strides_host[1], x_strides_host[2], x_strides_host[3]};
  const Strides4 sy{y_strides_host[0], y_strides_host[1], y_strides_host[2], y_strides_host[3]};
  hipStream_t s = as_stream(stream);

  for (int64_t n = 0; n < N; ++n) {
    const int64_t in_elems = 2 * (int64_t)H * W * 3;
    k_lpips_input<<<(unsigned)((in_elems + kThreads - 1) / kThreads), kThreads, 0, s>>>(
        x, y, sx, sy, n, H, W, normalize, blob + L.shift, 1, buf[0]);
    FSN_LAUNCH_CHECK("k_lpips_input");
    int cur = 0, stage = 0, Hs = H, Ws = W;
    for (int l = 0; l < kLayers; ++l) {
      if (kPoolIn[l]) ++stage;
      ConvArgs a{};
      const int64_t in_img = (int64_t)Hs * Ws * kCin[l], out_img = (int64_t)d.H[stage] * d.W[stage] * kCout[l];
      a.in = buf[cur];
      a.in2 = buf[cur] + in_img;
      a.out = buf[cur ^ 1];
      a.out2 = buf[cur ^ 1] + out_img;
      a.split = 1;
      forward_layer(l, a, blob, L, d, stage, Hs, Ws, 2, s);
      FSN_LAUNCH_CHECK("k_lpips_conv");
      cur ^= 1;
      Hs = a.H;
      Ws = a.W;
      const int t = kTapOf[l];
      if (t >= 0) {
        const int64_t hw = (int64_t)a.H * a.W;
        k_lpips_head<<<(unsigned)fin.count[t], kThreads, 0, s>>>(buf[cur], buf[cur] + hw * kTapC[t], hw, kTapC[t],
                                                                 blob + L.lin[t], partials + fin.off[t], 0);
        FSN_LAUNCH_CHECK("k_lpips_head");
      }
    }
    k_lpips_finish<<<1, kThreads, 0, s>>>(partials, 0, fin, n, N, out, per_layer);
    FSN_LAUNCH_CHECK("k_lpips_finish");
  }
  return FSN_OK;
}

extern "C" int64_t fsn_lpips_grad_pack_bytes(void) { return grad_blob_layout().total * (int64_t)sizeof(float); }

extern "C" int fsn_lpips_grad_pack(const float* const* conv_w_host, void* packed_grad, fsn_stream_t stream) {
  FSN_REQUIRE(conv_w_host && packed_grad, FSN_E_INVALID, "fsn_lpips_grad_pack: null pointer");
  for (int l = 0; l < kLayers; ++l)
    FSN_REQUIRE(conv_w_host[l], FSN_E_INVALID, "fsn_lpips_grad_pack: null pointer (layer %d)", l);
  const GradBlobLayout G = grad_blob_layout();
  float* dst = static_cast<float*>(packed_grad);
  hipStream_t s = as_stream(stream);
  k_lpips_pack_dgrad_first<<<(27 * 64 + kThreads - 1) / kThreads, kThreads, 0, s>>>(conv_w_host[0], dst + G.w[0]);
  for (int l = 1; l < kLayers; ++l) {
    const int64_t n = (int64_t)kCin[l] * 9 * kCout[l];
    k_lpips_pack_dgrad<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, s>>>(conv_w_host[l], kCin[l], kCout[l],
                                                                                      dst + G.w[l]);
  }
  FSN_LAUNCH_CHECK("fsn_lpips_grad_pack");
  return FSN_OK;
}

extern "C" int64_t fsn_lpips_train_workspace_floats(int64_t B, int H, int W, int want_dx, int want_dy) {
  const int rc = check_train_shape("fsn_lpips_train_workspace_floats", B, H, W, want_dx, want_dy);
  if (rc != FSN_OK) return rc;
  return train_layout(B, H, W, want_dx, want_dy).total;
}

extern "C" int fsn_lpips_vgg_fwd_save(const void* packed, const float* x, const float* y, int64_t B, int H, int W,
                                      const int64_t* x_strides_host, const int64_t* y_strides_host, int normalize,
                                      int want_dx, int want_dy, float* out, float* per_layer, float* workspace,
                                      fsn_stream_t stream) {
  const int rc = check_train_shape("fsn_lpips_vgg_fwd_save", B, H, W, want_dx, want_dy);
  if (rc != FSN_OK) return rc;
  FSN_REQUIRE(packed && x && y && out && workspace, FSN_E_INVALID, "fsn_lpips_vgg_fwd_save: null pointer");
  FSN_REQUIRE(x_strides_host && y_strides_host, FSN_E_INVALID, "fsn_lpips_vgg_fwd_save: null stride array");

  const BlobLayout L = blob_layout();
  const float* blob = static_cast<const float*>(packed);
  const Dims d = stage_dims(H, W);
  const TrainLayout T = train_layout(B, H, W, want_dx, want_dy);
  double* partials = reinterpret_cast<double*>(workspace + T.partials);
  FinishArgs fin{};
  int64_t off = 0;
  for (int t = 0; t < kTaps; ++t) {
    const int64_t hw = (int64_t)d.H[t] * d.W[t];
    fin.off[t] = off;
    fin.count[t] = head_blocks(hw);
    fin.inv_hw[t] = 1.0 / (double)hw;
    off += fin.count[t];
  }
  const Strides4 sx{x_strides_host[0], x_strides_host[1], x_strides_host[2], x_strides_host[3]};
  const Strides4 sy{y_strides_host[0], y_strides_host[1], y_strides_host[2], y_strides_host[3]};
  hipStream_t s = as_stream(stream);
  const int want[2] = {want_dx ? 1 : 0, want_dy ? 1 : 0};

  const int64_t in_elems = 2 * (int64_t)H * W * 3;
  k_lpips_input<<<dim3((unsigned)((in_elems + kThreads - 1) / kThreads), (unsigned)B), kThreads, 0, s>>>(
      x, y, sx, sy, 0, H, W, normalize, blob + L.shift, B, workspace + T.in0);
  FSN_LAUNCH_CHECK("k_lpips_input");

  // where group `side` (0: the x images, 1: the y images) keeps layer l's output; l = -1: the normalised input
  int pcur = 0;  // the ping-pong buffer that holds the latest unsaved activation
  auto where = [&](int l, int side, int64_t img, int pp) -> float* {
    if (l < 0 || kTapOf[l] >= 0) return workspace + (l < 0 ? T.in0 : T.act[l]) + side * B * img;
    if (want[side]) return workspace + T.act[l] + (side == 1 && want[0] ? B * img : 0);
    return workspace + T.pp[pp];
  };
  int stage = 0, Hs = H, Ws = W;
  for (int l = 0; l < kLayers; ++l) {
    if (kPoolIn[l]) ++stage;
    const int64_t in_img = (int64_t)Hs * Ws * kCin[l], out_img = (int64_t)d.H[stage] * d.W[stage] * kCout[l];
    ConvArgs a{};
    a.in = where(l - 1, 0, in_img, pcur);
    a.in2 = where(l - 1, 1, in_img, pcur);
    a.out = where(l, 0, out_img, pcur ^ 1);
    a.out2 = where(l, 1, out_img, pcur ^ 1);
    a.split = (int)B;
    forward_layer(l, a, blob, L, d, stage, Hs, Ws, (int)(2 * B), s);
    FSN_LAUNCH_CHECK("k_lpips_conv");
    Hs = a.H;
    Ws = a.W;
    const int t = kTapOf[l];
    if (t >= 0) {
      const int64_t hw = (int64_t)a.H * a.W;
      k_lpips_head<<<dim3((unsigned)fin.count[t], (unsigned)B), kThreads, 0, s>>>(
          a.out, a.out2, hw, kTapC[t], blob + L.lin[t], partials + fin.off[t], T.pair_partials);
      FSN_LAUNCH_CHECK("k_lpips_head");
    } else {
      pcur ^= 1;
    }
  }
  k_lpips_finish<<<(unsigned)B, kThreads, 0, s>>>(partials, T.pair_partials, fin, 0, B, out, per_layer);
  FSN_LAUNCH_CHECK("k_lpips_finish");
  return FSN_OK;
}

template <int BN, int EPI>
static void launch_dgrad(const ConvArgs& a, int tiles, int images, hipStream_t s) {
  launch_conv<BN, kModePlain, EPI>(a, tiles, images, s);
}

extern "C" int fsn_lpips_vgg_bwd(const void* packed, const void* packed_grad, int64_t B, int H, int W, int normalize,
                                 int want_dx, int want_dy, const double* upstream, float* workspace, float* dx,
                                 const int64_t* dx_strides_host, float* dy, const int64_t* dy_strides_host,
                                 fsn_stream_t stream) {
  const int rc = check_train_shape("fsn_lpips_vgg_bwd", B, H, W, want_dx, want_dy);
  if (rc != FSN_OK) return rc;
  FSN_REQUIRE(packed && packed_grad && upstream && workspace, FSN_E_INVALID, "fsn_lpips_vgg_bwd: null pointer");
  FSN_REQUIRE(!want_dx || (dx && dx_strides_host), FSN_E_INVALID, "fsn_lpips_vgg_bwd: dx wanted without a tensor");
  FSN_REQUIRE(!want_dy || (dy && dy_strides_host), FSN_E_INVALID, "fsn_lpips_vgg_bwd: dy wanted without a tensor");

  const BlobLayout L = blob_layout();
  const GradBlobLayout G = grad_blob_layout();
  const float* blob = static_cast<const float*>(packed);
  const float* gblob = static_cast<const float*>(packed_grad);
  const Dims d = stage_dims(H, W);
  const TrainLayout T = train_layout(B, H, W, want_dx, want_dy);
  hipStream_t s = as_stream(stream);
  const bool wx = want_dx != 0, wy = want_dy != 0;
  float* gbuf[2] = {workspace + T.g[0], workspace + T.g[1]};
  int cur = 0;  // gbuf[cur]: the gradient the next kernel reads

  // the tap kernel of tap t (stage t): gbuf[cur] holds the pooled gradient (if any); writes gbuf[cur ^ 1]
  auto tap_bwd = [&](int t, int l, bool pooled) {
    const int64_t img = (int64_t)d.H[t] * d.W[t] * kTapC[t];
    TapBwdArgs a{};
    a.fx = workspace + T.act[l];
    a.fy = a.fx + B * img;
    a.lin = blob + L.lin[t];
    a.up = upstream;
    a.H = d.H[t];
    a.W = d.W[t];
    a.C = kTapC[t];
    if (pooled) {
      a.Hp = d.H[t + 1];
      a.Wp = d.W[t + 1];
      const int64_t pimg = (int64_t)a.Hp * a.Wp * kTapC[t];
      a.px = wx ? gbuf[cur] : nullptr;
      a.py = wy ? gbuf[cur] + (wx ? B * pimg : 0) : nullptr;
      if (!a.px) a.px = a.py;  // (non-null marks "pooled"; the x side is not written then)
    }
    a.gx = wx ? gbuf[cur ^ 1] : nullptr;
    a.gy = wy ? gbuf[cur ^ 1] + (wx ? B * img : 0) : nullptr;
    const int64_t hw = (int64_t)a.H * a.W;
    k_lpips_tap_bwd<<<dim3((unsigned)((hw + kTapPix - 1) / kTapPix), (unsigned)B), kThreads, 0, s>>>(a);
    cur ^= 1;
  };

  tap_bwd(4, 12, false);
  FSN_LAUNCH_CHECK("k_lpips_tap_bwd");
  int stage = kTaps - 1;
  for (int l = kLayers - 1; l >= 1; --l) {
    // the data gradient of layer l: the forward's GEMM with Cin and Cout exchanged, on the back-propagated images
    ConvArgs a{};
    a.in = a.in2 = gbuf[cur];
    a.out = a.out2 = gbuf[cur ^ 1];
    a.split = T.nb;
    a.w = gblob + G.w[l];
    a.b = nullptr;
    a.mask = kPoolIn[l] ? nullptr : workspace + T.act[l - 1];
    a.H = d.H[stage];
    a.W = d.W[stage];
    a.Ws = a.W;
    a.Cin = kCout[l];
    a.Cout = kCin[l];
    a.Kp = 9 * kCout[l];
    a.tiles_w = (a.W + kTileW - 1) / kTileW;
    a.in_img = (int64_t)a.H * a.W * kCout[l];
    a.out_img = (int64_t)a.H * a.W * kCin[l];
    const int tiles = ((a.H + kTileH - 1) / kTileH) * a.tiles_w;
    if (kCin[l] == 64) {
      if (kPoolIn[l])
        launch_dgrad<64, kEpiRaw>(a, tiles, T.nb, s);
      else
        launch_dgrad<64, kEpiMask>(a, tiles, T.nb, s);
    } else {
      if (kPoolIn[l])
        launch_dgrad<128, kEpiRaw>(a, tiles, T.nb, s);
      else
        launch_dgrad<128, kEpiMask>(a, tiles, T.nb, s);
    }
    FSN_LAUNCH_CHECK("k_lpips_conv (data gradient)");
    cur ^= 1;
    if (kPoolIn[l]) {
      --stage;
      tap_bwd(stage, l - 1, true);
      FSN_LAUNCH_CHECK("k_lpips_tap_bwd");
    }
  }
  // gbuf[cur]: the gradient w.r.t. conv1_1's pre-activation
  const int64_t HW = (int64_t)H * W;
  for (int side = 0; side < 2; ++side) {
    if (!(side ? wy : wx)) continue;
    const int64_t* st = side ? dy_strides_host : dx_strides_host;
    FirstBwdArgs a{};
    a.g = gbuf[cur] + (side == 1 && wx ? B * HW * 64 : 0);
    a.w = gblob + G.w[0];
    a.scale = blob + L.scale;
    a.d = side ? dy : dx;
    a.s = Strides4{st[0], st[1], st[2], st[3]};
    a.H = H;
    a.W = W;
    a.normalize = normalize;
    k_lpips_first_bwd<<<dim3((unsigned)((HW + kFirstPix - 1) / kFirstPix), (unsigned)B), kThreads, 0, s>>>(a);
    FSN_LAUNCH_CHECK("k_lpips_first_bwd");
  }
  return FSN_OK;
}
