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
#include "common.hpp"

#include <cmath>

namespace fsn {

// debug build: the LDS indices of k_lpips_conv are range-checked (common.hpp), read by fsn_debug_report_lpips
FSN_DEBUG_DEFINE_RECORD(g_dbg_lpips)
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
// both images of pair n -> act [2][H][W][3]: (v' - shift) / scale with v' = 2v - 1 under normalize (float32, the
// scaling layer's arithmetic)
__global__ void __launch_bounds__(kThreads) k_lpips_input(const float* __restrict__ x, const float* __restrict__ y,
                                                          Strides4 sx, Strides4 sy, int64_t n, int H, int W,
                                                          int normalize, const float* __restrict__ shift_scale,
                                                          float* __restrict__ act) {
  const int64_t per = (int64_t)H * W * 3;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= 2 * per) return;
  const int img = (int)(i / per);
  const int64_t e = i - img * per, p = e / 3;
  const int c = (int)(e - p * 3);
  const int h = (int)(p / W), w = (int)(p - (int64_t)h * W);
  const Strides4 s = img ? sy : sx;
  const float* src = img ? y : x;
  float v = src[n * s.n + c * s.c + h * s.h + w * s.w];
  if (normalize) v = 2.f * v - 1.f;
  act[i] = (v - shift_scale[c]) / shift_scale[4 + c];
}

// ---------------------------------------------------------------- convolution
struct ConvArgs {
  const float* in;  // source activations [2][Hs][Ws][Cin]
  float* out;       // [2][H][W][Cout]
  const float* w;   // packed [Cout][Kp]
  const float* b;   // [Cout]
  int H, W;         // output (= input after the pool) size
  int Ws;           // source width (the pooled-input mode reads 2x2 windows of it)
  int Cin, Cout, Kp, tiles_w;
  int64_t in_img, out_img;  // floats per image
};

enum { kModeFirst = 0, kModePlain = 1, kModePool = 2 };

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

template <int BN, int MODE>
__global__ void __launch_bounds__(kThreads) k_lpips_conv(ConvArgs a) {
  constexpr int TN = BN / 64;                   // 32 x 32 accumulator tiles per wave along N (the wave's M: 2 tiles)
  constexpr int BLD = BN * kBK / 4 / kThreads;  // float4 loads of B per thread and chunk
  __shared__ __attribute__((aligned(16))) float As[kBM][kLds];
  __shared__ __attribute__((aligned(16))) float Bs[BN][kLds];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1, li = lane & 31, lh = lane >> 5;
  const int tile = blockIdx.x, img = blockIdx.z, n0 = blockIdx.y * BN;
  const int h0 = (tile / a.tiles_w) * kTileH, w0 = (tile % a.tiles_w) * kTileW;
  const float* in = a.in + img * a.in_img;
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
  float* out = a.out + img * a.out_img;
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) {
    const int n = n0 + (BN / 2) * wn + 32 * tn + li;
    const float bn = a.b[n];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        int h, w;
        tile_pixel(64 * wm + 32 * tm + (r & 3) + 8 * (r >> 2) + 4 * lh, h0, w0, h, w);
        if (h < H && w < W) {
          const float v = acc[tm][tn][r] + bn;
          out[((int64_t)h * W + w) * a.Cout + n] = v < 0.f ? 0.f : v;  // ReLU (a NaN stays a NaN)
        }
      }
  }
}

// ---------------------------------------------------------------- head
// per pixel p of a tap [2][HW][C]: sum_c lin[c] (fx / (|fx| + 1e-10) - fy / (|fy| + 1e-10))^2 in float64; one
// partial (the workgroup's sum) per kHeadPix pixels
__global__ void __launch_bounds__(kThreads) k_lpips_head(const float* __restrict__ act, int64_t HW, int C,
                                                         const float* __restrict__ lin, double* __restrict__ partials) {
  __shared__ double red[kThreads / 64];
  const int64_t p = (int64_t)blockIdx.x * kHeadPix + threadIdx.x;
  double v = 0.0;
  if (p < HW) {
    const float* fx = act + p * C;
    const float* fy = act + (HW + p) * C;
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
  if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

struct FinishArgs {
  int64_t off[kTaps], count[kTaps];  // each tap's partials
  double inv_hw[kTaps];
};

// pair n: each tap's partials in a fixed order -> its spatial mean; out[n] = the sum over the taps
__global__ void __launch_bounds__(kThreads) k_lpips_finish(const double* __restrict__ partials, FinishArgs f, int64_t n,
                                                           int64_t N, float* __restrict__ out,
                                                           float* __restrict__ per_layer) {
  __shared__ double red[kThreads / 64];
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

template <int BN, int MODE>
static void launch_conv(const ConvArgs& a, int tiles, hipStream_t s) {
  k_lpips_conv<BN, MODE><<<dim3((unsigned)tiles, (unsigned)(a.Cout / BN), 2), kThreads, 0, s>>>(a);
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
        x, y, sx, sy, n, H, W, normalize, blob + L.shift, buf[0]);
    FSN_LAUNCH_CHECK("k_lpips_input");
    int cur = 0, stage = 0, Hs = H, Ws = W;
    for (int l = 0; l < kLayers; ++l) {
      if (kPoolIn[l]) ++stage;
      ConvArgs a{};
      a.in = buf[cur];
      a.out = buf[cur ^ 1];
      a.w = blob + L.w[l];
      a.b = blob + L.b[l];
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
        launch_conv<64, kModeFirst>(a, tiles, s);
      else if (kCout[l] == 64)
        launch_conv<64, kModePlain>(a, tiles, s);
      else if (kPoolIn[l])
        launch_conv<128, kModePool>(a, tiles, s);
      else
        launch_conv<128, kModePlain>(a, tiles, s);
      FSN_LAUNCH_CHECK("k_lpips_conv");
      cur ^= 1;
      Hs = a.H;
      Ws = a.W;
      const int t = kTapOf[l];
      if (t >= 0) {
        k_lpips_head<<<(unsigned)fin.count[t], kThreads, 0, s>>>(buf[cur], (int64_t)a.H * a.W, kTapC[t],
                                                                 blob + L.lin[t], partials + fin.off[t]);
        FSN_LAUNCH_CHECK("k_lpips_head");
      }
    }
    k_lpips_finish<<<1, kThreads, 0, s>>>(partials, fin, n, N, out, per_layer);
    FSN_LAUNCH_CHECK("k_lpips_finish");
  }
  return FSN_OK;
}

extern "C" int fsn_debug_report_lpips(uint32_t* out_host) {
  FSN_REQUIRE(out_host, FSN_E_INVALID, "fsn_debug_report_lpips: null pointer");
#ifdef FSN_DEBUG
  FSN_HIP(hipDeviceSynchronize());
  unsigned zero[4] = {0u, 0u, 0u, 0u};
  FSN_HIP(hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_dbg_lpips), sizeof(unsigned) * 4));
  FSN_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_dbg_lpips), zero, sizeof(zero)));
  return FSN_OK;
#else
  FSN_REQUIRE(false, FSN_E_UNSUPPORTED, "fsn_debug_report_lpips: not a debug build (make -C fs-nerf_amd/csrc debug)");
#endif
}
