// warp.hip — depth-warp sampling ("Depth-warp consistency"): the operator under the cross-view
// reprojection losses of few-shot NeRFs (GeCoNeRF, SPARF, ConsistentNeRF).  A rendered ray and its depth are taken to
// the colour that a training photograph shows at that 3-D point: point -> source camera frame -> pixel coordinates ->
// four uint8 taps, converted as the ray batch converts its pixel (raydata.hip) -> bilinear blend.  Gradients go back to
// the depth and to the ray.  The definition is this package's own; include/fsnerf_hip.h has it step by step.
// ONE launch each way, one thread per row: no LDS, no atomics, no workspace, nothing saved - the backward forms the
// projection and the taps again from the inputs.  Rows are independent: every output is bitwise reproducible.
// Every step is a float32 operation in the order written (-ffp-contract=off): tests/warp_ref.py follows the forward bit
// for bit.  The pinhole convention is ray_dev.hpp's (pinhole_dir_cam_k: the camera looks down -z, y up, pixel index w is
// the coordinate u = w), restated here and not shared: that header is inlined into the render kernels, whose code must
// not move with this one.
#include "common.hpp"

namespace fsn {

// debug build: a source view outside [-1, n_views) (-1 is the documented "no source") and a tap offset outside the
// images are recorded (count, source line, value, extent), read by fsn_debug_report("warp").  In every build such a row
// is invalid and reads no image byte.
FSN_DEBUG_DEFINE_RECORD(warp)

struct WarpArgs {
  const float* rays_o;      // [n, 3]
  const float* rays_d;      // [n, 3]
  const float* depth;       // [n]
  const int64_t* src_view;  // [n]
  int64_t n;
  const float* poses;  // [n_views, 12]
  int64_t n_views;
  const uint8_t* images;  // [n_views, H, W, C]
  int H, W, C, white_bkgd;
  const float* K;    // [1 or n_views, 4]
  int64_t k_stride;  // 0: one shared row
  float z_min, border;
};

// Row r up to its validity and its cell: what the forward and the backward share.
struct WarpRow {
  const float* M;  // the source pose
  int64_t view;
  float d[3], t, fx, fy, xc, yc, z, u, v, fu, fv;
  int x0, y0;
  bool in_range, valid;
};

__device__ __forceinline__ void warp_project(const WarpArgs& a, int64_t r, WarpRow& w) {
  const int64_t s = a.src_view[r];
  w.view = s;
  w.in_range = s >= 0 && s < a.n_views;
  w.valid = false;
  if (!w.in_range) {
#ifdef FSN_DEBUG
    if (s != -1) fsn_dbg_note(g_dbg_warp, __LINE__, s, a.n_views);
#endif
    return;
  }
  const float* M = a.poses + 12 * s;
  const float* K = a.K + a.k_stride * s;
  w.M = M;
  const float t = a.depth[r];
  w.t = t;
  float p[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    w.d[k] = a.rays_d[3 * r + k];
    const float X = a.rays_o[3 * r + k] + t * w.d[k];
    p[k] = X - M[4 * k + 3];
  }
  // R^T p: column j of the rotation is M[j], M[4 + j], M[8 + j]
  w.xc = (M[0] * p[0] + M[4] * p[1]) + M[8] * p[2];
  w.yc = (M[1] * p[0] + M[5] * p[1]) + M[9] * p[2];
  const float zc = (M[2] * p[0] + M[6] * p[1]) + M[10] * p[2];
  w.z = -zc;
  w.fx = K[0];
  w.fy = K[1];
  w.u = K[2] + w.fx * (w.xc / w.z);
  w.v = K[3] - w.fy * (w.yc / w.z);
  // (every comparison is false for a NaN)
  const float u_hi = (float)(a.W - 1) - a.border, v_hi = (float)(a.H - 1) - a.border;
  w.valid = isfinite(t) && t > 0.f && w.z >= a.z_min && w.u >= a.border && w.u <= u_hi && w.v >= a.border && w.v <= v_hi;
  if (!w.valid) return;
  w.x0 = min((int)floorf(w.u), a.W - 2);
  w.y0 = min((int)floorf(w.v), a.H - 2);
  w.fu = w.u - (float)w.x0;
  w.fv = w.v - (float)w.y0;
}

// The pixel at byte offset `off` as the ray batch converts it (raydata.hip, write_ray_row): byte / 255 and, with
// white_bkgd, c * a + (1 - a) in three float32 operations.  A four-channel pixel is one aligned 32-bit load.
__device__ __forceinline__ void warp_tap(const WarpArgs& a, int64_t off, float (&c)[3]) {
#ifdef FSN_DEBUG
  const int64_t extent = a.n_views * a.H * a.W * a.C;
  if (off < 0 || off + a.C > extent) {
    fsn_dbg_note(g_dbg_warp, __LINE__, off, extent);
    c[0] = c[1] = c[2] = 0.f;
    return;
  }
#endif
  if (a.C == 4) {
    const uint32_t px = *reinterpret_cast<const uint32_t*>(a.images + off);
    c[0] = (float)(px & 0xffu) / 255.0f;
    c[1] = (float)((px >> 8) & 0xffu) / 255.0f;
    c[2] = (float)((px >> 16) & 0xffu) / 255.0f;
    if (a.white_bkgd) {
      const float al = (float)(px >> 24) / 255.0f;
      const float rest = 1.0f - al;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float m = c[k] * al;
        c[k] = m + rest;
      }
    }
  } else {
    const uint8_t* px = a.images + off;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (float)px[k] / 255.0f;
  }
}

// The four taps of a valid row's cell: c00 at (y0, x0), c10 at (y0, x0 + 1), c01 at (y0 + 1, x0), c11 at (y0 + 1, x0 + 1).
__device__ __forceinline__ void warp_taps(const WarpArgs& a, const WarpRow& w, float (&c00)[3], float (&c10)[3],
                                          float (&c01)[3], float (&c11)[3]) {
  const int64_t row = (int64_t)a.W * a.C;
  const int64_t off = ((w.view * a.H + w.y0) * a.W + w.x0) * a.C;
  warp_tap(a, off, c00);
  warp_tap(a, off + a.C, c10);
  warp_tap(a, off + row, c01);
  warp_tap(a, off + row + a.C, c11);
}

__device__ __forceinline__ float quiet(float x) { return x != x ? __builtin_nanf("") : x; }

__global__ void __launch_bounds__(256) k_warp_sample_fwd(WarpArgs a, float* __restrict__ colour,
                                                         uint8_t* __restrict__ valid, float* __restrict__ uvz) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  WarpRow w;
  warp_project(a, r, w);
  float col[3] = {0.f, 0.f, 0.f};
  if (w.valid) {
    float c00[3], c10[3], c01[3], c11[3];
    warp_taps(a, w, c00, c10, c01, c11);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float top = c00[k] + w.fu * (c10[k] - c00[k]);
      const float bot = c01[k] + w.fu * (c11[k] - c01[k]);
      col[k] = top + w.fv * (bot - top);
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) colour[3 * r + k] = col[k];
  valid[r] = w.valid ? 1 : 0;
  if (uvz) {
    uvz[3 * r + 0] = w.in_range ? quiet(w.u) : 0.f;
    uvz[3 * r + 1] = w.in_range ? quiet(w.v) : 0.f;
    uvz[3 * r + 2] = w.in_range ? quiet(w.z) : 0.f;
  }
}

__global__ void __launch_bounds__(256) k_warp_sample_bwd(WarpArgs a, const float* __restrict__ d_colour,
                                                         float* __restrict__ d_depth, float* __restrict__ d_rays_o,
                                                         float* __restrict__ d_rays_d) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.n) return;
  WarpRow w;
  warp_project(a, r, w);
  float gp[3] = {0.f, 0.f, 0.f};
  float gt = 0.f;
  if (w.valid) {
    float c00[3], c10[3], c01[3], c11[3];
    warp_taps(a, w, c00, c10, c01, c11);
    float gu = 0.f, gv = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float g = d_colour[3 * r + k];
      const float du0 = c10[k] - c00[k], du1 = c11[k] - c01[k];
      const float top = c00[k] + w.fu * du0;
      const float bot = c01[k] + w.fu * du1;
      const float dcu = du0 + w.fv * (du1 - du0);
      const float dcv = bot - top;
      gu += g * dcu;
      gv += g * dcv;
    }
    const float gufx = gu * w.fx, gvfy = gv * w.fy;
    const float g_xc = gufx / w.z;
    const float g_yc = -(gvfy / w.z);
    const float g_z = (-gufx * w.xc + gvfy * w.yc) / (w.z * w.z);
    const float g_zc = -g_z;
    const float* M = w.M;
#pragma unroll
    for (int k = 0; k < 3; ++k) gp[k] = (M[4 * k + 0] * g_xc + M[4 * k + 1] * g_yc) + M[4 * k + 2] * g_zc;
    gt = (gp[0] * w.d[0] + gp[1] * w.d[1]) + gp[2] * w.d[2];
  }
  if (d_depth) d_depth[r] = gt;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (d_rays_o) d_rays_o[3 * r + k] = gp[k];
    if (d_rays_d) d_rays_d[3 * r + k] = w.valid ? w.t * gp[k] : 0.f;  // (an invalid row's t may be a NaN)
  }
}

}  // namespace fsn

using namespace fsn;

// The checks and the argument block of both entry points.  n == 0: out->n stays 0 and nothing is launched.
static int warp_args(const char* who, const float* rays_o, const float* rays_d, const float* depth, const int64_t* src_view,
                     int64_t n, const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C,
                     int white_bkgd, const float* K, int64_t m, float z_min, float border, WarpArgs* out) {
  FSN_REQUIRE(n >= 0 && n_views >= 0, FSN_E_INVALID, "%s: negative n or n_views", who);
  FSN_REQUIRE(C == 3 || C == 4, FSN_E_INVALID, "%s: %d channels (the images are RGB or RGBA bytes: 3 or 4)", who, C);
  FSN_REQUIRE(!white_bkgd || C == 4, FSN_E_INVALID,
              "%s: white_bkgd composes over the alpha channel and needs 4-channel images, got %d", who, C);
  FSN_REQUIRE(H >= 2 && W >= 2, FSN_E_INVALID, "%s: images of %d x %d pixels have no bilinear cell (H, W >= 2)", who, H, W);
  FSN_REQUIRE(m == 1 || m == n_views, FSN_E_INVALID, "%s: a camera table of %lld rows (1, or one per view: %lld)", who,
              (long long)m, (long long)n_views);
  FSN_REQUIRE(z_min > 0.f && z_min < INFINITY, FSN_E_INVALID, "%s: z_min %g must be positive and finite", who, (double)z_min);
  FSN_REQUIRE(border >= 0.f && border < INFINITY, FSN_E_INVALID, "%s: border %g must be finite and not negative", who,
              (double)border);
  FSN_REQUIRE(n_views <= ((int64_t)1 << 60) / ((int64_t)H * W), FSN_E_UNSUPPORTED, "%s: more than 2^62 image bytes", who);
  FSN_REQUIRE(n <= (int64_t)256 * 0x7fffffff, FSN_E_UNSUPPORTED, "%s: more than 2^39 rows in one call", who);
  if (n == 0) return FSN_OK;
  FSN_REQUIRE(rays_o && rays_d && depth && src_view, FSN_E_INVALID, "%s: null rays_o, rays_d, depth or src_view", who);
  FSN_REQUIRE(poses && images && K, FSN_E_INVALID, "%s: null poses, images or K", who);
  FSN_REQUIRE(C != 4 || (reinterpret_cast<uintptr_t>(images) & 3u) == 0, FSN_E_INVALID,
              "%s: four-channel images are read a pixel at a time and must be 4-byte aligned", who);
  *out = WarpArgs{rays_o, rays_d, depth, src_view, n, poses, n_views, images, H, W, C, white_bkgd ? 1 : 0, K,
                  m == 1 ? 0 : 4, z_min, border};
  return FSN_OK;
}

extern "C" int fsn_warp_sample_fwd(const float* rays_o, const float* rays_d, const float* depth, const int64_t* src_view,
                                   int64_t n, const float* poses, int64_t n_views, const uint8_t* images, int H, int W,
                                   int C, int white_bkgd, const float* K, int64_t m, float z_min, float border,
                                   float* colour, uint8_t* valid, float* uvz, fsn_stream_t stream) {
  WarpArgs a{};
  const int rc = warp_args("fsn_warp_sample_fwd", rays_o, rays_d, depth, src_view, n, poses, n_views, images, H, W, C,
                           white_bkgd, K, m, z_min, border, &a);
  if (rc || a.n == 0) return rc;
  FSN_REQUIRE(colour && valid, FSN_E_INVALID, "fsn_warp_sample_fwd: null colour or valid");
  k_warp_sample_fwd<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(a, colour, valid, uvz);
  FSN_LAUNCH_CHECK("k_warp_sample_fwd");
  return FSN_OK;
}

extern "C" int fsn_warp_sample_bwd(const float* rays_o, const float* rays_d, const float* depth, const int64_t* src_view,
                                   int64_t n, const float* poses, int64_t n_views, const uint8_t* images, int H, int W,
                                   int C, int white_bkgd, const float* K, int64_t m, float z_min, float border,
                                   const float* d_colour, float* d_depth, float* d_rays_o, float* d_rays_d,
                                   fsn_stream_t stream) {
  WarpArgs a{};
  const int rc = warp_args("fsn_warp_sample_bwd", rays_o, rays_d, depth, src_view, n, poses, n_views, images, H, W, C,
                           white_bkgd, K, m, z_min, border, &a);
  if (rc || a.n == 0) return rc;
  FSN_REQUIRE(d_colour, FSN_E_INVALID, "fsn_warp_sample_bwd: null d_colour");
  if (!(d_depth || d_rays_o || d_rays_d)) return FSN_OK;  // nothing wanted
  k_warp_sample_bwd<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(a, d_colour, d_depth, d_rays_o, d_rays_d);
  FSN_LAUNCH_CHECK("k_warp_sample_bwd");
  return FSN_OK;
}
