// pose_refine.hip — learnable camera poses behind the data layer (this package's own: the reference keeps its poses
// fixed).  View v carries a correction xi_v = (omega_v, tau_v) on top of its stored pose [R0_v | t0_v]:
//   R_v = exp([omega_v]x) R0_v,   t_v = t0_v + tau_v,   exp([omega]x) = I + A K + B K^2,  K = [omega]x,  theta = |omega|,
//   A = sin(theta) / theta,   B = (1 - cos(theta)) / theta^2.
// k_pose_compose writes the corrected 3x4 matrices the loaders' launches read (one thread per view); k_ray_pose_grad is
// the backward of "flat ray index -> ray of the corrected pose" (pinhole_ray, + ndc_ray), reduced per view:
//   (index, dL/drays_o, dL/drays_d) -> dL/dxi [n, 6]
// in ONE launch, no atomics, a fixed summation order: one workgroup per view, its threads stride over the batch and
// keep the entries of their view, 12 partial sums each (dL/dR = sum g_d (x) dir_cam, dL/dt = sum g_o), a butterfly
// inside the wave, LDS across the sixteen waves, and thread 0 finishes with the derivative of the composition.
// (1024 threads: the walk is a chain of dependent loads per thread, so a view's time is the number of strides - 4 for
// a 4096-ray batch: 16 us over 8 views and 14 us over 100; with 256 threads the same launches took 24 us and 17 us.)
#include "common.hpp"
#include "ray_dev.hpp"

namespace fsn {

// debug build: an index outside [0, n_views*H*W) is recorded (count, source line, index, N - both truncated to 32
// bits), read by fsn_debug_report("pose_refine").  In every build such an entry contributes nothing.
FSN_DEBUG_DEFINE_RECORD(pose_refine)

// Below theta^2 = 2^-6 (theta = 0.125) the Taylor forms: their first dropped terms, theta^6 / 5040 and theta^6 / 40320,
// are under 2^-30 there.  Above it A = sin(theta) / theta and B = 0.5 (sin(theta/2) / (theta/2))^2 - (1 - cos(theta)) /
// theta^2 without its cancellation - so that both branches carry float32 rounding only and meet at the threshold.
constexpr float kPoseTaylorTheta2 = 0.015625f;

// m[12] = [exp([omega]x) R0 | t0 + tau], rows 0..2 of the corrected camera-to-world matrix.  xi = 0 gives p0 back value
// for value: K = 0, so every entry is 1 * r + 0 * r' + 0 * r''.
__device__ __forceinline__ void pose_compose(const float* __restrict__ p0, const float* __restrict__ xi, float (&m)[12]) {
  const float wx = xi[0], wy = xi[1], wz = xi[2];
  const float xx = wx * wx, yy = wy * wy, zz = wz * wz;
  const float th2 = (xx + yy) + zz;
  float A, B;
  if (th2 < kPoseTaylorTheta2) {
    A = 1.0f - th2 / 6.0f + th2 * th2 / 120.0f;
    B = 0.5f - th2 / 24.0f + th2 * th2 / 720.0f;
  } else {
    const float th = sqrtf(th2), h = 0.5f * th;
    const float sh = sinf(h) / h;
    A = sinf(th) / th;
    B = 0.5f * (sh * sh);
  }
  // E = I + A K + B K^2,  K^2 = omega omega^T - theta^2 I
  const float E[9] = {1.0f - B * (yy + zz),        B * (wx * wy) - A * wz,       B * (wx * wz) + A * wy,
                      B * (wx * wy) + A * wz,      1.0f - B * (xx + zz),         B * (wy * wz) - A * wx,
                      B * (wx * wz) - A * wy,      B * (wy * wz) + A * wx,       1.0f - B * (xx + yy)};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) m[4 * i + j] = (E[3 * i] * p0[j] + E[3 * i + 1] * p0[4 + j]) + E[3 * i + 2] * p0[8 + j];
    m[4 * i + 3] = p0[4 * i + 3] + xi[3 + i];
  }
}

__global__ void __launch_bounds__(256) k_pose_compose(const float* __restrict__ poses0, const float* __restrict__ xi,
                                                      int64_t n, float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  float m[12];
  pose_compose(poses0 + 12 * v, xi + 6 * v, m);
#pragma unroll
  for (int k = 0; k < 12; ++k) out[12 * v + k] = m[k];
}

// The derivative of the composition, once per view (thread 0), in float64: with G = dL/dR and R = E R0,
//   dE = [J dw]x E  (J = I + B K + C K^2 the left Jacobian of SO(3), C = (theta - sin(theta)) / theta^3), so
//   dL/domega = J^T u,  u = vee(N - N^T),  N = G R^T,  J^T = I - B K + C K^2.
__device__ void pose_compose_bwd(const float* __restrict__ p0, const float* __restrict__ xi, const float (&g)[12],
                                 float* __restrict__ grad_xi) {
  const double wx = xi[0], wy = xi[1], wz = xi[2];
  const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
  double A, B, Cc;
  if (th2 < 1e-4) {
    A = 1.0 - th2 / 6.0 + th2 * th2 / 120.0;
    B = 0.5 - th2 / 24.0 + th2 * th2 / 720.0;
    Cc = 1.0 / 6.0 - th2 / 120.0 + th2 * th2 / 5040.0;
  } else {
    A = sin(th) / th;
    B = (1.0 - cos(th)) / th2;
    Cc = (th - sin(th)) / (th2 * th);
  }
  const double E[9] = {1.0 - B * (wy * wy + wz * wz), B * wx * wy - A * wz,          B * wx * wz + A * wy,
                       B * wx * wy + A * wz,          1.0 - B * (wx * wx + wz * wz), B * wy * wz - A * wx,
                       B * wx * wz - A * wy,          B * wy * wz + A * wx,          1.0 - B * (wx * wx + wy * wy)};
  double R[9], N[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      R[3 * i + j] = E[3 * i] * (double)p0[j] + E[3 * i + 1] * (double)p0[4 + j] + E[3 * i + 2] * (double)p0[8 + j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      N[3 * i + j] = (double)g[4 * i] * R[3 * j] + (double)g[4 * i + 1] * R[3 * j + 1] + (double)g[4 * i + 2] * R[3 * j + 2];
  const double u[3] = {N[7] - N[5], N[2] - N[6], N[3] - N[1]};
  const double k1[3] = {wy * u[2] - wz * u[1], wz * u[0] - wx * u[2], wx * u[1] - wy * u[0]};        // omega x u
  const double k2[3] = {wy * k1[2] - wz * k1[1], wz * k1[0] - wx * k1[2], wx * k1[1] - wy * k1[0]};  // omega x (omega x u)
  for (int k = 0; k < 3; ++k) {
    grad_xi[k] = (float)(u[k] - B * k1[k] + Cc * k2[k]);
    grad_xi[3 + k] = g[4 * k + 3];
  }
}

struct PoseGradArgs {
  const float* poses0;     // [n, 12]
  const float* xi;         // [n, 6]
  const int64_t* index;    // [count]
  const float* grad_o;     // [count, 3] or null
  const float* grad_d;     // [count, 3] or null
  int64_t per_view, n_rays, count;
  int W, ndc;
  float half_w, half_h, focal, sx, sy, near, two_near;
  float* grad_xi;          // [n, 6]
  float* grad_poses;       // [n, 12] or null
};

constexpr int kPoseGradThreads = 1024, kPoseGradWaves = kPoseGradThreads / 64;

__global__ void __launch_bounds__(kPoseGradThreads) k_ray_pose_grad(PoseGradArgs a) {
  const int64_t view = blockIdx.x;
  const int64_t lo = view * a.per_view, hi = lo + a.per_view;
  float m[12];
  pose_compose(a.poses0 + 12 * view, a.xi + 6 * view, m);  // (the matrix the batch's rays were formed with)
  float acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.f;
  for (int64_t i = threadIdx.x; i < a.count; i += kPoseGradThreads) {
    const int64_t idx = a.index[i];
#ifdef FSN_DEBUG
    if (view == 0 && (idx < 0 || idx >= a.n_rays)) fsn_dbg_note(g_dbg_pose_refine, __LINE__, idx, a.n_rays);
#endif
    if (idx < lo || idx >= hi) continue;  // another view's ray, or no ray at all
    const unsigned pix = (unsigned)(idx - lo), W = (unsigned)a.W;  // (per_view < 2^31: the host checked)
    const int h = (int)(pix / W), w = (int)(pix % W);
    float c[3], go[3], gd[3];
    pinhole_dir_cam(a.half_w, a.half_h, a.focal, h, w, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      go[k] = a.grad_o ? a.grad_o[3 * i + k] : 0.f;
      gd[k] = a.grad_d ? a.grad_d[3 * i + k] : 0.f;
    }
    if (a.ndc) {
      float o[3], d[3];
      pinhole_ray(m, a.half_w, a.half_h, a.focal, h, w, o, d);
      ndc_ray_bwd(o, d, a.sx, a.sy, a.near, a.two_near, go, gd);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      acc[4 * k + 0] += gd[k] * c[0];
      acc[4 * k + 1] += gd[k] * c[1];
      acc[4 * k + 2] += gd[k] * c[2];
      acc[4 * k + 3] += go[k];
    }
  }
  __shared__ float part[kPoseGradWaves][12];
  const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    const float s = wave_sum(acc[k]);
    if (lane == 0) part[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float g[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      float s = part[0][k];
      for (int w = 1; w < kPoseGradWaves; ++w) s += part[w][k];  // (in wave order, every time)
      g[k] = s;
    }
    if (a.grad_poses) {
#pragma unroll
      for (int k = 0; k < 12; ++k) a.grad_poses[12 * view + k] = g[k];
    }
    pose_compose_bwd(a.poses0 + 12 * view, a.xi + 6 * view, g, a.grad_xi + 6 * view);
  }
}

}  // namespace fsn

using namespace fsn;

extern "C" int fsn_pose_compose(const float* poses0, const float* xi, int64_t n, float* poses_out, fsn_stream_t stream) {
  FSN_REQUIRE(n >= 0, FSN_E_INVALID, "fsn_pose_compose: negative view count %lld", (long long)n);
  FSN_REQUIRE(poses0 && xi && poses_out, FSN_E_INVALID, "fsn_pose_compose: null pointer");
  if (n == 0) return FSN_OK;
  FSN_REQUIRE((n + 255) / 256 <= 0x7fffffff, FSN_E_UNSUPPORTED, "fsn_pose_compose: too many views");
  k_pose_compose<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(poses0, xi, n, poses_out);
  FSN_LAUNCH_CHECK("k_pose_compose");
  return FSN_OK;
}

extern "C" int fsn_ray_pose_grad(const float* poses0, const float* xi, int64_t n_views, int H, int W, double focal, int ndc,
                                 double near, const int64_t* index, const float* grad_o, const float* grad_d, int64_t count,
                                 float* grad_xi, float* grad_poses, fsn_stream_t stream) {
  FSN_REQUIRE(n_views >= 0 && H > 0 && W > 0 && focal > 0, FSN_E_INVALID,
              "fsn_ray_pose_grad: bad geometry n=%lld H=%d W=%d focal=%g", (long long)n_views, H, W, focal);
  FSN_REQUIRE(count >= 0, FSN_E_INVALID, "fsn_ray_pose_grad: negative count %lld", (long long)count);
  FSN_REQUIRE((int64_t)H * W <= 0x7fffffff, FSN_E_UNSUPPORTED, "fsn_ray_pose_grad: more than 2^31 pixels per view");
  FSN_REQUIRE(n_views <= 0x7fffffff, FSN_E_UNSUPPORTED, "fsn_ray_pose_grad: too many views");
  FSN_REQUIRE(poses0 && xi && grad_xi, FSN_E_INVALID, "fsn_ray_pose_grad: null poses0, xi or grad_xi");
  FSN_REQUIRE(count == 0 || index, FSN_E_INVALID, "fsn_ray_pose_grad: null index list");
  if (n_views == 0) return FSN_OK;
  PoseGradArgs a{};
  a.poses0 = poses0;
  a.xi = xi;
  a.index = index;
  a.grad_o = grad_o;
  a.grad_d = grad_d;
  a.per_view = (int64_t)H * W;
  a.n_rays = n_views * a.per_view;
  a.count = count;
  a.W = W;
  a.ndc = ndc ? 1 : 0;
  // the same roundings as fsn_ray_batch
  a.half_w = (float)(W * 0.5);
  a.half_h = (float)(H * 0.5);
  a.focal = (float)focal;
  a.sx = (float)(-1.0 / (W / (2.0 * focal)));
  a.sy = (float)(-1.0 / (H / (2.0 * focal)));
  a.near = (float)near;
  a.two_near = (float)(2.0 * near);
  a.grad_xi = grad_xi;
  a.grad_poses = grad_poses;
  k_ray_pose_grad<<<(unsigned)n_views, kPoseGradThreads, 0, as_stream(stream)>>>(a);  // (count = 0: every view's gradient is 0)
  FSN_LAUNCH_CHECK("k_ray_pose_grad");
  return FSN_OK;
}
