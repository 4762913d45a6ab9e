// pose_refine.hip — learnable camera poses behind the data layer (this package's own: the reference keeps its poses
// fixed).  View v carries a correction xi_v = (omega_v, tau_v) on top of its stored pose [R0_v | t0_v]:
//   R_v = exp([omega_v]x) R0_v,   t_v = t0_v + tau_v,   exp([omega]x) = I + A K + B K^2,  K = [omega]x,  theta = |omega|,
//   A = sin(theta) / theta,   B = (1 - cos(theta)) / theta^2.
// k_pose_compose writes the corrected 3x4 matrices the loaders' launches read (one thread per view); k_ray_view_grad is
// the backward of "flat ray index -> ray of the corrected pose" (pinhole_ray, + ndc_ray), reduced per view:
//   (index, dL/drays_o, dL/drays_d) -> dL/dxi [n, 6]
// in ONE launch, no atomics, a fixed summation order: one workgroup per view, its threads stride over the batch and
// keep the entries of their view, 12 partial sums each (dL/dR = sum g_d (x) dir_cam, dL/dt = sum g_o), a butterfly
// inside the wave, LDS across the sixteen waves - thread k adds sum k in wave order - and thread 0 finishes with the
// derivative of the composition.
// (1024 threads: the walk is a chain of dependent loads per thread, so a view's time is the number of strides - 4 for
// a 4096-ray batch: 16 us over 8 views and 14 us over 100; with 256 threads the same launches took 24 us and 17 us.)
// The learnable intrinsics: k_intrinsics_compose forms the camera table K = (fx, fy, cx, cy) from its parameter phi,
// k_ray_view_grad<true> is the same walk over that table with four more sums (this view's share of dL/dK), and
// k_intrinsics_grad_* chain dL/dK to dL/dphi.  fsn_ray_pose_grad launches <false>, fsn_ray_camera_grad <true>.
#include "common.hpp"
#include "pinhole_consts.hpp"
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

// The per-view gradient walk, written once for both entry points.  kTable = false (fsn_ray_pose_grad): the intrinsics
// are the launch constants, twelve sums, grad_poses on request.  kTable = true (fsn_ray_camera_grad): they are the
// view's row of the camera table K, xi may be null (no correction), and four more sums give this view's rays' share
// of dL/d(fx, fy, cx, cy).  Per ray, with g_c = R^T g_d, u = ((w - cx)/fx, -(h - cy)/fy, -1), c = u / |u|:
//   g_u = (g_c - c (c . g_c)) / |u|,   dL/dfx = -g_u0 u_0 / fx,  dL/dcx = -g_u0 / fx,
//                                      dL/dfy = -g_u1 u_1 / fy,  dL/dcy =  g_u1 / fy.
// The stored intrinsics are K = (focal, focal, W/2, H/2), so both instantiations perform the same float operations in
// the same order on the twelve pose sums: with the stored intrinsics in K, grad_xi is the same bit for bit.
struct ViewGradArgs {
  const float* poses0;     // [n, 12]
  const float* xi;         // [n, 6] (kTable: or null)
  const int64_t* index;    // [count]
  const float* grad_o;     // [count, 3] or null
  const float* grad_d;     // [count, 3] or null
  int64_t per_view, n_rays, count;
  int W, ndc;
  PinholeConsts pc;        // (kTable: half_w, half_h and focal are not read - the table's row is)
  float* grad_xi;          // [n, 6] (kTable: or null)
  float* grad_poses;       // !kTable: [n, 12] or null
  const float* K;          // kTable: [k_rows, 4]
  int64_t k_stride;        // kTable: 0 (one shared row) or 4
  float* grad_K_views;     // kTable: [n, 4]
};

constexpr int kPoseGradThreads = 1024, kPoseGradWaves = kPoseGradThreads / 64;
__device__ const float kZeroXi[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // xi = null: no correction

template <bool kTable>
__global__ void __launch_bounds__(kPoseGradThreads) k_ray_view_grad(ViewGradArgs a) {
  constexpr int kSums = kTable ? 16 : 12;
  const int64_t view = blockIdx.x;
  const int64_t lo = view * a.per_view, hi = lo + a.per_view;
  const float* p0 = a.poses0 + 12 * view;
  bool plain = false;  // kTable: xi = null, the stored pose as it is
  if constexpr (kTable) plain = !a.xi;
  const float* xi = plain ? kZeroXi : a.xi + 6 * view;
  float m[12];  // (the matrix the batch's rays were formed with)
  if (plain) {
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = p0[k];
  } else {
    pose_compose(p0, xi, m);
  }
  float fx = a.pc.focal, fy = a.pc.focal, cx = a.pc.half_w, cy = a.pc.half_h;
  if constexpr (kTable) {
    const float* Kv = a.K + a.k_stride * view;
    fx = Kv[0], fy = Kv[1], cx = Kv[2], cy = Kv[3];
  }
  float acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.f;
  for (int64_t i = threadIdx.x; i < a.count; i += kPoseGradThreads) {
    const int64_t idx = a.index[i];
#ifdef FSN_DEBUG
    if (view == 0 && (idx < 0 || idx >= a.n_rays)) fsn_dbg_note(g_dbg_pose_refine, __LINE__, idx, a.n_rays);
#endif
    if (idx < lo || idx >= hi) continue;  // another view's ray, or no ray at all: skipped before any other access
    const unsigned pix = (unsigned)(idx - lo), W = (unsigned)a.W;  // (per_view < 2^31: the host checked)
    const int h = (int)(pix / W), w = (int)(pix % W);
    float c[3], go[3], gd[3];
    pinhole_dir_cam_k(fx, fy, cx, cy, h, w, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      go[k] = a.grad_o ? a.grad_o[3 * i + k] : 0.f;
      gd[k] = a.grad_d ? a.grad_d[3 * i + k] : 0.f;
    }
    if (a.ndc) {
      float o[3], d[3];
      rotate_dir_cam(m, c, o, d);
      ndc_ray_bwd(o, d, a.pc.sx, a.pc.sy, a.pc.near, a.pc.two_near, go, gd);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      acc[4 * k + 0] += gd[k] * c[0];
      acc[4 * k + 1] += gd[k] * c[1];
      acc[4 * k + 2] += gd[k] * c[2];
      acc[4 * k + 3] += go[k];
    }
    if constexpr (kTable) {  // the intrinsics' share: u and |u| as pinhole_dir_cam_k forms them
      const float u0 = ((float)w - cx) / fx, u1 = -((float)h - cy) / fy;
      const float nrm = sqrtf(u0 * u0 + u1 * u1 + 1.0f);
      float gc[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) gc[j] = (m[j] * gd[0] + m[4 + j] * gd[1]) + m[8 + j] * gd[2];
      const float cg = (c[0] * gc[0] + c[1] * gc[1]) + c[2] * gc[2];
      const float gu0 = (gc[0] - c[0] * cg) / nrm, gu1 = (gc[1] - c[1] * cg) / nrm;
      acc[12] += -(gu0 * u0) / fx;
      acc[13] += -(gu1 * u1) / fy;
      acc[14] += -gu0 / fx;
      acc[15] += gu1 / fy;
    }
  }
  __shared__ float part[kPoseGradWaves][kSums];
  __shared__ float total[kSums];
  const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int k = 0; k < kSums; ++k) {
    const float s = wave_sum(acc[k]);
    if (lane == 0) part[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < kSums) {  // thread k adds sum k over the waves, in wave order every time
    float s = part[0][threadIdx.x];
    for (int w = 1; w < kPoseGradWaves; ++w) s += part[w][threadIdx.x];
    total[threadIdx.x] = s;
    if constexpr (kTable) {
      if (threadIdx.x >= 12) a.grad_K_views[4 * view + (threadIdx.x - 12)] = s;
    } else {
      if (a.grad_poses) a.grad_poses[12 * view + threadIdx.x] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && a.grad_xi) {
    float g[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) g[k] = total[k];
    pose_compose_bwd(p0, xi, g, a.grad_xi + 6 * view);
  }
}

// ---- learnable intrinsics: a table K = (fx, fy, cx, cy) [m, 4] on the device, m = 1 (shared) or n_views,
// formed from the parameter phi [m, 4] (zeros at the start) and the dataset's (H, W, f0):
//   fx = f0 exp(phi_0),  fy = f0 exp(phi_1) (tie_focal: fy = fx),  cx = W/2 + W phi_2,  cy = H/2 + H phi_3.
// phi = 0 gives (f0, f0, half_w, half_h) of pinhole_consts value for value: expf(0) = 1 and x + W * 0 = x.
__device__ __forceinline__ void intrinsics_compose(const float* __restrict__ phi, float focal0, float half_w, float half_h,
                                                   float Wf, float Hf, int tie, float (&K)[4]) {
  K[0] = focal0 * expf(phi[0]);
  K[1] = tie ? K[0] : focal0 * expf(phi[1]);
  K[2] = half_w + Wf * phi[2];
  K[3] = half_h + Hf * phi[3];
}

__global__ void __launch_bounds__(256) k_intrinsics_compose(const float* __restrict__ phi, int64_t m, float focal0,
                                                            float half_w, float half_h, float Wf, float Hf, int tie,
                                                            float* __restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  float K[4];
  intrinsics_compose(phi + 4 * r, focal0, half_w, half_h, Wf, Hf, tie, K);
#pragma unroll
  for (int k = 0; k < 4; ++k) out[4 * r + k] = K[k];
}

// The chain K -> phi: dL/dphi_0 = fx dL/dfx (+ fy dL/dfy when tied, and then dL/dphi_1 = 0), dL/dphi_1 = fy dL/dfy,
// dL/dphi_2 = W dL/dcx, dL/dphi_3 = H dL/dcy, in float64 over the float32 table values.
__device__ __forceinline__ void intrinsics_chain(const float* __restrict__ phi, const double (&gK)[4], float focal0, float Wf,
                                                 float Hf, int tie, float* __restrict__ grad_phi) {
  const double fx = (double)(focal0 * expf(phi[0]));
  if (tie) {
    grad_phi[0] = (float)(fx * gK[0] + fx * gK[1]);
    grad_phi[1] = 0.f;
  } else {
    grad_phi[0] = (float)(fx * gK[0]);
    grad_phi[1] = (float)((double)(focal0 * expf(phi[1])) * gK[1]);
  }
  grad_phi[2] = (float)((double)Wf * gK[2]);
  grad_phi[3] = (float)((double)Hf * gK[3]);
}

// per-view parameters: one thread per view
__global__ void __launch_bounds__(256) k_intrinsics_grad_rows(const float* __restrict__ phi, const float* __restrict__ gKv,
                                                              int64_t n, float focal0, float Wf, float Hf, int tie,
                                                              float* __restrict__ grad_phi) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const double gK[4] = {gKv[4 * v], gKv[4 * v + 1], gKv[4 * v + 2], gKv[4 * v + 3]};
  intrinsics_chain(phi + 4 * v, gK, focal0, Wf, Hf, tie, grad_phi + 4 * v);
}

// one shared row: ONE workgroup sums the views in float64 in a fixed order - thread (slot, column) adds the views of
// its contiguous share [slot per, (slot + 1) per) in view order, thread 0 adds the 64 slots in slot order.
constexpr int kIntrGradSlots = 64;
__global__ void __launch_bounds__(4 * kIntrGradSlots) k_intrinsics_grad_shared(const float* __restrict__ phi,
                                                                               const float* __restrict__ gKv, int64_t n,
                                                                               float focal0, float Wf, float Hf, int tie,
                                                                               float* __restrict__ grad_phi) {
  __shared__ double part[kIntrGradSlots][4];
  const int col = (int)(threadIdx.x & 3), slot = (int)(threadIdx.x >> 2);
  const int64_t per = (n + kIntrGradSlots - 1) / kIntrGradSlots;
  const int64_t v0 = min(slot * per, n), v1 = min(v0 + per, n);
  __shared__ double total[4];
  double s = 0.0;
#pragma unroll 4
  for (int64_t v = v0; v < v1; ++v) s += (double)gKv[4 * v + col];
  part[slot][col] = s;
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = part[0][threadIdx.x];
#pragma unroll 4
    for (int j = 1; j < kIntrGradSlots; ++j) t += part[j][threadIdx.x];
    total[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double gK[4] = {total[0], total[1], total[2], total[3]};
    intrinsics_chain(phi, gK, focal0, Wf, Hf, tie, grad_phi);
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

// The body of fsn_ray_pose_grad (K null: `focal` is the stored focal, grad_poses optional) and of fsn_ray_camera_grad
// (K the camera table; `focal` = focal0 still fixes the NDC map, a fixed warp of space).
static int ray_view_grad_call(const char* who, const float* poses0, const float* xi, int64_t n_views, int H, int W,
                              double focal, const float* K, int64_t k_rows, int ndc, double near, const int64_t* index,
                              const float* grad_o, const float* grad_d, int64_t count, float* grad_xi, float* grad_poses,
                              float* grad_K_views, bool table, fsn_stream_t stream) {
  FSN_REQUIRE(n_views >= 0 && H > 0 && W > 0 && focal > 0, FSN_E_INVALID, "%s: bad geometry n=%lld H=%d W=%d %s=%g", who,
              (long long)n_views, H, W, table ? "focal0" : "focal", focal);
  FSN_REQUIRE(count >= 0, FSN_E_INVALID, "%s: negative count %lld", who, (long long)count);
  FSN_REQUIRE((int64_t)H * W <= 0x7fffffff, FSN_E_UNSUPPORTED, "%s: more than 2^31 pixels per view", who);
  FSN_REQUIRE(n_views <= 0x7fffffff, FSN_E_UNSUPPORTED, "%s: too many views", who);
  if (table) {
    FSN_REQUIRE(poses0 && K && grad_K_views, FSN_E_INVALID, "%s: null poses0, K or grad_K_views", who);
    FSN_REQUIRE(k_rows == 1 || k_rows == n_views, FSN_E_INVALID, "%s: a camera table of %lld rows (1, or one per view: %lld)",
                who, (long long)k_rows, (long long)n_views);
  } else {
    FSN_REQUIRE(poses0 && xi && grad_xi, FSN_E_INVALID, "%s: null poses0, xi or grad_xi", who);
  }
  FSN_REQUIRE(count == 0 || index, FSN_E_INVALID, "%s: null index list", who);
  if (n_views == 0) return FSN_OK;
  ViewGradArgs a{};
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
  a.pc = pinhole_consts(H, W, focal, near);
  a.grad_xi = grad_xi;
  a.grad_poses = grad_poses;
  a.K = K;
  a.k_stride = k_rows == 1 ? 0 : 4;
  a.grad_K_views = grad_K_views;
  // (count = 0: every view's gradient is 0)
  if (table)
    k_ray_view_grad<true><<<(unsigned)n_views, kPoseGradThreads, 0, as_stream(stream)>>>(a);
  else
    k_ray_view_grad<false><<<(unsigned)n_views, kPoseGradThreads, 0, as_stream(stream)>>>(a);
  FSN_LAUNCH_CHECK("k_ray_view_grad");
  return FSN_OK;
}

extern "C" int fsn_ray_pose_grad(const float* poses0, const float* xi, int64_t n_views, int H, int W, double focal, int ndc,
                                 double near, const int64_t* index, const float* grad_o, const float* grad_d, int64_t count,
                                 float* grad_xi, float* grad_poses, fsn_stream_t stream) {
  return ray_view_grad_call("fsn_ray_pose_grad", poses0, xi, n_views, H, W, focal, nullptr, 0, ndc, near, index, grad_o,
                            grad_d, count, grad_xi, grad_poses, nullptr, false, stream);
}

extern "C" int fsn_intrinsics_compose(const float* phi, int64_t m, int H, int W, double focal0, int tie_focal, float* K_out,
                                      fsn_stream_t stream) {
  FSN_REQUIRE(m >= 0 && H > 0 && W > 0 && focal0 > 0, FSN_E_INVALID,
              "fsn_intrinsics_compose: bad geometry m=%lld H=%d W=%d focal0=%g", (long long)m, H, W, focal0);
  FSN_REQUIRE(phi && K_out, FSN_E_INVALID, "fsn_intrinsics_compose: null pointer");
  if (m == 0) return FSN_OK;
  FSN_REQUIRE((m + 255) / 256 <= 0x7fffffff, FSN_E_UNSUPPORTED, "fsn_intrinsics_compose: too many rows");
  const PinholeConsts pc = pinhole_consts(H, W, focal0, 0.0);  // phi = 0 gives fsn_ray_batch's launch constants
  k_intrinsics_compose<<<(unsigned)((m + 255) / 256), 256, 0, as_stream(stream)>>>(
      phi, m, pc.focal, pc.half_w, pc.half_h, (float)W, (float)H, tie_focal ? 1 : 0, K_out);
  FSN_LAUNCH_CHECK("k_intrinsics_compose");
  return FSN_OK;
}

extern "C" int fsn_ray_camera_grad(const float* poses0, const float* xi, int64_t n_views, int H, int W, double focal0,
                                   const float* K, int64_t k_rows, int ndc, double near, const int64_t* index,
                                   const float* grad_o, const float* grad_d, int64_t count, float* grad_xi,
                                   float* grad_K_views, fsn_stream_t stream) {
  return ray_view_grad_call("fsn_ray_camera_grad", poses0, xi, n_views, H, W, focal0, K, k_rows, ndc, near, index, grad_o,
                            grad_d, count, grad_xi, nullptr, grad_K_views, true, stream);
}

extern "C" int fsn_intrinsics_grad(const float* phi, const float* grad_K_views, int64_t n_views, int64_t m, int H, int W,
                                   double focal0, int tie_focal, float* grad_phi, fsn_stream_t stream) {
  FSN_REQUIRE(n_views >= 0 && H > 0 && W > 0 && focal0 > 0, FSN_E_INVALID,
              "fsn_intrinsics_grad: bad geometry n=%lld H=%d W=%d focal0=%g", (long long)n_views, H, W, focal0);
  FSN_REQUIRE(m == 1 || m == n_views, FSN_E_INVALID,
              "fsn_intrinsics_grad: a parameter of %lld rows (1, or one per view: %lld)", (long long)m, (long long)n_views);
  FSN_REQUIRE(phi && grad_phi && (grad_K_views || n_views == 0), FSN_E_INVALID, "fsn_intrinsics_grad: null pointer");
  const int tie = tie_focal ? 1 : 0;
  if (m == 1) {  // (no view at all: the sum is empty and the row is written as 0)
    k_intrinsics_grad_shared<<<1, 4 * kIntrGradSlots, 0, as_stream(stream)>>>(phi, grad_K_views, n_views, (float)focal0,
                                                                              (float)W, (float)H, tie, grad_phi);
    FSN_LAUNCH_CHECK("k_intrinsics_grad_shared");
    return FSN_OK;
  }
  if (n_views == 0) return FSN_OK;
  FSN_REQUIRE((n_views + 255) / 256 <= 0x7fffffff, FSN_E_UNSUPPORTED, "fsn_intrinsics_grad: too many views");
  k_intrinsics_grad_rows<<<(unsigned)((n_views + 255) / 256), 256, 0, as_stream(stream)>>>(
      phi, grad_K_views, n_views, (float)focal0, (float)W, (float)H, tie, grad_phi);
  FSN_LAUNCH_CHECK("k_intrinsics_grad_rows");
  return FSN_OK;
}
