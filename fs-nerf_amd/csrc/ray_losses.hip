// ray_losses.hip — the few-shot geometry losses ("Few-shot geometry losses"): the entropy of a ray's
// termination distribution (InfoNeRF), the depth KL term on the compositor's weights (DS-NeRF's "sigma loss") and the
// l2 total variation of a rendered depth patch (RegNeRF's compute_tv_norm).  The definitions are this package's own.
// The two ray losses run one wavefront per ray on ray_dev.hpp's skeleton (ray_work / ray_launch), the lanes striding
// over the ray's samples; the patch loss runs one wavefront per patch forward and one thread per pixel backward.
// No LDS, no atomics, every sum in a fixed order; each backward writes every entry of its output once (after a memset).
#include "common.hpp"
#include "ray_dev.hpp"

namespace fsn {

// ------------------------------------------------------------------ ray entropy (InfoNeRF)
// u_i = max(v_i, 0), s = sum u_i, p_i = u_i / (s + eps), H_r = -scale c_r sum_i p_i log(p_i + eps).  Two passes over
// the ray: s, then the sum.  A ray with c_r == 0 is skipped (value 0), as is one without samples.
__device__ __forceinline__ float entropy_mass(const float* __restrict__ v_, int S, int lane) {
  float ls = 0.f;
  for (int i = lane; i < S; i += 64) ls += fmaxf(v_[i], 0.f);
  return wave_sum(ls);
}

__global__ void k_ray_entropy_fwd(const float* __restrict__ v, SpanArgs sp, int64_t R, const float* __restrict__ c,
                                  float eps, float scale, float* __restrict__ out) {
  RayWork rw;
  const bool any = ray_work(sp, R, rw);
  if (rw.r >= R) return;
  const float cr = c ? c[rw.r] : 1.0f;
  if (!any || cr == 0.f) {
    if (rw.lane == 0) out[rw.r] = 0.f;
    return;
  }
  const float* v_ = v + rw.beg;
  const float den = entropy_mass(v_, rw.S, rw.lane) + eps;
  float acc = 0.f;
  for (int i = rw.lane; i < rw.S; i += 64) {
    const float p = fmaxf(v_[i], 0.f) / den;
    acc += p * logf(p + eps);
  }
  acc = wave_sum(acc);
  if (rw.lane == 0) out[rw.r] = -(scale * cr) * acc;
}

// f'(p) = -log(p + eps) - p / (p + eps);  dH_r/dv_k = g_r scale c_r ( f'(p_k) - sum_i p_i f'(p_i) ) / (s + eps) where
// v_k >= 0 (torch.clamp(min=0) passes the gradient at equality), 0 below.  Skipped rays keep the memset's zeros.
__global__ void k_ray_entropy_bwd(const float* __restrict__ v, SpanArgs sp, int64_t R, const float* __restrict__ c,
                                  float eps, float scale, const float* __restrict__ d_out, float* __restrict__ d_v) {
  RayWork rw;
  if (!ray_work(sp, R, rw)) return;
  const float cr = c ? c[rw.r] : 1.0f;
  if (cr == 0.f) return;
  const float* v_ = v + rw.beg;
  float* d_ = d_v + rw.beg;
  const float den = entropy_mass(v_, rw.S, rw.lane) + eps;
  auto fprime = [&](float p) { return -logf(p + eps) - p / (p + eps); };
  float acc = 0.f;
  for (int i = rw.lane; i < rw.S; i += 64) {
    const float p = fmaxf(v_[i], 0.f) / den;
    acc += p * fprime(p);
  }
  acc = wave_sum(acc);
  const float k = d_out[rw.r] * (scale * cr);
  for (int i = rw.lane; i < rw.S; i += 64) {
    const float vi = v_[i];
    const float p = fmaxf(vi, 0.f) / den;
    d_[i] = vi >= 0.f ? k * (fprime(p) - acc) / den : 0.f;
  }
}

// ------------------------------------------------------------------ depth KL (DS-NeRF's "sigma loss")
// L_r = sum_i -log(max(w_i, 0) + eps) exp(-(m_i - depth_r)^2 / (2 var_r)) dt_i for a supervised ray: depth_r and var_r
// both finite and > 0.  Any other ray gives 0 and no gradient.
__device__ __forceinline__ bool kl_supervised(float depth, float var) {
  return isfinite(depth) && depth > 0.f && isfinite(var) && var > 0.f;
}
__device__ __forceinline__ float kl_gauss(float t0, float t1, float depth, float var) {
  const float dm = (t0 + t1) / 2.0f - depth;
  return expf(-(dm * dm) / (2.0f * var));
}

__global__ void k_depth_kl_fwd(const float* __restrict__ w, const float* __restrict__ t0, const float* __restrict__ t1,
                               SpanArgs sp, int64_t R, const float* __restrict__ depth, const float* __restrict__ var,
                               float eps, float* __restrict__ out) {
  RayWork rw;
  const bool any = ray_work(sp, R, rw);
  if (rw.r >= R) return;
  const float dr = depth[rw.r], vr = var[rw.r];
  if (!any || !kl_supervised(dr, vr)) {
    if (rw.lane == 0) out[rw.r] = 0.f;
    return;
  }
  const float* w_ = w + rw.beg; const float* a_ = t0 + rw.beg; const float* e_ = t1 + rw.beg;
  float acc = 0.f;
  for (int i = rw.lane; i < rw.S; i += 64)
    acc += -logf(fmaxf(w_[i], 0.f) + eps) * kl_gauss(a_[i], e_[i], dr, vr) * (e_[i] - a_[i]);
  acc = wave_sum(acc);
  if (rw.lane == 0) out[rw.r] = acc;
}

// dL_r/dw_k = -g_r exp(...)_k dt_k / (w_k + eps) where w_k >= 0, 0 below
__global__ void k_depth_kl_bwd(const float* __restrict__ w, const float* __restrict__ t0, const float* __restrict__ t1,
                               SpanArgs sp, int64_t R, const float* __restrict__ depth, const float* __restrict__ var,
                               float eps, const float* __restrict__ d_out, float* __restrict__ d_w) {
  RayWork rw;
  if (!ray_work(sp, R, rw)) return;
  const float dr = depth[rw.r], vr = var[rw.r];
  if (!kl_supervised(dr, vr)) return;
  const float* w_ = w + rw.beg; const float* a_ = t0 + rw.beg; const float* e_ = t1 + rw.beg;
  float* d_ = d_w + rw.beg;
  const float g = d_out[rw.r];
  for (int i = rw.lane; i < rw.S; i += 64) {
    const float wi = w_[i];
    d_[i] = wi >= 0.f ? -g * kl_gauss(a_[i], e_[i], dr, vr) * (e_[i] - a_[i]) / (wi + eps) : 0.f;
  }
}

// ------------------------------------------------------------------ patch depth smoothness (RegNeRF, l2)
// S_b = sum over the anchors (i, j), i < P-1, j < Q-1, of (d[i,j] - d[i,j+1])^2 + (d[i,j] - d[i+1,j])^2.  One wave per
// patch (four per block), the lanes striding over the anchors; a patch without anchors (P or Q is 1) gives 0.
__global__ void k_patch_tv_fwd(const float* __restrict__ d, int64_t B, int P, int Q, float* __restrict__ out) {
  const int lane = lane_id();
  const int64_t b = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (b >= B) return;
  const float* d_ = d + b * (int64_t)P * Q;
  const int64_t qa = Q - 1, n_anchor = (int64_t)(P - 1) * qa;
  float acc = 0.f;
  for (int64_t a = lane; a < n_anchor; a += 64) {
    const int64_t i = a / qa, j = a - i * qa;
    const float c = d_[i * Q + j];
    const float dh = c - d_[i * Q + j + 1], dv = c - d_[(i + 1) * Q + j];
    acc += dh * dh + dv * dv;
  }
  acc = wave_sum(acc);
  if (lane == 0) out[b] = acc;
}

// Gather form: pixel (i, j) of patch b takes part in its own anchor's two differences (i < P-1 and j < Q-1), in the
// horizontal difference of the anchor to its left (j >= 1, i < P-1) and in the vertical one of the anchor above
// (i >= 1, j < Q-1); the terms are added in that order.
__global__ void k_patch_tv_bwd(const float* __restrict__ d, int64_t n_pix, int P, int Q, const float* __restrict__ d_out,
                               float* __restrict__ d_d) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_pix) return;
  const int64_t pq = (int64_t)P * Q;
  const int64_t b = k / pq, rem = k - b * pq;
  const int i = (int)(rem / Q), j = (int)(rem - (int64_t)i * Q);
  const float c = d[k];
  float acc = 0.f;
  if (i < P - 1 && j < Q - 1) acc += 2.0f * (c - d[k + 1]) + 2.0f * (c - d[k + Q]);
  if (j >= 1 && i < P - 1) acc += -2.0f * (d[k - 1] - c);
  if (i >= 1 && j < Q - 1) acc += -2.0f * (d[k - Q] - c);
  d_d[k] = d_out[b] * acc;
}

}  // namespace fsn

using namespace fsn;

// what the two ray losses' forwards share after ray_launch: nothing to launch -> zero `out` when every ray is empty
static int ray_loss_empty_fwd(int64_t N, int64_t n_rays, float* out, fsn_stream_t stream) {
  if (N == 0 && n_rays > 0 && out) FSN_HIP(hipMemsetAsync(out, 0, (size_t)n_rays * sizeof(float), as_stream(stream)));
  return FSN_OK;
}
// ... and their backwards: samples without a ray to own them (n_rays == 0) still get their zero
static int ray_loss_empty_bwd(int64_t N, float* d_in, fsn_stream_t stream) {
  if (N > 0 && d_in) FSN_HIP(hipMemsetAsync(d_in, 0, (size_t)N * sizeof(float), as_stream(stream)));
  return FSN_OK;
}

extern "C" int fsn_ray_entropy_fwd(const float* values, const int64_t* ray_indices, int64_t N, int64_t n_rays,
                                   const float* ray_weight, float eps, float scale, float* out, fsn_stream_t stream) {
  RayLaunch L;
  if (int rc = ray_launch("fsn_ray_entropy_fwd", ray_indices, nullptr, N, n_rays, 0, false, &L)) return rc;
  if (!L.launch) return ray_loss_empty_fwd(N, n_rays, out, stream);
  FSN_REQUIRE(values && out, FSN_E_INVALID, "fsn_ray_entropy_fwd: null pointer");
  FSN_REQUIRE(eps > 0.f, FSN_E_INVALID, "fsn_ray_entropy_fwd: eps must be positive");
  k_ray_entropy_fwd<<<L.grid, 256, 0, as_stream(stream)>>>(values, L.sp, n_rays, ray_weight, eps, scale, out);
  FSN_LAUNCH_CHECK("k_ray_entropy_fwd");
  return FSN_OK;
}

extern "C" int fsn_ray_entropy_bwd(const float* values, const int64_t* ray_indices, int64_t N, int64_t n_rays,
                                   const float* ray_weight, float eps, float scale, const float* d_out, float* d_values,
                                   fsn_stream_t stream) {
  RayLaunch L;
  if (int rc = ray_launch("fsn_ray_entropy_bwd", ray_indices, nullptr, N, n_rays, 0, false, &L)) return rc;
  if (!L.launch) return ray_loss_empty_bwd(N, d_values, stream);
  FSN_REQUIRE(values && d_out && d_values, FSN_E_INVALID, "fsn_ray_entropy_bwd: null pointer");
  FSN_REQUIRE(eps > 0.f, FSN_E_INVALID, "fsn_ray_entropy_bwd: eps must be positive");
  FSN_HIP(hipMemsetAsync(d_values, 0, (size_t)N * sizeof(float), as_stream(stream)));
  k_ray_entropy_bwd<<<L.grid, 256, 0, as_stream(stream)>>>(values, L.sp, n_rays, ray_weight, eps, scale, d_out, d_values);
  FSN_LAUNCH_CHECK("k_ray_entropy_bwd");
  return FSN_OK;
}

extern "C" int fsn_depth_kl_fwd(const float* weights, const float* t_starts, const float* t_ends,
                                const int64_t* ray_indices, int64_t N, int64_t n_rays, const float* depth,
                                const float* var, float eps, float* out, fsn_stream_t stream) {
  RayLaunch L;
  if (int rc = ray_launch("fsn_depth_kl_fwd", ray_indices, nullptr, N, n_rays, 0, false, &L)) return rc;
  if (!L.launch) return ray_loss_empty_fwd(N, n_rays, out, stream);
  FSN_REQUIRE(weights && t_starts && t_ends && depth && var && out, FSN_E_INVALID, "fsn_depth_kl_fwd: null pointer");
  FSN_REQUIRE(eps > 0.f, FSN_E_INVALID, "fsn_depth_kl_fwd: eps must be positive");
  k_depth_kl_fwd<<<L.grid, 256, 0, as_stream(stream)>>>(weights, t_starts, t_ends, L.sp, n_rays, depth, var, eps, out);
  FSN_LAUNCH_CHECK("k_depth_kl_fwd");
  return FSN_OK;
}

extern "C" int fsn_depth_kl_bwd(const float* weights, const float* t_starts, const float* t_ends,
                                const int64_t* ray_indices, int64_t N, int64_t n_rays, const float* depth,
                                const float* var, float eps, const float* d_out, float* d_weights, fsn_stream_t stream) {
  RayLaunch L;
  if (int rc = ray_launch("fsn_depth_kl_bwd", ray_indices, nullptr, N, n_rays, 0, false, &L)) return rc;
  if (!L.launch) return ray_loss_empty_bwd(N, d_weights, stream);
  FSN_REQUIRE(weights && t_starts && t_ends && depth && var && d_out && d_weights, FSN_E_INVALID,
              "fsn_depth_kl_bwd: null pointer");
  FSN_REQUIRE(eps > 0.f, FSN_E_INVALID, "fsn_depth_kl_bwd: eps must be positive");
  FSN_HIP(hipMemsetAsync(d_weights, 0, (size_t)N * sizeof(float), as_stream(stream)));
  k_depth_kl_bwd<<<L.grid, 256, 0, as_stream(stream)>>>(weights, t_starts, t_ends, L.sp, n_rays, depth, var, eps, d_out,
                                                       d_weights);
  FSN_LAUNCH_CHECK("k_depth_kl_bwd");
  return FSN_OK;
}

// sizes of both patch entry points: B >= 0, P, Q >= 1, and a grid that fits
static int patch_tv_sizes(const char* who, int64_t B, int P, int Q) {
  FSN_REQUIRE(B >= 0 && P >= 1 && Q >= 1, FSN_E_INVALID, "%s: bad sizes", who);
  FSN_REQUIRE(B <= 0x7fffffff && (double)B * P * Q <= 256.0 * 0x7fffffff, FSN_E_INVALID, "%s: bad sizes (too many pixels)",
              who);
  return FSN_OK;
}

extern "C" int fsn_patch_tv_fwd(const float* depth, int64_t B, int P, int Q, float* out, fsn_stream_t stream) {
  if (int rc = patch_tv_sizes("fsn_patch_tv_fwd", B, P, Q)) return rc;
  if (B == 0) return FSN_OK;
  FSN_REQUIRE(depth && out, FSN_E_INVALID, "fsn_patch_tv_fwd: null pointer");
  k_patch_tv_fwd<<<(unsigned)((B + 3) / 4), 256, 0, as_stream(stream)>>>(depth, B, P, Q, out);
  FSN_LAUNCH_CHECK("k_patch_tv_fwd");
  return FSN_OK;
}

extern "C" int fsn_patch_tv_bwd(const float* depth, int64_t B, int P, int Q, const float* d_out, float* d_depth,
                                fsn_stream_t stream) {
  if (int rc = patch_tv_sizes("fsn_patch_tv_bwd", B, P, Q)) return rc;
  if (B == 0) return FSN_OK;
  FSN_REQUIRE(depth && d_out && d_depth, FSN_E_INVALID, "fsn_patch_tv_bwd: null pointer");
  const int64_t n_pix = B * (int64_t)P * Q;
  FSN_HIP(hipMemsetAsync(d_depth, 0, (size_t)n_pix * sizeof(float), as_stream(stream)));
  if (P == 1 || Q == 1) return FSN_OK;  // no anchors: the zeros are the gradient
  k_patch_tv_bwd<<<(unsigned)((n_pix + 255) / 256), 256, 0, as_stream(stream)>>>(depth, n_pix, P, Q, d_out, d_depth);
  FSN_LAUNCH_CHECK("k_patch_tv_bwd");
  return FSN_OK;
}
