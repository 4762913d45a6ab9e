// composite_grad.hip — the backward of the packed volume integration (every output of fsn_composite_packed_fwd may
// carry a cotangent: colors, opacity, depth, weights, alphas, trans) and the distortion loss on the compositor's
// weights, the first consumer of dL/dweights.  ONE kernel serves both entry points: fsn_composite_packed_bwd (the
// timed training step: colors and opacity only) is fsn_composite_packed_bwd_full with the other cotangents NULL.
// One wavefront per ray on ray_dev.hpp's skeleton (ray_work / ray_launch); the backward's equations are its
// density_bwd_ray, which this kernel gives q_i and the d_rgb store.  No LDS, no atomics, every sum in a fixed order.
// DESIGN.md, "Full compositor backward".
#include "common.hpp"
#include "ray_dev.hpp"

namespace fsn {

// Per ray, samples i in packed order: dt_i = t1_i - t0_i, m_i = (t0_i + t1_i)/2, T_i = exp(-sum_{j<i} sigma_j dt_j),
// e_i = exp(-sigma_i dt_i), alpha_i = 1 - e_i, w_i = T_i alpha_i, O = sum w, D = sum w m / max(O, eps).  With the
// cotangents g (colors), g_O, g_D per ray and u_i, a_i, tau_i per sample (weights, alphas, trans):
//   k_i = (m_i - D)/O  for O >= eps (torch.clamp passes the gradient at equality),  m_i/eps otherwise
//   q_i = g.c_i - g.bkgd + g_O + g_D k_i + u_i
//   dL/dalpha_i = A_i = q_i T_i + a_i,   dL/dT_i = B_i = q_i alpha_i + tau_i
//   dL/dsigma_i = dt_i ( A_i e_i - sum_{j>i} B_j T_j ),   dL/dc_i = w_i g          (A, B, the suffix: density_bwd_ray)
// Every optional pointer is a kernel argument, so its NULL branch is wave-uniform and nothing is loaded through it.
// (d_colors and d_opacity included: an absent one is zero).  With d_depth = d_w = d_a = d_tr = NULL what is left is
//   q_i = g.c_i - g.bkgd + g_O,   dL/dsigma_i = dt_i ( q_i T_i e_i - sum_{j>i} q_j w_j ).
__global__ void k_composite_packed_bwd_full(const float* __restrict__ sig, const float* __restrict__ rgb,
                                            const float* __restrict__ t0, const float* __restrict__ t1, SpanArgs sp,
                                            int64_t R, float b0, float b1, float b2,
                                            const float* __restrict__ d_colors, const float* __restrict__ d_opacity,
                                            const float* __restrict__ opacity, const float* __restrict__ depth,
                                            const float* __restrict__ d_depth, const float* __restrict__ d_w,
                                            const float* __restrict__ d_a, const float* __restrict__ d_tr,
                                            float* __restrict__ d_sig, float* __restrict__ d_rgb) {
  RayWork w;
  if (!ray_work(sp, R, w)) return;
  const int64_t r = w.r, beg = w.beg;
  const float* c_ = rgb + 3 * beg; const float* a_ = t0 + beg; const float* e_ = t1 + beg;
  const float* u_ = d_w ? d_w + beg : nullptr;
  const float g0 = d_colors ? d_colors[3 * r] : 0.f, g1 = d_colors ? d_colors[3 * r + 1] : 0.f,
              g2 = d_colors ? d_colors[3 * r + 2] : 0.f;
  const float gop = d_opacity ? d_opacity[r] : 0.f;
  const float gb = g0 * b0 + g1 * b1 + g2 * b2;
  float ks = 0.f, kd = 0.f;  // g_D k_i = ks (m_i - kd)
  if (d_depth) {
    const float O = opacity[r];
    const bool regular = O >= kFltEps;
    ks = d_depth[r] / (regular ? O : kFltEps);
    kd = regular ? depth[r] : 0.f;
  }
  auto q_of = [&](int i) {
    float q = (g0 * c_[3 * i] + g1 * c_[3 * i + 1] + g2 * c_[3 * i + 2]) - gb + gop;
    if (d_depth) q += ks * ((a_[i] + e_[i]) / 2.0f - kd);
    if (u_) q += u_[i];
    return q;
  };
  float* dc_ = d_rgb + 3 * beg;
  density_bwd_ray(sig + beg, a_, e_, w.i0, w.i1, true, q_of, d_tr ? d_tr + beg : nullptr, d_a ? d_a + beg : nullptr,
                  nullptr, d_sig + beg, [&](int i, float wi) {
                    dc_[3 * i + 0] = wi * g0;
                    dc_[3 * i + 1] = wi * g1;
                    dc_[3 * i + 2] = wi * g2;
                  });
}

// ------------------------------------------------------------------ distortion loss (mip-NeRF 360, interval form)
// L_r = sum_i [ 2 w_i (m_i W_i - V_i) + w_i^2 dt_i / 3 ],  W_i = sum_{j<i} w_j,  V_i = sum_{j<i} w_j m_j:
// one wavefront per ray, two scans (of w and of w m), the lanes' partial sums added by the wave's butterfly.  A ray
// without samples gives 0.
__global__ void k_distortion_fwd(const float* __restrict__ w, const float* __restrict__ t0, const float* __restrict__ t1,
                                 SpanArgs sp, int64_t R, float* __restrict__ out) {
  RayWork rw;
  if (!ray_work(sp, R, rw)) {
    if (rw.r < R && rw.lane == 0) out[rw.r] = 0.f;
    return;
  }
  const int64_t r = rw.r, beg = rw.beg;
  const int lane = rw.lane, i0 = rw.i0, i1 = rw.i1;
  const float* w_ = w + beg; const float* a_ = t0 + beg; const float* e_ = t1 + beg;
  float lw = 0.f, lv = 0.f;
  for (int i = i0; i < i1; ++i) {
    lw += w_[i];
    lv += w_[i] * ((a_[i] + e_[i]) / 2.0f);
  }
  float wtot, vtot;
  float W = wave_excl_scan(lw, wtot), V = wave_excl_scan(lv, vtot);
  float acc = 0.f;
  for (int i = i0; i < i1; ++i) {
    const float wi = w_[i], m = (a_[i] + e_[i]) / 2.0f;
    acc += 2.0f * wi * (m * W - V) + wi * wi * (e_[i] - a_[i]) / 3.0f;
    W += wi;
    V += wi * m;
  }
  acc = wave_sum(acc);
  if (lane == 0) out[r] = acc;
}

// dL_r/dw_k = 2 ( m_k W_k - V_k + V'_k - m_k W'_k ) + 2 w_k dt_k / 3,  W'_k = sum_{j>k} w_j,  V'_k = sum_{j>k} w_j m_j
// (suffix = total - prefix - own term), times the ray's cotangent d_out[r].
__global__ void k_distortion_bwd(const float* __restrict__ w, const float* __restrict__ t0, const float* __restrict__ t1,
                                 SpanArgs sp, int64_t R, const float* __restrict__ d_out, float* __restrict__ d_w) {
  RayWork rw;
  if (!ray_work(sp, R, rw)) return;
  const int64_t beg = rw.beg;
  const int i0 = rw.i0, i1 = rw.i1;
  const float* w_ = w + beg; const float* a_ = t0 + beg; const float* e_ = t1 + beg;
  const float g = d_out[rw.r];
  float lw = 0.f, lv = 0.f;
  for (int i = i0; i < i1; ++i) {
    lw += w_[i];
    lv += w_[i] * ((a_[i] + e_[i]) / 2.0f);
  }
  float wtot, vtot;
  float W = wave_excl_scan(lw, wtot), V = wave_excl_scan(lv, vtot);
  for (int i = i0; i < i1; ++i) {
    const float wi = w_[i], m = (a_[i] + e_[i]) / 2.0f;
    const float Ws = wtot - W - wi, Vs = vtot - V - wi * m;
    d_w[beg + i] = g * (2.0f * ((m * W - V) + (Vs - m * Ws)) + 2.0f * wi * (e_[i] - a_[i]) / 3.0f);
    W += wi;
    V += wi * m;
  }
}

}  // namespace fsn

using namespace fsn;

// the shared checks, the two memsets and the launch of both compositor-backward entry points
static int composite_bwd_launch(const char* who, const float* sigmas, const float* rgbs, const float* t_starts,
                                const float* t_ends, const int64_t* ray_indices, int64_t N, int64_t R,
                                const float* bkgd_host, const float* d_colors, const float* d_opacity, const float* opacity,
                                const float* depth, const float* d_depth, const float* d_weights, const float* d_alphas,
                                const float* d_trans, float* d_sigmas, float* d_rgbs, fsn_stream_t stream) {
  FSN_REQUIRE(N >= 0 && R >= 0, FSN_E_INVALID, "%s: bad sizes", who);
  FSN_REQUIRE(!d_depth || (opacity && depth), FSN_E_INVALID, "%s: d_depth needs the forward's opacity and depth", who);
  RayLaunch L;
  if (int rc = ray_launch(who, ray_indices, nullptr, N, R, 0, false, &L)) return rc;
  if (!L.launch) return FSN_OK;
  FSN_REQUIRE(sigmas && rgbs && t_starts && t_ends && d_sigmas && d_rgbs, FSN_E_INVALID, "%s: null pointer", who);
  const float b0 = bkgd_host ? bkgd_host[0] : 0.f, b1 = bkgd_host ? bkgd_host[1] : 0.f, b2 = bkgd_host ? bkgd_host[2] : 0.f;
  FSN_HIP(hipMemsetAsync(d_sigmas, 0, (size_t)N * sizeof(float), as_stream(stream)));
  FSN_HIP(hipMemsetAsync(d_rgbs, 0, (size_t)N * 3 * sizeof(float), as_stream(stream)));
  k_composite_packed_bwd_full<<<L.grid, 256, 0, as_stream(stream)>>>(sigmas, rgbs, t_starts, t_ends, L.sp, R, b0, b1, b2,
                                                                    d_colors, d_opacity, opacity, depth, d_depth, d_weights,
                                                                    d_alphas, d_trans, d_sigmas, d_rgbs);
  FSN_LAUNCH_CHECK("k_composite_packed_bwd_full");
  return FSN_OK;
}

extern "C" int fsn_composite_packed_bwd_full(const float* sigmas, const float* rgbs, const float* t_starts,
                                             const float* t_ends, const int64_t* ray_indices, int64_t N, int64_t R,
                                             const float* bkgd_host, const float* d_colors, const float* d_opacity,
                                             const float* opacity, const float* depth, const float* d_depth,
                                             const float* d_weights, const float* d_alphas, const float* d_trans,
                                             float* d_sigmas, float* d_rgbs, fsn_stream_t stream) {
  return composite_bwd_launch("fsn_composite_packed_bwd_full", sigmas, rgbs, t_starts, t_ends, ray_indices, N, R,
                              bkgd_host, d_colors, d_opacity, opacity, depth, d_depth, d_weights, d_alphas, d_trans,
                              d_sigmas, d_rgbs, stream);
}

// colors and opacity only (the training step); unlike the full form it requires d_colors
extern "C" int fsn_composite_packed_bwd(const float* sigmas, const float* rgbs, const float* t_starts, const float* t_ends,
                                        const int64_t* ray_indices, int64_t N, int64_t R, const float* bkgd_host,
                                        const float* d_colors, const float* d_opacity, float* d_sigmas, float* d_rgbs,
                                        fsn_stream_t stream) {
  FSN_REQUIRE(d_colors || N <= 0 || R <= 0, FSN_E_INVALID, "fsn_composite_packed_bwd: null pointer");
  return composite_bwd_launch("fsn_composite_packed_bwd", sigmas, rgbs, t_starts, t_ends, ray_indices, N, R, bkgd_host,
                              d_colors, d_opacity, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d_sigmas, d_rgbs,
                              stream);
}

extern "C" int fsn_distortion_fwd(const float* weights, const float* t_starts, const float* t_ends,
                                  const int64_t* ray_indices, int64_t N, int64_t n_rays, float* out, fsn_stream_t stream) {
  RayLaunch L;
  if (int rc = ray_launch("fsn_distortion_fwd", ray_indices, nullptr, N, n_rays, 0, false, &L)) return rc;
  if (!L.launch) {
    if (N == 0 && n_rays > 0 && out)  // every ray is empty
      FSN_HIP(hipMemsetAsync(out, 0, (size_t)n_rays * sizeof(float), as_stream(stream)));
    return FSN_OK;
  }
  FSN_REQUIRE(weights && t_starts && t_ends && out, FSN_E_INVALID, "fsn_distortion_fwd: null pointer");
  k_distortion_fwd<<<L.grid, 256, 0, as_stream(stream)>>>(weights, t_starts, t_ends, L.sp, n_rays, out);
  FSN_LAUNCH_CHECK("k_distortion_fwd");
  return FSN_OK;
}

extern "C" int fsn_distortion_bwd(const float* weights, const float* t_starts, const float* t_ends,
                                  const int64_t* ray_indices, int64_t N, int64_t n_rays, const float* d_out,
                                  float* d_weights, fsn_stream_t stream) {
  RayLaunch L;
  if (int rc = ray_launch("fsn_distortion_bwd", ray_indices, nullptr, N, n_rays, 0, false, &L)) return rc;
  if (!L.launch) return FSN_OK;
  FSN_REQUIRE(weights && t_starts && t_ends && d_out && d_weights, FSN_E_INVALID, "fsn_distortion_bwd: null pointer");
  FSN_HIP(hipMemsetAsync(d_weights, 0, (size_t)N * sizeof(float), as_stream(stream)));
  k_distortion_bwd<<<L.grid, 256, 0, as_stream(stream)>>>(weights, t_starts, t_ends, L.sp, n_rays, d_out, d_weights);
  FSN_LAUNCH_CHECK("k_distortion_bwd");
  return FSN_OK;
}
