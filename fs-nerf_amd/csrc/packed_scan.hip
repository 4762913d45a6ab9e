// packed_scan.hip — the packed volume-rendering primitives behind render/volrend.py: per-ray scans (sum / product,
// inclusive / exclusive) with their backwards, weights / transmittance / alphas from densities or from alphas with the
// backward, the visibility rule (on densities and on alphas), the per-ray accumulation with its backward, and pack_info.
// One wavefront per ray, four rays per 256-thread block: ray_work / ray_launch, the density forms' trans_walk and
// density_bwd_ray, and the cross-lane scans (wave_excl_scan / _prod / _affine_rev) are ray_dev.hpp's.  No LDS, no
// atomics, every sum in a fixed order, float32, -ffp-contract=off.  The two elementwise parts (k_accumulate_bwd)
// stride the lanes over the ray's samples instead: nothing is summed across samples there.
// DESIGN.md, "Packed volume-rendering primitives".
#include "common.hpp"
#include "ray_dev.hpp"

namespace fsn {

__global__ void k_pack_info(const int64_t* __restrict__ ri, int64_t N, int64_t R, int64_t* __restrict__ info) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const auto [beg, S] = ray_span(ri, N, r);
  info[2 * r] = beg;
  info[2 * r + 1] = S;
}

// out[k] = sum / product of x[j], j < k (exclusive) or j <= k (inclusive), within the ray
__global__ void k_packed_scan_fwd(const float* __restrict__ x, SpanArgs sp, int64_t R, int prod, int exclusive,
                                  float* __restrict__ out) {
  RayWork w;
  if (!ray_work(sp, R, w)) return;
  const int64_t beg = w.beg;
  const int i0 = w.i0, i1 = w.i1;
  const float* x_ = x + beg;
  float* o_ = out + beg;
  if (prod) {
    float lp = 1.0f;
    for (int i = i0; i < i1; ++i) lp *= x_[i];
    float run = wave_excl_scan_prod(lp);
    for (int i = i0; i < i1; ++i) {
      const float v = x_[i];
      const float inc = run * v;
      o_[i] = exclusive ? run : inc;
      run = inc;
    }
  } else {
    float ls = 0.f;
    for (int i = i0; i < i1; ++i) ls += x_[i];
    float tot;
    float run = wave_excl_scan(ls, tot);
    for (int i = i0; i < i1; ++i) {
      const float inc = run + x_[i];
      o_[i] = exclusive ? run : inc;
      run = inc;
    }
  }
}

// Backward of the scan, division-free.  With P_k = prod_{j<k} x_j (1 for a sum) and g = d_out:
//   exclusive:  d_x[k] = P_k S_k,  S_k = g[k+1] + x[k+1] S_{k+1}
//   inclusive:  d_x[k] = P_k S_k,  S_k = g[k]   + x[k+1] S_{k+1}           (S = 0 past the ray's end; x = 1 for a sum)
// Both are H = f_k(f_{k+1}(... f_{S-1}(0))) of the maps f_j(s) = g[j] + a_j s, a_j = x[j] (exclusive, S_k = H_{k+1}) or
// a_j = x[j+1] (inclusive, S_k = H_k).  A lane composes its samples' maps into one (A, B), the lanes' maps are scanned
// from the ray's end, and the lane walks its samples backwards; the product form then multiplies by P_k going forwards.
__global__ void k_packed_scan_bwd(const float* __restrict__ x, const float* __restrict__ g, SpanArgs sp, int64_t R,
                                  int prod, int exclusive, float* __restrict__ d_x) {
  RayWork w;
  if (!ray_work(sp, R, w)) return;
  const int64_t beg = w.beg;
  const int i0 = w.i0, i1 = w.i1;
  const int S = w.S;
  const float* x_ = prod ? x + beg : nullptr;
  const float* g_ = g + beg;
  float* o_ = d_x + beg;
  auto a_of = [&](int j) -> float {
    if (!prod) return 1.0f;
    const int k = exclusive ? j : j + 1;
    return k < S ? x_[k] : 0.0f;
  };
  float A = 1.0f, B = 0.f;
  for (int i = i1 - 1; i >= i0; --i) {
    const float a = a_of(i);
    B = g_[i] + a * B;
    A = a * A;
  }
  float s = wave_excl_scan_affine_rev(A, B);
  for (int i = i1 - 1; i >= i0; --i) {
    const float h = g_[i] + a_of(i) * s;
    o_[i] = exclusive ? s : h;
    s = h;
  }
  if (prod) {
    float lp = 1.0f;
    for (int i = i0; i < i1; ++i) lp *= x_[i];
    float run = wave_excl_scan_prod(lp);
    for (int i = i0; i < i1; ++i) {
      o_[i] = run * o_[i];  // (this lane's own store above)
      run = run * x_[i];
    }
  }
}

// from_alpha = 0: composite_ray's walk (trans_walk, ray_dev.hpp) - dt = t1 - t0, alpha = 1 - exp(-sigma dt),
// T = exp(-exclusive sum sigma dt); from_alpha = 1: T = exclusive product of (1 - alpha).  T is multiplied by prefix[i]
// when given; w = T alpha.  Any output may be NULL.
__global__ void k_packed_weights_fwd(const float* __restrict__ v, const float* __restrict__ t0, const float* __restrict__ t1,
                                     SpanArgs sp, int64_t R, int from_alpha, const float* __restrict__ prefix,
                                     float* __restrict__ weights, float* __restrict__ trans, float* __restrict__ alphas) {
  RayWork w;
  if (!ray_work(sp, R, w)) return;
  const int64_t beg = w.beg;
  const int i0 = w.i0, i1 = w.i1;
  const float* v_ = v + beg;
  const float* p_ = prefix ? prefix + beg : nullptr;
  float* w_ = weights ? weights + beg : nullptr;
  float* tr_ = trans ? trans + beg : nullptr;
  float* al_ = alphas ? alphas + beg : nullptr;
  if (!from_alpha) {
    const float* a_ = t0 + beg;
    const float* e_ = t1 + beg;
    trans_walk(i0, i1, [&](int i) { return v_[i] * (e_[i] - a_[i]); }, [&](int i, float T, float e) {
      const float alpha = 1.0f - e;
      if (p_) T = T * p_[i];
      const float wt = T * alpha;
      if (w_) w_[i] = wt;
      if (al_) al_[i] = alpha;
      if (tr_) tr_[i] = T;
    });
  } else {
    float lp = 1.0f;
    for (int i = i0; i < i1; ++i) lp *= 1.0f - v_[i];
    float run = wave_excl_scan_prod(lp);
    for (int i = i0; i < i1; ++i) {
      const float alpha = v_[i];
      float T = run;
      if (p_) T = T * p_[i];
      const float wt = T * alpha;
      run = run * (1.0f - alpha);
      if (w_) w_[i] = wt;
      if (al_) al_[i] = alpha;
      if (tr_) tr_[i] = T;
    }
  }
}

// Cotangents u (weights), tau (trans), a (alphas), each nullable (a kernel argument: the NULL branch is wave-uniform);
// p = prefix_trans (1 when absent), T the ray's own transmittance, so that trans = T p and w = T p alpha.
// Density form: density_bwd_ray (ray_dev.hpp), the compositor backward's routine, with q_i = u_i:
//   A_i = u_i T_i p_i + a_i,  B_i T_i = (u_i alpha_i + tau_i) p_i T_i,  d_sigma_i = dt_i (A_i e_i - sum_{j>i} B_j T_j)
// Alpha form, x = 1 - alpha, P_k = prod_{j<k} x_j, g_i = (u_i alpha_i + tau_i) p_i = dL/dP_i:
//   d_alpha_k = u_k P_k p_k + a_k - P_k S_k,   S_k = g_{k+1} + x_{k+1} S_{k+1}   (the exclusive product's backward)
__global__ void k_packed_weights_bwd(const float* __restrict__ v, const float* __restrict__ t0, const float* __restrict__ t1,
                                     SpanArgs sp, int64_t R, int from_alpha, const float* __restrict__ prefix,
                                     const float* __restrict__ d_w, const float* __restrict__ d_tr,
                                     const float* __restrict__ d_a, float* __restrict__ d_v) {
  RayWork w;
  if (!ray_work(sp, R, w)) return;
  const int64_t beg = w.beg;
  const int i0 = w.i0, i1 = w.i1;
  const float* v_ = v + beg;
  const float* p_ = prefix ? prefix + beg : nullptr;
  const float* u_ = d_w ? d_w + beg : nullptr;
  const float* tau_ = d_tr ? d_tr + beg : nullptr;
  const float* da_ = d_a ? d_a + beg : nullptr;
  float* o_ = d_v + beg;
  if (!from_alpha) {
    density_bwd_ray(v_, t0 + beg, t1 + beg, i0, i1, u_ != nullptr, [&](int i) { return u_[i]; }, tau_, da_, p_, o_,
                    [](int, float) {});
  } else {
    auto g_of = [&](int i) {
      float g = 0.f;
      if (u_) g += u_[i] * v_[i];
      if (tau_) g += tau_[i];
      if (p_) g = g * p_[i];
      return g;
    };
    float A = 1.0f, B = 0.f, lp = 1.0f;
    for (int i = i1 - 1; i >= i0; --i) {
      const float xi = 1.0f - v_[i];
      B = g_of(i) + xi * B;
      A = xi * A;
    }
    for (int i = i0; i < i1; ++i) lp *= 1.0f - v_[i];
    float s = wave_excl_scan_affine_rev(A, B);
    for (int i = i1 - 1; i >= i0; --i) {
      o_[i] = s;  // S_i
      s = g_of(i) + (1.0f - v_[i]) * s;
    }
    float run = wave_excl_scan_prod(lp);
    for (int i = i0; i < i1; ++i) {
      float d = 0.f;
      if (u_) d += u_[i] * (p_ ? run * p_[i] : run);
      if (da_) d += da_[i];
      o_[i] = d - run * o_[i];  // (this lane's own store above)
      run = run * (1.0f - v_[i]);
    }
  }
}

// keep[i] = T_i >= eps && alpha_i >= alpha_thre, both entry points.  from_alpha = 0: v = sigmas, T and alpha by the
// compositor's walk; from_alpha = 1: v = alphas, T = exclusive product of 1 - alpha.
__global__ void k_packed_visibility(const float* __restrict__ v, const float* __restrict__ t0, const float* __restrict__ t1,
                                    SpanArgs sp, int64_t R, int from_alpha, float eps, float alpha_thre,
                                    uint8_t* __restrict__ keep) {
  RayWork w;
  if (!ray_work(sp, R, w)) return;
  const int64_t beg = w.beg;
  const int i0 = w.i0, i1 = w.i1;
  const float* v_ = v + beg;
  uint8_t* k_ = keep + beg;
  if (!from_alpha) {
    const float* a_ = t0 + beg;
    const float* e_ = t1 + beg;
    trans_walk(i0, i1, [&](int i) { return v_[i] * (e_[i] - a_[i]); },
               [&](int i, float T, float e) { k_[i] = (T >= eps && 1.0f - e >= alpha_thre) ? 1 : 0; });
  } else {
    float lp = 1.0f;
    for (int i = i0; i < i1; ++i) lp *= 1.0f - v_[i];
    float run = wave_excl_scan_prod(lp);
    for (int i = i0; i < i1; ++i) {
      const float alpha = v_[i];
      k_[i] = (run >= eps && alpha >= alpha_thre) ? 1 : 0;
      run = run * (1.0f - alpha);
    }
  }
}

// out[r, c] = sum_i w_i v_ic (values NULL: sum_i w_i, C = 1).  Four channels at a time: each lane sums its own samples,
// the lanes' sums are added by the wave's butterfly.  A ray without samples gives 0.
__global__ void k_accumulate_fwd(const float* __restrict__ w, const float* __restrict__ vals, int C, SpanArgs sp,
                                 int64_t R, float* __restrict__ out) {
  RayWork rw;
  const bool work = ray_work(sp, R, rw);
  const int64_t r = rw.r, beg = rw.beg;
  const int lane = rw.lane, i0 = rw.i0, i1 = rw.i1;
  if (r >= R) return;
  if (!work) {
    for (int c = lane; c < C; c += 64) out[r * C + c] = 0.f;
    return;
  }
  const float* w_ = w + beg;
  const float* v_ = vals ? vals + beg * C : nullptr;
  for (int c0 = 0; c0 < C; c0 += 4) {
    const int nc = min(4, C - c0);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = i0; i < i1; ++i) {
      const float wi = w_[i];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < nc) acc[k] += v_ ? wi * v_[(int64_t)i * C + c0 + k] : wi;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float t = wave_sum(acc[k]);
      if (lane == 0 && k < nc) out[r * C + c0 + k] = t;
    }
  }
}

// d_w[i] = sum_c g[r,c] v_ic (values NULL: g[r]),  d_v[i,c] = w_i g[r,c]: elementwise, the lanes stride over the ray
__global__ void k_accumulate_bwd(const float* __restrict__ g, const float* __restrict__ w, const float* __restrict__ vals,
                                 int C, SpanArgs sp, int64_t R, float* __restrict__ d_w, float* __restrict__ d_v) {
  RayWork rw;
  if (!ray_work(sp, R, rw)) return;
  const int64_t beg = rw.beg;
  const int S = rw.S, lane = rw.lane;
  const float* g_ = g + rw.r * C;
  if (d_w) {
    for (int i = lane; i < S; i += 64) {
      float acc = 0.f;
      if (vals) {
        const float* v_ = vals + (beg + i) * C;
        for (int c = 0; c < C; ++c) acc += g_[c] * v_[c];
      } else {
        acc = g_[0];
      }
      d_w[beg + i] = acc;
    }
  }
  if (d_v) {
    const int64_t n = (int64_t)S * C;
    for (int64_t k = lane; k < n; k += 64) d_v[beg * C + k] = w[beg + k / C] * g_[k % C];
  }
}

}  // namespace fsn

using namespace fsn;

// the shared checks of an entry point over (ray_indices, packed_info, N, R, dense_S): ray_launch (ray_dev.hpp)
#define FSN_SPAN_CHECK(who) \
  RayLaunch L;              \
  if (int rc_ = ray_launch(who, ray_indices, packed_info, N, R, dense_S, false, &L)) return rc_

extern "C" int fsn_pack_info(const int64_t* ray_indices, int64_t N, int64_t R, int64_t* packed_info, fsn_stream_t stream) {
  FSN_REQUIRE(N >= 0 && R >= 0, FSN_E_INVALID, "fsn_pack_info: bad sizes");
  if (R == 0) return FSN_OK;
  if (N == 0) {  // every ray is empty: start 0, count 0
    if (packed_info) FSN_HIP(hipMemsetAsync(packed_info, 0, (size_t)R * 2 * sizeof(int64_t), as_stream(stream)));
    return FSN_OK;
  }
  FSN_REQUIRE(ray_indices && packed_info, FSN_E_INVALID, "fsn_pack_info: null pointer");
  FSN_REQUIRE((R + 255) / 256 <= 0x7fffffff, FSN_E_INVALID, "fsn_pack_info: bad sizes (too many rays)");
  k_pack_info<<<(unsigned)((R + 255) / 256), 256, 0, as_stream(stream)>>>(ray_indices, N, R, packed_info);
  FSN_LAUNCH_CHECK("k_pack_info");
  return FSN_OK;
}

extern "C" int fsn_packed_scan_fwd(const float* x, const int64_t* ray_indices, const int64_t* packed_info, int64_t N,
                                   int64_t R, int dense_S, int op, int exclusive, float* out, fsn_stream_t stream) {
  FSN_REQUIRE(op == FSN_SCAN_SUM || op == FSN_SCAN_PROD, FSN_E_INVALID, "fsn_packed_scan_fwd: op %d is neither sum nor prod", op);
  FSN_SPAN_CHECK("fsn_packed_scan_fwd");
  if (!L.launch) return FSN_OK;
  FSN_REQUIRE(x && out, FSN_E_INVALID, "fsn_packed_scan_fwd: null pointer");
  k_packed_scan_fwd<<<L.grid, 256, 0, as_stream(stream)>>>(x, L.sp, R, op == FSN_SCAN_PROD, exclusive != 0, out);
  FSN_LAUNCH_CHECK("k_packed_scan_fwd");
  return FSN_OK;
}

extern "C" int fsn_packed_scan_bwd(const float* x, const float* d_out, const int64_t* ray_indices,
                                   const int64_t* packed_info, int64_t N, int64_t R, int dense_S, int op, int exclusive,
                                   float* d_x, fsn_stream_t stream) {
  FSN_REQUIRE(op == FSN_SCAN_SUM || op == FSN_SCAN_PROD, FSN_E_INVALID, "fsn_packed_scan_bwd: op %d is neither sum nor prod", op);
  FSN_SPAN_CHECK("fsn_packed_scan_bwd");
  if (!L.launch) return FSN_OK;
  FSN_REQUIRE((x || op == FSN_SCAN_SUM) && d_out && d_x, FSN_E_INVALID, "fsn_packed_scan_bwd: null pointer");
  // a ray_indices / packed_info table need not cover every sample: what no ray owns gets 0
  FSN_HIP(hipMemsetAsync(d_x, 0, (size_t)N * sizeof(float), as_stream(stream)));
  k_packed_scan_bwd<<<L.grid, 256, 0, as_stream(stream)>>>(x, d_out, L.sp, R, op == FSN_SCAN_PROD, exclusive != 0, d_x);
  FSN_LAUNCH_CHECK("k_packed_scan_bwd");
  return FSN_OK;
}

extern "C" int fsn_packed_weights_fwd(const float* v, const float* t_starts, const float* t_ends,
                                      const int64_t* ray_indices, const int64_t* packed_info, int64_t N, int64_t R,
                                      int dense_S, int from_alpha, const float* prefix_trans, float* weights, float* trans,
                                      float* alphas, fsn_stream_t stream) {
  FSN_SPAN_CHECK("fsn_packed_weights_fwd");
  if (!L.launch) return FSN_OK;
  FSN_REQUIRE(v && (from_alpha || (t_starts && t_ends)), FSN_E_INVALID, "fsn_packed_weights_fwd: null pointer");
  k_packed_weights_fwd<<<L.grid, 256, 0, as_stream(stream)>>>(v, t_starts, t_ends, L.sp, R, from_alpha != 0, prefix_trans,
                                                           weights, trans, alphas);
  FSN_LAUNCH_CHECK("k_packed_weights_fwd");
  return FSN_OK;
}

extern "C" int fsn_packed_weights_bwd(const float* v, const float* t_starts, const float* t_ends,
                                      const int64_t* ray_indices, const int64_t* packed_info, int64_t N, int64_t R,
                                      int dense_S, int from_alpha, const float* prefix_trans, const float* d_weights,
                                      const float* d_trans, const float* d_alphas, float* d_v, fsn_stream_t stream) {
  FSN_SPAN_CHECK("fsn_packed_weights_bwd");
  if (!L.launch) return FSN_OK;
  FSN_REQUIRE(v && d_v && (from_alpha || (t_starts && t_ends)), FSN_E_INVALID, "fsn_packed_weights_bwd: null pointer");
  FSN_HIP(hipMemsetAsync(d_v, 0, (size_t)N * sizeof(float), as_stream(stream)));
  k_packed_weights_bwd<<<L.grid, 256, 0, as_stream(stream)>>>(v, t_starts, t_ends, L.sp, R, from_alpha != 0, prefix_trans,
                                                           d_weights, d_trans, d_alphas, d_v);
  FSN_LAUNCH_CHECK("k_packed_weights_bwd");
  return FSN_OK;
}

// (no memset here: ray_indices covers every sample, and the caller's keep array stays as it is past them)
extern "C" int fsn_packed_visibility(const float* sigmas, const float* t_starts, const float* t_ends,
                                     const int64_t* ray_indices, int64_t N, int64_t R, float early_stop_eps,
                                     float alpha_thre, uint8_t* keep, fsn_stream_t stream) {
  RayLaunch L;
  if (int rc = ray_launch("fsn_packed_visibility", ray_indices, nullptr, N, R, 0, false, &L)) return rc;
  if (!L.launch) return FSN_OK;
  FSN_REQUIRE(sigmas && t_starts && t_ends && keep, FSN_E_INVALID, "fsn_packed_visibility: null pointer");
  k_packed_visibility<<<L.grid, 256, 0, as_stream(stream)>>>(sigmas, t_starts, t_ends, L.sp, R, 0, early_stop_eps,
                                                            alpha_thre, keep);
  FSN_LAUNCH_CHECK("k_packed_visibility");
  return FSN_OK;
}

extern "C" int fsn_packed_visibility_alpha(const float* alphas, const int64_t* ray_indices, const int64_t* packed_info,
                                           int64_t N, int64_t R, int dense_S, float early_stop_eps, float alpha_thre,
                                           uint8_t* keep, fsn_stream_t stream) {
  FSN_SPAN_CHECK("fsn_packed_visibility_alpha");
  if (!L.launch) return FSN_OK;
  FSN_REQUIRE(alphas && keep, FSN_E_INVALID, "fsn_packed_visibility_alpha: null pointer");
  FSN_HIP(hipMemsetAsync(keep, 0, (size_t)N, as_stream(stream)));
  k_packed_visibility<<<L.grid, 256, 0, as_stream(stream)>>>(alphas, nullptr, nullptr, L.sp, R, 1, early_stop_eps,
                                                            alpha_thre, keep);
  FSN_LAUNCH_CHECK("k_packed_visibility");
  return FSN_OK;
}

extern "C" int fsn_accumulate_fwd(const float* weights, const float* values, int C, const int64_t* ray_indices,
                                  const int64_t* packed_info, int64_t N, int64_t R, int dense_S, float* out,
                                  fsn_stream_t stream) {
  FSN_REQUIRE(C >= 1, FSN_E_INVALID, "fsn_accumulate_fwd: bad sizes (C >= 1)");
  FSN_SPAN_CHECK("fsn_accumulate_fwd");
  if (!L.launch) {
    if (N == 0 && R > 0 && out)  // every ray is empty
      FSN_HIP(hipMemsetAsync(out, 0, (size_t)R * C * sizeof(float), as_stream(stream)));
    return FSN_OK;
  }
  FSN_REQUIRE(weights && out, FSN_E_INVALID, "fsn_accumulate_fwd: null pointer");
  FSN_REQUIRE(values || C == 1, FSN_E_INVALID, "fsn_accumulate_fwd: bad sizes (C must be 1 without values)");
  k_accumulate_fwd<<<L.grid, 256, 0, as_stream(stream)>>>(weights, values, C, L.sp, R, out);
  FSN_LAUNCH_CHECK("k_accumulate_fwd");
  return FSN_OK;
}

extern "C" int fsn_accumulate_bwd(const float* d_out, const float* weights, const float* values, int C,
                                  const int64_t* ray_indices, const int64_t* packed_info, int64_t N, int64_t R,
                                  int dense_S, float* d_weights, float* d_values, fsn_stream_t stream) {
  FSN_REQUIRE(C >= 1, FSN_E_INVALID, "fsn_accumulate_bwd: bad sizes (C >= 1)");
  FSN_SPAN_CHECK("fsn_accumulate_bwd");
  if (!L.launch) return FSN_OK;
  FSN_REQUIRE(d_out && (d_weights || d_values) && (!d_values || (weights && values)), FSN_E_INVALID,
              "fsn_accumulate_bwd: null pointer");
  FSN_REQUIRE(values || C == 1, FSN_E_INVALID, "fsn_accumulate_bwd: bad sizes (C must be 1 without values)");
  if (d_weights) FSN_HIP(hipMemsetAsync(d_weights, 0, (size_t)N * sizeof(float), as_stream(stream)));
  if (d_values) FSN_HIP(hipMemsetAsync(d_values, 0, (size_t)N * C * sizeof(float), as_stream(stream)));
  k_accumulate_bwd<<<L.grid, 256, 0, as_stream(stream)>>>(d_out, weights, values, C, L.sp, R, d_weights, d_values);
  FSN_LAUNCH_CHECK("k_accumulate_bwd");
  return FSN_OK;
}
