// propnet.hip — the proposal-network sampler behind render/pdf.py and render/propnet.py: inverse-CDF importance sampling
// of n intervals from a per-ray histogram (with the s -> t transform), the same fused behind the transmittance walk
// (the no-grad step between two proposal evaluations), the dense searchsorted, and the interlevel proposal loss with its
// backward.  Dense rows only: every tensor is [R, .].  One wavefront per ray, four rays per 256-thread block (ray_work /
// ray_launch with dense_S, ray_dev.hpp); no atomics, every sum in a fixed order, float32, -ffp-contract=off.
// The two sampler kernels stage the ray's edges and cdf in LDS (the fused one PRODUCES its cdf, and a lane's edges are
// midpoints of its neighbours' centres, which go through LDS as well); the search and loss kernels only read their rows
// and search them in global memory, as packed_scan.hip does.  DESIGN.md, "Proposal-network estimator".
#include "common.hpp"
#include "ray_dev.hpp"

namespace fsn {

// number of entries of the sorted a[0..n) that are <= q  (searchsorted(a, q, right=True))
__device__ __forceinline__ int count_le(const float* a, int n, float q) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] <= q) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// first index of the sorted a[0..n) that is >= key
__device__ __forceinline__ int first_ge(const float* a, int n, float key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// _transform_stot: s in [0, 1] -> t in [near, far]
__device__ __forceinline__ float stot(int transform, float s, float near, float far) {
  if (transform == FSN_STOT_UNIFORM) return s * far + (1.0f - s) * near;
  return 1.0f / (s * (1.0f / far) + (1.0f - s) * (1.0f / near));
}

// importance_sampling for ONE ray by ONE wave.  v_s / c_s: the ray's edges and cdf [S+1] in LDS; x_s: n floats of LDS
// for the centres.  Centre i: u = (i + b) / n, k = clamp(#{c <= u} - 1, 0, S-1), x = v[k] + frac (v[k+1] - v[k]) with
// frac = clamp((u - c[k]) / (c[k+1] - c[k]), 0, 1) (0 on a flat stretch).  Edge j: the midpoint of centres j-1 and j;
// the two ends mirror the first / last centre about its inner edge and stay inside [v[0], v[S]] (the second clamp of
// each end never acts on a monotone cdf: it is there for input outside the contract).  n == 1: (v[0], v[S]).
__device__ __forceinline__ void importance_ray(const float* v_s, const float* c_s, int S, int n, float b, int transform,
                                               float near, float far, float* x_s, float* __restrict__ s_out,
                                               float* __restrict__ x_out, float* __restrict__ t_out, int lane) {
  const float fn = (float)n;
  for (int i = lane; i < n; i += 64) {
    const float u = ((float)i + b) / fn;
    const int k = min(max(count_le(c_s, S + 1, u) - 1, 0), S - 1);
    const float c0 = c_s[k];
    const float den = c_s[k + 1] - c0;
    float frac = 0.f;
    if (den > 0.f) frac = fminf(fmaxf((u - c0) / den, 0.f), 1.0f);
    const float v0 = v_s[k];
    const float x = v0 + frac * (v_s[k + 1] - v0);
    x_s[i] = x;
    if (x_out) x_out[i] = x;
  }
  __builtin_amdgcn_wave_barrier();
  const float lo = v_s[0], hi = v_s[S];
  for (int j = lane; j <= n; j += 64) {
    float e;
    if (n == 1) {
      e = j == 0 ? lo : hi;
    } else if (j == 0) {
      const float e1 = (x_s[0] + x_s[1]) * 0.5f;
      e = fminf(fmaxf(2.0f * x_s[0] - e1, lo), hi);
    } else if (j == n) {
      const float em = (x_s[n - 2] + x_s[n - 1]) * 0.5f;
      e = fmaxf(fminf(2.0f * x_s[n - 1] - em, hi), lo);
    } else {
      e = (x_s[j - 1] + x_s[j]) * 0.5f;
    }
    s_out[j] = e;
    if (t_out) t_out[j] = stot(transform, e, near, far);
  }
}

// this wave's LDS: edges [S+1], cdf [S+1], centres [n]
struct PropLds {
  float *v, *c, *x;
};
__device__ __forceinline__ PropLds prop_lds(float* lds, int S, int n) {
  float* base = lds + (size_t)(threadIdx.x >> 6) * (2 * (S + 1) + n);
  return {base, base + (S + 1), base + 2 * (S + 1)};
}

struct PropOut {
  float* s_edges;  // [R, n+1]
  float* centres;  // [R, n] or null
  float* t_edges;  // [R, n+1] or null
};

// sp: dense rows of S (the intervals in)
__global__ void k_importance_sample(const float* __restrict__ vals, const float* __restrict__ cdfs, SpanArgs sp, int64_t R,
                                    int n, const float* __restrict__ b, int transform, float near, float far, PropOut o) {
  extern __shared__ float prop_smem[];
  RayWork w;
  if (!ray_work(sp, R, w)) return;
  const int S = w.S, lane = w.lane;
  const PropLds l = prop_lds(prop_smem, S, n);
  const float* v_ = vals + w.r * (S + 1);
  const float* c_ = cdfs + w.r * (S + 1);
  for (int i = lane; i <= S; i += 64) {
    l.v[i] = v_[i];
    l.c[i] = c_[i];
  }
  __builtin_amdgcn_wave_barrier();
  importance_ray(l.v, l.c, S, n, b ? b[w.r] : 0.5f, transform, near, far, l.x, o.s_edges + w.r * (n + 1),
                 o.centres ? o.centres + w.r * n : nullptr, o.t_edges ? o.t_edges + w.r * (n + 1) : nullptr, lane);
}

// cdfs = 1 - cat(trans, 0) of the proposal's densities on its own intervals (trans_walk: the values of
// fsn_packed_weights_fwd on t_starts = t_edges[:-1], t_ends = t_edges[1:], bit for bit), then importance_ray on them.
__global__ void k_prop_resample(const float* __restrict__ s_edges, const float* __restrict__ t_edges,
                                const float* __restrict__ sigmas, SpanArgs sp, int64_t R, int n, const float* __restrict__ b,
                                int transform, float near, float far, float* __restrict__ cdfs_out, PropOut o) {
  extern __shared__ float prop_smem[];
  RayWork w;
  if (!ray_work(sp, R, w)) return;
  const int S = w.S, lane = w.lane;
  const PropLds l = prop_lds(prop_smem, S, n);
  const float* se = s_edges + w.r * (S + 1);
  const float* te = t_edges + w.r * (S + 1);
  const float* sg = sigmas + w.beg;
  float* cd = cdfs_out + w.r * (S + 1);
  for (int i = lane; i <= S; i += 64) l.v[i] = se[i];
  trans_walk(w.i0, w.i1, [&](int i) { return sg[i] * (te[i + 1] - te[i]); }, [&](int i, float T, float) {
    const float c = 1.0f - T;
    l.c[i] = c;
    cd[i] = c;
  });
  if (lane == 0) {
    l.c[S] = 1.0f;
    cd[S] = 1.0f;
  }
  __builtin_amdgcn_wave_barrier();
  importance_ray(l.v, l.c, S, n, b ? b[w.r] : 0.5f, transform, near, far, l.x, o.s_edges + w.r * (n + 1),
                 o.centres ? o.centres + w.r * n : nullptr, o.t_edges ? o.t_edges + w.r * (n + 1) : nullptr, lane);
}

// sp: dense rows of Q (the queries); keys [R, K].  h = #{key <= q}: ids_left = max(h-1, 0), ids_right = min(h, K-1)
__global__ void k_searchsorted_dense(const float* __restrict__ keys, const float* __restrict__ q, SpanArgs sp, int64_t R,
                                     int K, int64_t* __restrict__ ids_left, int64_t* __restrict__ ids_right) {
  RayWork w;
  if (!ray_work(sp, R, w)) return;
  const float* k_ = keys + w.r * K;
  for (int i = w.lane; i < w.S; i += 64) {
    const int h = count_le(k_, K, q[w.beg + i]);
    ids_left[w.beg + i] = max(h - 1, 0);
    ids_right[w.beg + i] = min(h, K - 1);
  }
}

// Interval i of the interlevel loss: w = cq[i+1] - cq[i], wo = ck[ids_right(q[i+1])] - ck[ids_left(q[i])] over the key
// edges k[0..S]; -> max(w - wo, 0), or 0 where w <= 0.  w_eps = w + 1e-7.
__device__ __forceinline__ float prop_excess(const float* __restrict__ q, const float* __restrict__ cq,
                                             const float* __restrict__ k, const float* __restrict__ ck, int S, int i,
                                             float& w_eps) {
  const float w = cq[i + 1] - cq[i];
  w_eps = w + 1e-7f;
  if (!(w > 0.f)) return 0.f;
  const int hr = count_le(k, S + 1, q[i + 1]), hl = count_le(k, S + 1, q[i]);
  const float wo = ck[min(hr, S)] - ck[max(hl - 1, 0)];
  return fmaxf(w - wo, 0.f);
}

// sp: dense rows of n (the query intervals)
__global__ void k_prop_loss_fwd(const float* __restrict__ q, const float* __restrict__ cq, const float* __restrict__ k,
                                const float* __restrict__ ck, SpanArgs sp, int64_t R, int S, float* __restrict__ loss) {
  RayWork w;
  if (!ray_work(sp, R, w)) return;
  const int n = w.S;
  const float* q_ = q + w.r * (n + 1);
  const float* cq_ = cq + w.r * (n + 1);
  const float* k_ = k + w.r * (S + 1);
  const float* ck_ = ck + w.r * (S + 1);
  for (int i = w.lane; i < n; i += 64) {
    float w_eps;
    const float d = prop_excess(q_, cq_, k_, ck_, S, i, w_eps);
    loss[w.beg + i] = d * d / w_eps;
  }
}

// d_ck[m] = sum_{i: ids_right(q[i+1]) = m} coef_i - sum_{i: ids_left(q[i]) = m} coef_i,  coef_i = -2 max(w - wo, 0) /
// (w + 1e-7) g_i.  Pass 1 puts the ray's coef in LDS (n floats per wave); pass 2: key entry m per lane.  With h(x) =
// #{k <= x}: ids_right(x) >= m <=> m == 0 or k[m-1] <= x, and ids_left(x) >= m <=> m == 0 or k[m] <= x, so each index
// set is one run of the sorted queries, found by two searches over q; the run is summed in ascending i.
__global__ void k_prop_loss_bwd(const float* __restrict__ q, const float* __restrict__ cq, const float* __restrict__ k,
                                const float* __restrict__ ck, const float* __restrict__ g, SpanArgs sp, int64_t R, int S,
                                float* __restrict__ d_ck) {
  extern __shared__ float prop_smem[];
  RayWork w;
  if (!ray_work(sp, R, w)) return;
  const int n = w.S, lane = w.lane;
  float* coef = prop_smem + (size_t)(threadIdx.x >> 6) * n;
  const float* q_ = q + w.r * (n + 1);
  const float* cq_ = cq + w.r * (n + 1);
  const float* k_ = k + w.r * (S + 1);
  const float* ck_ = ck + w.r * (S + 1);
  for (int i = lane; i < n; i += 64) {
    float w_eps;
    const float d = prop_excess(q_, cq_, k_, ck_, S, i, w_eps);
    coef[i] = -2.0f * d / w_eps * g[w.beg + i];
  }
  __builtin_amdgcn_wave_barrier();
  float* o_ = d_ck + w.r * (S + 1);
  for (int m = lane; m <= S; m += 64) {
    const int a0 = m == 0 ? 0 : first_ge(q_ + 1, n, k_[m - 1]);
    const int a1 = m == S ? n : first_ge(q_ + 1, n, k_[m]);
    const int b0 = m == 0 ? 0 : first_ge(q_, n, k_[m]);
    const int b1 = m == S ? n : first_ge(q_, n, k_[m + 1]);
    float sa = 0.f, sb = 0.f;
    for (int i = a0; i < a1; ++i) sa += coef[i];
    for (int i = b0; i < b1; ++i) sb += coef[i];
    o_[m] = sa - sb;
  }
}

}  // namespace fsn

using namespace fsn;

// the checks the sampler entry points share, in front of the launch -> rc, L
static int prop_sampler_check(const char* who, int64_t R, int S, int n, int transform, float near, float far, RayLaunch* L) {
  FSN_REQUIRE(R >= 0 && S >= 1 && n >= 1, FSN_E_INVALID, "%s: bad sizes (R >= 0, S >= 1, n >= 1)", who);
  FSN_REQUIRE(S <= FSN_PROP_MAX_ROW && n <= FSN_PROP_MAX_ROW, FSN_E_UNSUPPORTED,
              "%s: rows of %d intervals in and %d out: the kernel holds at most %d each", who, S, n, FSN_PROP_MAX_ROW);
  FSN_REQUIRE(transform == FSN_STOT_NONE || transform == FSN_STOT_UNIFORM || transform == FSN_STOT_LINDISP, FSN_E_INVALID,
              "%s: transform %d is none of FSN_STOT_NONE / _UNIFORM / _LINDISP", who, transform);
  FSN_REQUIRE(transform != FSN_STOT_LINDISP || (near > 0.f && far > 0.f), FSN_E_INVALID,
              "%s: lindisp needs near > 0 and far > 0", who);
  return ray_launch(who, nullptr, nullptr, R * S, R, S, false, L);
}

static inline size_t prop_lds_bytes(int S, int n) { return (size_t)4 * (2 * (S + 1) + n) * sizeof(float); }

extern "C" int fsn_importance_sample(const float* vals, const float* cdfs, int64_t R, int S, int n, const float* b,
                                     int transform, float near, float far, float* s_edges, float* centres, float* t_edges,
                                     fsn_stream_t stream) {
  RayLaunch L;
  if (int rc = prop_sampler_check("fsn_importance_sample", R, S, n, transform, near, far, &L)) return rc;
  if (!L.launch) return FSN_OK;
  FSN_REQUIRE(vals && cdfs && s_edges && (transform == FSN_STOT_NONE || t_edges), FSN_E_INVALID,
              "fsn_importance_sample: null pointer");
  const PropOut o{s_edges, centres, transform == FSN_STOT_NONE ? nullptr : t_edges};
  k_importance_sample<<<L.grid, 256, prop_lds_bytes(S, n), as_stream(stream)>>>(vals, cdfs, L.sp, R, n, b, transform, near,
                                                                               far, o);
  FSN_LAUNCH_CHECK("k_importance_sample");
  return FSN_OK;
}

extern "C" int fsn_prop_resample(const float* s_edges, const float* t_edges, const float* sigmas, int64_t R, int S, int n,
                                 const float* b, int transform, float near, float far, float* cdfs, float* s_out,
                                 float* centres, float* t_out, fsn_stream_t stream) {
  RayLaunch L;
  if (int rc = prop_sampler_check("fsn_prop_resample", R, S, n, transform, near, far, &L)) return rc;
  if (!L.launch) return FSN_OK;
  FSN_REQUIRE(s_edges && t_edges && sigmas && cdfs && s_out && (transform == FSN_STOT_NONE || t_out), FSN_E_INVALID,
              "fsn_prop_resample: null pointer");
  const PropOut o{s_out, centres, transform == FSN_STOT_NONE ? nullptr : t_out};
  k_prop_resample<<<L.grid, 256, prop_lds_bytes(S, n), as_stream(stream)>>>(s_edges, t_edges, sigmas, L.sp, R, n, b,
                                                                           transform, near, far, cdfs, o);
  FSN_LAUNCH_CHECK("k_prop_resample");
  return FSN_OK;
}

extern "C" int fsn_searchsorted_dense(const float* keys, const float* values, int64_t R, int K, int Q, int64_t* ids_left,
                                      int64_t* ids_right, fsn_stream_t stream) {
  FSN_REQUIRE(R >= 0 && K >= 1 && Q >= 0, FSN_E_INVALID, "fsn_searchsorted_dense: bad sizes (R >= 0, K >= 1, Q >= 0)");
  RayLaunch L;
  if (int rc = ray_launch("fsn_searchsorted_dense", nullptr, nullptr, R * Q, R, Q, false, &L)) return rc;
  if (!L.launch) return FSN_OK;
  FSN_REQUIRE(keys && values && ids_left && ids_right, FSN_E_INVALID, "fsn_searchsorted_dense: null pointer");
  k_searchsorted_dense<<<L.grid, 256, 0, as_stream(stream)>>>(keys, values, L.sp, R, K, ids_left, ids_right);
  FSN_LAUNCH_CHECK("k_searchsorted_dense");
  return FSN_OK;
}

static int prop_loss_check(const char* who, int64_t R, int n, int S, RayLaunch* L) {
  FSN_REQUIRE(R >= 0 && S >= 1 && n >= 1, FSN_E_INVALID, "%s: bad sizes (R >= 0, S >= 1, n >= 1)", who);
  FSN_REQUIRE(S <= FSN_PROP_MAX_ROW && n <= FSN_PROP_MAX_ROW, FSN_E_UNSUPPORTED,
              "%s: rows of %d query and %d key intervals: the kernel holds at most %d each", who, n, S, FSN_PROP_MAX_ROW);
  return ray_launch(who, nullptr, nullptr, R * n, R, n, false, L);
}

extern "C" int fsn_prop_loss_fwd(const float* q_edges, const float* q_cdfs, const float* k_edges, const float* k_cdfs,
                                 int64_t R, int n, int S, float* loss, fsn_stream_t stream) {
  RayLaunch L;
  if (int rc = prop_loss_check("fsn_prop_loss_fwd", R, n, S, &L)) return rc;
  if (!L.launch) return FSN_OK;
  FSN_REQUIRE(q_edges && q_cdfs && k_edges && k_cdfs && loss, FSN_E_INVALID, "fsn_prop_loss_fwd: null pointer");
  k_prop_loss_fwd<<<L.grid, 256, 0, as_stream(stream)>>>(q_edges, q_cdfs, k_edges, k_cdfs, L.sp, R, S, loss);
  FSN_LAUNCH_CHECK("k_prop_loss_fwd");
  return FSN_OK;
}

extern "C" int fsn_prop_loss_bwd(const float* q_edges, const float* q_cdfs, const float* k_edges, const float* k_cdfs,
                                 const float* d_loss, int64_t R, int n, int S, float* d_k_cdfs, fsn_stream_t stream) {
  RayLaunch L;
  if (int rc = prop_loss_check("fsn_prop_loss_bwd", R, n, S, &L)) return rc;
  if (!L.launch) return FSN_OK;
  FSN_REQUIRE(q_edges && q_cdfs && k_edges && k_cdfs && d_loss && d_k_cdfs, FSN_E_INVALID, "fsn_prop_loss_bwd: null pointer");
  k_prop_loss_bwd<<<L.grid, 256, (size_t)4 * n * sizeof(float), as_stream(stream)>>>(q_edges, q_cdfs, k_edges, k_cdfs, d_loss,
                                                                                    L.sp, R, S, d_k_cdfs);
  FSN_LAUNCH_CHECK("k_prop_loss_bwd");
  return FSN_OK;
}
