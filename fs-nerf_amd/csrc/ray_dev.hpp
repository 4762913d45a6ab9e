// ray_dev.hpp — wave-level (64-lane) device routines for the per-ray parts of the path: the one-wave-per-ray
// skeleton (where a ray's samples are, which of them a lane owns, the host checks of such a launch), the transmittance
// walk that every density-form kernel is built on (trans_walk), volume integration and its density backward, and
// hierarchical resampling.  One wavefront owns one ray; used by the standalone kernels (ray_ops.hip, packed_scan.hip,
// composite_grad.hip, input_grad.hip) and by the fused render kernels.  Compiled with -ffp-contract=off so the float op
// sequence is the one written here (it mirrors oracle/fsnerf_oracle.py).
#pragma once
#include "common.hpp"

namespace fsn {

constexpr float kFltEps = 1.1920928955078125e-07f;

__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// exclusive prefix sum over the 64 lanes (Hillis-Steele on __shfl_up); total returned to all.
__device__ __forceinline__ float wave_excl_scan(float v, float& total) {
  const int lane = lane_id();
  float inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    float o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  total = __shfl(inc, 63, 64);
  return inc - v;
}

// exclusive prefix product over the 64 lanes (lane 0 gets 1); no division, so a zero factor stays exact
__device__ __forceinline__ float wave_excl_scan_prod(float v) {
  const int lane = lane_id();
  float inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    float o = __shfl_up(inc, d, 64);
    if (lane >= d) inc = o * inc;
  }
  const float before = __shfl_up(inc, 1, 64);
  return lane > 0 ? before : 1.0f;
}

// Lane l holds the affine map M_l(s) = a s + b.  Returns M_{l+1}(M_{l+2}(... M_63(0))) (lane 63: 0): the exclusive scan
// of the maps under composition, taken from the wave's END (Hillis-Steele on __shfl_down).  With a = 1 it is the
// exclusive suffix sum of b in a fixed order, without a "total - prefix" subtraction.
__device__ __forceinline__ float wave_excl_scan_affine_rev(float a, float b) {
  const int lane = lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float oa = __shfl_down(a, d, 64), ob = __shfl_down(b, d, 64);
    if (lane + d < 64) {
      b = a * ob + b;
      a = a * oa;
    }
  }
  const float after = __shfl_down(b, 1, 64);
  return lane < 63 ? after : 0.0f;
}

// first index of the sorted a[0..n) that is >= key
__device__ __forceinline__ int64_t ray_lower_bound(const int64_t* __restrict__ a, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// samples [beg, beg + S) of ray r in packed order (ri: the sorted ray index of each of the N samples)
struct RaySpan {
  int64_t beg;
  int S;
};
__device__ __forceinline__ RaySpan ray_span(const int64_t* __restrict__ ri, int64_t N, int64_t r) {
  // (both searches over all of [0, N): they share their first probes, which the second then finds in the cache.
  // profiles/r07_bench_composite_bwd.jsonl has both forms timed: tag branch-span-from-beg started the second at `beg`)
  const int64_t beg = ray_lower_bound(ri, N, r);
  return {beg, (int)(ray_lower_bound(ri, N, r + 1) - beg)};
}

// Where a ray's samples are: exactly one of sorted ray_indices [N] (searched by ray_span), packed_info [R,2] = (start,
// count) (read, and clamped into [0, N] so that a wrong table cannot send a wave out of the arrays), dense rows of
// dense_S samples.  (N == 0 with no table at all: every ray is empty, nothing is read.)
struct SpanArgs {
  const int64_t* ri;
  const int64_t* pi;
  int64_t N;
  int dense_S;
};

__device__ __forceinline__ RaySpan span_of(const SpanArgs& sp, int64_t r) {
  if (sp.dense_S > 0) return {r * sp.dense_S, sp.dense_S};
  if (sp.pi) {
    const int64_t beg = min(max(sp.pi[2 * r], (int64_t)0), sp.N);
    const int64_t cnt = min(max(sp.pi[2 * r + 1], (int64_t)0), min(sp.N - beg, (int64_t)0x7fffffff));
    return {beg, (int)cnt};
  }
  return ray_span(sp.ri, sp.N, r);
}

// lane l owns the contiguous samples [l per, (l+1) per) of a ray's S, per = ceil(S/64)
__device__ __forceinline__ void lane_range(int S, int lane, int& i0, int& i1) {
  const int per = (S + 63) >> 6;
  i0 = lane * per;  // (past the ray's end for the last lanes of a short ray: [i0, i1) is empty then)
  i1 = min(i0 + per, S);
}

// The per-ray skeleton of every one-wave-per-ray kernel (four rays per 256-thread block, grid = ceil(R/4)): this
// wave's ray r, its samples [beg, beg + S) and this lane's share [i0, i1) of them (relative to beg).  ray_work()
// returns whether the ray has samples; r >= R tells a wave past the last ray from an empty one (S == 0).  Kernels
// that stride the lanes over the ray (i = lane; i < S; i += 64) take r, beg, S and lane from it.  `first`: the grid
// covers the rays [first, R) only (a row subset: ray_hist.hip); every other kernel starts at ray 0.
struct RayWork {
  int64_t r, beg;
  int S, lane, i0, i1;
};
__device__ __forceinline__ bool ray_work(const SpanArgs& sp, int64_t R, RayWork& w, int64_t first = 0) {
  w.lane = lane_id();
  w.r = first + (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (the wave's: scalar)
  w.beg = 0;
  w.S = 0;
  if (w.r < R) {
    const RaySpan span = span_of(sp, w.r);
    w.beg = span.beg;
    w.S = max(span.S, 0);
  }
  lane_range(w.S, w.lane, w.i0, w.i1);
  return w.S > 0;
}

// The host side of such a launch: the checks every one-wave-per-ray entry point shares.  -> FSN_OK with launch = 0
// when there is nothing to launch: R == 0, or N == 0 unless the kernel still has something to write for rays without
// samples (launch_empty: the compositor's background, the regulariser's NaN marks).
struct RayLaunch {
  SpanArgs sp;
  unsigned grid;
  int launch;
};
static inline int ray_launch(const char* who, const int64_t* ri, const int64_t* pi, int64_t N, int64_t R, int dense_S,
                             bool launch_empty, RayLaunch* L) {
  *L = RayLaunch{SpanArgs{ri, pi, N, dense_S}, (unsigned)((R + 3) / 4), 0};
  FSN_REQUIRE(N >= 0 && R >= 0 && dense_S >= 0, FSN_E_INVALID, "%s: bad sizes", who);
  const int modes = (ri ? 1 : 0) + (pi ? 1 : 0) + (dense_S > 0 ? 1 : 0);
  FSN_REQUIRE(modes <= 1, FSN_E_INVALID, "%s: more than one of ray_indices, packed_info and dense_S given", who);
  if (R == 0 || (N == 0 && !launch_empty)) return FSN_OK;
  FSN_REQUIRE((R + 3) / 4 <= 0x7fffffff, FSN_E_INVALID, "%s: bad sizes (too many rays)", who);
  if (N > 0) {
    FSN_REQUIRE(modes == 1, FSN_E_INVALID, "%s: null pointer (one of ray_indices, packed_info and dense_S is needed)", who);
    FSN_REQUIRE(dense_S == 0 || (R <= N && N / R == dense_S && N % R == 0), FSN_E_INVALID,
                "%s: bad sizes (dense rows need N == R * dense_S)", who);
  } else {
    L->sp = SpanArgs{nullptr, nullptr, 0, 0};  // every ray is empty: no table is read
  }
  L->launch = 1;
  return FSN_OK;
}

// The transmittance walk.  sdt_of(i) = sigma_i dt_i of the lane's samples [i0, i1): sdt_before() sums them and returns
// the sum over the lanes before this one (wave_excl_scan); trans_walk() hands body(i, T_i, e_i) every sample in order,
// T_i = exp(-sum_{j<i} sigma_j dt_j), e_i = exp(-sigma_i dt_i) - so alpha_i = 1.0f - e_i and w_i = T_i alpha_i.  The
// one definition of this arithmetic: the compositor, the fused kernels' weights and cull, the visibility rule, the
// density primitives and the backwards all run it, which is why their results agree bit for bit.  The samples may be
// in global memory or in LDS (the functor does the addressing).
template <class SdtOf>
__device__ __forceinline__ float sdt_before(int i0, int i1, SdtOf sdt_of) {
  float lsum = 0.f;
  for (int i = i0; i < i1; ++i) lsum += sdt_of(i);
  float total;
  return wave_excl_scan(lsum, total);
}
template <class SdtOf, class Body>
__device__ __forceinline__ void trans_walk(int i0, int i1, float run, SdtOf sdt_of, Body body) {
  for (int i = i0; i < i1; ++i) {
    const float sdt = sdt_of(i);
    const float e = expf(-sdt), T = expf(-run);
    run += sdt;
    body(i, T, e);
  }
}
template <class SdtOf, class Body>
__device__ __forceinline__ void trans_walk(int i0, int i1, SdtOf sdt_of, Body body) {
  trans_walk(i0, i1, sdt_before(i0, i1, sdt_of), sdt_of, body);
}

struct CompositeOut {
  float* colors;   // [3]
  float* opacity;  // [1]
  float* depth;    // [1]
  float* weights;  // [S] or null
  float* alphas;   // [S] or null
  float* trans;    // [S] or null
};

// nerfacc volrend.rendering arithmetic (call site src/render/rendering.py:89-96) for ONE ray
// by ONE wave: dt=t1-t0, alpha=1-exp(-sigma dt), T=exp(-exclusive_sum(sigma dt)), w=T alpha,
// colors=sum w rgb (+bkgd(1-opacity)), opacity=sum w, depth=sum w (t0+t1)/2 / max(opacity,eps).
// Lane l owns the contiguous samples [l*per, (l+1)*per); pointers may be global or LDS.
__device__ __forceinline__ void composite_ray(const float* __restrict__ sig, const float* __restrict__ rgb,
                                              const float* __restrict__ t0, const float* __restrict__ t1,
                                              int S, bool has_bkgd, float b0, float b1, float b2,
                                              const CompositeOut& o) {
  const int lane = lane_id();
  int i0, i1;
  lane_range(S, lane, i0, i1);
  float ar = 0.f, ag = 0.f, ab = 0.f, ao = 0.f, ad = 0.f;
  trans_walk(i0, i1, [&](int i) { return sig[i] * (t1[i] - t0[i]); }, [&](int i, float T, float e) {
    const float a = t0[i], b = t1[i];
    const float alpha = 1.0f - e;
    const float w = T * alpha;
    ar += w * rgb[3 * i + 0];
    ag += w * rgb[3 * i + 1];
    ab += w * rgb[3 * i + 2];
    ao += w;
    ad += w * (a + b) / 2.0f;
    if (o.weights) o.weights[i] = w;
    if (o.alphas) o.alphas[i] = alpha;
    if (o.trans) o.trans[i] = T;
  });
  ar = wave_sum(ar);
  ag = wave_sum(ag);
  ab = wave_sum(ab);
  ao = wave_sum(ao);
  ad = wave_sum(ad);
  if (lane == 0) {
    const float dep = ad / fmaxf(ao, kFltEps);
    if (has_bkgd) {
      const float k = 1.0f - ao;
      ar = ar + b0 * k;
      ag = ag + b1 * k;
      ab = ab + b2 * k;
    }
    o.colors[0] = ar;
    o.colors[1] = ag;
    o.colors[2] = ab;
    o.opacity[0] = ao;
    o.depth[0] = dep;
  }
}

// weights only (density pass of the hierarchical sampler): w[i] = T_i * alpha_i
__device__ __forceinline__ void weights_ray(const float* __restrict__ sig, const float* __restrict__ edges,
                                            int S, float* __restrict__ w_out) {
  int i0, i1;
  lane_range(S, lane_id(), i0, i1);
  trans_walk(i0, i1, [&](int i) { return sig[i] * (edges[i + 1] - edges[i]); },
             [&](int i, float T, float e) { w_out[i] = T * (1.0f - e); });
}

// The density backward for ONE ray by ONE wave ("Full compositor backward"): with T_i, e_i, alpha_i as in
// trans_walk, p_i = prefix[i] (1 when absent), q_i = dL/dw_i (has_q: q_of(i); else absent), tau_i = dL/dtrans_i and
// a_i = dL/dalpha_i (each nullable):
//   A_i = q_i T_i p_i + a_i,   B_i T_i = (q_i alpha_i + tau_i) p_i T_i,   dL/dsigma_i = dt_i (A_i e_i - sum_{j>i} B_j T_j)
// Pass 1 sums B_j T_j over the lane's samples, the suffix is total - prefix (wave_excl_scan), pass 2 walks again and
// hands per_sample(i, w_i) each sample (the compositor's d_rgb).  Every optional operand is wave-uniform.  The pointers
// are the ray's own (sample i of the ray at [i]).
template <class QOf, class PerSample>
__device__ __forceinline__ void density_bwd_ray(const float* __restrict__ sig, const float* __restrict__ t0,
                                                const float* __restrict__ t1, int i0, int i1, bool has_q, QOf q_of,
                                                const float* __restrict__ tau, const float* __restrict__ a,
                                                const float* __restrict__ prefix, float* __restrict__ d_sig,
                                                PerSample per_sample) {
  auto sdt_of = [&](int i) { return sig[i] * (t1[i] - t0[i]); };
  auto bt_of = [&](int i, float q, float T, float w) {
    float bt = 0.f;
    if (has_q) bt = q * w;
    if (tau) bt += tau[i] * T;
    return bt;
  };
  const float run = sdt_before(i0, i1, sdt_of);
  float lq = 0.f;
  trans_walk(i0, i1, run, sdt_of, [&](int i, float T, float e) {
    if (prefix) T = T * prefix[i];
    lq += bt_of(i, has_q ? q_of(i) : 0.f, T, T * (1.0f - e));
  });
  float qtot;
  const float qbefore = wave_excl_scan(lq, qtot);  // sum of B_j T_j over the lanes before this one
  float suffix = qtot - qbefore;                    // over this lane's samples and all later ones
  trans_walk(i0, i1, run, sdt_of, [&](int i, float T, float e) {
    if (prefix) T = T * prefix[i];
    const float w = T * (1.0f - e);
    const float q = has_q ? q_of(i) : 0.f;
    suffix -= bt_of(i, q, T, w);  // now: over j > i
    float A = 0.f;
    if (has_q) A = q * T;
    if (a) A += a[i];
    d_sig[i] = (t1[i] - t0[i]) * (A * e - suffix);
    per_sample(i, w);
  });
}

// torch.linspace(0,1,n) element i, float32 (symmetric evaluation like ATen's CPU kernel)
__device__ __forceinline__ float linspace01(int i, int n) {
  if (n <= 1) return 0.f;
  const float step = 1.0f / (float)(n - 1);
  return (i < n / 2) ? (float)i * step : 1.0f - (float)(n - 1 - i) * step;
}

// Hierarchical resampling for ONE ray by ONE wave (build's definition, oracle sample_pdf +
// merge_edges): inverse-CDF samples of pdf=(max(w,0)+1e-5)/sum over `edges`, merged with the
// edges and sorted ascending into out[S+1+n_imp].  cdf_s (>= S+1 floats) and vals_s
// (>= S+1+pow2ceil(n_imp) floats) are this wave's LDS scratch; u is [n_imp] or null (deterministic).
__device__ __forceinline__ void sample_pdf_merge_ray(const float* __restrict__ edges,
                                                     const float* __restrict__ w, int S, int n_imp,
                                                     const float* __restrict__ u, float* cdf_s,
                                                     float* vals_s, float* __restrict__ out) {
  const int lane = lane_id();
  const int per = (S + 63) >> 6;
  const int i0 = lane * per;
  const int i1 = min(i0 + per, S);
  float lsum = 0.f;
  for (int i = i0; i < i1; ++i) lsum += fmaxf(w[i], 0.f) + 1e-5f;
  const float tot = wave_sum(lsum);
  float lp = 0.f;
  for (int i = i0; i < i1; ++i) lp += (fmaxf(w[i], 0.f) + 1e-5f) / tot;
  float dummy;
  float run = wave_excl_scan(lp, dummy);
  for (int i = i0; i < i1; ++i) {
    run += (fmaxf(w[i], 0.f) + 1e-5f) / tot;
    cdf_s[i + 1] = run;
  }
  if (lane == 0) cdf_s[0] = 0.f;
  for (int i = lane; i <= S; i += 64) vals_s[i] = edges[i];
  __builtin_amdgcn_wave_barrier();
  for (int k = lane; k < n_imp; k += 64) {
    const float uk = u ? u[k] : linspace01(k, n_imp);
    int lo = 0, hi = S + 1;  // searchsorted(cdf, u, right=True): #entries <= u
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cdf_s[mid] <= uk) lo = mid + 1; else hi = mid;
    }
    const int below = max(lo - 1, 0), above = min(lo, S);
    const float c0 = cdf_s[below], c1 = cdf_s[above];
    const float e0 = edges[below], e1 = edges[above];
    float denom = c1 - c0;
    if (denom < 1e-5f) denom = 1.0f;
    vals_s[S + 1 + k] = e0 + (uk - c0) / denom * (e1 - e0);
  }
  __builtin_amdgcn_wave_barrier();
  float* smp = vals_s + (S + 1);  // the n_imp importance samples
  // Deterministic u is increasing and the inverse CDF is monotone, so the samples are normally sorted
  // already; explicit (random) u leaves them unordered.  Check, and sort only when needed.
  bool unsorted = false;
  for (int k = lane; k + 1 < n_imp; k += 64) unsorted |= smp[k] > smp[k + 1];
  if (__any(unsorted)) {
    // bitonic sort in LDS, padded with +inf to a power of two
    int n2 = 1;
    while (n2 < n_imp) n2 <<= 1;
    for (int k = n_imp + lane; k < n2; k += 64) smp[k] = __builtin_huge_valf();
    __builtin_amdgcn_wave_barrier();
    for (int k = 2; k <= n2; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = lane; i < n2; i += 64) {
          const int l = i ^ j;
          if (l > i) {
            const float a = smp[i], b = smp[l];
            const bool up = (i & k) == 0;
            if ((a > b) == up) { smp[i] = b; smp[l] = a; }
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  // Merge of two sorted lists by rank: an edge goes to (its index + #samples strictly below it), a
  // sample to (its index + #edges <= it): a permutation for any ties, O(log n) LDS reads per element.
  for (int i = lane; i <= S; i += 64) {
    const float v = vals_s[i];
    int lo = 0, hi = n_imp;  // lower_bound over the sorted samples
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (smp[mid] < v) lo = mid + 1; else hi = mid;
    }
    out[i + lo] = v;
  }
  for (int k = lane; k < n_imp; k += 64) {
    const float v = smp[k];
    int lo = 0, hi = S + 1;  // upper_bound over the sorted edges
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (vals_s[mid] <= v) lo = mid + 1; else hi = mid;
    }
    out[k + lo] = v;
  }
}

// Pinhole ray of pixel (h, w) (src/utils/utilities.py:57-80): d_cam = [(w - W/2)/f, -(h - H/2)/f, -1], unit length,
// rotated by the pose's 3x3 block (row-major [3][4] in m), origin = its last column.  The one definition used by
// k_get_rays and by the fused render kernel when it generates its own rays.
// (pinhole_dir_cam: its unit camera-frame direction alone)
__device__ __forceinline__ void pinhole_dir_cam(float half_w, float half_h, float focal, int h, int w, float (&c)[3]) {
  float dx = ((float)w - half_w) / focal;
  float dy = -((float)h - half_h) / focal;
  float dz = -1.0f;
  const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
  c[0] = dx / nrm;
  c[1] = dy / nrm;
  c[2] = dz / nrm;
}
__device__ __forceinline__ void pinhole_ray(const float* __restrict__ m, float half_w, float half_h, float focal, int h,
                                            int w, float (&o)[3], float (&d)[3]) {
  float c[3];
  pinhole_dir_cam(half_w, half_h, focal, h, w, c);
  const float dx = c[0], dy = c[1], dz = c[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d[k] = (dx * m[4 * k + 0] + dy * m[4 * k + 1]) + dz * m[4 * k + 2];
    o[k] = m[4 * k + 3];
  }
}
// The same two under a camera table K = (fx, fy, cx, cy) (learnable intrinsics): d_cam = [(w - cx)/fx,
// -(h - cy)/fy, -1].  The stored intrinsics are K = (focal, focal, W/2, H/2): the same operations on the same values, so
// the same bits.  (Restated, not shared: the functions above are inlined into the render kernels, whose code must not
// move with this one.)
__device__ __forceinline__ void pinhole_dir_cam_k(float fx, float fy, float cx, float cy, int h, int w, float (&c)[3]) {
  float dx = ((float)w - cx) / fx;
  float dy = -((float)h - cy) / fy;
  float dz = -1.0f;
  const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
  c[0] = dx / nrm;
  c[1] = dy / nrm;
  c[2] = dz / nrm;
}
__device__ __forceinline__ void rotate_dir_cam(const float* __restrict__ m, const float (&c)[3], float (&o)[3],
                                               float (&d)[3]) {
  const float dx = c[0], dy = c[1], dz = c[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d[k] = (dx * m[4 * k + 0] + dy * m[4 * k + 1]) + dz * m[4 * k + 2];
    o[k] = m[4 * k + 3];
  }
}
__device__ __forceinline__ void pinhole_ray_k(const float* __restrict__ m, const float* __restrict__ K, int h, int w,
                                              float (&o)[3], float (&d)[3]) {
  float c[3];
  pinhole_dir_cam_k(K[0], K[1], K[2], K[3], h, w, c);
  rotate_dir_cam(m, c, o, d);
}

// World ray -> normalised device coordinates (src/utils/utilities.py:84-120), in place.  The one definition used by
// k_to_ndc, k_build_rays (ray_ops.hip) and k_ray_batch (raydata.hip).
__device__ __forceinline__ void ndc_ray(float (&o)[3], float (&d)[3], float sx, float sy, float near, float two_near) {
  const float dx = d[0], dy = d[1], dz = d[2];
  float ox = o[0], oy = o[1], oz = o[2];
  const float t = -(near + oz) / dz;
  ox = ox + t * dx;
  oy = oy + t * dy;
  oz = oz + t * dz;
  o[0] = sx * ox / oz;
  o[1] = sy * oy / oz;
  o[2] = 1.0f + two_near / oz;
  d[0] = sx * (dx / dz - ox / oz);
  d[1] = sy * (dy / dz - oy / oz);
  d[2] = -two_near / oz;
}

// The backward of ndc_ray: (o, d) the WORLD ray it was given, (go, gd) = dL/d(its outputs) on entry and dL/d(o, d) on
// return.  The forward's intermediates are formed again with its own operations; the chain is the plain reverse sweep
// (the intersection p = o + t d is kept a function of its inputs, as autograd through the forward keeps it).
__device__ __forceinline__ void ndc_ray_bwd(const float (&o)[3], const float (&d)[3], float sx, float sy, float near,
                                            float two_near, float (&go)[3], float (&gd)[3]) {
  const float dx = d[0], dy = d[1], dz = d[2];
  const float t = -(near + o[2]) / dz;
  const float px = o[0] + t * dx, py = o[1] + t * dy, pz = o[2] + t * dz;
  const float ux = sx * (go[0] - gd[0]), uy = sy * (go[1] - gd[1]), uz = two_near * (go[2] - gd[2]);
  const float gpx = ux / pz, gpy = uy / pz;
  const float gpz = -((ux * px + uy * py) + uz) / (pz * pz);
  const float bx = sx * gd[0], by = sy * gd[1];
  const float gt = (gpx * dx + gpy * dy) + gpz * dz;  // dL/dt through p = o + t d
  go[0] = gpx;
  go[1] = gpy;
  go[2] = gpz - gt / dz;  // t = -(near + o_z) / d_z
  gd[0] = bx / dz + t * gpx;
  gd[1] = by / dz + t * gpy;
  gd[2] = (t * gpz - (bx * dx + by * dy) / (dz * dz)) - gt * t / dz;
}

// edge i of the fixed-count stratified sampler (oracle.stratified_edges)
__device__ __forceinline__ float stratified_edge(float near, float step, int S, int i, int u_mode,
                                                 const float* __restrict__ u_ray) {
  const float fi = (float)i;
  if (u_mode == 0) return near + fi * step;
  if (u_mode == 1) return near + (fi + u_ray[0]) * step;
  const float lo = near + fmaxf(fi - 0.5f, 0.0f) * step;
  const float hi = near + fminf(fi + 0.5f, (float)S) * step;
  return lo + (hi - lo) * u_ray[i];
}

}  // namespace fsn
