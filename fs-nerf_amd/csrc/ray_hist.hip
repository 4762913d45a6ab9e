// ray_hist.hip — a ray's termination distribution on a fixed depth axis, and the KL divergence between the
// distributions of neighbouring pixels of a rendered patch ("Neighbouring-ray KL"): this package's own
// definition of InfoNeRF's second term, its "information gain reduction".  Packed rays have differing sample counts, so
// two rays are compared bin by bin on common bins of [t_min, t_max], not sample by sample.  The histogram runs one
// wavefront per ray on ray_dev.hpp's skeleton (ray_work / ray_launch, sorted ray_indices only), the patch term one
// wavefront per pixel.  No LDS, no atomics, every sum in a fixed order; each backward memsets its output first.
#include "common.hpp"
#include "ray_dev.hpp"

namespace fsn {

// ------------------------------------------------------------------ termination histogram
// The axis: h = (t_max - t_min) / B and edge b = t_min + (float)b h, both float32 - these values ARE the edges
// (fsn_ray_hist_edges hands them out; tests/ray_hist_ref.py takes them as given).
struct HistAxis {
  float t_min, h;
  int B;
};
static inline float hist_bin_width(float t_min, float t_max, int B) { return (t_max - t_min) / (float)B; }
__host__ __device__ __forceinline__ float hist_edge(const HistAxis& ax, int b) { return ax.t_min + (float)b * ax.h; }

// sample i counts iff its bounds are finite and its width positive; then u_i = max(v_i, 0)
__device__ __forceinline__ bool hist_ok(float a, float c) { return isfinite(a) && isfinite(c) && c - a > 0.f; }
// the part of [a, c) inside bin [e0, e1), over the sample's width
__device__ __forceinline__ float hist_frac(float a, float c, float e0, float e1) {
  return fmaxf(fminf(c, e1) - fmaxf(a, e0), 0.f) / (c - a);
}

// s_r = sum_i u_i: a lane-strided sum and wave_sum, as the entropy's mass
__device__ __forceinline__ float hist_mass(const float* __restrict__ v_, const float* __restrict__ a_,
                                           const float* __restrict__ c_, int S, int lane) {
  float ls = 0.f;
  for (int i = lane; i < S; i += 64)
    if (hist_ok(a_[i], c_[i])) ls += fmaxf(v_[i], 0.f);
  return wave_sum(ls);
}

// Row q of `out` [n_rows, B] is ray first + q.  The lanes own the bins b = lane, lane + 64, ...; every lane walks all of
// the ray's samples in ascending order (the loads are wave-uniform), so H_rb is ONE sequential float32 sum from +0 with
// no cross-lane step: it does not depend on the samples being sorted, and a NumPy loop restates it bit for bit.
__global__ void k_ray_hist_fwd(const float* __restrict__ v, const float* __restrict__ t0, const float* __restrict__ t1,
                               SpanArgs sp, int64_t first, int64_t R_end, HistAxis ax, int normalize, float eps,
                               float* __restrict__ out) {
  RayWork rw;
  const bool any = ray_work(sp, R_end, rw, first);
  if (rw.r >= R_end) return;
  float* o_ = out + (rw.r - first) * ax.B;
  if (!any) {
    for (int b = rw.lane; b < ax.B; b += 64) o_[b] = 0.f;
    return;
  }
  const float* v_ = v + rw.beg; const float* a_ = t0 + rw.beg; const float* c_ = t1 + rw.beg;
  const float den = normalize ? hist_mass(v_, a_, c_, rw.S, rw.lane) + eps : 1.0f;
  for (int b = rw.lane; b < ax.B; b += 64) {
    const float e0 = hist_edge(ax, b), e1 = hist_edge(ax, b + 1);
    float acc = 0.f;
    for (int i = 0; i < rw.S; ++i) {
      const float a = a_[i], c = c_[i];
      if (hist_ok(a, c)) acc += fmaxf(v_[i], 0.f) * hist_frac(a, c, e0, e1);
    }
    o_[b] = normalize ? acc / den : acc;
  }
}

// d u_i = sum_b G_rb f_ib, with normalize (sum_b G_rb f_ib - sum_b G_rb P_rb) / (s_r + eps); d v_i = d u_i where the
// sample counts and v_i >= 0 (torch.clamp's rule), 0 elsewhere.  P is the forward's saved output.  The lanes stride the
// samples; each loops over the bins its interval can touch - the bins of its two ends, widened by one on each side and
// clamped to [0, B-1]: the guard ov > 0 drops the extra ones, so a rounding of the index can never lose a bin.
__global__ void k_ray_hist_bwd(const float* __restrict__ v, const float* __restrict__ t0, const float* __restrict__ t1,
                               SpanArgs sp, int64_t first, int64_t R_end, HistAxis ax, int normalize, float eps,
                               const float* __restrict__ P, const float* __restrict__ G, float* __restrict__ d_v) {
  RayWork rw;
  if (!ray_work(sp, R_end, rw, first)) return;
  const float* v_ = v + rw.beg; const float* a_ = t0 + rw.beg; const float* c_ = t1 + rw.beg;
  float* d_ = d_v + rw.beg;
  const float* g_ = G + (rw.r - first) * ax.B;
  float gp = 0.f, den = 1.0f;
  if (normalize) {
    const float* p_ = P + (rw.r - first) * ax.B;
    for (int b = rw.lane; b < ax.B; b += 64) gp += g_[b] * p_[b];
    gp = wave_sum(gp);
    den = hist_mass(v_, a_, c_, rw.S, rw.lane) + eps;
  }
  const float top = (float)(ax.B - 1);
  for (int i = rw.lane; i < rw.S; i += 64) {
    const float a = a_[i], c = c_[i];
    if (!(hist_ok(a, c) && v_[i] >= 0.f)) continue;  // (the memset's zero stays)
    // (clamped as floats first: a far-away bound must not overflow the conversion)
    const int b_lo = (int)fminf(fmaxf(floorf((a - ax.t_min) / ax.h) - 1.0f, 0.f), top);
    const int b_hi = (int)fminf(fmaxf(floorf((c - ax.t_min) / ax.h) + 1.0f, 0.f), top);
    float acc = 0.f;
    for (int b = b_lo; b <= b_hi; ++b) {
      const float f = hist_frac(a, c, hist_edge(ax, b), hist_edge(ax, b + 1));
      if (f > 0.f) acc += g_[b] * f;
    }
    d_[i] = normalize ? (acc - gp) / den : acc;
  }
}

// ------------------------------------------------------------------ KL between neighbouring pixels of a patch
// D(p, q) = sum_b p_b (log(p_b + eps) - log(q_b + eps)); pixel (i, j) owns its right pair (j < Pw-1) and its down pair
// (i < Ph-1).  A pair counts iff both of its pixels' weights are non-zero (c is 0/1; NULL: all ones); any other pair is
// skipped - nothing of it is computed.  One wave per pixel (four per block), the lanes striding over the bins.
struct NklPix {
  int64_t k;  // pixel, flat over [B, Ph, Pw]
  int i, j;
};
__device__ __forceinline__ NklPix nkl_pixel(int64_t n_pix, int Ph, int Pw) {
  NklPix p;
  p.k = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t rem = p.k % ((int64_t)Ph * Pw);
  p.i = (int)(rem / Pw);
  p.j = (int)(rem - (int64_t)p.i * Pw);
  return p;
}
__device__ __forceinline__ bool nkl_on(const float* __restrict__ c, int64_t k) { return !c || c[k] != 0.f; }

__global__ void k_patch_nkl_fwd(const float* __restrict__ P, const float* __restrict__ c, int64_t n_pix, int Ph, int Pw,
                                int B, float eps, float* __restrict__ out) {
  const int lane = lane_id();
  const NklPix px = nkl_pixel(n_pix, Ph, Pw);
  if (px.k >= n_pix) return;
  const bool own = nkl_on(c, px.k);
  const bool right = own && px.j < Pw - 1 && nkl_on(c, px.k + 1);
  const bool down = own && px.i < Ph - 1 && nkl_on(c, px.k + Pw);
  const float* p_ = P + px.k * B;
  const float* qr_ = p_ + B;
  const float* qd_ = p_ + (int64_t)Pw * B;
  float ar = 0.f, ad = 0.f;
  if (right || down) {
    for (int b = lane; b < B; b += 64) {
      const float p = p_[b], lp = logf(p + eps);
      if (right) ar += p * (lp - logf(qr_[b] + eps));
      if (down) ad += p * (lp - logf(qd_[b] + eps));
    }
    ar = wave_sum(ar);
    ad = wave_sum(ad);
  }
  if (lane == 0) out[px.k] = (right ? ar : 0.f) + (down ? ad : 0.f);
}

// dD/dp_b = log(p_b + eps) - log(q_b + eps) + p_b / (p_b + eps),  dD/dq_b = -p_b / (q_b + eps).  Gather form: bin b of
// pixel (i, j) adds its own right pair, its own down pair, the left neighbour's right pair and the upper neighbour's
// down pair (where it is the q), in that order; each lane writes its bins once.
__global__ void k_patch_nkl_bwd(const float* __restrict__ P, const float* __restrict__ c, int64_t n_pix, int Ph, int Pw,
                                int B, float eps, const float* __restrict__ G, float* __restrict__ d_P) {
  const int lane = lane_id();
  const NklPix px = nkl_pixel(n_pix, Ph, Pw);
  if (px.k >= n_pix) return;
  const bool own = nkl_on(c, px.k);
  const bool right = own && px.j < Pw - 1 && nkl_on(c, px.k + 1);
  const bool down = own && px.i < Ph - 1 && nkl_on(c, px.k + Pw);
  const bool left = own && px.j >= 1 && nkl_on(c, px.k - 1);
  const bool up = own && px.i >= 1 && nkl_on(c, px.k - Pw);
  if (!(right || down || left || up)) return;  // (the memset's zeros are the gradient)
  const float* p_ = P + px.k * B;
  const int64_t row = (int64_t)Pw * B;
  const float g_own = G[px.k];
  const float g_left = left ? G[px.k - 1] : 0.f, g_up = up ? G[px.k - Pw] : 0.f;
  for (int b = lane; b < B; b += 64) {
    const float p = p_[b], pe = p + eps, lp = logf(pe);
    float acc = 0.f;
    if (right) acc += g_own * ((lp - logf(p_[b + B] + eps)) + p / pe);
    if (down) acc += g_own * ((lp - logf(p_[b + row] + eps)) + p / pe);
    if (left) acc += g_left * -(p_[b - B] / pe);
    if (up) acc += g_up * -(p_[b - row] / pe);
    d_P[px.k * B + b] = acc;
  }
}

}  // namespace fsn

using namespace fsn;

// what the two histogram entry points check alike: the row subset and the axis
static int ray_hist_args(const char* who, int64_t n_rays, int64_t first_ray, int64_t n_rows, int bins, float t_min,
                         float t_max, float eps, HistAxis* ax) {
  FSN_REQUIRE(n_rays >= 0 && first_ray >= 0 && n_rows >= 0 && first_ray <= n_rays && n_rows <= n_rays - first_ray,
              FSN_E_INVALID, "%s: bad sizes (the rows [first_ray, first_ray + n_rows) are not rays of [0, n_rays))", who);
  FSN_REQUIRE(bins >= 1 && bins <= 4096, FSN_E_INVALID, "%s: bad sizes (1 <= bins <= 4096)", who);
  FSN_REQUIRE(std::isfinite(t_min) && std::isfinite(t_max) && t_min < t_max, FSN_E_INVALID,
              "%s: t_min < t_max, both finite, is required", who);
  FSN_REQUIRE(eps > 0.f, FSN_E_INVALID, "%s: eps must be positive", who);
  *ax = HistAxis{t_min, hist_bin_width(t_min, t_max, bins), bins};
  FSN_REQUIRE(ax->h > 0.f && std::isfinite(ax->h), FSN_E_INVALID, "%s: t_max - t_min has no float32 bin width", who);
  return FSN_OK;
}

extern "C" int fsn_ray_hist_edges(int bins, float t_min, float t_max, float* edges_host) {
  HistAxis ax;
  if (int rc = ray_hist_args("fsn_ray_hist_edges", 0, 0, 0, bins, t_min, t_max, 1.0f, &ax)) return rc;
  FSN_REQUIRE(edges_host, FSN_E_INVALID, "fsn_ray_hist_edges: null pointer");
  for (int b = 0; b <= bins; ++b) edges_host[b] = hist_edge(ax, b);
  return FSN_OK;
}

extern "C" int fsn_ray_hist_fwd(const float* values, const float* t_starts, const float* t_ends,
                                const int64_t* ray_indices, int64_t N, int64_t n_rays, int64_t first_ray, int64_t n_rows,
                                int bins, float t_min, float t_max, int normalize, float eps, float* out,
                                fsn_stream_t stream) {
  RayLaunch L;
  if (int rc = ray_launch("fsn_ray_hist_fwd", ray_indices, nullptr, N, n_rays, 0, false, &L)) return rc;
  HistAxis ax;
  if (int rc = ray_hist_args("fsn_ray_hist_fwd", n_rays, first_ray, n_rows, bins, t_min, t_max, eps, &ax)) return rc;
  if (n_rows == 0) return FSN_OK;
  FSN_REQUIRE(out, FSN_E_INVALID, "fsn_ray_hist_fwd: null pointer");
  if (!L.launch) {  // (n_rows > 0, so n_rays > 0: N == 0, every ray is empty)
    FSN_HIP(hipMemsetAsync(out, 0, (size_t)n_rows * bins * sizeof(float), as_stream(stream)));
    return FSN_OK;
  }
  FSN_REQUIRE(values && t_starts && t_ends, FSN_E_INVALID, "fsn_ray_hist_fwd: null pointer");
  k_ray_hist_fwd<<<(unsigned)((n_rows + 3) / 4), 256, 0, as_stream(stream)>>>(
      values, t_starts, t_ends, L.sp, first_ray, first_ray + n_rows, ax, normalize, eps, out);
  FSN_LAUNCH_CHECK("k_ray_hist_fwd");
  return FSN_OK;
}

extern "C" int fsn_ray_hist_bwd(const float* values, const float* t_starts, const float* t_ends,
                                const int64_t* ray_indices, int64_t N, int64_t n_rays, int64_t first_ray, int64_t n_rows,
                                int bins, float t_min, float t_max, int normalize, float eps, const float* hist,
                                const float* d_out, float* d_values, fsn_stream_t stream) {
  RayLaunch L;
  if (int rc = ray_launch("fsn_ray_hist_bwd", ray_indices, nullptr, N, n_rays, 0, false, &L)) return rc;
  HistAxis ax;
  if (int rc = ray_hist_args("fsn_ray_hist_bwd", n_rays, first_ray, n_rows, bins, t_min, t_max, eps, &ax)) return rc;
  if (N == 0) return FSN_OK;
  const bool run = L.launch && n_rows > 0;
  FSN_REQUIRE(d_values && (!run || (values && t_starts && t_ends && d_out && (hist || !normalize))), FSN_E_INVALID,
              "fsn_ray_hist_bwd: null pointer");
  // samples of the rays outside the rows (and of no ray at all) keep this zero
  FSN_HIP(hipMemsetAsync(d_values, 0, (size_t)N * sizeof(float), as_stream(stream)));
  if (!run) return FSN_OK;
  k_ray_hist_bwd<<<(unsigned)((n_rows + 3) / 4), 256, 0, as_stream(stream)>>>(
      values, t_starts, t_ends, L.sp, first_ray, first_ray + n_rows, ax, normalize, eps, hist, d_out, d_values);
  FSN_LAUNCH_CHECK("k_ray_hist_bwd");
  return FSN_OK;
}

// sizes of the patch entry points: B >= 0, Ph, Pw >= 1, 1 <= bins <= 4096, and a grid that fits
static int patch_nkl_sizes(const char* who, int64_t B, int Ph, int Pw, int bins, float eps) {
  FSN_REQUIRE(B >= 0 && Ph >= 1 && Pw >= 1 && bins >= 1 && bins <= 4096, FSN_E_INVALID, "%s: bad sizes", who);
  FSN_REQUIRE((double)B * Ph * Pw <= 4.0 * 0x7fffffff, FSN_E_INVALID, "%s: bad sizes (too many pixels)", who);
  FSN_REQUIRE(eps > 0.f, FSN_E_INVALID, "%s: eps must be positive", who);
  return FSN_OK;
}

extern "C" int64_t fsn_patch_nkl_pairs(int64_t B, int Ph, int Pw) {
  if (int rc = patch_nkl_sizes("fsn_patch_nkl_pairs", B, Ph, Pw, 1, 1.0f)) return rc;
  return B * ((int64_t)Ph * (Pw - 1) + (int64_t)(Ph - 1) * Pw);
}

extern "C" int fsn_patch_nkl_fwd(const float* P, const float* pair_weight, int64_t B, int Ph, int Pw, int bins, float eps,
                                 float* out, fsn_stream_t stream) {
  if (int rc = patch_nkl_sizes("fsn_patch_nkl_fwd", B, Ph, Pw, bins, eps)) return rc;
  if (B == 0) return FSN_OK;
  FSN_REQUIRE(P && out, FSN_E_INVALID, "fsn_patch_nkl_fwd: null pointer");
  const int64_t n_pix = B * (int64_t)Ph * Pw;
  k_patch_nkl_fwd<<<(unsigned)((n_pix + 3) / 4), 256, 0, as_stream(stream)>>>(P, pair_weight, n_pix, Ph, Pw, bins, eps, out);
  FSN_LAUNCH_CHECK("k_patch_nkl_fwd");
  return FSN_OK;
}

extern "C" int fsn_patch_nkl_bwd(const float* P, const float* pair_weight, int64_t B, int Ph, int Pw, int bins, float eps,
                                 const float* d_out, float* d_P, fsn_stream_t stream) {
  if (int rc = patch_nkl_sizes("fsn_patch_nkl_bwd", B, Ph, Pw, bins, eps)) return rc;
  if (B == 0) return FSN_OK;
  FSN_REQUIRE(P && d_out && d_P, FSN_E_INVALID, "fsn_patch_nkl_bwd: null pointer");
  const int64_t n_pix = B * (int64_t)Ph * Pw;
  FSN_HIP(hipMemsetAsync(d_P, 0, (size_t)n_pix * bins * sizeof(float), as_stream(stream)));
  if (Ph == 1 && Pw == 1) return FSN_OK;  // no pairs: the zeros are the gradient
  k_patch_nkl_bwd<<<(unsigned)((n_pix + 3) / 4), 256, 0, as_stream(stream)>>>(P, pair_weight, n_pix, Ph, Pw, bins, eps, d_out,
                                                                             d_P);
  FSN_LAUNCH_CHECK("k_patch_nkl_bwd");
  return FSN_OK;
}
