// occ_dev.hpp — device code of the occupancy-grid sampler shared by the standalone kernels (occgrid.hip) and the fused
// occupancy render kernel (render_occ.hip): the grid lookup and the per-ray lattice march, ONE definition so that both
// produce the same samples bit for bit.  The rule itself is this build's definition of the estimator contract
// (occgrid.hip's header; oracle.occgrid_march mirrors it).
#pragma once
#include "common.hpp"

namespace fsn {

struct GridDev {
  float amin[3], amax[3];  // region of interest (level 0)
  int32_t res, levels;
};

inline int make_grid(const float* aabb_host, int res, int levels, GridDev& G) {
  FSN_REQUIRE(aabb_host, FSN_E_INVALID, "occupancy grid: null aabb");
  FSN_REQUIRE(res >= 1 && res <= 1024 && levels >= 1 && levels <= 8, FSN_E_INVALID, "occupancy grid: bad resolution / levels");
  for (int a = 0; a < 3; ++a) {
    G.amin[a] = aabb_host[a];
    G.amax[a] = aabb_host[3 + a];
    FSN_REQUIRE(G.amax[a] > G.amin[a], FSN_E_INVALID, "occupancy grid: empty aabb");
  }
  G.res = res; G.levels = levels;
  return FSN_OK;
}

// occupancy of the cell holding point p: finest level whose box contains p; false outside all boxes
__device__ __forceinline__ bool grid_occupied(const GridDev& G, const uint32_t* __restrict__ bits, float px, float py,
                                              float pz) {
  const float p[3] = {px, py, pz};
  float c[3], h[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    c[a] = (G.amin[a] + G.amax[a]) / 2.0f;
    h[a] = (G.amax[a] - G.amin[a]) / 2.0f;
  }
  float s = 1.0f;
  for (int l = 0; l < G.levels; ++l, s *= 2.0f) {
    bool in = true;
    int ci[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float lo = c[a] - h[a] * s, hi = c[a] + h[a] * s;
      in = in && p[a] >= lo && p[a] <= hi;
      int q = (int)floorf((p[a] - lo) / (hi - lo) * (float)G.res);
      ci[a] = min(max(q, 0), G.res - 1);
    }
    if (in) {
      const int64_t cell = (int64_t)l * G.res * G.res * G.res + ((int64_t)ci[0] * G.res + ci[1]) * G.res + ci[2];
      return (bits[cell >> 5] >> (cell & 31)) & 1u;
    }
  }
  return false;
}

// The lattice of one ray: t_k = near_r + k step, k >= k0, while t_k < t_hi.
struct RayLattice {
  float near_r, t_lo, t_hi;
  int32_t k0;
  bool any;  // the ray meets the outermost box inside [near, far)
};

__device__ __forceinline__ RayLattice ray_lattice(const GridDev& G, const float (&o)[3], const float (&d)[3],
                                                  float near_plane, float far_plane, float step, bool has_u, float u_r) {
  const float sc = (float)(1 << (G.levels - 1));
  float tmin = -__builtin_huge_valf(), tmax = __builtin_huge_valf();
  bool miss = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float c = (G.amin[a] + G.amax[a]) / 2.0f, h = (G.amax[a] - G.amin[a]) / 2.0f * sc;
    const float lo = c - h, hi = c + h;
    if (d[a] == 0.0f) {
      miss = miss || o[a] < lo || o[a] > hi;
    } else {
      const float ta = (lo - o[a]) / d[a], tb = (hi - o[a]) / d[a];
      tmin = fmaxf(tmin, fminf(ta, tb));
      tmax = fminf(tmax, fmaxf(ta, tb));
    }
  }
  RayLattice L;
  L.near_r = has_u ? near_plane + u_r * step : near_plane;
  L.t_lo = fmaxf(tmin, L.near_r);
  L.t_hi = fminf(tmax, far_plane);
  L.any = !miss && L.t_hi > L.t_lo;
  int k0 = L.any ? (int)ceilf((L.t_lo - L.near_r) / step) : 0;
  L.k0 = k0 < 0 ? 0 : k0;
  return L;
}

// One wavefront marches one ray, 64 lattice points per iteration; `sink(ts, te, keep, mask, total)` sees every
// iteration (keep: this lane's point is a sample; mask: ballot of keep; total: samples before this iteration).
// Returns the ray's sample count.
template <class Sink>
__device__ __forceinline__ int march_ray(const GridDev& G, const uint32_t* __restrict__ bits, const float (&o)[3],
                                         const float (&d)[3], const RayLattice& L, float step, int32_t max_steps,
                                         Sink&& sink) {
  const int lane = (int)(threadIdx.x & 63);
  int total = 0;
  if (!L.any) return 0;
  for (int it = 0; it < max_steps; it += 64) {
    const int k = L.k0 + it + lane;
    const float ts = L.near_r + (float)k * step;
    const float te = ts + step;
    const bool in_range = (it + lane) < max_steps && ts >= L.t_lo && ts < L.t_hi;
    bool keep = false;
    if (in_range) {
      const float tm = (ts + te) / 2.0f;
      keep = grid_occupied(G, bits, o[0] + d[0] * tm, o[1] + d[1] * tm, o[2] + d[2] * tm);
    }
    const uint64_t m = __ballot(keep);
    sink(ts, te, keep, m, total);
    total += __popcll(m);
    // wave-uniform exit: the first lane's lattice point of the NEXT iteration is already past the box
    const float ts_next = L.near_r + (float)(L.k0 + it + 64) * step;
    if (!(ts_next < L.t_hi)) break;
  }
  return total;
}

// Per-ray bounds (k_occ_march; +-inf where fsn_occgrid_march_ex got none, and for fsn_occgrid_march):
// t_lo = max(t_enter, near_r, t_min_r), t_hi = min(t_exit, far_plane, t_max_r), in that order; the lattice itself
// (near_r, step) is ray_lattice's.  +-inf bounds are allowed; t_max_r <= t_min_r leaves no samples.
__device__ __forceinline__ RayLattice ray_lattice_bounded(const GridDev& G, const float (&o)[3], const float (&d)[3],
                                                          float near_plane, float far_plane, float step, bool has_u,
                                                          float u_r, float t_min_r, float t_max_r) {
  RayLattice L = ray_lattice(G, o, d, near_plane, far_plane, step, has_u, u_r);
  L.t_lo = fmaxf(L.t_lo, t_min_r);
  L.t_hi = fminf(L.t_hi, t_max_r);
  L.any = L.any && L.t_hi > L.t_lo;  // (tightening never revives a ray that missed)
  int k0 = L.any ? (int)ceilf((L.t_lo - L.near_r) / step) : 0;
  L.k0 = k0 < 0 ? 0 : k0;
  return L;
}

// Cone regime (cone_angle > 0, near_plane >= 0): the step grows with distance, dt(t) = max(t cone_angle, step), in
// blocks of 64 intervals of ONE width, so that the block recurrence is wave-uniform and every lane's interval follows
// from the block start with one multiply and one add:
//   t_0 = t_lo + (u ? u_r dt(t_lo) : 0);  block b: dt_b = dt(t_b), ts_j = t_b + j dt_b, te_j = t_b + (j + 1) dt_b,
//   t_{b+1} = t_b + 64 dt_b (= te_63); interval j of block b is a sample iff 64 b + j < max_steps, ts_j < t_hi and
//   the cell of its midpoint is occupied; the march ends after the block with !(t_{b+1} < t_hi).
// te_j is bitwise ts_{j+1}: consecutive samples of a ray in a full grid are contiguous.  `L`: the (bounded) range of
// the ray with near_r = near_plane (no lattice shift: u moves the first block's start).  Same sink as march_ray.
template <class Sink>
__device__ __forceinline__ int march_ray_cone(const GridDev& G, const uint32_t* __restrict__ bits, const float (&o)[3],
                                              const float (&d)[3], const RayLattice& L, float step, float cone_angle,
                                              bool has_u, float u_r, int32_t max_steps, Sink&& sink) {
  const int lane = (int)(threadIdx.x & 63);
  int total = 0;
  if (!L.any) return 0;
  float tb = has_u ? L.t_lo + u_r * fmaxf(L.t_lo * cone_angle, step) : L.t_lo;
  for (int it = 0; it < max_steps; it += 64) {
    const float dtb = fmaxf(tb * cone_angle, step);
    const float ts = tb + (float)lane * dtb;
    const float te = tb + (float)(lane + 1) * dtb;
    const bool in_range = (it + lane) < max_steps && ts < L.t_hi;
    bool keep = false;
    if (in_range) {
      const float tm = (ts + te) / 2.0f;
      keep = grid_occupied(G, bits, o[0] + d[0] * tm, o[1] + d[1] * tm, o[2] + d[2] * tm);
    }
    const uint64_t m = __ballot(keep);
    sink(ts, te, keep, m, total);
    total += __popcll(m);
    tb = tb + 64.0f * dtb;  // wave-uniform and exact: every lane computes the same value
    if (!(tb < L.t_hi)) break;
  }
  return total;
}

// The choice of regime, ONE definition for k_occ_march (occgrid.hip) and k_render_occ (render_occ.hip): the ray's range
// with its per-ray bounds (+-inf: none; the cone regime has no lattice shift, so `has_u` does not reach the range), then
// march_ray_cone for cone_angle > 0 and march_ray otherwise - a wave-uniform branch.  A count pass and the fill pass
// that follows it call both functions with the same arguments.
__device__ __forceinline__ RayLattice ray_range(const GridDev& G, const float (&o)[3], const float (&d)[3], float near_plane,
                                                float far_plane, float step, float cone_angle, bool has_u, float u_r,
                                                float t_min_r, float t_max_r) {
  return ray_lattice_bounded(G, o, d, near_plane, far_plane, step, !(cone_angle > 0.0f) && has_u, u_r, t_min_r, t_max_r);
}
template <class Sink>
__device__ __forceinline__ int march_ray_regime(const GridDev& G, const uint32_t* __restrict__ bits, const float (&o)[3],
                                                const float (&d)[3], const RayLattice& L, float step, float cone_angle,
                                                bool has_u, float u_r, int32_t max_steps, Sink&& sink) {
  return cone_angle > 0.0f ? march_ray_cone(G, bits, o, d, L, step, cone_angle, has_u, u_r, max_steps, sink)
                           : march_ray(G, bits, o, d, L, step, max_steps, sink);
}

// ---------------------------------------------------------------- update_every_n_steps: one draw of the cell selection
// Shared by k_occ_select (occgrid.hip) and the fused refresh (occ_refresh.hip): ONE definition, so that both produce the
// same cell and the same point bit for bit.  The rule is stated at k_occ_select.
__device__ __host__ __forceinline__ uint32_t occ_mix(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
__device__ __host__ __forceinline__ uint32_t occ_rand(uint32_t i, uint32_t k, uint32_t seed_lo, uint32_t seed_hi) {
  return occ_mix(occ_mix(i + seed_lo) ^ (seed_hi + 0x9e3779b9u * (k + 1u)));
}

// order-preserving integer key of a float (0 is below every key: "untouched" in the pending array)
__device__ __forceinline__ uint32_t occ_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct OccDraw {
  int32_t cell;  // cell index inside the level, or -1 for an unused occupied draw
  float x, y, z;
};

// draw i of a level (bits / prefix: that level's words and popcount prefix; lo / hi: its box).  all_cells: draw i IS
// cell i (warm-up).  A sentinel draw still gets a point: the one of its uniform cell r(i, 0) % res^3.
__device__ __forceinline__ OccDraw occ_draw(const uint32_t* __restrict__ bits, const int32_t* __restrict__ prefix, int res,
                                            int64_t i, int64_t n_draws, int64_t n_uniform, int all_cells, uint32_t seed_lo,
                                            uint32_t seed_hi, float lox, float loy, float loz, float hix, float hiy,
                                            float hiz) {
  const uint32_t res3 = (uint32_t)res * res * res;
  const int n_words = (int)(res3 >> 5);
  uint32_t cell;
  bool unused = false;
  if (all_cells) {
    cell = (uint32_t)i;
  } else {
    const uint32_t r = occ_rand((uint32_t)i, 0u, seed_lo, seed_hi);
    cell = r % res3;
    if (i >= n_uniform) {  // (prefix is only read here: it may be null when nothing is drawn from it)
      const int32_t total = prefix[n_words];
      const int64_t q = i - n_uniform, n_occupied = n_draws - n_uniform;
      int32_t j;  // the j-th occupied cell of the level
      if ((int64_t)total > n_occupied) {
        j = (int32_t)(r % (uint32_t)total);
      } else {
        j = (int32_t)q;
        unused = q >= (int64_t)total;
      }
      if (!unused) {
        int lo = 0, hi = n_words;  // last word w with prefix[w] <= j
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (prefix[mid] <= j) lo = mid; else hi = mid; }
        uint32_t m = bits[lo];
        for (int b = j - prefix[lo]; b > 0; --b) m &= m - 1u;  // drop the lowest set bits below the wanted one
        cell = ((uint32_t)lo << 5) + (uint32_t)(__ffs((int)m) - 1);
      }
    }
  }
  const uint32_t ix = cell / ((uint32_t)res * res), iy = (cell / (uint32_t)res) % (uint32_t)res, iz = cell % (uint32_t)res;
  const float inv24 = 1.0f / 16777216.0f;
  const float u0 = (float)(occ_rand((uint32_t)i, 1u, seed_lo, seed_hi) >> 8) * inv24;
  const float u1 = (float)(occ_rand((uint32_t)i, 2u, seed_lo, seed_hi) >> 8) * inv24;
  const float u2 = (float)(occ_rand((uint32_t)i, 3u, seed_lo, seed_hi) >> 8) * inv24;
  const float fr = (float)res;
  OccDraw d;
  d.cell = unused ? -1 : (int32_t)cell;
  d.x = lox + (((float)ix + u0) / fr) * (hix - lox);
  d.y = loy + (((float)iy + u1) / fr) * (hiy - loy);
  d.z = loz + (((float)iz + u2) / fr) * (hiz - loz);
  return d;
}

// box of level `lvl`: the roi scaled by 2^lvl about its centre (OccGridEstimator.level_aabb)
inline void level_box(const float* aabb_host, int lvl, float (&lo)[3], float (&hi)[3]) {
  for (int a = 0; a < 3; ++a) {
    const double c = ((double)aabb_host[a] + (double)aabb_host[3 + a]) / 2.0;
    const double h = ((double)aabb_host[3 + a] - (double)aabb_host[a]) / 2.0 * (double)(1 << lvl);
    lo[a] = (float)(c - h);
    hi[a] = (float)(c + h);
  }
}

// popcount prefix of `levels` consecutive levels' bit fields (occgrid.hip): prefix[l * (n_words + 1) + w]
int launch_occ_word_prefix(const uint32_t* bits, int n_words, int levels, int32_t* prefix, hipStream_t s);

}  // namespace fsn
