// occgrid.hip — occupancy-grid sampler for the `estimator` slot of render_rays:
// what the reference actually renders with (nerfacc OccGridEstimator; call sites src/render/rendering.py:66-74,
// src/run-nerf.py:96-98, 288-295).  nerfacc's source is not part of the reference, so the arithmetic below is
// THIS build's definition of the same contract ("occupancy sampler"; oracle/fsnerf_oracle.py mirrors it
// operation for operation):
//
//  * grid: `levels` nested boxes around the region of interest (level l = roi scaled by 2^l about its centre),
//    res^3 cells each, cell index (ix*res + iy)*res + iz; `occs` fp32 per cell, `bits` one bit per cell.
//  * march: per ray a lattice t_k = near_r + k*step, near_r = near_plane (+ u_r*step when stratified: the whole
//    march shifts); the interval [t_k, t_k + step) is a sample iff it starts inside [max(t_enter, near_r),
//    min(t_exit, far_plane)) of the outermost box and the cell of its MIDPOINT, at the finest level containing
//    the midpoint, is occupied.  One wavefront per ray, 64 lattice points per iteration, ballot + popcount
//    ranks; two passes (count, fill) around an exclusive scan of the counts.
//    ONE kernel (k_occ_march) serves fsn_occgrid_march and fsn_occgrid_march_ex: the latter adds per-ray bounds
//    [t_min_r, t_max_r] and the cone regime (cone_angle > 0): the step grows with distance, dt = max(t cone_angle, step),
//    taken once per block of 64 intervals (occ_dev.hpp, march_ray_cone; include/fsnerf_hip.h has the definition,
//    tests/occ_cone_ref.py restates it).  The plain entry point is the extended one with no bounds and cone_angle 0.
//  * visibility: T_i = exp(-sum_{j<i} sigma_j dt_j) per ray (prefix scan), keep iff T_i >= early_stop_eps and
//    alpha_i >= alpha_thre (fsn_packed_visibility: k_packed_visibility in packed_scan.hip, on ray_dev.hpp's trans_walk).
//  * update: occs[c] = max(occs[c]*decay, occ_c) for the evaluated cells; bit = occs > threshold.
#include "common.hpp"
#include "occ_dev.hpp"

namespace fsn {

// pass 0: counts[r]; pass 1: fill ray_indices / t_starts / t_ends at offsets[r].  Per-ray bounds t_min / t_max (either
// may be null: -inf / +inf) and the cone regime (cone_angle > 0: march_ray_cone; == 0: the lattice inside the tightened
// range, a wave-uniform branch).  Both entry points launch this kernel; the plain one passes no bounds and cone 0.
template <bool FILL>
__global__ void k_occ_march(const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t R, GridDev G,
                            const uint32_t* __restrict__ bits, float near_plane, float far_plane, float step,
                            const float* __restrict__ u, int32_t max_steps, const float* __restrict__ t_min,
                            const float* __restrict__ t_max, float cone_angle, int64_t* __restrict__ counts,
                            const int64_t* __restrict__ offsets, int64_t* __restrict__ ray_indices,
                            float* __restrict__ t_starts, float* __restrict__ t_ends) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r >= R) return;
  const float o[3] = {rays_o[3 * r], rays_o[3 * r + 1], rays_o[3 * r + 2]};
  const float d[3] = {rays_d[3 * r], rays_d[3 * r + 1], rays_d[3 * r + 2]};
  const float u_r = u ? u[r] : 0.f;
  const float lo_r = t_min ? t_min[r] : -__builtin_huge_valf(), hi_r = t_max ? t_max[r] : __builtin_huge_valf();
  const RayLattice L = ray_range(G, o, d, near_plane, far_plane, step, cone_angle, u != nullptr, u_r, lo_r, hi_r);
  const int64_t base_out = FILL ? offsets[r] : 0;
  auto sink = [&](float ts, float te, bool keep, uint64_t m, int before) {
    if (FILL && keep) {
      const int64_t pos = base_out + before + __popcll(m & ((1ull << lane) - 1ull));
      ray_indices[pos] = r;
      t_starts[pos] = ts;
      t_ends[pos] = te;
    }
  };
  const int total = march_ray_regime(G, bits, o, d, L, step, cone_angle, u != nullptr, u_r, max_steps, sink);
  if (!FILL && lane == 0) counts[r] = total;
}

// ray_aabb_intersect: one thread per (ray, box); the slab arithmetic is ray_lattice's (division form; a zero direction
// component tests the origin against the slab).  hit = !miss && min(t_exit, far) > max(t_enter, near); a hit writes
// those two clipped values, a miss writes miss_value twice.
__global__ void k_ray_aabb(const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t R,
                           const float* __restrict__ aabbs, int32_t M, float near_plane, float far_plane,
                           float miss_value, float* __restrict__ t_mins, float* __restrict__ t_maxs,
                           uint8_t* __restrict__ hits) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= R * M) return;
  const int64_t r = i / M;
  const float* box = aabbs + 6 * (i - r * M);
  float tmin = -__builtin_huge_valf(), tmax = __builtin_huge_valf();
  bool miss = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = box[a], hi = box[3 + a], oa = rays_o[3 * r + a], da = rays_d[3 * r + a];
    if (da == 0.0f) {
      miss = miss || oa < lo || oa > hi;
    } else {
      const float ta = (lo - oa) / da, tb = (hi - oa) / da;
      tmin = fmaxf(tmin, fminf(ta, tb));
      tmax = fminf(tmax, fmaxf(ta, tb));
    }
  }
  const float t0 = fmaxf(tmin, near_plane), t1 = fminf(tmax, far_plane);
  const bool hit = !miss && t1 > t0;
  t_mins[i] = hit ? t0 : miss_value;
  t_maxs[i] = hit ? t1 : miss_value;
  hits[i] = hit ? 1 : 0;
}

__global__ void k_occ_ema(float* __restrict__ occs, const int64_t* __restrict__ cells, const float* __restrict__ vals,
                          int64_t n, float decay) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t c = cells[i];
  if (c < 0) return;  // an unused draw of fsn_occgrid_select
  occs[c] = fmaxf(occs[c] * decay, vals[i]);
}

// ---------------------------------------------------------------- update_every_n_steps: cell selection on the device
// (run-nerf.py:288-295 -> OccGridEstimator.update_every_n_steps; round 3 chose the cells with randint / nonzero / unique /
// stack torch ops - two host syncs - and expanded the bit field to bools on every call.)  Past the warm-up an update
// re-evaluates n_uniform cells drawn uniformly (with replacement) and n_occupied cells from the OCCUPIED ones, each at
// a random point inside the cell.  The occupied half follows nerfacc's rule (OccGridEstimator.
// _sample_uniform_and_occupied_cells): a level with m <= n_occupied occupied cells takes each of them exactly once
// (draw n_uniform + q -> the q-th occupied cell in index order, q < m; the draws q >= m are the sentinel cell -1, which
// the EMA skips); only m > n_occupied draws n_occupied of them uniformly with replacement.  The draw count stays
// n_uniform + n_occupied either way and nothing is read back to the host.  Counter-based randomness (a 32-bit mixing
// hash of (seed, draw index, stream): no generator state on the device, the oracle restates it): draw i of stream k is
// r(i, k) = mix(mix(i + seed_lo) ^ (seed_hi + 0x9e3779b9 (k + 1))).
// (occ_mix / occ_rand and the draw itself, occ_draw: occ_dev.hpp, shared with the fused refresh of occ_refresh.hip.)
// exclusive prefix of the per-word popcounts of one level's bit field (n_words words): prefix[w], prefix[n_words] = total.
// One block of 1024 threads per level (block b: words b*n_words .., prefix b*(n_words+1) ..): contiguous chunks per
// thread, block scan of the chunk sums.
__global__ __launch_bounds__(1024) void k_occ_word_prefix(const uint32_t* __restrict__ bits, int n_words, int32_t* __restrict__ prefix) {
  __shared__ int32_t part[1024];
  bits += (int64_t)blockIdx.x * n_words;
  prefix += (int64_t)blockIdx.x * (n_words + 1);
  const int per = (n_words + 1023) / 1024;
  const int w0 = threadIdx.x * per, w1 = min(w0 + per, n_words);
  int32_t sum = 0;
  for (int w = w0; w < w1; ++w) sum += __popc(bits[w]);
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {  // Hillis-Steele inclusive scan
    const int32_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  int32_t run = part[threadIdx.x] - sum;
  for (int w = w0; w < w1; ++w) { prefix[w] = run; run += __popc(bits[w]); }
  if (threadIdx.x == 1023) prefix[n_words] = part[1023];
}

// draw i -> cell of level `lvl` (global index, or -1 for an unused occupied draw) and a point inside it (occ_draw).
__global__ void k_occ_select(const uint32_t* __restrict__ bits, const int32_t* __restrict__ prefix, int res, int64_t lvl_cell0,
                             int64_t n_draws, int64_t n_uniform, int all_cells, uint32_t seed_lo, uint32_t seed_hi,
                             float lox, float loy, float loz, float hix, float hiy, float hiz,
                             int64_t* __restrict__ cells, float* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_draws) return;
  const OccDraw d = occ_draw(bits, prefix, res, i, n_draws, n_uniform, all_cells, seed_lo, seed_hi, lox, loy, loz, hix, hiy, hiz);
  cells[i] = d.cell < 0 ? (int64_t)-1 : lvl_cell0 + (int64_t)d.cell;
  x[3 * i + 0] = d.x;
  x[3 * i + 1] = d.y;
  x[3 * i + 2] = d.z;
}

// EMA with duplicate cells (draws with replacement): pending[c] = max over the draws that hit c (order-preserving
// integer keys, 0 = untouched), then ONE pass over all cells applies occs = max(occs * decay, pending) and clears it.
__global__ void k_occ_scatter_max(uint32_t* __restrict__ pending, const int64_t* __restrict__ cells,
                                  const float* __restrict__ vals, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t c = cells[i];
  const float v = vals[i];
  if (c >= 0 && v == v) atomicMax(pending + c, occ_key(v));  // (NaN never enters the grid; c = -1: unused draw)
}
__global__ void k_occ_ema_pending(float* __restrict__ occs, uint32_t* __restrict__ pending, int64_t n_cells, float decay) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cells) return;
  const uint32_t k = pending[c];
  if (k == 0u) return;
  const float v = __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
  occs[c] = fmaxf(occs[c] * decay, v);
  pending[c] = 0u;
}

// bits word w = cells 32w .. 32w+31; threshold read from device memory (it is a mean computed on the device)
__global__ void k_occ_binarize(const float* __restrict__ occs, int64_t n_cells, const float* __restrict__ thre,
                               uint32_t* __restrict__ bits) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool on = c < n_cells && occs[c] > thre[0];
  const uint64_t m = __ballot(on);
  const int lane = threadIdx.x & 63;
  if (lane == 0 && c < n_cells) bits[c >> 5] = (uint32_t)m;
  if (lane == 32 && c < n_cells) bits[c >> 5] = (uint32_t)(m >> 32);
}

int launch_occ_word_prefix(const uint32_t* bits, int n_words, int levels, int32_t* prefix, hipStream_t s) {
  k_occ_word_prefix<<<(unsigned)levels, 1024, 0, s>>>(bits, n_words, prefix);
  FSN_LAUNCH_CHECK("k_occ_word_prefix");
  return FSN_OK;
}

}  // namespace fsn

using namespace fsn;

// the argument checks and the count / fill launch of both march entry points (`who` prefixes the messages; the plain
// entry point passes cone_angle 0, which the two cone checks let through)
static int occ_march_launch(const char* who, const float* rays_o, const float* rays_d, int64_t R, const float* aabb_host,
                            int res, int levels, const uint32_t* bits, float near_plane, float far_plane, float step,
                            const float* u, int max_steps, const float* t_min, const float* t_max, float cone_angle,
                            int64_t* counts, const int64_t* offsets, int64_t* ray_indices, float* t_starts, float* t_ends,
                            fsn_stream_t stream) {
  GridDev G;
  const int rc = make_grid(aabb_host, res, levels, G);
  if (rc != FSN_OK) return rc;
  FSN_REQUIRE(R >= 0 && step > 0.f && max_steps > 0, FSN_E_INVALID, "%s: bad arguments", who);
  FSN_REQUIRE(cone_angle >= 0.f, FSN_E_INVALID, "%s: cone_angle must not be negative", who);
  FSN_REQUIRE(!(cone_angle > 0.f && near_plane < 0.f), FSN_E_INVALID, "%s: the cone regime needs near_plane >= 0", who);
  if (R == 0) return FSN_OK;
  FSN_REQUIRE(rays_o && rays_d && bits, FSN_E_INVALID, "%s: null pointer", who);
  const unsigned grid = (unsigned)((R + 3) / 4);
  if (offsets) {
    FSN_REQUIRE(ray_indices && t_starts && t_ends, FSN_E_INVALID, "%s: fill pass needs the outputs", who);
    k_occ_march<true><<<grid, 256, 0, as_stream(stream)>>>(rays_o, rays_d, R, G, bits, near_plane, far_plane, step, u,
                                                           max_steps, t_min, t_max, cone_angle, nullptr, offsets,
                                                           ray_indices, t_starts, t_ends);
  } else {
    FSN_REQUIRE(counts, FSN_E_INVALID, "%s: count pass needs `counts`", who);
    k_occ_march<false><<<grid, 256, 0, as_stream(stream)>>>(rays_o, rays_d, R, G, bits, near_plane, far_plane, step, u,
                                                            max_steps, t_min, t_max, cone_angle, counts, nullptr, nullptr,
                                                            nullptr, nullptr);
  }
  FSN_LAUNCH_CHECK("k_occ_march");
  return FSN_OK;
}

extern "C" int fsn_occgrid_march(const float* rays_o, const float* rays_d, int64_t R, const float* aabb_host, int res,
                                 int levels, const uint32_t* bits, float near_plane, float far_plane, float step,
                                 const float* u, int max_steps, int64_t* counts, const int64_t* offsets,
                                 int64_t* ray_indices, float* t_starts, float* t_ends, fsn_stream_t stream) {
  return occ_march_launch("fsn_occgrid_march", rays_o, rays_d, R, aabb_host, res, levels, bits, near_plane, far_plane, step,
                          u, max_steps, nullptr, nullptr, 0.f, counts, offsets, ray_indices, t_starts, t_ends, stream);
}

extern "C" int fsn_occgrid_march_ex(const float* rays_o, const float* rays_d, int64_t R, const float* aabb_host, int res,
                                    int levels, const uint32_t* bits, float near_plane, float far_plane, float step,
                                    const float* u, int max_steps, const float* t_min, const float* t_max,
                                    float cone_angle, int64_t* counts, const int64_t* offsets, int64_t* ray_indices,
                                    float* t_starts, float* t_ends, fsn_stream_t stream) {
  return occ_march_launch("fsn_occgrid_march_ex", rays_o, rays_d, R, aabb_host, res, levels, bits, near_plane, far_plane,
                          step, u, max_steps, t_min, t_max, cone_angle, counts, offsets, ray_indices, t_starts, t_ends,
                          stream);
}

extern "C" int fsn_ray_aabb_intersect(const float* rays_o, const float* rays_d, int64_t R, const float* aabbs, int M,
                                      float near_plane, float far_plane, float miss_value, float* t_mins, float* t_maxs,
                                      uint8_t* hits, fsn_stream_t stream) {
  FSN_REQUIRE(R >= 0 && M >= 0 && R * (int64_t)M < (1ll << 40), FSN_E_INVALID, "fsn_ray_aabb_intersect: bad sizes");
  if (R == 0 || M == 0) return FSN_OK;
  FSN_REQUIRE(rays_o && rays_d && aabbs && t_mins && t_maxs && hits, FSN_E_INVALID, "fsn_ray_aabb_intersect: null pointer");
  const int64_t n = R * (int64_t)M;
  k_ray_aabb<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(rays_o, rays_d, R, aabbs, M, near_plane,
                                                                         far_plane, miss_value, t_mins, t_maxs, hits);
  FSN_LAUNCH_CHECK("k_ray_aabb");
  return FSN_OK;
}

extern "C" int fsn_occgrid_update(float* occs, int64_t n_cells, const int64_t* cells, const float* vals, int64_t n,
                                  float decay, const float* threshold_dev, uint32_t* bits, fsn_stream_t stream) {
  FSN_REQUIRE(occs && bits && n_cells > 0 && n_cells % 64 == 0 && n >= 0, FSN_E_INVALID, "fsn_occgrid_update: bad arguments");
  if (n > 0) {
    FSN_REQUIRE(cells && vals, FSN_E_INVALID, "fsn_occgrid_update: null pointer");
    k_occ_ema<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(occs, cells, vals, n, decay);
    FSN_LAUNCH_CHECK("k_occ_ema");
  }
  if (threshold_dev) {
    k_occ_binarize<<<(unsigned)((n_cells + 255) / 256), 256, 0, as_stream(stream)>>>(occs, n_cells, threshold_dev, bits);
    FSN_LAUNCH_CHECK("k_occ_binarize");
  }
  return FSN_OK;
}

extern "C" int fsn_occgrid_select(const uint32_t* bits, int res, int levels, int lvl, const float* aabb_host, int all_cells,
                                  int64_t n_uniform, int64_t n_occupied, uint64_t seed, int32_t* prefix_scratch,
                                  int64_t* cells, float* x, fsn_stream_t stream) {
  GridDev G;
  const int rc = make_grid(aabb_host, res, levels, G);
  if (rc != FSN_OK) return rc;
  FSN_REQUIRE(lvl >= 0 && lvl < levels && n_uniform >= 0 && n_occupied >= 0, FSN_E_INVALID, "fsn_occgrid_select: bad arguments");
  const int64_t res3 = (int64_t)res * res * res;
  FSN_REQUIRE(res3 % 32 == 0 && res3 < (1ll << 31), FSN_E_UNSUPPORTED, "fsn_occgrid_select: res^3 must be a multiple of 32 below 2^31");
  const int64_t n = all_cells ? res3 : n_uniform + n_occupied;
  if (n == 0) return FSN_OK;
  FSN_REQUIRE(bits && cells && x && (all_cells || n_occupied == 0 || prefix_scratch), FSN_E_INVALID, "fsn_occgrid_select: null pointer");
  hipStream_t s = as_stream(stream);
  const uint32_t* lb = bits + lvl * (res3 >> 5);
  if (!all_cells && n_occupied > 0) {
    k_occ_word_prefix<<<1, 1024, 0, s>>>(lb, (int)(res3 >> 5), prefix_scratch);
    FSN_LAUNCH_CHECK("k_occ_word_prefix");
  }
  float lo[3], hi[3];
  level_box(aabb_host, lvl, lo, hi);
  k_occ_select<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(lb, prefix_scratch, res, (int64_t)lvl * res3, n,
                                                           (!all_cells && n_occupied == 0) ? n : n_uniform, all_cells ? 1 : 0,
                                                           (uint32_t)seed, (uint32_t)(seed >> 32), lo[0], lo[1], lo[2], hi[0],
                                                           hi[1], hi[2], cells, x);
  FSN_LAUNCH_CHECK("k_occ_select");
  return FSN_OK;
}

extern "C" int fsn_occgrid_update_multi(float* occs, int64_t n_cells, uint32_t* pending, const int64_t* cells,
                                        const float* vals, int64_t n, float decay, fsn_stream_t stream) {
  FSN_REQUIRE(occs && pending && n_cells > 0 && n >= 0, FSN_E_INVALID, "fsn_occgrid_update_multi: bad arguments");
  if (n == 0) return FSN_OK;
  FSN_REQUIRE(cells && vals, FSN_E_INVALID, "fsn_occgrid_update_multi: null pointer");
  hipStream_t s = as_stream(stream);
  k_occ_scatter_max<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(pending, cells, vals, n);
  FSN_LAUNCH_CHECK("k_occ_scatter_max");
  k_occ_ema_pending<<<(unsigned)((n_cells + 255) / 256), 256, 0, s>>>(occs, pending, n_cells, decay);
  FSN_LAUNCH_CHECK("k_occ_ema_pending");
  return FSN_OK;
}

extern "C" int fsn_occgrid_apply_pending(float* occs, int64_t n_cells, uint32_t* pending, float decay, fsn_stream_t stream) {
  FSN_REQUIRE(n_cells >= 0, FSN_E_INVALID, "fsn_occgrid_apply_pending: bad arguments");
  if (n_cells == 0) return FSN_OK;
  FSN_REQUIRE(occs && pending, FSN_E_INVALID, "fsn_occgrid_apply_pending: null pointer");
  k_occ_ema_pending<<<(unsigned)((n_cells + 255) / 256), 256, 0, as_stream(stream)>>>(occs, pending, n_cells, decay);
  FSN_LAUNCH_CHECK("k_occ_ema_pending");
  return FSN_OK;
}
