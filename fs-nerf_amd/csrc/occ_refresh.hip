// occ_refresh.hip — OccGridEstimator.update_every_n_steps in one launch for all levels (run-nerf.py:288-295, which the
// reference runs under autocast): per draw the cell and the jittered point of k_occ_select (occ_dev.hpp occ_draw, the
// same counters, seeds and operation order), the density-only pass of the packed network through the tile loop of
// k_mlp_fwd in a single-pass mode, occ = sigma * step in float32, and the duplicate-safe maximum into `pending`
// (occ_key, as k_occ_scatter_max).  Points, cells and densities never go to memory; fsn_occgrid_apply_pending
// (k_occ_ema_pending) and the threshold / k_occ_binarize follow as in the unfused path.
// k_occ_refresh is fsn::VariantPlain (mlp_dev.hpp): single-pass modes only, where no variant switch applies.
#include "common.hpp"
#include "mlp_dev.hpp"
#include "mlp_layout.hpp"
#include "occ_dev.hpp"

namespace fsn {

constexpr int kOccMaxLevels = 8;  // make_grid's limit

struct OccLevel {  // 8 words per level, copied to LDS: a lane's level is not wave-uniform where two levels share a tile
  uint32_t seed_lo, seed_hi;
  float lo[3], hi[3];
};

struct OccRefreshArgs {
  NetParams net;
  const float* pos_mask;
  const uint32_t* bits;
  const int32_t* prefix;  // levels x (res^3/32 + 1), null when nothing is drawn from the occupied cells
  uint32_t* pending;
  OccLevel lv[kOccMaxLevels];
  int32_t res, levels, all_cells;
  int32_t n_draws, n_uniform;  // per level
  float step;
};

// sample source of the tile loop: this lane's point, staged in LDS by the lane that drew it
struct DrawSrc {
  const float* p;  // [x, y, z, cell] in LDS
  __device__ __forceinline__ void pos(float& x, float& y, float& z) const { x = p[0]; y = p[1]; z = p[2]; }
  __device__ __forceinline__ void dir(float& x, float& y, float& z) const { x = 0.f; y = 0.f; z = 1.f; }  // (density only: unused)
};

// Persistent workgroups over the concatenated draws of all levels (draw d = level d / n_draws, index d % n_draws), tile
// and lane layout of k_mlp_fwd: wave w owns draws tile0 + 16 NG w + l, l < 16 NG.  Lane l draws that one (cell and
// point), stages it in the wave's own LDS slots - the tile loop reads a point more than once (skip layers), and six
// registers held across it make the 256-wide instantiations spill - and lane l is also the one that holds its density
// afterwards (lanes 0-15 group 0, 16-31 group 1).  The writing lanes hold consecutive draws, so the warm-up, whose
// draw i is cell i, issues its atomics on consecutive words.  LDS: [weight ring 64 KiB][aux + masks][level table 256 B]
// [draws 128 NG x 4 words] - below k_mlp_fwd's.
template <int NT, int PREC>
__global__ __launch_bounds__(kThreads) void k_occ_refresh(OccRefreshArgs a) {
  constexpr int NG = groups_per_wave<NT, PREC>(), TILE = 128 * NG;
  __shared__ __attribute__((aligned(1024))) char smem[kRingBytes + (kAuxCapFloats + 96) * 4 + kOccMaxLevels * sizeof(OccLevel) + TILE * 16];
  float* aux_lds = reinterpret_cast<float*>(smem + kRingBytes);
  OccLevel* lv_lds = reinterpret_cast<OccLevel*>(aux_lds + kAuxCapFloats + 96);
  float* in_lds = reinterpret_cast<float*>(lv_lds + kOccMaxLevels);
  NetDev net;
  load_net(a.net, a.pos_mask, nullptr, aux_lds, net);
#pragma unroll
  for (int l = 0; l < kOccMaxLevels; ++l)
    if ((int)threadIdx.x == l) lv_lds[l] = a.lv[l];
  __syncthreads();
  const int32_t total = a.levels * a.n_draws;
  const int32_t res3 = a.res * a.res * a.res, n_words = res3 >> 5;
  const int32_t ntiles = (total + TILE - 1) / TILE;
  WStream st;
  st.init(smem, nullptr, 0, 0, a.net.blob + a.net.stream_off, (uint32_t)a.net.nph_density, 1);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  ARing ring;
  prime_ring<VariantPlain, PREC, NT>(st, ring);
  for (int32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // each wave stages (and later reads) only its own 16 NG draws: no workgroup barrier
    if (lane < 16 * NG) {
      int32_t d = tile * TILE + wave * (16 * NG) + lane;
      const bool live = d < total;
      d = live ? d : total - 1;  // (past the end: the last draw's point again, cell -1)
      const int32_t lvl = d / a.n_draws, i = d - lvl * a.n_draws;
      const OccLevel L = lv_lds[lvl];
      const int32_t* pf = a.prefix ? a.prefix + (int64_t)lvl * (n_words + 1) : nullptr;
      const OccDraw o = occ_draw(a.bits + (int64_t)lvl * n_words, pf, a.res, i, a.n_draws, a.n_uniform, a.all_cells,
                                 L.seed_lo, L.seed_hi, L.lo[0], L.lo[1], L.lo[2], L.hi[0], L.hi[1], L.hi[2]);
      const int32_t cell = (live && o.cell >= 0) ? lvl * res3 + o.cell : -1;  // global index; -1: unused draw
      f32x4 v = {o.x, o.y, o.z, __int_as_float(cell)};
      *reinterpret_cast<f32x4*>(in_lds + (wave * (16 * NG) + lane) * 4) = v;
    }
    __builtin_amdgcn_wave_barrier();
    DrawSrc src[NG];
    FSN_PER_GROUP(q, src[q] = DrawSrc{in_lds + tile_slot<NG>(wave, lane, q) * 4};);
    float sigma[NG], rgb[NG][3] = {};
    mlp_tile<VariantPlain, NT, PREC, false>(st, net, src, ring, sigma, rgb);
    if (tile_stores<NG>(lane)) {
      const float occ = sigma[tile_store_group<NG>(lane)] * a.step;  // (every lane holds every group's result)
      const int32_t cell = __float_as_int(in_lds[(wave * (16 * NG) + lane) * 4 + 3]);  // (this lane drew it)
      if (cell >= 0 && occ == occ) atomicMax(a.pending + cell, occ_key(occ));  // (NaN never enters the grid)
    }
    __builtin_amdgcn_wave_barrier();  // (the slots are rewritten for the next tile)
  }
  st.drain();
}

template <int NT, int PREC>
static int launch_occ_refresh(const OccRefreshArgs& a, int cus, hipStream_t s) {
  constexpr int TILE = 128 * groups_per_wave<NT, PREC>();
  const int64_t ntiles = ((int64_t)a.levels * a.n_draws + TILE - 1) / TILE;
  const unsigned grid = (unsigned)(ntiles < cus ? ntiles : cus);
  k_occ_refresh<NT, PREC><<<grid, kThreads, 0, s>>>(a);
  FSN_LAUNCH_CHECK("k_occ_refresh");
  return FSN_OK;
}

}  // namespace fsn

using namespace fsn;

extern "C" int fsn_occgrid_refresh(const fsn_mlp_desc* desc, int prec, const void* blob, const float* pos_mask,
                                   const uint32_t* bits, int res, int levels, const float* aabb_host, int all_cells,
                                   int64_t n_uniform, int64_t n_occupied, const uint64_t* seeds_host, float step,
                                   int32_t* prefix_scratch, uint32_t* pending, uint32_t* status, fsn_stream_t stream) {
  FSN_REQUIRE(desc && n_uniform >= 0 && n_occupied >= 0, FSN_E_INVALID, "fsn_occgrid_refresh: bad arguments");
  using Modes = PrecModes<FSN_PREC_BF16, FSN_PREC_FP16>;
  FSN_REQUIRE(prec_in(Modes{}, prec), FSN_E_UNSUPPORTED,
              "fsn_occgrid_refresh: precision mode %d (the single-pass modes FSN_PREC_FP16 / FSN_PREC_BF16)", prec);
  NetGeom G;
  const char* why;
  int rc = build_geom(*desc, prec, G, &why);
  FSN_REQUIRE(rc == FSN_OK, rc, "fsn_occgrid_refresh: %s", why);
  GridDev grid;
  rc = make_grid(aabb_host, res, levels, grid);
  if (rc != FSN_OK) return rc;
  const int64_t res3 = (int64_t)res * res * res;
  FSN_REQUIRE(res3 % 32 == 0 && res3 * levels < (1ll << 31), FSN_E_UNSUPPORTED,
              "fsn_occgrid_refresh: res^3 must be a multiple of 32 and levels * res^3 below 2^31");
  const int64_t n = all_cells ? res3 : n_uniform + n_occupied;
  FSN_REQUIRE(n * levels < (1ll << 31) - 256, FSN_E_UNSUPPORTED, "fsn_occgrid_refresh: 2^31 draws or more");  // (tile-rounded, in int32)
  if (n == 0) return FSN_OK;
  const bool from_occupied = !all_cells && n_occupied > 0;
  FSN_REQUIRE(blob && bits && seeds_host && pending && (!from_occupied || prefix_scratch), FSN_E_INVALID,
              "fsn_occgrid_refresh: null pointer");
  FSN_REQUIRE(G.aux_floats <= kAuxCapFloats, FSN_E_UNSUPPORTED, "fsn_occgrid_refresh: network too deep for the LDS aux area");
  const int cus = fsn_device_cus();
  if (cus <= 0) return FSN_E_HIP;
  OccRefreshArgs a{};
  a.net = net_params(*desc, G, blob, status);
  a.pos_mask = pos_mask;
  a.bits = bits; a.prefix = from_occupied ? prefix_scratch : nullptr; a.pending = pending;
  for (int l = 0; l < levels; ++l) {
    a.lv[l].seed_lo = (uint32_t)seeds_host[l];
    a.lv[l].seed_hi = (uint32_t)(seeds_host[l] >> 32);
    level_box(aabb_host, l, a.lv[l].lo, a.lv[l].hi);
  }
  a.res = res; a.levels = levels; a.all_cells = all_cells ? 1 : 0;
  a.n_draws = (int32_t)n;
  a.n_uniform = (int32_t)(from_occupied || all_cells ? n_uniform : n);  // (nothing from the occupied cells: all draws uniform)
  a.step = step;
  hipStream_t s = as_stream(stream);
  if (from_occupied) {
    rc = launch_occ_word_prefix(bits, (int)(res3 >> 5), levels, prefix_scratch, s);
    if (rc != FSN_OK) return rc;
  }
  return dispatch_net(Modes{}, desc->d_hidden, prec,
                      [&](auto NT, auto PREC) { return launch_occ_refresh<NT(), PREC()>(a, cus, s); });
}
