// render_occ.hip — the path the reference itself renders with (src/render/rendering.py:58-107 with nerfacc's
// OccGridEstimator in the estimator slot, src/run-nerf.py:96-98, 288-295) in ONE launch, without a host sync for the
// data-dependent sample count:
//   occupancy-grid march -> density pass (sigma_fn) -> visibility cull -> full pass (rgb_sigma_fn) -> packed volume
//   integration,
// per BATCH of rays inside a persistent workgroup.  A batch is as many whole rays as fit the LDS sample list
// (kCap samples, kMaxRays rays), pulled in chunks of up to 8 (one wave marches one ray) from a global work counter, so
// that dense and empty rays balance across the chip; a ray that no longer fits is carried into the next batch.  The
// chunk size is GUIDED (round 4): a pull takes remaining / (2 x workgroups) rays, at most 8 and at least 1, so a
// training-sized launch (4096 rays = 16 per workgroup, one dense ray = up to 8 MLP tiles) ends with single-ray pulls
// instead of 8-ray commitments - the tail of the launch is one ray's work, not one chunk's (~3.5 ms of a 3.5-ms launch
// before).  Rays are independent and integrated by one wave each: the results do not depend on the chunking.  The sample
// list, densities, keep flags, colours live in LDS; the two MLP passes run on the matrix cores over 128-sample tiles
// of the list (mlp_dev.hpp) with the weight stream running on from tile to tile and batch to batch - both kinds of
// tile stream the same blob from its first phase, a tile announces its length when it starts (WStream::begin_tile).
// HBM traffic: the rays in (or none: generated from the pose), 20 B per ray out, the bit grid through L2.
// Every sample is evaluated independently of its tile position and every ray is integrated by one wave with the
// arithmetic of the standalone kernels (occ_dev.hpp, ray_dev.hpp): the image does not depend on how batches form and is
// the unfused path's (march -> k_mlp_fwd -> k_packed_visibility -> k_mlp_fwd -> k_composite).
// The march is k_occ_march's in either regime (occ_dev.hpp: ray_range / march_ray_regime - per-ray bounds, and for
// cone_angle > 0 blocks of 64 intervals whose width grows with distance; include/fsnerf_hip.h has the definition at
// fsn_occgrid_march_ex), so every candidate carries its own interval END and nothing below assumes a common width.
#include "common.hpp"
// k_render_occ is fsn::VariantFused (mlp_dev.hpp), as k_render_fused: hand-scheduled k-loop of the x3 modes, bf16x3 on
// one accumulator.
#include "mlp_dev.hpp"
#include "occ_dev.hpp"
#include "ray_dev.hpp"

namespace fsn {

FSN_DEBUG_DEFINE_RECORD(occ)
#define FSN_DEBUG_RECORD g_dbg_occ

constexpr int kCap = 2048;      // samples of a batch (candidates; kept samples are a subset)
constexpr int kMaxRays = 128;   // rays of a batch

struct OccKArgs {
  NetParams net;
  fsn_occ_render_args a;
  GridDev G;
  float cam_hw, cam_hh, cam_f;
  int32_t use_vis;
  // fsn_render_rays_occgrid_ex: the march's regime and per-ray bounds, the slot rows of the interval ends
  float cone_angle;
  const float* t_min;
  const float* t_max;
  float* sample_t1;
};

struct OccLds {
  fsn_occ_render_args a;
  GridDev G;
  float cam_hw, cam_hh, cam_f;
  int32_t use_vis;
  float cone_angle;
  const float* t_min;
  const float* t_max;
  float* sample_t1;
  // batch state (written by thread 0 between barriers)
  int64_t chunk_base, carry_base;
  int32_t chunk_from, carry_from, chunk_take, carry_take, stop, n_cand, n_kept, n_rays;
  int32_t cnt[kWaves];
  // rays of the batch
  float rays[kMaxRays * 6];
  int64_t ray_id[kMaxRays];
  int32_t cand_off[kMaxRays], cand_cnt[kMaxRays], kept_off[kMaxRays + 1], kept_cnt[kMaxRays];
  // candidate samples (march order: sorted by ray slot, then t): interval [t0c, t1c), the ends as the march's sink
  // receives them (the cone regime's te is not bitwise ts + width)
  float t0c[kCap], sigc[kCap];
  uint16_t slotc[kCap];
  uint8_t keepf[kCap];
  // kept samples.  t1c shares sigk's storage: the ends are written by the batch's march and last read by the
  // compaction (-> t1k); sigk is written by the full pass, which follows the compaction, and read until the barrier
  // that ends the batch (the sampler mode never touches it).
  float t0k[kCap], t1k[kCap], rgbk[3 * kCap];
  union {
    float sigk[kCap];
    float t1c[kCap];
  };
  uint16_t slotk[kCap];
};

constexpr int kOccLdsBytes = kRingBytes + (kAuxCapFloats + 96) * 4 + (int)sizeof(OccLds);
static_assert(kOccLdsBytes <= 160 * 1024, "LDS budget");

// sample source: interval [t0, t1) of ray `ray`: x = o + d (t0 + t1) / 2 (rendering.py:59-61, 77-79)
struct OccSrc {
  const float* ray;
  float t0, t1;
  __device__ __forceinline__ void pos(float& x, float& y, float& z) const {
    const float tm = t0 + t1;
    x = ray[0] + ray[3] * tm / 2.0f;
    y = ray[1] + ray[4] * tm / 2.0f;
    z = ray[2] + ray[5] * tm / 2.0f;
  }
  __device__ __forceinline__ void dir(float& x, float& y, float& z) const { x = ray[3]; y = ray[4]; z = ray[5]; }
};

__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// exclusive prefix sum of an int over the 64 lanes; total to all
__device__ __forceinline__ int wave_excl_scan_i(int v, int& total) {
  const int lane = lane_id();
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  total = __shfl(inc, 63, 64);
  return inc - v;
}

// EX: the launch has a cone angle or per-ray bounds (fsn_render_rays_occgrid_ex).  Without them (EX = false) the march
// is the plain lattice's and an interval end is its start + step, computed where it is used: the code of the kernel
// before it knew the extended march - as a run-time branch with the ends always stored, the default frame was 0.5 %
// slower (tools/bench_occ_cone.py).  Both instantiations give the same uniform-regime results bit for bit.
template <int NT, int PREC, bool EX>
__global__ __launch_bounds__(kThreads) void k_render_occ(OccKArgs k) {
  __shared__ __attribute__((aligned(1024))) char smem[kOccLdsBytes];
  float* aux = reinterpret_cast<float*>(smem + kRingBytes);
  OccLds& S = *reinterpret_cast<OccLds*>(smem + kRingBytes + (kAuxCapFloats + 96) * 4);
  int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;  // (laundered per batch below: render.hip)
  if (tid == 0) {
    S.a = k.a; S.G = k.G; S.cam_hw = k.cam_hw; S.cam_hh = k.cam_hh; S.cam_f = k.cam_f; S.use_vis = k.use_vis;
    S.cone_angle = k.cone_angle; S.t_min = k.t_min; S.t_max = k.t_max; S.sample_t1 = k.sample_t1;
    S.carry_from = kWaves; S.carry_base = 0; S.carry_take = 0;
  }
  __syncthreads();
  const fsn_occ_render_args& a = S.a;
  NetDev net;
  load_net(k.net, a.pos_mask, a.dir_mask, aux, net);
  __syncthreads();
  WStream st;
  st.init(smem, nullptr, 0, 0, k.net.blob + k.net.stream_off, WStream::kDynamicPhases, 1);
  const uint32_t nph_density = (uint32_t)k.net.nph_density, nph_full = (uint32_t)k.net.nph_full;
  ARing ring;
  prime_ring<VariantFused, PREC, NT>(st, ring);

  // interval end of candidate / kept sample i
  auto cand_end = [&](int i) -> float {
    if constexpr (EX) return FSN_AT(S.t1c, i);
    else return FSN_AT(S.t0c, i) + a.step;
  };
  auto kept_end = [&](int i) -> float {
    if constexpr (EX) return FSN_AT(S.t1k, i);
    else return FSN_AT(S.t0k, i) + a.step;
  };
  // this wave's ray of a chunk -> registers (every lane holds the same values)
  auto fetch_ray = [&](int64_t ray, float (&o)[3], float (&d)[3]) {
    if (a.rays_o) {
#pragma unroll
      for (int c = 0; c < 3; ++c) { o[c] = a.rays_o[3 * ray + c]; d[c] = a.rays_d[3 * ray + c]; }
    } else {
      const int h = a.cam_row0 + (int)(ray / a.cam_W), w = (int)(ray % a.cam_W);
      pinhole_ray(a.cam_pose, S.cam_hw, S.cam_hh, S.cam_f, h, w, o, d);
    }
  };

  for (;;) {
    {
      int t_ = threadIdx.x;
      asm volatile("" : "+v"(t_));
      tid = t_; wave = __builtin_amdgcn_readfirstlane(t_ >> 6); lane = t_ & 63;
    }
    // ------------------------------------------------------------ build a batch
    if (tid == 0) { S.n_cand = 0; S.n_rays = 0; S.stop = 0; }
    __syncthreads();
    for (;;) {
      if (tid == 0) {
        if (S.carry_from < kWaves) {
          S.chunk_base = S.carry_base; S.chunk_from = S.carry_from; S.chunk_take = S.carry_take; S.carry_from = kWaves;
        } else {
          // guided chunk size from a (possibly stale) look at the queue: remaining / (2 x workgroups), 1 .. 8 rays
          unsigned long long* wc = reinterpret_cast<unsigned long long*>(a.work_counter);
          const long long seen = (long long)__hip_atomic_load(wc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          long long take = (a.R - seen) / (2ll * (long long)gridDim.x);
          take = take < 1 ? 1 : (take > kWaves ? kWaves : take);
          S.chunk_base = (int64_t)atomicAdd(wc, (unsigned long long)take);
          S.chunk_from = 0;
          S.chunk_take = (int32_t)take;
        }
      }
      __syncthreads();
      // (values read back from LDS arrive in VGPRs; these are workgroup-uniform and live across the barriers below:
      // kept scalar, they are not spilled per lane - 8-byte spill stores per lane and batch were 2 GB of scratch
      // writes per frame)
      const int64_t base = uniform_i64(S.chunk_base);
      const int from = __builtin_amdgcn_readfirstlane(S.chunk_from), take = __builtin_amdgcn_readfirstlane(S.chunk_take);
      if (base >= a.R) break;  // (workgroup-uniform: read from LDS)
      const int64_t ray = base + wave;
      const bool active = wave >= from && wave < take && ray < a.R;
      float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 1.f};
      RayLattice L;
      L.any = false; L.near_r = L.t_lo = L.t_hi = 0.f; L.k0 = 0;
      int c = 0;
      // (EX: the march of occ_dev.hpp in either regime, as k_occ_march runs it: count here, fill below)
      const float cone = EX ? S.cone_angle : 0.f;
      float u_r = 0.f;
      if (active) {
        fetch_ray(ray, o, d);
        u_r = a.u ? a.u[ray] : 0.f;
        if constexpr (EX) {
          const float lo_r = S.t_min ? S.t_min[ray] : -__builtin_huge_valf(), hi_r = S.t_max ? S.t_max[ray] : __builtin_huge_valf();
          L = ray_range(S.G, o, d, a.near_plane, a.far_plane, a.step, cone, a.u != nullptr, u_r, lo_r, hi_r);
          c = march_ray_regime(S.G, a.bits, o, d, L, a.step, cone, a.u != nullptr, u_r, a.max_steps,
                               [](float, float, bool, uint64_t, int) {});
        } else {
          L = ray_lattice(S.G, o, d, a.near_plane, a.far_plane, a.step, a.u != nullptr, u_r);
          c = march_ray(S.G, a.bits, o, d, L, a.step, a.max_steps, [](float, float, bool, uint64_t, int) {});
        }
      }
      if (lane == 0) FSN_AT(S.cnt, wave) = active ? c : -1;
      __syncthreads();
      // accept the chunk's rays in order while they fit (every thread evaluates the same recurrence)
      int nc = S.n_cand, nr = S.n_rays, my_off = -1, my_slot = 0, first_rej = kWaves;
      bool stop = false;
      for (int w = from; w < kWaves; ++w) {
        const int cw = FSN_AT(S.cnt, w);
        if (cw < 0) continue;
        if (!stop && nr < kMaxRays && nc + cw <= kCap) {
          if (w == wave) { my_off = nc; my_slot = nr; }
          nc += cw;
          nr += 1;
        } else if (!stop) {
          stop = true;
          first_rej = w;
        }
      }
      __syncthreads();
      if (tid == 0) {
        S.n_cand = nc; S.n_rays = nr;
        if (stop) { S.carry_base = base; S.carry_from = first_rej; S.carry_take = take; S.stop = 1; }
        else if (take < kWaves) S.stop = 1;  // the queue is running out: this (small) chunk is the whole batch
      }
      if (my_off >= 0) {
        if (lane == 0) {
#pragma unroll
          for (int q = 0; q < 3; ++q) { FSN_AT(S.rays, 6 * my_slot + q) = o[q]; FSN_AT(S.rays, 6 * my_slot + 3 + q) = d[q]; }
          FSN_AT(S.ray_id, my_slot) = ray;
          FSN_AT(S.cand_off, my_slot) = my_off;
          FSN_AT(S.cand_cnt, my_slot) = c;
        }
        auto fill = [&](float ts, float te, bool keep, uint64_t m, int before) {
          if (keep) {
            const int pos = my_off + before + __popcll(m & ((1ull << lane) - 1ull));
            FSN_AT(S.t0c, pos) = ts;
            if constexpr (EX) FSN_AT(S.t1c, pos) = te;
            FSN_AT(S.slotc, pos) = (uint16_t)my_slot;
          }
        };
        if constexpr (EX) march_ray_regime(S.G, a.bits, o, d, L, a.step, cone, a.u != nullptr, u_r, a.max_steps, fill);
        else march_ray(S.G, a.bits, o, d, L, a.step, a.max_steps, fill);
      }
      __syncthreads();
      if (S.stop) break;
    }
    const int n_rays = __builtin_amdgcn_readfirstlane(S.n_rays), n_cand = __builtin_amdgcn_readfirstlane(S.n_cand);
    if (n_rays == 0) break;  // no ray left for this workgroup (uniform)

    // ------------------------------------------------------------ density pass + visibility (estimator.sampling)
    // (single-pass modes of 256-wide networks: 256-sample tiles, two sample groups per wave sharing every A operand -
    // mlp_tile with NG = 2, the arithmetic per sample is that of NG = 1; this is what the opt-in bf16 visibility cull runs)
    constexpr int NG = groups_per_wave<NT, PREC>(), TILE = 128 * NG;
    if (S.use_vis && n_cand > 0) {
      for (int sub = 0; sub * TILE < n_cand; ++sub) {
        // slot of this lane's sample in group 0 (group 1: 16 further); past the end the last sample again
        const int idx0 = sub * TILE + tile_slot<NG>(wave, lane, 0);
        OccSrc src[NG];
        FSN_PER_GROUP(q, const int ic = min(idx0 + 16 * q, n_cand - 1);
                            src[q] = OccSrc{FSN_SPAN(S.rays, 6 * FSN_AT(S.slotc, ic), 6), FSN_AT(S.t0c, ic), cand_end(ic)};);
        float sigma[NG], rgb[NG][3];
        st.begin_tile(nph_density);
        mlp_tile<VariantFused, NT, PREC, false>(st, net, src, ring, sigma, rgb);
        if (tile_stores<NG>(lane)) {
          const int qs = tile_store_group<NG>(lane), idx = idx0 + 16 * qs;  // (the sample this lane stores)
          if (idx < n_cand) FSN_AT(S.sigc, idx) = sigma[qs];
        }
      }
      lds_barrier();
      // keep flags per ray: k_packed_visibility's rule on the same walk (trans_walk, ray_dev.hpp), one wave per ray
      for (int r = wave; r < n_rays; r += kWaves) {
        const int Sn = FSN_AT(S.cand_cnt, r), beg = FSN_AT(S.cand_off, r);
        int i0, i1;
        lane_range(Sn, lane, i0, i1);
        int nk = 0;
        trans_walk(i0, i1, [&](int i) { return FSN_AT(S.sigc, beg + i) * (cand_end(beg + i) - FSN_AT(S.t0c, beg + i)); },
                   [&](int i, float T, float e) {
                     const bool kp = T >= a.early_stop_eps && 1.0f - e >= a.alpha_thre;
                     FSN_AT(S.keepf, beg + i) = kp ? 1 : 0;
                     nk += kp ? 1 : 0;
                   });
        int tk;
        wave_excl_scan_i(nk, tk);
        if (lane == 0) FSN_AT(S.kept_cnt, r) = tk;
      }
    } else {
      for (int i = tid; i < n_cand; i += kThreads) FSN_AT(S.keepf, i) = 1;
      for (int r = tid; r < n_rays; r += kThreads) FSN_AT(S.kept_cnt, r) = FSN_AT(S.cand_cnt, r);
    }
    lds_barrier();
    if (wave == 0) {  // exclusive scan of the kept counts over the batch's rays (<= 128: two per lane)
      const int c0 = 2 * lane < n_rays ? FSN_AT(S.kept_cnt, 2 * lane) : 0, c1 = 2 * lane + 1 < n_rays ? FSN_AT(S.kept_cnt, 2 * lane + 1) : 0;
      int tot;
      const int ex = wave_excl_scan_i(c0 + c1, tot);
      if (2 * lane < n_rays) FSN_AT(S.kept_off, 2 * lane) = ex;
      if (2 * lane + 1 < n_rays) FSN_AT(S.kept_off, 2 * lane + 1) = ex + c0;
      if (lane == 0) S.n_kept = tot;
    }
    lds_barrier();
    for (int r = wave; r < n_rays; r += kWaves) {  // compaction, order preserved
      const int Sn = FSN_AT(S.cand_cnt, r), beg = FSN_AT(S.cand_off, r), ko = FSN_AT(S.kept_off, r);
      const int per = (Sn + 63) >> 6;
      const int i0 = lane * per, i1 = min(i0 + per, Sn);
      int nk = 0;
      for (int i = i0; i < i1; ++i) nk += FSN_AT(S.keepf, beg + i);
      int tk;
      int pos = ko + wave_excl_scan_i(nk, tk);
      for (int i = i0; i < i1; ++i) {
        if (FSN_AT(S.keepf, beg + i)) {
          FSN_AT(S.t0k, pos) = FSN_AT(S.t0c, beg + i);
          FSN_AT(S.t1k, pos) = cand_end(beg + i);
          FSN_AT(S.slotk, pos) = (uint16_t)r;
          ++pos;
        }
      }
    }
    lds_barrier();
    if (a.sample_t0 && !a.ex_weights) {  // sampler mode: the kept samples are the result
      for (int r = wave; r < n_rays; r += kWaves) {
        const int64_t ray = FSN_AT(S.ray_id, r);
        const int ko = FSN_AT(S.kept_off, r), Sk = FSN_AT(S.kept_cnt, r);
        for (int i = lane; i < Sk; i += 64) a.sample_t0[ray * a.sample_cap + i] = FSN_AT(S.t0k, ko + i);
        if constexpr (EX)
          if (S.sample_t1)  // (cone regime: the ends are not t0 + step)
            for (int i = lane; i < Sk; i += 64) S.sample_t1[ray * a.sample_cap + i] = FSN_AT(S.t1k, ko + i);
        if (lane == 0) {
          if (a.n_cand) a.n_cand[ray] = FSN_AT(S.cand_cnt, r);
          a.n_kept[ray] = Sk;
        }
      }
      lds_barrier();
      continue;
    }
    // ------------------------------------------------------------ full pass (rgb_sigma_fn) + packed integration
    const int n_kept = __builtin_amdgcn_readfirstlane(S.n_kept);
    for (int sub = 0; sub * TILE < n_kept; ++sub) {
      // slot of this lane's sample in group 0 (group 1: 16 further); past the end the last sample again
      const int idx0 = sub * TILE + tile_slot<NG>(wave, lane, 0);
      OccSrc src[NG];
      FSN_PER_GROUP(q, const int ic = min(idx0 + 16 * q, n_kept - 1);
                       src[q] = OccSrc{FSN_SPAN(S.rays, 6 * FSN_AT(S.slotk, ic), 6), FSN_AT(S.t0k, ic), kept_end(ic)};);
      float sigma[NG], rgb[NG][3];
      st.begin_tile(nph_full);
      mlp_tile<VariantFused, NT, PREC, true>(st, net, src, ring, sigma, rgb);
      if (tile_stores<NG>(lane)) {
        const int qs = tile_store_group<NG>(lane), idx = idx0 + 16 * qs;
        if (idx < n_kept) {
          FSN_AT(S.sigk, idx) = sigma[qs];
          FSN_AT(S.rgbk, 3 * idx + 0) = rgb[qs][0];
          FSN_AT(S.rgbk, 3 * idx + 1) = rgb[qs][1];
          FSN_AT(S.rgbk, 3 * idx + 2) = rgb[qs][2];
        }
      }
    }
    lds_barrier();
    for (int r = wave; r < n_rays; r += kWaves) {
      const int64_t ray = FSN_AT(S.ray_id, r);
      const int ko = FSN_AT(S.kept_off, r), Sk = FSN_AT(S.kept_cnt, r);
      // (EXTRAS mode: the per-sample weights / alphas / trans go straight into the ray's slot row)
      const int64_t row = a.ex_weights ? ray * a.sample_cap : 0;
      CompositeOut o{a.colors + 3 * ray, a.opacity + ray, a.depth + ray, a.ex_weights ? a.ex_weights + row : nullptr,
                     a.ex_weights ? a.ex_alphas + row : nullptr, a.ex_weights ? a.ex_trans + row : nullptr};
      composite_ray(FSN_SPAN(S.sigk, ko, Sk), FSN_SPAN(S.rgbk, 3 * ko, 3 * Sk), FSN_SPAN(S.t0k, ko, Sk), FSN_SPAN(S.t1k, ko, Sk), Sk,
                    true, a.bkgd[0], a.bkgd[1], a.bkgd[2], o);
      if (a.ex_weights) {
        for (int i = lane; i < Sk; i += 64) {
          a.sample_t0[row + i] = FSN_AT(S.t0k, ko + i);
          a.ex_sigmas[row + i] = FSN_AT(S.sigk, ko + i);
        }
        if constexpr (EX)
          if (S.sample_t1)
            for (int i = lane; i < Sk; i += 64) S.sample_t1[row + i] = FSN_AT(S.t1k, ko + i);
        for (int i = lane; i < 3 * Sk; i += 64) a.ex_rgbs[3 * row + i] = FSN_AT(S.rgbk, 3 * ko + i);
      }
      if (lane == 0) {
        if (a.n_cand) a.n_cand[ray] = FSN_AT(S.cand_cnt, r);
        if (a.n_kept) a.n_kept[ray] = Sk;
      }
    }
    lds_barrier();
  }
  st.drain();
}

template <int NT, int PREC>
static int launch_occ(const OccKArgs& k, int cus, hipStream_t s) {
  const int64_t chunks = (k.a.R + kWaves - 1) / kWaves;
  const unsigned grid = (unsigned)(chunks < cus ? chunks : cus);
  // (sample_t1 alone - end rows asked for in the uniform regime without bounds - is served by the extended kernel too)
  if (k.cone_angle > 0.f || k.t_min || k.t_max || k.sample_t1) k_render_occ<NT, PREC, true><<<grid, kThreads, 0, s>>>(k);
  else k_render_occ<NT, PREC, false><<<grid, kThreads, 0, s>>>(k);
  FSN_LAUNCH_CHECK("k_render_occ");
  return FSN_OK;
}

}  // namespace fsn

using namespace fsn;

// the argument checks and the launch of both render entry points (`who` prefixes the messages; the plain entry point
// passes cone_angle 0 and no bounds / end rows, which the new checks let through)
static int occ_render_launch(const char* who, const fsn_mlp_desc* desc, int prec, const void* blob,
                             const fsn_occ_render_args* args, float cone_angle, const float* t_min, const float* t_max,
                             float* sample_t1, fsn_stream_t stream) {
  FSN_REQUIRE(desc && args, FSN_E_INVALID, "%s: null pointer", who);
  const fsn_occ_render_args& a = *args;
  FSN_REQUIRE(a.R >= 0 && a.step > 0.f && a.max_steps > 0, FSN_E_INVALID, "%s: bad sizes", who);
  FSN_REQUIRE(cone_angle >= 0.f, FSN_E_INVALID, "%s: cone_angle must not be negative", who);
  FSN_REQUIRE(!(cone_angle > 0.f && a.near_plane < 0.f), FSN_E_INVALID, "%s: the cone regime needs near_plane >= 0", who);
  using Modes = PrecModes<FSN_PREC_BF16X3, FSN_PREC_BF16, FSN_PREC_FP16X3, FSN_PREC_FP16, FSN_PREC_FP16X3U>;
  FSN_REQUIRE(prec_in(Modes{}, prec), FSN_E_UNSUPPORTED, "%s: precision mode %d", who, prec);
  NetGeom G;
  const char* why;
  int rc = build_geom(*desc, prec, G, &why);
  FSN_REQUIRE(rc == FSN_OK, rc, "%s: %s", who, why);
  OccKArgs k;
  rc = make_grid(a.aabb, a.res, a.levels, k.G);
  if (rc != FSN_OK) return rc;
  if (a.R == 0) return FSN_OK;
  FSN_REQUIRE(a.rays_o || !(t_min || t_max), FSN_E_INVALID, "%s: per-ray t_min / t_max need ray arrays, not a camera", who);
  FSN_REQUIRE(!(cone_angle > 0.f && a.sample_t0 && !sample_t1), FSN_E_INVALID,
              "%s: the sampler / extras mode in the cone regime needs sample_t1", who);
  FSN_REQUIRE(blob && a.bits && a.work_counter, FSN_E_INVALID, "%s: null pointer", who);
  if (a.ex_weights)
    FSN_REQUIRE(a.sample_t0 && a.ex_alphas && a.ex_trans && a.ex_sigmas && a.ex_rgbs && a.colors && a.opacity && a.depth,
                FSN_E_INVALID, "%s: the extras mode needs sample_t0, all five ex_* arrays and the per-ray outputs", who);
  if (a.sample_t0) {
    FSN_REQUIRE(a.n_kept && a.sample_cap >= a.max_steps, FSN_E_INVALID,
                "%s: the sampler / extras mode needs n_kept and sample_cap >= max_steps", who);
  } else {
    FSN_REQUIRE(a.colors && a.opacity && a.depth, FSN_E_INVALID, "%s: null output pointer", who);
  }
  FSN_REQUIRE(a.max_steps <= kCap, FSN_E_UNSUPPORTED, "%s: max_steps %d > %d samples of one ray group (use the unfused path)",
              who, a.max_steps, kCap);
  if (a.rays_o) {
    FSN_REQUIRE(a.rays_d, FSN_E_INVALID, "%s: rays_o without rays_d", who);
  } else {
    FSN_REQUIRE(a.cam_H > 0 && a.cam_W > 0 && a.cam_focal > 0 && a.cam_row0 >= 0 &&
                    a.R <= (int64_t)(a.cam_H - a.cam_row0) * a.cam_W,
                FSN_E_INVALID, "%s: no rays and no valid camera", who);
  }
  FSN_REQUIRE(G.aux_floats <= kAuxCapFloats, FSN_E_UNSUPPORTED, "%s: network too deep for LDS", who);
  // WStream::begin_tile: a tile starts with kLook + 1 of its phases staged.  build_geom's smallest density pass
  // (2 layers x 128, no skip, single pass) has exactly 3.
  FSN_REQUIRE(G.nph_density >= kLook + 1, FSN_E_UNSUPPORTED, "%s: a pass of %d phases is shorter than the weight stream's look-ahead",
              who, G.nph_density);
  k.net = net_params(*desc, G, blob, a.status);
  k.a = a;
  k.cam_hw = (float)(a.cam_W * 0.5);
  k.cam_hh = (float)(a.cam_H * 0.5);
  k.cam_f = (float)a.cam_focal;
  k.use_vis = (a.early_stop_eps > 0.f || a.alpha_thre > 0.f) ? 1 : 0;
  k.cone_angle = cone_angle;
  k.t_min = t_min;
  k.t_max = t_max;
  k.sample_t1 = a.sample_t0 ? sample_t1 : nullptr;  // (the end rows belong to the sampler / extras mode)
  const int cus = fsn_device_cus();
  if (cus <= 0) return FSN_E_HIP;
  hipStream_t s = as_stream(stream);
  FSN_HIP(hipMemsetAsync(a.work_counter, 0, sizeof(unsigned long long), s));
  return dispatch_net(Modes{}, desc->d_hidden, prec, [&](auto NT, auto PREC) { return launch_occ<NT(), PREC()>(k, cus, s); });
}

extern "C" int fsn_render_rays_occgrid(const fsn_mlp_desc* desc, int prec, const void* blob,
                                       const fsn_occ_render_args* args, fsn_stream_t stream) {
  return occ_render_launch("fsn_render_rays_occgrid", desc, prec, blob, args, 0.f, nullptr, nullptr, nullptr, stream);
}

extern "C" int fsn_render_rays_occgrid_ex(const fsn_mlp_desc* desc, int prec, const void* blob,
                                          const fsn_occ_render_args* args, float cone_angle, const float* t_min,
                                          const float* t_max, float* sample_t1, fsn_stream_t stream) {
  return occ_render_launch("fsn_render_rays_occgrid_ex", desc, prec, blob, args, cone_angle, t_min, t_max, sample_t1, stream);
}

namespace fsn {
struct GatherEx {  // EXTRAS mode: slot rows -> packed arrays (weights, alphas, trans, sigmas; rgbs x3), or all null
  const float* slot[5];
  float* out[5];
};
// (t1s: the cone regime's end rows, or null: t_end = t_start + step)
__global__ void k_occ_gather(const int32_t* __restrict__ n_kept, const int64_t* __restrict__ offsets,
                             const float* __restrict__ t0s, const float* __restrict__ t1s, int cap, int64_t R, float step,
                             int64_t* __restrict__ ri, float* __restrict__ ts, float* __restrict__ te, GatherEx ex) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + wave;
  if (r >= R) return;
  const int n = n_kept[r];
  const int64_t off = offsets[r];
  for (int i = lane; i < n; i += 64) {
    const float t = t0s[r * cap + i];
    ri[off + i] = r;
    ts[off + i] = t;
    te[off + i] = t1s ? t1s[r * cap + i] : t + step;
  }
  if (ex.slot[0]) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      for (int i = lane; i < n; i += 64) ex.out[k][off + i] = ex.slot[k][r * cap + i];
    for (int i = lane; i < 3 * n; i += 64) ex.out[4][3 * off + i] = ex.slot[4][3 * r * cap + i];
  }
}
}  // namespace fsn

// the checks and the launch of the three gather entry points (`slots` / `out` both null: samples only)
static int occ_gather_launch(const char* who, const int32_t* n_kept, const int64_t* offsets, const float* sample_t0,
                             const float* sample_t1, int sample_cap, int64_t R, float step, int64_t* ray_indices,
                             float* t_starts, float* t_ends, bool extras, const float* const* slots, float* const* out,
                             fsn_stream_t stream) {
  FSN_REQUIRE(R >= 0 && sample_cap > 0, FSN_E_INVALID, "%s: bad sizes", who);
  if (R == 0) return FSN_OK;
  FSN_REQUIRE(n_kept && offsets && sample_t0 && ray_indices && t_starts && t_ends && (!extras || (slots && out)),
              FSN_E_INVALID, "%s: null pointer", who);
  GatherEx ex{};
  if (extras)
    for (int k = 0; k < 5; ++k) {
      FSN_REQUIRE(slots[k] && out[k], FSN_E_INVALID, "%s: null slot / output array %d", who, k);
      ex.slot[k] = slots[k];
      ex.out[k] = out[k];
    }
  k_occ_gather<<<(unsigned)((R + 3) / 4), 256, 0, as_stream(stream)>>>(n_kept, offsets, sample_t0, sample_t1, sample_cap, R,
                                                                       step, ray_indices, t_starts, t_ends, ex);
  FSN_LAUNCH_CHECK("k_occ_gather");
  return FSN_OK;
}

extern "C" int fsn_occ_gather_samples(const int32_t* n_kept, const int64_t* offsets, const float* sample_t0, int sample_cap,
                                      int64_t R, float step, int64_t* ray_indices, float* t_starts, float* t_ends,
                                      fsn_stream_t stream) {
  return occ_gather_launch("fsn_occ_gather_samples", n_kept, offsets, sample_t0, nullptr, sample_cap, R, step, ray_indices,
                           t_starts, t_ends, false, nullptr, nullptr, stream);
}

extern "C" int fsn_occ_gather_extras(const int32_t* n_kept, const int64_t* offsets, const float* sample_t0, int sample_cap,
                                     int64_t R, float step, int64_t* ray_indices, float* t_starts, float* t_ends,
                                     const float* const* slots, float* const* out, fsn_stream_t stream) {
  return occ_gather_launch("fsn_occ_gather_extras", n_kept, offsets, sample_t0, nullptr, sample_cap, R, step, ray_indices,
                           t_starts, t_ends, true, slots, out, stream);
}

extern "C" int fsn_occ_gather_ex(const int32_t* n_kept, const int64_t* offsets, const float* sample_t0,
                                 const float* sample_t1, int sample_cap, int64_t R, float step, int64_t* ray_indices,
                                 float* t_starts, float* t_ends, const float* const* slots, float* const* out,
                                 fsn_stream_t stream) {
  FSN_REQUIRE(!slots == !out, FSN_E_INVALID, "fsn_occ_gather_ex: slots and outputs come together");
  return occ_gather_launch("fsn_occ_gather_ex", n_kept, offsets, sample_t0, sample_t1, sample_cap, R, step, ray_indices,
                           t_starts, t_ends, slots != nullptr, slots, out, stream);
}
