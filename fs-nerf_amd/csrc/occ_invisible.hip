// occ_invisible.hip — OccGridEstimator.mark_invisible_cells: the cells no training camera sees leave the grid for good.
// nerfacc's source is not part of the reference; nerfacc tests ONE lattice point per cell, which can remove cells that
// rays do cross.  A removed cell is a permanent hole in this grid, so the rule here is a conservative frustum / box
// test, and it is THIS build's definition (tests/occ_invisible_ref.py restates it in NumPy float32,
// operation for operation - the library is built without floating-point contraction):
//
//  * cell box: level l's box [lo, hi] (level_box's arithmetic: double, rounded once), cell width w_a = (hi_a - lo_a) /
//    res, cell (ix, iy, iz) = [lo + i w, lo + (i + 1) w] per axis; its centre is the mean of the two ends.
//  * camera (16 floats): world -> camera map m[0..11] (row major [3,4]; camera x right, y down, z = depth forward), then
//    fx, fy, cx, cy.  A point p has X = ((m0 x + m1 y) + m2 z) + m3 (Y, D alike) and five margins
//      g0 = D - near_plane, g1 = fx X + cx D, g2 = (W - cx) D - fx X, g3 = fy Y + cy D, g4 = (H - cy) D - fy Y.
//  * a camera COVERS a cell unless, for one of the five margins, all 8 corners are negative (the plane cull: it never
//    drops a cell the frustum intersects); a cell is TOO NEAR a camera when its centre has g1..g4 >= 0 and
//    0 <= D < near_plane.  visible = (covering cameras >= min_views) and too near to none.
//  * NDC grids (the reference's LLFF path, to_ndc with the given near): the box is clipped to z' <= 1 - 1e-6 (a cell
//    with nothing left is invisible: it holds no real point), and the 8 corners and the centre of the clipped box go
//    back to scene space first, z = 2 near / (z' - 1), x = ((-x') z) wf, y = ((-y') z) hf with wf = W / (2 f),
//    hf = H / (2 f).  The map is projective and every kept point has z < 0, so the preimage of the box is the convex
//    hull of those corners and the cull stays conservative.
//
// The masked end of an update (fsn_occgrid_update_masked) keeps nerfacc's convention occs == -1 at the invisible cells
// (the EMA kernels write max(-0.95, occ) there), takes the threshold from the VISIBLE cells only and never sets an
// invisible cell's bit: two launches, no host synchronisation, the sum in a fixed order.
#include "common.hpp"
#include "occ_dev.hpp"

namespace fsn {

struct VisArgs {
  float w, h, near_plane;     // image size, near plane (depth along the optical axis)
  int32_t n_cams, min_views;
  int32_t ndc;                // the grid lives in NDC space
  float ndc_wf, ndc_hf, ndc_near;
};

// one wave per 64 consecutive cells; the camera loop is wave-uniform (cams is read through a uniform address)
__global__ __launch_bounds__(256) void k_occ_visibility(GridDev G, int64_t n_cells, const float* __restrict__ cams,
                                                         VisArgs A, uint32_t* __restrict__ visible) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool vis = false;
  if (c < n_cells) {
    const int64_t res = G.res, res3 = res * res * res;
    const int l = (int)(c / res3);
    const int64_t q = c - (int64_t)l * res3;
    const int idx[3] = {(int)(q / (res * res)), (int)((q / res) % res), (int)(q % res)};
    float e[3][2];  // the two ends of the cell per axis
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double cd = ((double)G.amin[a] + (double)G.amax[a]) / 2.0;  // level_box
      const double hd = ((double)G.amax[a] - (double)G.amin[a]) / 2.0 * (double)(1 << l);
      const float lo = (float)(cd - hd), hi = (float)(cd + hd);
      const float w = (hi - lo) / (float)G.res;
      e[a][0] = lo + (float)idx[a] * w;
      e[a][1] = lo + (float)(idx[a] + 1) * w;
    }
    bool any_left = true;
    if (A.ndc) {
      const float zmax = 1.0f - 1e-6f;
      any_left = e[2][0] <= zmax;
      e[2][1] = fminf(e[2][1], zmax);
    }
    if (any_left) {
      float p[9][3];  // 8 corners (bit 2: x end, bit 1: y end, bit 0: z end), then the centre
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        p[k][0] = e[0][(k >> 2) & 1];
        p[k][1] = e[1][(k >> 1) & 1];
        p[k][2] = e[2][k & 1];
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) p[8][a] = (e[a][0] + e[a][1]) / 2.0f;
      if (A.ndc) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const float z = (2.0f * A.ndc_near) / (p[k][2] - 1.0f);
          p[k][0] = ((-p[k][0]) * z) * A.ndc_wf;
          p[k][1] = ((-p[k][1]) * z) * A.ndc_hf;
          p[k][2] = z;
        }
      }
      int covering = 0;
      bool too_near = false;
      for (int n = 0; n < A.n_cams; ++n) {
        const float* __restrict__ m = cams + 16 * (int64_t)n;
        const float fx = m[12], fy = m[13], cx = m[14], cy = m[15];
        const float wx = A.w - cx, hy = A.h - cy;
        bool neg0 = true, neg1 = true, neg2 = true, neg3 = true, neg4 = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const float X = ((m[0] * p[k][0] + m[1] * p[k][1]) + m[2] * p[k][2]) + m[3];
          const float Y = ((m[4] * p[k][0] + m[5] * p[k][1]) + m[6] * p[k][2]) + m[7];
          const float D = ((m[8] * p[k][0] + m[9] * p[k][1]) + m[10] * p[k][2]) + m[11];
          const float g0 = D - A.near_plane;
          const float g1 = fx * X + cx * D;
          const float g2 = wx * D - fx * X;
          const float g3 = fy * Y + cy * D;
          const float g4 = hy * D - fy * Y;
          if (k < 8) {
            neg0 = neg0 && g0 < 0.0f;
            neg1 = neg1 && g1 < 0.0f;
            neg2 = neg2 && g2 < 0.0f;
            neg3 = neg3 && g3 < 0.0f;
            neg4 = neg4 && g4 < 0.0f;
          } else {
            too_near = too_near || (g1 >= 0.0f && g2 >= 0.0f && g3 >= 0.0f && g4 >= 0.0f && D >= 0.0f && D < A.near_plane);
          }
        }
        covering += (neg0 || neg1 || neg2 || neg3 || neg4) ? 0 : 1;
      }
      vis = covering >= A.min_views && !too_near;
    }
  }
  const uint64_t mk = __ballot(vis);
  if (lane == 0 && c < n_cells) visible[c >> 5] = (uint32_t)mk;
  if (lane == 32 && c < n_cells) visible[c >> 5] = (uint32_t)(mk >> 32);
}

// ---------------------------------------------------------------- the masked end of an update
constexpr int MASK_BLOCKS = 1024;  // partial sums: scratch holds 2 * MASK_BLOCKS doubles (sums, then counts)

// sum over the 256 threads of a block, in a fixed order; every thread gets it
__device__ __forceinline__ double block_sum_256(double v, double* sh) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();  // (sh may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// pass 1: occs = -1 at the invisible cells (revive: a visible cell still holding -1 from an earlier mask restarts at
// 0); per block the sum and the count of the visible cells' occs.
__global__ __launch_bounds__(256) void k_occ_mask_reduce(float* __restrict__ occs, const uint32_t* __restrict__ visible,
                                                          int64_t n_cells, int revive, double* __restrict__ partial) {
  __shared__ double sh[4];
  double sum = 0.0, cnt = 0.0;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n_cells; c += (int64_t)gridDim.x * 256) {
    const bool vis = (visible[c >> 5] >> (c & 31)) & 1u;
    float v = occs[c];
    if (!vis) {
      if (v != -1.0f) occs[c] = -1.0f;
    } else {
      if (revive && v == -1.0f) { v = 0.0f; occs[c] = v; }
      sum += (double)v;
      cnt += 1.0;
    }
  }
  sum = block_sum_256(sum, sh);
  cnt = block_sum_256(cnt, sh);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = sum;
    partial[MASK_BLOCKS + blockIdx.x] = cnt;
  }
}

// pass 2: threshold = min(mean of occs over the visible cells, occ_thre) (no visible cell: occ_thre), every block sums
// the partials in the same order; bits = (occs > threshold) & visible, a wave per 64 cells as in k_occ_binarize.
__global__ __launch_bounds__(256) void k_occ_mask_binarize(const float* __restrict__ occs, const uint32_t* __restrict__ visible,
                                                            int64_t n_cells, const double* __restrict__ partial,
                                                            int n_partial, float occ_thre, uint32_t* __restrict__ bits) {
  __shared__ double sh[4];
  double sum = 0.0, cnt = 0.0;
  for (int i = threadIdx.x; i < n_partial; i += 256) {
    sum += partial[i];
    cnt += partial[MASK_BLOCKS + i];
  }
  sum = block_sum_256(sum, sh);
  cnt = block_sum_256(cnt, sh);
  const float thr = cnt > 0.0 ? fminf((float)(sum / cnt), occ_thre) : occ_thre;
  const int lane = threadIdx.x & 63;
  // (n_cells % 64 == 0: a wave is inside the grid or outside it as a whole)
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n_cells; c += (int64_t)gridDim.x * 256) {
    const bool on = occs[c] > thr;
    const uint64_t m = __ballot(on);
    if (lane == 0) bits[c >> 5] = (uint32_t)m & visible[c >> 5];
    if (lane == 32) bits[c >> 5] = (uint32_t)(m >> 32) & visible[c >> 5];
  }
}

}  // namespace fsn

using namespace fsn;

extern "C" int fsn_occgrid_visibility(const float* aabb_host, int res, int levels, const float* cams, int n_cams, int width,
                                      int height, float near_plane, int min_views, int ndc, float ndc_wf, float ndc_hf,
                                      float ndc_near, uint32_t* visible, fsn_stream_t stream) {
  GridDev G;
  const int rc = make_grid(aabb_host, res, levels, G);
  if (rc != FSN_OK) return rc;
  const int64_t n_cells = (int64_t)levels * res * res * res;
  FSN_REQUIRE(n_cells % 64 == 0, FSN_E_INVALID, "fsn_occgrid_visibility: levels * res^3 must be a multiple of 64");
  FSN_REQUIRE(cams && visible, FSN_E_INVALID, "fsn_occgrid_visibility: null pointer");
  FSN_REQUIRE(n_cams >= 1, FSN_E_INVALID, "fsn_occgrid_visibility: needs at least one camera");
  FSN_REQUIRE(min_views >= 1, FSN_E_INVALID, "fsn_occgrid_visibility: min_views must be at least 1");
  FSN_REQUIRE(near_plane >= 0.f, FSN_E_INVALID, "fsn_occgrid_visibility: near_plane must not be negative");
  FSN_REQUIRE(width > 0 && height > 0, FSN_E_INVALID, "fsn_occgrid_visibility: the image size must be positive");
  FSN_REQUIRE(!ndc || (ndc_wf > 0.f && ndc_hf > 0.f && ndc_near > 0.f), FSN_E_INVALID,
              "fsn_occgrid_visibility: an NDC grid needs W/2f, H/2f and near > 0");
  VisArgs A;
  A.w = (float)width; A.h = (float)height; A.near_plane = near_plane;
  A.n_cams = n_cams; A.min_views = min_views;
  A.ndc = ndc ? 1 : 0; A.ndc_wf = ndc_wf; A.ndc_hf = ndc_hf; A.ndc_near = ndc_near;
  k_occ_visibility<<<(unsigned)((n_cells + 255) / 256), 256, 0, as_stream(stream)>>>(G, n_cells, cams, A, visible);
  FSN_LAUNCH_CHECK("k_occ_visibility");
  return FSN_OK;
}

extern "C" int fsn_occgrid_update_masked(float* occs, int64_t n_cells, const uint32_t* visible, float occ_thre, int revive,
                                         double* scratch, uint32_t* bits, fsn_stream_t stream) {
  FSN_REQUIRE(occs && visible && scratch, FSN_E_INVALID, "fsn_occgrid_update_masked: null pointer");
  FSN_REQUIRE(n_cells > 0 && n_cells % 64 == 0, FSN_E_INVALID, "fsn_occgrid_update_masked: n_cells must be a positive multiple of 64");
  const int64_t want = (n_cells + 255) / 256;
  const int nb = (int)(want < MASK_BLOCKS ? want : MASK_BLOCKS);
  hipStream_t s = as_stream(stream);
  k_occ_mask_reduce<<<(unsigned)nb, 256, 0, s>>>(occs, visible, n_cells, revive ? 1 : 0, scratch);
  FSN_LAUNCH_CHECK("k_occ_mask_reduce");
  if (!bits) return FSN_OK;  // occs only (the mark itself: bits &= visible is the caller's)
  k_occ_mask_binarize<<<(unsigned)nb, 256, 0, s>>>(occs, visible, n_cells, scratch, nb, occ_thre, bits);
  FSN_LAUNCH_CHECK("k_occ_mask_binarize");
  return FSN_OK;
}
