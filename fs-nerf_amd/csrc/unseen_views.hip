// unseen_views.hip — random poses no photograph was taken from, and patches of their rays (this package's own
// definition, after RegNeRF's pose sampling; DESIGN.md section 7, include/fsnerf_hip.h has the equations).
// A pose draw g is a pure function of (dist, seed, g): counter-based random numbers (the splitmix64 finaliser of
// ray_perm.hpp keyed by (seed, g, slot)), no state anywhere, no transcendental function - every operation below is a
// float32 +, -, *, / or sqrtf and the library is built with -ffp-contract=off, so tests/unseen_ref.py restates the
// kernels bit for bit in NumPy.
//
// Slots.  Of pose draw g:  0, 1, 2   origin (shell: height z, radius r, unused; box: x, y, z)
//                          3, 4, 5   target = focus + jitter * (2 u - 1)
//                          6 + 2k, 7 + 2k   try k < kUnseenTries of the azimuth's disc rejection (shell)
//         of patch q:      38, 39    anchor row, anchor column
// (g and q share the key's middle word; their slots are disjoint, so a pose and a patch never read the same number.)
//
// k_unseen_patch_batch: ONE launch, one thread per output row; every thread of a patch recomputes the patch's pose
// (at most 6 + 32 mixes and about a hundred flops, against a second launch and a [count,12] round trip through
// memory).  No LDS, no atomics, no index read from memory: nothing here to range-check, so no debug record.
// The launch constants and the anchor lattice are those of fsn_ray_patch_batch (pinhole_consts.hpp).
#include <cmath>

#include "common.hpp"
#include "pinhole_consts.hpp"
#include "ray_dev.hpp"
#include "ray_perm.hpp"

namespace fsn {

constexpr int kUnseenTries = 16;        // (1 - pi/4)^16 = 2e-11: the chance of the (1, 0) fallback per pose
constexpr int kUnseenSlotAnchor = 38;   // 6 + 2 * kUnseenTries
constexpr float kUnseenTinyLen2 = 1e-20f;    // |origin - target|^2 below this: the camera looks down -up
constexpr float kUnseenTinyCross2 = 1e-8f;   // |up x zc|^2 below this: e1 takes up's place

FSN_HD uint64_t unseen_base(uint64_t seed, uint64_t g) { return ray_perm_mix(seed ^ ray_perm_mix(g)); }
FSN_HD uint64_t unseen_bits(uint64_t base, int slot) { return ray_perm_mix(base + (uint64_t)slot); }
FSN_HD float unseen_u(uint64_t base, int slot) { return (float)(uint32_t)(unseen_bits(base, slot) >> 40) * 5.9604644775390625e-08f; }
// uniform on [0, n), n < 2^31
FSN_HD int unseen_below(uint64_t base, int slot, int n) {
  return (int)(((unseen_bits(base, slot) >> 32) * (uint64_t)n) >> 32);
}

__device__ __forceinline__ void cross3(const float (&a)[3], const float (&b)[3], float (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ float len2(const float (&a)[3]) { return (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]; }

// pose draw g of `ds` -> m: rows 0..2 of the camera-to-world matrix, row-major [3][4]
__device__ __forceinline__ void unseen_pose(const fsn_unseen_dist& ds, uint64_t seed, uint64_t g, float (&m)[12]) {
  const uint64_t base = unseen_base(seed, g);
  float origin[3];
  if (ds.mode == FSN_UNSEEN_SHELL) {
    const float z = fminf(ds.z_lo + unseen_u(base, 0) * (ds.z_hi - ds.z_lo), ds.z_hi);
    const float r = fminf(ds.r_lo + unseen_u(base, 1) * (ds.r_hi - ds.r_lo), ds.r_hi);
    float c = 1.0f, s = 0.0f;
    for (int k = 0; k < kUnseenTries; ++k) {
      const float a = 2.0f * unseen_u(base, 6 + 2 * k) - 1.0f, b = 2.0f * unseen_u(base, 7 + 2 * k) - 1.0f;
      const float q = a * a + b * b;
      if (q > 0.0f && q <= 1.0f) {
        const float root = sqrtf(q);
        c = a / root;
        s = b / root;
        break;
      }
    }
    const float h = sqrtf(1.0f - z * z);
    const float hc = h * c, hs = h * s;
#pragma unroll
    for (int k = 0; k < 3; ++k) origin[k] = ds.centre[k] + r * ((hc * ds.e1[k] + hs * ds.e2[k]) + z * ds.up[k]);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) origin[k] = fminf(ds.lo[k] + unseen_u(base, k) * (ds.hi[k] - ds.lo[k]), ds.hi[k]);
  }
  float v[3], zc[3], x[3], xc[3], yc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = origin[k] - (ds.focus[k] + ds.jitter * (2.0f * unseen_u(base, 3 + k) - 1.0f));
  const float vv = len2(v);
  if (vv < kUnseenTinyLen2) {
#pragma unroll
    for (int k = 0; k < 3; ++k) zc[k] = ds.up[k];
  } else {
    const float n = sqrtf(vv);
#pragma unroll
    for (int k = 0; k < 3; ++k) zc[k] = v[k] / n;
  }
  cross3(ds.up, zc, x);
  float xx = len2(x);
  if (xx < kUnseenTinyCross2) {
    cross3(ds.e1, zc, x);
    xx = len2(x);
  }
  const float xn = sqrtf(xx);
#pragma unroll
  for (int k = 0; k < 3; ++k) xc[k] = x[k] / xn;
  cross3(zc, xc, yc);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    m[4 * k + 0] = xc[k];
    m[4 * k + 1] = yc[k];
    m[4 * k + 2] = zc[k];
    m[4 * k + 3] = origin[k];
  }
}

__global__ void __launch_bounds__(256) k_unseen_poses(fsn_unseen_dist ds, uint64_t seed, int64_t first, int64_t count,
                                                      float* __restrict__ poses_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  float m[12];
  unseen_pose(ds, seed, (uint64_t)(first + i), m);
#pragma unroll
  for (int k = 0; k < 12; ++k) poses_out[12 * i + k] = m[k];
}

struct UnseenPatchArgs {
  fsn_unseen_dist ds;
  uint64_t seed;
  int64_t first, count, per_pose;
  int P, dilation, AH, AW, ndc;
  PinholeConsts pc;
  float* rays_o;
  float* rays_d;
  float* poses_out;
  int64_t* anchors_out;
};

__global__ void __launch_bounds__(256) k_unseen_patch_batch(UnseenPatchArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t pp = (int64_t)a.P * a.P;
  if (i >= a.count * pp) return;
  const int64_t b = i / pp;
  const int in_patch = (int)(i - b * pp), pi = in_patch / a.P, pj = in_patch - pi * a.P;
  const uint64_t q = (uint64_t)(a.first + b);
  float m[12];
  unseen_pose(a.ds, a.seed, q / (uint64_t)a.per_pose, m);
  const uint64_t qbase = unseen_base(a.seed, q);
  const int row0 = unseen_below(qbase, kUnseenSlotAnchor, a.AH), col0 = unseen_below(qbase, kUnseenSlotAnchor + 1, a.AW);
  if (in_patch == 0) {
    if (a.poses_out) {
#pragma unroll
      for (int k = 0; k < 12; ++k) a.poses_out[12 * b + k] = m[k];
    }
    if (a.anchors_out) a.anchors_out[b] = (int64_t)row0 * a.AW + col0;
  }
  if (a.rays_o || a.rays_d) {
    float o[3], d[3];
    pinhole_ray(m, a.pc.half_w, a.pc.half_h, a.pc.focal, row0 + pi * a.dilation, col0 + pj * a.dilation, o, d);
    if (a.ndc) ndc_ray(o, d, a.pc.sx, a.pc.sy, a.pc.near, a.pc.two_near);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (a.rays_d) a.rays_d[3 * i + k] = d[k];
      if (a.rays_o) a.rays_o[3 * i + k] = o[k];
    }
  }
}

static inline bool finite3(const float (&v)[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// the checks both entry points share
static int unseen_check_dist(const char* who, const fsn_unseen_dist* d) {
  FSN_REQUIRE(d, FSN_E_INVALID, "%s: null distribution", who);
  FSN_REQUIRE(d->mode == FSN_UNSEEN_SHELL || d->mode == FSN_UNSEEN_BOX, FSN_E_INVALID, "%s: unknown mode %d", who, d->mode);
  FSN_REQUIRE(finite3(d->focus) && finite3(d->up) && finite3(d->e1) && finite3(d->e2) && std::isfinite(d->jitter) &&
                  d->jitter >= 0.0f,
              FSN_E_INVALID, "%s: focus, up, e1, e2 must be finite and jitter finite and not negative", who);
  if (d->mode == FSN_UNSEEN_SHELL) {
    FSN_REQUIRE(finite3(d->centre) && std::isfinite(d->r_hi) && d->r_lo >= 0.0f && d->r_lo <= d->r_hi, FSN_E_INVALID,
                "%s: bad shell radius range [%g, %g] or centre (0 <= r_lo <= r_hi, finite)", who, d->r_lo, d->r_hi);
    FSN_REQUIRE(d->z_lo > -1.0f && d->z_lo <= d->z_hi && d->z_hi < 1.0f, FSN_E_INVALID,
                "%s: bad shell height range [%g, %g] (-1 < z_lo <= z_hi < 1)", who, d->z_lo, d->z_hi);
  } else {
    FSN_REQUIRE(finite3(d->lo) && finite3(d->hi) && d->lo[0] <= d->hi[0] && d->lo[1] <= d->hi[1] && d->lo[2] <= d->hi[2],
                FSN_E_INVALID, "%s: bad box (lo <= hi, finite)", who);
  }
  return FSN_OK;
}

}  // namespace fsn

using namespace fsn;

extern "C" int fsn_unseen_poses(const fsn_unseen_dist* dist_host, uint64_t seed, int64_t first_draw, int64_t count,
                                float* poses_out, fsn_stream_t stream) {
  if (int rc = unseen_check_dist("fsn_unseen_poses", dist_host)) return rc;
  FSN_REQUIRE(first_draw >= 0 && count >= 0 && first_draw <= ((int64_t)1 << 62) && count <= ((int64_t)1 << 38),
              FSN_E_INVALID, "fsn_unseen_poses: bad first_draw %lld or count %lld", (long long)first_draw, (long long)count);
  if (count == 0) return FSN_OK;
  FSN_REQUIRE(poses_out, FSN_E_INVALID, "fsn_unseen_poses: null pointer");
  k_unseen_poses<<<(unsigned)((count + 255) / 256), 256, 0, as_stream(stream)>>>(*dist_host, seed, first_draw, count, poses_out);
  FSN_LAUNCH_CHECK("k_unseen_poses");
  return FSN_OK;
}

extern "C" int fsn_unseen_patch_batch(const fsn_unseen_dist* dist_host, uint64_t seed, int64_t first_patch, int64_t count,
                                      int64_t patches_per_pose, int H, int W, double focal, int P, int dilation, int ndc,
                                      double near, float* rays_o, float* rays_d, float* poses_out, int64_t* anchors_out,
                                      fsn_stream_t stream) {
  if (int rc = unseen_check_dist("fsn_unseen_patch_batch", dist_host)) return rc;
  FSN_REQUIRE(H > 0 && W > 0 && focal > 0, FSN_E_INVALID, "fsn_unseen_patch_batch: bad geometry H=%d W=%d focal=%g", H, W, focal);
  PatchLattice lat;
  if (int rc = patch_lattice("fsn_unseen_patch_batch", H, W, P, dilation, &lat)) return rc;
  FSN_REQUIRE(patches_per_pose >= 1, FSN_E_INVALID, "fsn_unseen_patch_batch: patches_per_pose %lld (at least 1)",
              (long long)patches_per_pose);
  FSN_REQUIRE(first_patch >= 0 && count >= 0 && first_patch <= ((int64_t)1 << 62), FSN_E_INVALID,
              "fsn_unseen_patch_batch: bad first_patch %lld or count %lld", (long long)first_patch, (long long)count);
  if (count == 0) return FSN_OK;
  FSN_REQUIRE(rays_o || rays_d || poses_out || anchors_out, FSN_E_INVALID,
              "fsn_unseen_patch_batch: null pointer for every output");
  const int64_t pp = (int64_t)P * P;
  FSN_REQUIRE(count <= ((int64_t)1 << 38) / pp, FSN_E_UNSUPPORTED, "fsn_unseen_patch_batch: more than 2^38 rows in one call");
  UnseenPatchArgs a{};
  a.ds = *dist_host;
  a.seed = seed;
  a.first = first_patch;
  a.count = count;
  a.per_pose = patches_per_pose;
  a.P = P;
  a.dilation = dilation;
  a.AH = (int)lat.AH;
  a.AW = (int)lat.AW;
  a.ndc = ndc ? 1 : 0;
  a.pc = pinhole_consts(H, W, focal, near);  // (fsn_ray_patch_batch's: the same rays for the same pose and pixel)
  a.rays_o = rays_o;
  a.rays_d = rays_d;
  a.poses_out = poses_out;
  a.anchors_out = anchors_out;
  k_unseen_patch_batch<<<(unsigned)((count * pp + 255) / 256), 256, 0, as_stream(stream)>>>(a);
  FSN_LAUNCH_CHECK("k_unseen_patch_batch");
  return FSN_OK;
}
