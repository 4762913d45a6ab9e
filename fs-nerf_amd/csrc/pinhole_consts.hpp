// pinhole_consts.hpp — the host-side geometry every ray entry point shares: the launch constants of pinhole_ray /
// ndc_ray (ray_dev.hpp) and the lattice of patch anchors.  The constants are formed HERE and nowhere else, because every
// bit-for-bit claim of the data layer (a served row = the row of fsn_build_rays' tables = the reference's) rests on all
// entry points rounding them the same way: each is formed in double, as Python forms it (src/utils/utilities.py:67),
// and then rounded to float32.
#pragma once
#include "common.hpp"

namespace fsn {

struct PinholeConsts {
  float half_w, half_h, focal;  // pinhole_ray
  float sx, sy, near, two_near;  // ndc_ray
};

static inline PinholeConsts pinhole_consts(int H, int W, double focal, double near) {
  PinholeConsts c;
  c.half_w = (float)(W * 0.5);
  c.half_h = (float)(H * 0.5);
  c.focal = (float)focal;
  c.sx = (float)(-1.0 / (W / (2.0 * focal)));
  c.sy = (float)(-1.0 / (H / (2.0 * focal)));
  c.near = (float)near;
  c.two_near = (float)(2.0 * near);
  return c;
}

// P x P patches at `dilation` in an H x W image: a patch spans ext pixels, its top-left pixel (the anchor) runs over
// an AH x AW lattice.
struct PatchLattice {
  int64_t ext, AH, AW;
};

static inline int patch_lattice(const char* who, int H, int W, int P, int dilation, PatchLattice* lat) {
  FSN_REQUIRE(P >= 1 && dilation >= 1, FSN_E_INVALID, "%s: bad patch P=%d dilation=%d (both at least 1)", who, P, dilation);
  const int64_t ext = (int64_t)(P - 1) * dilation + 1;
  FSN_REQUIRE(ext <= H && ext <= W, FSN_E_INVALID,
              "%s: a patch of %d pixels at dilation %d spans %lld pixels and does not fit the %dx%d image", who, P, dilation,
              (long long)ext, H, W);
  *lat = PatchLattice{ext, H - ext + 1, W - ext + 1};
  return FSN_OK;
}

}  // namespace fsn
