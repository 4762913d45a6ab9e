// raydata.hip — the training loop's data layer on the device (reference: src/nerfdata/datasets/{blender,llff}.py and the
// loaders of src/nerfdata/splitter.py:123-132).  The ray tables are pure functions of (pose, pixel), so a batch needs
// nothing resident but the uint8 images and the poses: ONE launch, one thread per output ray,
//   position in the epoch -> shuffled ray index (ray_perm.hpp) -> (view, row, column) -> ray (+ NDC) -> colour.
// Rays: pinhole_ray / ndc_ray (ray_dev.hpp) with the arguments of k_build_rays (pinhole_consts.hpp forms them for both):
// bit for bit row `index` of its tables.
// Colours: bit for bit the reference's float images, which fixes the arithmetic (the library is built with
// -ffp-contract=off):
//   byte v -> (float)v / 255.0f   (the reference divides in float64 and rounds to float32: the same float for all 256
//                                  bytes; a multiplication by 1.0f / 255.0f is not)
//   white background (blender.py:114-117): c * a + (1.0f - a), three separate float32 operations in that order.
// A latency-bound gather of a few hundred KB: 12-byte rows rule out 16-byte vector stores; plain coalesced stores.
// k_ray_patch_batch serves P x P patches the same way: position -> shuffled ANCHOR (the patch's top-left pixel) ->
// the patch's pixels.  Both kernels only find (flat ray index, view, row, column); the row itself - ray, NDC, stores,
// colour - is written by the one write_ray_row, so a patch's rows are k_ray_batch's by construction.
// fsn_ray_batch_k / fsn_ray_patch_batch_k serve the same batches over a camera table K = (fx, fy, cx, cy) on the device
// (learnable intrinsics): the same two kernels, instantiated with kTable = true.
// fsn_ray_batch_aux / fsn_ray_patch_batch_aux also serve the rows of the dataset's auxiliary float planes (depth, masks,
// monocular priors; DESIGN 7 "Data layer"): the same two kernels again, instantiated with kAux = true.
#include "common.hpp"
#include "pinhole_consts.hpp"
#include "ray_dev.hpp"
#include "ray_perm.hpp"

namespace fsn {

// debug build: an explicit index outside [0, N) is recorded (count, source line, index, N - both truncated to 32 bits),
// read by fsn_debug_report("raydata").  In every build such a thread leaves its output rows untouched.
FSN_DEBUG_DEFINE_RECORD(raydata)

struct RayBatchArgs {
  const float* poses;      // [n, 12]
  const uint8_t* images;   // [n, H, W, C]
  const int64_t* indices;  // explicit order: [count]
  int64_t n_rays, per_view, start, count;
  int W, C, ndc, white_bkgd, order;
  PinholeConsts pc;
  RayPerm perm;
  float* rays_o;
  float* rays_d;
  float* rgb;
  int64_t* index;
};

// The camera table of the learnable intrinsics (fsn_ray_batch_k / fsn_ray_patch_batch_k): row v * stride of
// K = (fx, fy, cx, cy) [k_rows, 4] is view v's, stride = 0 for one shared row.  kTable = false is the stored-intrinsics
// kernel: it never looks at the table.
struct CamTable {
  const float* K;
  int64_t stride;
};

// The auxiliary planes (fsn_ray_batch_aux / fsn_ray_patch_batch_aux): src [n_rays, channels] float32 words, row idx copied
// bit for bit (as 32-bit words: a NaN keeps its payload) to row i of out [rows, channels].  kAux = false never looks at it.
struct AuxPlanes {
  const uint32_t* src;
  uint32_t* out;
  int channels;
};

// Item b of the batch in the order asked for: a flat ray index (k_ray_batch) or an anchor (k_ray_patch_batch) of [0, n).
// false: an explicit entry outside the range, which never reaches memory.
__device__ __forceinline__ bool batch_item(const RayBatchArgs& a, int64_t b, int64_t n, int64_t& item) {
  if (a.order == FSN_RAY_ORDER_IDENTITY) {
    item = a.start + b;
  } else if (a.order == FSN_RAY_ORDER_PERMUTED) {
    item = (int64_t)ray_perm_at(a.perm, (uint64_t)(a.start + b));
  } else {
    item = a.indices[b];
    if (item < 0 || item >= n) {
#ifdef FSN_DEBUG
      fsn_dbg_note(g_dbg_raydata, __LINE__, item, n);
#endif
      return false;
    }
  }
  return true;
}

// Output row i for the flat ray index idx: the index, the ray (+ NDC) and the colour, each if asked for.  `pixel` gives
// idx's (view, row, column) and is called only when rays are wanted: k_ray_batch's 64-bit division lives in it, and a
// colour-only batch never pays for it.
template <bool kTable, bool kAux, class Pixel>
__device__ __forceinline__ void write_ray_row(const RayBatchArgs& a, const CamTable& cam, const AuxPlanes& aux, int64_t i,
                                              int64_t idx, Pixel pixel) {
  if (a.index) a.index[i] = idx;
  if constexpr (kAux) {
    const uint32_t* src = aux.src + idx * aux.channels;
    uint32_t* dst = aux.out + i * aux.channels;
    for (int k = 0; k < aux.channels; ++k) dst[k] = src[k];
  }
  if (a.rays_o || a.rays_d) {
    int64_t view;
    int row, col;
    pixel(view, row, col);
    float o[3], d[3];
    if constexpr (kTable)
      pinhole_ray_k(a.poses + 12 * view, cam.K + cam.stride * view, row, col, o, d);
    else
      pinhole_ray(a.poses + 12 * view, a.pc.half_w, a.pc.half_h, a.pc.focal, row, col, o, d);
    if (a.ndc) ndc_ray(o, d, a.pc.sx, a.pc.sy, a.pc.near, a.pc.two_near);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (a.rays_d) a.rays_d[3 * i + k] = d[k];
      if (a.rays_o) a.rays_o[3 * i + k] = o[k];
    }
  }
  if (a.rgb) {
    const uint8_t* px = a.images + idx * a.C;
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (float)px[k] / 255.0f;
    if (a.white_bkgd) {
      const float al = (float)px[3] / 255.0f;
      const float rest = 1.0f - al;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float m = c[k] * al;
        c[k] = m + rest;
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) a.rgb[3 * i + k] = c[k];
  }
}

template <bool kTable, bool kAux>
__global__ void __launch_bounds__(256) k_ray_batch(RayBatchArgs a, CamTable cam, AuxPlanes aux) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.count) return;
  int64_t idx;
  if (!batch_item(a, i, a.n_rays, idx)) return;
  write_ray_row<kTable, kAux>(a, cam, aux, i, idx, [&](int64_t& view, int& row, int& col) {
    view = idx / a.per_view;
    const int64_t pix = idx - view * a.per_view;
    row = (int)(pix / a.W);
    col = (int)(pix % a.W);
  });
}

// A batch of P x P patches (fsn_ray_patch_batch): one thread per output row (b P + i) P + j = pixel (i, j) of patch b.
// `r` is fsn_ray_batch's argument block read over ANCHORS (the patches' top-left pixels): start / count count
// patches, indices is the explicit anchor list, perm permutes [0, n_anchors); n_rays / per_view are not used.
struct RayPatchArgs {
  RayBatchArgs r;
  int64_t n_anchors, per_view_anchors;  // A, AH * AW
  int P, dilation, AW, H;
};

template <bool kTable, bool kAux>
__global__ void __launch_bounds__(256) k_ray_patch_batch(RayPatchArgs pa, CamTable cam, AuxPlanes aux) {
  const RayBatchArgs& a = pa.r;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t pp = (int64_t)pa.P * pa.P;
  if (i >= a.count * pp) return;
  const int64_t b = i / pp;
  const int in_patch = (int)(i - b * pp), pi = in_patch / pa.P, pj = in_patch - pi * pa.P;
  int64_t anchor;
  if (!batch_item(a, b, pa.n_anchors, anchor)) return;
  const int64_t v = anchor / pa.per_view_anchors, rest = anchor - v * pa.per_view_anchors;
  const int r = (int)(rest / pa.AW) + pi * pa.dilation, c = (int)(rest % pa.AW) + pj * pa.dilation;
  write_ray_row<kTable, kAux>(a, cam, aux, i, (v * pa.H + r) * a.W + c, [&](int64_t& view, int& row, int& col) {
    view = v;
    row = r;
    col = c;
  });
}

}  // namespace fsn

using namespace fsn;

// What the two batch calls share: the checks on (views, images, order, positions, pointers) and the argument block.
// `lat` null: a batch of rays, its items the n_views * H * W flat ray indices.  Else a batch of patches, its items the
// anchors of the lattice this forms from (P, dilation).  A call with nothing to do (count = 0) leaves out->count at 0.
static int ray_batch_args(const char* who, const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C,
                          double focal, int ndc, double near, int white_bkgd, int order, uint64_t seed, int64_t epoch,
                          const int64_t* list, int64_t start, int64_t count, int P, int dilation, PatchLattice* lat,
                          float* rays_o, float* rays_d, float* rgb, int64_t* index, const void* aux_out,
                          RayBatchArgs* out) {
  FSN_REQUIRE(n_views >= 0 && H > 0 && W > 0 && focal > 0, FSN_E_INVALID,
              "%s: bad geometry n=%lld H=%d W=%d focal=%g", who, (long long)n_views, H, W, focal);
  FSN_REQUIRE(C == 3 || C == 4, FSN_E_INVALID, "%s: %d channels (the images are RGB or RGBA bytes: 3 or 4)", who, C);
  FSN_REQUIRE(!white_bkgd || C == 4, FSN_E_INVALID,
              "%s: white_bkgd composes over the alpha channel and needs 4-channel images, got %d", who, C);
  FSN_REQUIRE(order == FSN_RAY_ORDER_IDENTITY || order == FSN_RAY_ORDER_PERMUTED || order == FSN_RAY_ORDER_EXPLICIT,
              FSN_E_INVALID, "%s: unknown order %d", who, order);
  if (lat)
    if (int rc = patch_lattice(who, H, W, P, dilation, lat)) return rc;
  FSN_REQUIRE(n_views <= ((int64_t)1 << 62) / ((int64_t)H * W), FSN_E_UNSUPPORTED, "%s: more than 2^62 rays", who);
  const int64_t per_view = (int64_t)H * W, n_rays = n_views * per_view;
  const int64_t n_items = lat ? n_views * lat->AH * lat->AW : n_rays;
  const char* item = lat ? "anchor" : "index";
  FSN_REQUIRE(start >= 0 && count >= 0 && epoch >= 0, FSN_E_INVALID, "%s: negative start, count or epoch", who);
  if (order == FSN_RAY_ORDER_EXPLICIT) {
    FSN_REQUIRE(start == 0, FSN_E_INVALID, "%s: an explicit %s list is served from its beginning (start = 0)", who, item);
  } else {
    FSN_REQUIRE(start <= n_items && count <= n_items - start, FSN_E_INVALID,
                "%s: positions [%lld, +%lld) leave the %lld %s of the dataset (start + count > %s)", who,
                (long long)start, (long long)count, (long long)n_items, lat ? "anchors" : "rays", lat ? "A" : "N");
  }
  if (lat) {  // (patches of rays alone need no image)
    FSN_REQUIRE(poses, FSN_E_INVALID, "%s: null poses", who);
    FSN_REQUIRE(images || !rgb, FSN_E_INVALID, "%s: null images with colours asked for (rgb)", who);
  } else {
    FSN_REQUIRE(poses && images, FSN_E_INVALID, "%s: null poses or images", who);
  }
  if (count == 0) return FSN_OK;
  FSN_REQUIRE(order != FSN_RAY_ORDER_EXPLICIT || list, FSN_E_INVALID, "%s: null %s list", who, item);
  FSN_REQUIRE(rays_o || rays_d || rgb || index || aux_out, FSN_E_INVALID, "%s: null pointer for every output", who);
  RayBatchArgs& a = *out;
  a.poses = poses;
  a.images = images;
  a.indices = list;
  a.n_rays = n_rays;
  a.per_view = per_view;
  a.start = start;
  a.count = count;
  a.W = W;
  a.C = C;
  a.ndc = ndc ? 1 : 0;
  a.white_bkgd = white_bkgd ? 1 : 0;
  a.order = order;
  a.pc = pinhole_consts(H, W, focal, near);
  if (order == FSN_RAY_ORDER_PERMUTED) a.perm = ray_perm_make((uint64_t)n_items, seed, (uint64_t)epoch);
  a.rays_o = rays_o;
  a.rays_d = rays_d;
  a.rgb = rgb;
  a.index = index;
  return FSN_OK;
}

// The two batch entry points, their camera-table twins and their aux forms share one body each: `cam` null = the stored
// intrinsics, `aux` null (or without an output) = no auxiliary rows.
static int ray_batch_call(const char* who, const CamTable* cam, const AuxPlanes* aux, const float* poses, int64_t n_views,
                          const uint8_t* images, int H, int W, int C, double focal, int ndc, double near, int white_bkgd,
                          int order, uint64_t seed, int64_t epoch, const int64_t* indices, int64_t start, int64_t count,
                          float* rays_o, float* rays_d, float* rgb, int64_t* index, fsn_stream_t stream) {
  RayBatchArgs a{};
  const int rc = ray_batch_args(who, poses, n_views, images, H, W, C, focal, ndc, near, white_bkgd, order, seed, epoch,
                                indices, start, count, 0, 0, nullptr, rays_o, rays_d, rgb, index,
                                aux ? aux->out : nullptr, &a);
  if (rc || a.count == 0) return rc;
  const unsigned grid = (unsigned)((count + 255) / 256);
  if (aux && aux->out) {
    if (cam)
      k_ray_batch<true, true><<<grid, 256, 0, as_stream(stream)>>>(a, *cam, *aux);
    else
      k_ray_batch<false, true><<<grid, 256, 0, as_stream(stream)>>>(a, CamTable{}, *aux);
  } else if (cam) {
    k_ray_batch<true, false><<<grid, 256, 0, as_stream(stream)>>>(a, *cam, AuxPlanes{});
  } else {
    k_ray_batch<false, false><<<grid, 256, 0, as_stream(stream)>>>(a, CamTable{}, AuxPlanes{});
  }
  FSN_LAUNCH_CHECK("k_ray_batch");
  return FSN_OK;
}

static int ray_patch_batch_call(const char* who, const CamTable* cam, const AuxPlanes* aux, const float* poses, int64_t n_views,
                                const uint8_t* images, int H, int W, int C, double focal, int ndc, double near,
                                int white_bkgd, int order, uint64_t seed, int64_t epoch, const int64_t* anchors,
                                int64_t start, int64_t count, int P, int dilation, float* rays_o, float* rays_d, float* rgb,
                                int64_t* index, fsn_stream_t stream) {
  RayPatchArgs pa{};
  PatchLattice lat{};
  const int rc = ray_batch_args(who, poses, n_views, images, H, W, C, focal, ndc, near, white_bkgd, order, seed, epoch,
                                anchors, start, count, P, dilation, &lat, rays_o, rays_d, rgb, index,
                                aux ? aux->out : nullptr, &pa.r);
  if (rc || pa.r.count == 0) return rc;
  const int64_t pp = (int64_t)P * P;
  FSN_REQUIRE(count <= ((int64_t)1 << 38) / pp, FSN_E_UNSUPPORTED, "%s: more than 2^38 rows in one call", who);
  pa.n_anchors = n_views * lat.AH * lat.AW;
  pa.per_view_anchors = lat.AH * lat.AW;
  pa.P = P;
  pa.dilation = dilation;
  pa.AW = (int)lat.AW;
  pa.H = H;
  const unsigned grid = (unsigned)((count * pp + 255) / 256);
  if (aux && aux->out) {
    if (cam)
      k_ray_patch_batch<true, true><<<grid, 256, 0, as_stream(stream)>>>(pa, *cam, *aux);
    else
      k_ray_patch_batch<false, true><<<grid, 256, 0, as_stream(stream)>>>(pa, CamTable{}, *aux);
  } else if (cam) {
    k_ray_patch_batch<true, false><<<grid, 256, 0, as_stream(stream)>>>(pa, *cam, AuxPlanes{});
  } else {
    k_ray_patch_batch<false, false><<<grid, 256, 0, as_stream(stream)>>>(pa, CamTable{}, AuxPlanes{});
  }
  FSN_LAUNCH_CHECK("k_ray_patch_batch");
  return FSN_OK;
}

// The camera table of the _k entry points: K [k_rows, 4], k_rows = 1 (shared by all views) or n_views.
static int cam_table(const char* who, const float* K, int64_t k_rows, int64_t n_views, CamTable* cam) {
  FSN_REQUIRE(K, FSN_E_INVALID, "%s: null camera table K", who);
  FSN_REQUIRE(k_rows == 1 || k_rows == n_views, FSN_E_INVALID,
              "%s: a camera table of %lld rows (1, or one per view: %lld)", who, (long long)k_rows, (long long)n_views);
  *cam = CamTable{K, k_rows == 1 ? 0 : 4};
  return FSN_OK;
}

extern "C" int fsn_ray_batch(const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C, double focal,
                             int ndc, double near, int white_bkgd, int order, uint64_t seed, int64_t epoch,
                             const int64_t* indices, int64_t start, int64_t count, float* rays_o, float* rays_d,
                             float* rgb, int64_t* index, fsn_stream_t stream) {
  return ray_batch_call("fsn_ray_batch", nullptr, nullptr, poses, n_views, images, H, W, C, focal, ndc, near, white_bkgd, order, seed,
                        epoch, indices, start, count, rays_o, rays_d, rgb, index, stream);
}

extern "C" int fsn_ray_batch_k(const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C, double focal,
                               const float* K, int64_t k_rows, int ndc, double near, int white_bkgd, int order,
                               uint64_t seed, int64_t epoch, const int64_t* indices, int64_t start, int64_t count,
                               float* rays_o, float* rays_d, float* rgb, int64_t* index, fsn_stream_t stream) {
  CamTable cam;
  if (int rc = cam_table("fsn_ray_batch_k", K, k_rows, n_views, &cam)) return rc;
  return ray_batch_call("fsn_ray_batch_k", &cam, nullptr, poses, n_views, images, H, W, C, focal, ndc, near, white_bkgd, order, seed,
                        epoch, indices, start, count, rays_o, rays_d, rgb, index, stream);
}

extern "C" int fsn_ray_patch_batch(const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C,
                                   double focal, int ndc, double near, int white_bkgd, int order, uint64_t seed,
                                   int64_t epoch, const int64_t* anchors, int64_t start, int64_t count, int P, int dilation,
                                   float* rays_o, float* rays_d, float* rgb, int64_t* index, fsn_stream_t stream) {
  return ray_patch_batch_call("fsn_ray_patch_batch", nullptr, nullptr, poses, n_views, images, H, W, C, focal, ndc, near, white_bkgd,
                              order, seed, epoch, anchors, start, count, P, dilation, rays_o, rays_d, rgb, index, stream);
}

extern "C" int fsn_ray_patch_batch_k(const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C,
                                     double focal, const float* K, int64_t k_rows, int ndc, double near, int white_bkgd,
                                     int order, uint64_t seed, int64_t epoch, const int64_t* anchors, int64_t start,
                                     int64_t count, int P, int dilation, float* rays_o, float* rays_d, float* rgb,
                                     int64_t* index, fsn_stream_t stream) {
  CamTable cam;
  if (int rc = cam_table("fsn_ray_patch_batch_k", K, k_rows, n_views, &cam)) return rc;
  return ray_patch_batch_call("fsn_ray_patch_batch_k", &cam, nullptr, poses, n_views, images, H, W, C, focal, ndc, near, white_bkgd,
                              order, seed, epoch, anchors, start, count, P, dilation, rays_o, rays_d, rgb, index, stream);
}

// The camera table and the planes of the _aux entry points: K null with k_rows = 0 is the stored intrinsics (*use_cam
// false); aux [n_rays, channels], 1 <= channels <= 4, aux_out null = no auxiliary rows.
static int aux_call_args(const char* who, const float* K, int64_t k_rows, int64_t n_views, const float* aux,
                         int aux_channels, float* aux_out, CamTable* cam, bool* use_cam, AuxPlanes* planes) {
  *use_cam = !(K == nullptr && k_rows == 0);
  if (*use_cam)
    if (int rc = cam_table(who, K, k_rows, n_views, cam)) return rc;
  FSN_REQUIRE(aux_channels >= 1 && aux_channels <= 4, FSN_E_INVALID, "%s: %d aux channels (1 to 4)", who, aux_channels);
  FSN_REQUIRE(aux || !aux_out, FSN_E_INVALID, "%s: aux_out without aux planes to read", who);
  *planes = AuxPlanes{reinterpret_cast<const uint32_t*>(aux), reinterpret_cast<uint32_t*>(aux_out), aux_channels};
  return FSN_OK;
}

extern "C" int fsn_ray_batch_aux(const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C,
                                 double focal, const float* K, int64_t k_rows, int ndc, double near, int white_bkgd,
                                 int order, uint64_t seed, int64_t epoch, const int64_t* indices, int64_t start,
                                 int64_t count, float* rays_o, float* rays_d, float* rgb, int64_t* index, const float* aux,
                                 int aux_channels, float* aux_out, fsn_stream_t stream) {
  CamTable cam{};
  AuxPlanes planes{};
  bool use_cam;
  if (int rc = aux_call_args("fsn_ray_batch_aux", K, k_rows, n_views, aux, aux_channels, aux_out, &cam, &use_cam, &planes))
    return rc;
  return ray_batch_call("fsn_ray_batch_aux", use_cam ? &cam : nullptr, &planes, poses, n_views, images, H, W, C, focal, ndc,
                        near, white_bkgd, order, seed, epoch, indices, start, count, rays_o, rays_d, rgb, index, stream);
}

extern "C" int fsn_ray_patch_batch_aux(const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C,
                                       double focal, const float* K, int64_t k_rows, int ndc, double near, int white_bkgd,
                                       int order, uint64_t seed, int64_t epoch, const int64_t* anchors, int64_t start,
                                       int64_t count, int P, int dilation, float* rays_o, float* rays_d, float* rgb,
                                       int64_t* index, const float* aux, int aux_channels, float* aux_out,
                                       fsn_stream_t stream) {
  CamTable cam{};
  AuxPlanes planes{};
  bool use_cam;
  if (int rc = aux_call_args("fsn_ray_patch_batch_aux", K, k_rows, n_views, aux, aux_channels, aux_out, &cam, &use_cam,
                             &planes))
    return rc;
  return ray_patch_batch_call("fsn_ray_patch_batch_aux", use_cam ? &cam : nullptr, &planes, poses, n_views, images, H, W, C,
                              focal, ndc, near, white_bkgd, order, seed, epoch, anchors, start, count, P, dilation, rays_o,
                              rays_d, rgb, index, stream);
}

extern "C" int fsn_ray_perm_host(int64_t N, uint64_t seed, int64_t epoch, int64_t start, int64_t count, int64_t* out_host) {
  FSN_REQUIRE(N >= 0 && N <= ((int64_t)1 << 62) && epoch >= 0, FSN_E_INVALID, "fsn_ray_perm_host: bad N or epoch");
  FSN_REQUIRE(start >= 0 && count >= 0 && start <= N && count <= N - start, FSN_E_INVALID,
              "fsn_ray_perm_host: positions [%lld, +%lld) leave [0, %lld)", (long long)start, (long long)count, (long long)N);
  if (count == 0) return FSN_OK;
  FSN_REQUIRE(out_host, FSN_E_INVALID, "fsn_ray_perm_host: null pointer");
  const RayPerm p = ray_perm_make((uint64_t)N, seed, (uint64_t)epoch);
  for (int64_t i = 0; i < count; ++i) out_host[i] = (int64_t)ray_perm_at(p, (uint64_t)(start + i));
  return FSN_OK;
}
