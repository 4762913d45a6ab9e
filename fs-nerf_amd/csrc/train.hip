// train.hip — C-ABI of the TRAINING step around the hot path: NeRF.forward with saved
// activations and its backward on the matrix cores (kernels in train_fused.hip; the input-gradient form's entry point
// is in input_grad.hip and shares train_bwd_checked below), and the loss-scale kernel k_grad_scale.  The backward of
// the volume integration is in composite_grad.hip.  The plain fp32 formulation with library GEMMs that the MFMA path
// was first checked against is NOT part of this library any more: it lives in tests/ref_fp32/ as a test-only helper.
//
// reference: src/core/models.py:111-143 (forward), src/run-nerf.py:243-285 (loss.backward()).
#include "common.hpp"
#include "mlp_layout.hpp"
#include "train_internal.hpp"

namespace fsn {

int check_desc(const fsn_mlp_desc* d) {
  FSN_REQUIRE(d, FSN_E_INVALID, "null desc");
  NetGeom G;
  const char* why;
  const int rc = build_geom(*d, FSN_PREC_FP16X3, G, &why);
  FSN_REQUIRE(rc == FSN_OK, rc, "training path: %s", why);
  return FSN_OK;
}

// The checks of both training-backward entry points, then fused_train_bwd.  Without `rq` (fsn_nerf_train_bwd) the
// weight gradients are required and so is n > 0; with it (fsn_nerf_train_bwd_inputs) n == 0 is a no-op and both
// gradient arrays may be null together.
int train_bwd_checked(const char* who, const fsn_mlp_desc* desc, int prec, const float* const* W, int64_t n, float* ws,
                      const float* out, const float* d_out, const float* grad_scale, float* const* dW, float* const* db,
                      int accumulate, float* stage_scales, uint32_t* stage_amax, uint32_t* status, fsn_stream_t stream,
                      const InputGradReq* rq) {
  const int rc = check_desc(desc);
  if (rc != FSN_OK) return rc;
  FSN_REQUIRE(prec_in(PrecTraining{}, prec), FSN_E_INVALID, "%s: unknown precision", who);
  if (rq) {
    FSN_REQUIRE(n >= 0, FSN_E_INVALID, "%s: n < 0", who);
    if (n == 0) return FSN_OK;
    FSN_REQUIRE(W && ws && out && d_out, FSN_E_INVALID, "%s: null pointer", who);
    FSN_REQUIRE((dW == nullptr) == (db == nullptr), FSN_E_INVALID,
                "%s: d_weights and d_biases go together (both NULL: input gradients only)", who);
  } else {
    FSN_REQUIRE(W && dW && db, FSN_E_INVALID, "%s: null pointer", who);
    FSN_REQUIRE(n > 0 && ws && out && d_out, FSN_E_INVALID, "%s: needs the forward's workspace (n > 0)", who);
  }
  FSN_REQUIRE(n < (1ll << 31), FSN_E_UNSUPPORTED, "%s: n too large for one call", who);
  FSN_REQUIRE((stage_scales == nullptr) == (stage_amax == nullptr), FSN_E_INVALID,
              "%s: stage_scales and stage_amax go together", who);
  if (rq && rq->rays)
    FSN_REQUIRE(rq->rays->rays_o && rq->rays->rays_d && rq->rays->ri && rq->rays->t0 && rq->rays->t1 && !rq->x && !rq->dirs,
                FSN_E_INVALID, "%s: the ray form takes all five ray pointers and neither x nor dirs", who);
  else if (rq)
    FSN_REQUIRE(rq->x && rq->dirs, FSN_E_INVALID, "%s: needs x and dirs, or the ray form's five pointers", who);
  return fused_train_bwd(desc, prec, W, n, ws, out, d_out, grad_scale, dW, db, accumulate != 0, stage_scales, stage_amax,
                         status, as_stream(stream), rq);
}

}  // namespace fsn

using namespace fsn;

extern "C" int64_t fsn_nerf_train_workspace_floats(const fsn_mlp_desc* desc, int prec, int64_t n) {
  if (check_desc(desc) != FSN_OK) return FSN_E_INVALID;
  FSN_REQUIRE(n >= 0, FSN_E_INVALID, "fsn_nerf_train_workspace_floats: n < 0");
  FSN_REQUIRE(prec_in(PrecTraining{}, prec), FSN_E_INVALID, "fsn_nerf_train_workspace_floats: unknown precision");
  return fused_train_workspace_floats(*desc, prec, n);
}

extern "C" int fsn_nerf_train_fwd(const fsn_mlp_desc* desc, int prec, const float* const* W, const float* const* b,
                                  const float* x, const float* dirs, const float* pos_mask, const float* dir_mask,
                                  int64_t n, float* ws, float* out, uint32_t* status, fsn_stream_t stream) {
  int rc = check_desc(desc);
  if (rc != FSN_OK) return rc;
  FSN_REQUIRE(prec_in(PrecTraining{}, prec), FSN_E_INVALID, "fsn_nerf_train_fwd: unknown precision");
  if (n == 0) return FSN_OK;
  FSN_REQUIRE(W && b && x && dirs && ws && out, FSN_E_INVALID, "fsn_nerf_train_fwd: null pointer");
  FSN_REQUIRE(n < (1ll << 31), FSN_E_UNSUPPORTED, "fsn_nerf_train_fwd: n too large for one call");
  return fused_train_fwd(desc, prec, W, b, x, dirs, pos_mask, dir_mask, n, ws, out, status, as_stream(stream));
}

extern "C" int fsn_nerf_train_fwd_rays(const fsn_mlp_desc* desc, int prec, const float* const* W, const float* const* b,
                                       const float* rays_o, const float* rays_d, const int64_t* ray_indices,
                                       const float* t_starts, const float* t_ends, const float* pos_mask,
                                       const float* dir_mask, int64_t n, float* ws, float* out, uint32_t* status,
                                       fsn_stream_t stream) {
  int rc = check_desc(desc);
  if (rc != FSN_OK) return rc;
  FSN_REQUIRE(prec_in(PrecTraining{}, prec), FSN_E_INVALID, "fsn_nerf_train_fwd_rays: unknown precision");
  if (n == 0) return FSN_OK;
  FSN_REQUIRE(W && b && rays_o && rays_d && ray_indices && t_starts && t_ends && ws && out, FSN_E_INVALID,
              "fsn_nerf_train_fwd_rays: null pointer");
  FSN_REQUIRE(n < (1ll << 31), FSN_E_UNSUPPORTED, "fsn_nerf_train_fwd_rays: n too large for one call");
  const TrainRays rays{rays_o, rays_d, t_starts, t_ends, ray_indices};
  return fused_train_fwd(desc, prec, W, b, nullptr, nullptr, pos_mask, dir_mask, n, ws, out, status, as_stream(stream), &rays);
}

extern "C" int fsn_nerf_train_bwd(const fsn_mlp_desc* desc, int prec, const float* const* W, int64_t n, float* ws,
                                  const float* out, const float* d_out, const float* grad_scale, float* const* dW,
                                  float* const* db, int accumulate, float* stage_scales, uint32_t* stage_amax,
                                  uint32_t* status, fsn_stream_t stream) {
  return train_bwd_checked("fsn_nerf_train_bwd", desc, prec, W, n, ws, out, d_out, grad_scale, dW, db, accumulate,
                           stage_scales, stage_amax, status, stream, nullptr);
}

// max |d_out| as the bits of a non-negative float (unsigned order = float order; a NaN's bits lie above infinity's and
// so survive the maximum), last workgroup forms the scale
__global__ void k_grad_scale(const float* __restrict__ x, int64_t n, float* __restrict__ buf) {
  uint32_t mx = 0u;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = ((reinterpret_cast<uintptr_t>(x) & 15u) == 0) ? n / 4 : 0;  // 16-byte loads over the aligned bulk
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
  for (int64_t i = tid; i < n4; i += nthr) {
    const u32x4 v = reinterpret_cast<const u32x4*>(x)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t b = v[k] & 0x7fffffffu;
      mx = b > mx ? b : mx;
    }
  }
  for (int64_t i = 4 * n4 + tid; i < n; i += nthr) {
    const uint32_t b = __float_as_uint(x[i]) & 0x7fffffffu;
    mx = b > mx ? b : mx;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)mx, m, 64);
    mx = o > mx ? o : mx;
  }
  uint32_t* w = reinterpret_cast<uint32_t*>(buf);
  __shared__ uint32_t last, wmax[4];
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {  // ONE atomic per workgroup (thousands of them on one address serialise: the launch took 50 us)
    const uint32_t a01 = wmax[0] > wmax[1] ? wmax[0] : wmax[1], a23 = wmax[2] > wmax[3] ? wmax[2] : wmax[3];
    atomicMax(w + 1, a01 > a23 ? a01 : a23);
    __threadfence();
    last = atomicAdd(w + 2, 1u) == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (last && threadIdx.x == 0) {
    __threadfence();
    const float amax = __uint_as_float(atomicMax(w + 1, 0u));
    float e = 0.f;
    const float q = 1024.0f / amax;  // inf for amax = 0 and for subnormal maxima, 0 for inf, NaN for NaN
    if (q > 0.f && q < __builtin_inff()) e = fminf(fmaxf(floorf(log2f(q)), -40.0f), 60.0f);  // (else 0, as nan_to_num did)
    buf[0] = ldexpf(1.0f, (int)e);
  }
}

extern "C" int fsn_grad_scale(const float* d_out, int64_t n, float* buf, fsn_stream_t stream) {
  FSN_REQUIRE(n >= 0 && buf && (n == 0 || d_out), FSN_E_INVALID, "fsn_grad_scale: bad arguments");
  int64_t blocks = (n + 256 * 16 - 1) / (256 * 16);
  blocks = blocks < 1 ? 1 : (blocks > 256 ? 256 : blocks);
  k_grad_scale<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(d_out, n, buf);
  FSN_LAUNCH_CHECK("k_grad_scale");
  return FSN_OK;
}
