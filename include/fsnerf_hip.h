/*
 * fsnerf_hip.h — C-ABI of libfsnerf_hip.so: the NeRF ray-rendering hot path of
 * a-lemus96/fs-nerf as hand-written HIP kernels for MI355X (gfx950 / CDNA4).
 *
 * The reference has no FFI of its own (it is 100 % Python): the path sits
 * behind Python callables.  Each entry point below therefore names the reference callable
 * (file:line under /root/reference) whose arithmetic it replaces; the Python host layer in
 * fs-nerf_amd/ keeps those callables' names and signatures and binds this library with ctypes
 * (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in `_host`;
 *   - tensors are dense row-major float32 unless stated; ray_indices is int64
 *     (reference contract, src/render/rendering.py:66,92);
 *   - the caller owns all memory; nothing is retained past the call's stream work;
 *   - all calls are asynchronous on `stream` (a hipStream_t; NULL = default stream);
 *   - return 0 on success, negative on error (FSN_E_*); the message is available from
 *     fsn_last_error() (thread-local).  Zero-sample / zero-ray inputs are not errors.
 */
#ifndef FSNERF_HIP_H
#define FSNERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fsn_stream_t; /* hipStream_t */

#define FSN_OK 0
#define FSN_E_INVALID (-1)     /* bad argument (null pointer, negative size, ...) */
#define FSN_E_UNSUPPORTED (-2) /* shape outside what the kernels are built for */
#define FSN_E_HIP (-3)         /* HIP runtime error (launch, no device, ...) */

/* arithmetic of the MLP contractions */
#define FSN_PREC_BF16X3 0 /* split-bf16 (hi+lo) x 3 MFMA passes, fp32 accumulate: ~1e-5 relative per product */
#define FSN_PREC_BF16 1   /* single bf16 MFMA pass, fp32 accumulate (BASELINE config 5).  The single-pass modes round
                             every operand to 16 bits and evaluate the encodings' sines with the hardware
                             instruction (|err| ~1e-4 rad, below that rounding) */
#define FSN_PREC_FP16X3 2 /* split-fp16 (hi + 2^-11 lo') x 3 MFMA passes, the two correction products in their own
                             accumulator: fp32-grade accuracy for layer scales from 2^-14 (6.1e-5) up to 65504 (both ends
                             reported through `status`, below) - the default "parity" mode */
#define FSN_PREC_FP16 3   /* single fp16 MFMA pass */
#define FSN_PREC_FP16X3U 4 /* round 4, inference entry points only: split-fp16 x 3 MFMA passes with UNSCALED low parts,
                             the three products of a unit in one accumulator, no merge in the epilogue (the arithmetic of
                             rounds 1-2: 6 % faster than FSN_PREC_FP16X3).  float32-grade because every layer's
                             activations are kept at 2^4 .. 2^10 by a power-of-two scale per layer that is folded into
                             the packed weights (fsn_mlp_pack_scaled; an exact transformation of the network, the outputs
                             are unscaled by the head weights) and calibrated from the layers' measured maxima
                             (fsn_mlp_layer_maxima).  Both ends of the calibration are reported through `status` */
#define FSN_PREC_FP16X2 6 /* two fp16 MFMA passes: activations high+low parts, weights' high part only (the x3 blob
                             layout; inference only).  Measured accuracy in DESIGN.md - not the parity mode */

/* Range guard of the fp16 modes.  Entry points that evaluate the MLP take `status`: a DEVICE pointer to one
 * uint32_t owned by the caller (or NULL = no report).  A kernel sets bit 0 (atomic OR, never clears) when a hidden
 * activation - or, in the training backward, a scaled gradient - reached fp16 infinity, i.e. left the range in
 * which FSN_PREC_FP16X3 / _FP16 / _FP16X2 are valid; the results of that launch are then not to be used (re-run in
 * FSN_PREC_BF16X3, which has the range of float32).  Bit 1 is the other end of the envelope of the split modes
 * (FSN_PREC_FP16X3 / _FP16X2, forward passes): in some layer the largest |activation| over a wavefront's 16 samples x
 * all features was non-zero but below 2^-14 (an fp16 subnormal); high + scaled low part then no longer carry 22 bits
 * relative to the layer's scale - results are finite and still ~bf16x3-grade, the caller decides (the Python host
 * re-runs in FSN_PREC_BF16X3).  FSN_PREC_FP16X3U keeps unscaled low parts (an fp16 subnormal, fixed 2^-24 resolution,
 * for |activation| < 2^-3): bit 1 there means that a wavefront's layer maximum was below 2^-4, i.e. the layer's scale
 * (fsn_mlp_pack_scaled) no longer fits the data - the caller re-calibrates and re-packs.  The bf16 modes set neither bit. */
#define FSN_STATUS_FP16_RANGE 1u
#define FSN_STATUS_FP16_SMALL 2u
#define FSN_STATUS_GRAD_RANGE 4u /* fsn_nerf_train_bwd with stage_scales: a stored gradient reached fp16 infinity - the
                                   call's gradients are zeroed, fsn_adam_step skips the update, the stage's scale drops
                                   (an event of the delayed gradient scaling like a loss scaler's, not a range fallback) */

int fsn_version(void);
/* Debug build only (make -C fs-nerf_amd/csrc debug -> libfsnerf_hip_dbg.so, -DFSN_DEBUG): the checked kernels'
 * indices are range-checked; a violation is recorded and clamped (or its thread skipped), not trapped (GPU sanitizers
 * are not available on this pool).  Each translation unit that checks keeps ONE record and registers it under a name:
 *   "render"     render.hip      every LDS index of k_render_fused
 *   "occ"        render_occ.hip  every LDS index of k_render_occ
 *   "raydata"    raydata.hip     explicit ray indices outside [0, N) and explicit patch anchors outside [0, A)
 *   "metrics"    metrics.hip     every LDS index of k_ssim_tile
 *   "ssim_grad"  ssim_grad.hip   every LDS index of the two kernels behind the SSIM gradient
 *   "lpips"      lpips.hip       every LDS index of k_lpips_conv and k_lpips_first_bwd
 *   "pose_refine" pose_refine.hip  ray indices outside [0, N) handed to fsn_ray_pose_grad / fsn_ray_camera_grad
 *   "warp"       warp.hip        source views outside [-1, n_views) and every tap offset of fsn_warp_sample_fwd / _bwd
 * A record is 4 uint32 = {violations, source line of the first, its index (or the end of its span), the extent}, the
 * last two truncated to 32 bits.  fsn_debug_report synchronises the device, copies the record of `unit` to out4 and
 * clears it; an unknown unit is FSN_E_INVALID (the message lists the known ones), the release library returns
 * FSN_E_UNSUPPORTED.  fsn_debug_units: the registered names, sorted and comma-separated ("" in the release library). */
int fsn_debug_report(const char* unit, uint32_t* out4);
const char* fsn_debug_units(void);
/* ... its negative control: a one-block launch with one deliberate out-of-range index and one out-of-range span into a
 * 32-element LDS array (the next fsn_debug_report("render") must say 2 violations, extent 32). */
int fsn_debug_selftest(void);
const char* fsn_last_error(void);
/* number of compute units of the current device (grid sizing), or negative on error */
int fsn_device_cus(void);

/* ---- a1: get_rays(pose, hwf, device)                     src/utils/utilities.py:36-82
 * pose_host: 12 floats = rows 0..2 of the camera-to-world matrix, row-major [3][4].
 * Rows [row0, row0+nrows) of the H x W image are produced (row0=0,nrows=H for a frame; a
 * rank renders its own row block).  rays_o, rays_d: [nrows*W, 3].  focal / near are doubles
 * because the reference forms W*0.5, 2*near and 1/(W/(2 focal)) in Python double precision
 * before rounding to float32 (utilities.py:67, 104-114).  Every entry point below that takes (H, W, focal, near) forms
 * these constants through the one pinhole_consts() of csrc/pinhole_consts.hpp. */
int fsn_get_rays(const float* pose_host, int H, int W, double focal, int row0, int nrows,
                 float* rays_o, float* rays_d, fsn_stream_t stream);

/* ---- a2: to_ndc(rays_o, rays_d, hwf, near)               src/utils/utilities.py:84-120 */
int fsn_to_ndc(const float* rays_o, const float* rays_d, int64_t n, int H, int W, double focal,
               double near, float* ndc_o, float* ndc_d, fsn_stream_t stream);

/* ---- f4: the datasets' ray tables       src/nerfdata/datasets/blender.py:174-191, llff.py:59-90
 * get_rays of ALL poses (DEVICE [n_poses, 12]: rows 0..2 of each camera-to-world matrix) in one launch, straight into
 * rays_o / rays_d [n_poses*H*W, 3] (pose-major, then row-major pixels: torch.stack(...).reshape(-1, 6) of the reference),
 * optionally mapped to NDC (utilities.py:84-120 with `near`), and - when aabb != NULL - the region of interest the
 * reference derives for its estimator (llff.py:77-84): aabb[0..2] = min, aabb[3..5] = max over all rays of {o, o + d},
 * divided by 2^(4-1); reduced inside the same launch (aabb_keys: 6 uint32 of DEVICE scratch).  Bit for bit the per-pose
 * fsn_get_rays / fsn_to_ndc / torch min-max sequence. */
int fsn_build_rays(const float* poses, int64_t n_poses, int H, int W, double focal, int ndc, double near,
                   float* rays_o, float* rays_d, float* aabb, uint32_t* aabb_keys, fsn_stream_t stream);

/* ---- the data layer: ray batches from the resident uint8 images and poses
 *                                          src/nerfdata/datasets/{blender,llff}.py, splitter.py:123-132
 * ONE launch, one thread per output ray: `count` rays starting at position `start` of an order over the
 * N = n_views*H*W rays of the dataset (flat ray index = view*H*W + h*W + w, the row of fsn_build_rays' tables):
 *   FSN_RAY_ORDER_IDENTITY   index = start + i
 *   FSN_RAY_ORDER_PERMUTED   index = perm(start + i; N, seed, epoch): a stateless bijection of [0, N) keyed by
 *                            (seed, epoch) (csrc/ray_perm.hpp: 4-round Feistel network + cycle walking); no N-sized table
 *   FSN_RAY_ORDER_EXPLICIT   index = indices[i] (DEVICE int64 [count]; start must be 0).  An index outside [0, N) never
 *                            reaches memory: its thread leaves its output rows untouched (and, in the debug build,
 *                            records it for fsn_debug_report("raydata")).
 * poses: DEVICE [n_views, 12] (rows 0..2 of camera-to-world); images: DEVICE uint8 [n_views, H, W, C], C = 3 or 4;
 * ndc / near as fsn_build_rays.  Outputs (DEVICE; each may be NULL = not wanted): rays_o, rays_d [count, 3] - bit for
 * bit row `index` of fsn_build_rays' tables; rgb [count, 3] - bit for bit the reference's float images: byte / 255 and,
 * with white_bkgd (C = 4 only), c * a + (1 - a) in three separate float32 operations (blender.py:114-117), else the
 * first three channels; index [count] int64 - the flat ray index served.
 * Errors (FSN_E_INVALID): null poses / images, C not in {3, 4}, white_bkgd with C = 3, start + count > N. */
#define FSN_RAY_ORDER_IDENTITY 0
#define FSN_RAY_ORDER_PERMUTED 1
#define FSN_RAY_ORDER_EXPLICIT 2
int fsn_ray_batch(const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C, double focal, int ndc,
                  double near, int white_bkgd, int order, uint64_t seed, int64_t epoch, const int64_t* indices,
                  int64_t start, int64_t count, float* rays_o, float* rays_d, float* rgb, int64_t* index,
                  fsn_stream_t stream);
/* A batch of P x P patches in ONE launch, one thread per output row: the data layer for losses that need several
 * rendered pixels at once (the SSIM term below, patch regularisers on depth).  With ext = (P-1)*dilation + 1,
 * AH = H - ext + 1 and AW = W - ext + 1, the ANCHORS (the patches' top-left pixels) number A = n_views*AH*AW;
 * anchor a is view v = a / (AH*AW), row r0 = (a % (AH*AW)) / AW, column c0 = a % AW; pixel (i, j) of its patch is image
 * pixel (r0 + i*dilation, c0 + j*dilation), flat ray index (v*H + r)*W + c.  `order`, `seed`, `epoch`, `start` and
 * `count` are those of the ray batch above read over anchors: start and count count PATCHES, the permutation is of
 * [0, A), `anchors` is the explicit DEVICE int64 [count] list (an anchor outside [0, A) leaves its P*P rows untouched
 * and is recorded in the debug build).  Outputs (each may be NULL): rays_o, rays_d, rgb [count*P*P, 3] and index
 * [count*P*P] int64, row (b*P + i)*P + j for pixel (i, j) of patch b - bit for bit the row the ray batch above serves
 * for that flat index in explicit order (one device function writes the rows of both).  images may be NULL when rgb is NULL: ray-only patches for any poses.
 * Errors (FSN_E_INVALID): P < 1, dilation < 1, ext > H or ext > W, start + count > A, and those of the ray batch. */
int fsn_ray_patch_batch(const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C, double focal,
                        int ndc, double near, int white_bkgd, int order, uint64_t seed, int64_t epoch,
                        const int64_t* anchors, int64_t start, int64_t count, int P, int dilation, float* rays_o,
                        float* rays_d, float* rgb, int64_t* index, fsn_stream_t stream);
/* The same permutation on the host (plain C++, no device is touched): out_host[i] = perm(start + i; N, seed, epoch) for
 * i < count, start + count <= N <= 2^62. */
int fsn_ray_perm_host(int64_t N, uint64_t seed, int64_t epoch, int64_t start, int64_t count, int64_t* out_host);

/* ---- learnable camera poses behind the data layer (this package's own)       csrc/pose_refine.hip
 * View v carries a correction xi_v = (omega_v, tau_v) (6 floats) on top of its stored pose [R0_v | t0_v]:
 *   R_v = exp([omega_v]x) R0_v (left-multiplied, world frame),  t_v = t0_v + tau_v,
 *   exp([omega]x) = I + A K + B K^2,  K = [omega]x,  A = sin(theta) / theta,  B = (1 - cos(theta)) / theta^2,  theta = |omega|
 * (Taylor forms below theta = 0.125; supported range theta < pi).  xi = 0 gives the stored pose back value for value.
 * fsn_pose_compose: poses0 [n, 12], xi [n, 6] -> poses_out [n, 12] (all DEVICE), one thread per view: the matrices that
 * fsn_ray_batch / fsn_ray_patch_batch are then launched over.
 * Errors (FSN_E_INVALID): n < 0, a null pointer. */
int fsn_pose_compose(const float* poses0, const float* xi, int64_t n, float* poses_out, fsn_stream_t stream);
/* The backward of "flat ray index -> ray of the corrected pose" (the rays fsn_ray_batch serves over fsn_pose_compose's
 * matrices, NDC map included when `ndc` is set; H, W, focal, ndc, near as there), reduced per view in ONE launch:
 * index [count] int64 (the batch's flat ray indices), grad_o / grad_d [count, 3] = dL/drays_o, dL/drays_d (either may be
 * NULL = zeros) -> grad_xi [n_views, 6] = (dL/domega, dL/dtau), WRITTEN (not accumulated) for every view: exactly 0 for
 * a view without a ray in the batch.  grad_poses [n_views, 12] (may be NULL): dL/d(the corrected 3x4 matrices).
 * No atomics and a fixed summation order: the same inputs give the same bits.  An index outside [0, n_views*H*W)
 * contributes nothing (and, in the debug build, is recorded for fsn_debug_report("pose_refine")).
 * Errors (FSN_E_INVALID): n_views < 0, H, W or focal <= 0, count < 0, null poses0 / xi / grad_xi, null index with
 * count > 0; FSN_E_UNSUPPORTED: H*W or n_views of 2^31 or more. */
int fsn_ray_pose_grad(const float* poses0, const float* xi, int64_t n_views, int H, int W, double focal, int ndc,
                      double near, const int64_t* index, const float* grad_o, const float* grad_d, int64_t count,
                      float* grad_xi, float* grad_poses, fsn_stream_t stream);

/* ---- learnable intrinsics behind the data layer (this package's own)
 *                                                                           csrc/pose_refine.hip, csrc/raydata.hip
 * A camera table K = (fx, fy, cx, cy), float32 [k_rows, 4] on the DEVICE, k_rows = 1 (shared by all views) or n_views.
 * The camera-frame direction of pixel (h, w) is u / |u|, u = ((w - cx)/fx, -(h - cy)/fy, -1): the arithmetic of
 * fsn_ray_batch with the table's values in place of its launch constants (focal, focal, (float)(W*0.5), (float)(H*0.5)).
 * fsn_intrinsics_compose: phi [m, 4] -> K_out [m, 4] (both DEVICE), one thread per row:
 *   fx = f0 exp(phi_0),  fy = f0 exp(phi_1) (tie_focal: fy = fx, phi_1 unused),  cx = W/2 + W phi_2,  cy = H/2 + H phi_3
 * with f0 = (float)focal0; phi = 0 gives fsn_ray_batch's launch constants value for value.
 * Errors (FSN_E_INVALID): m < 0, H, W or focal0 <= 0, a null pointer. */
int fsn_intrinsics_compose(const float* phi, int64_t m, int H, int W, double focal0, int tie_focal, float* K_out,
                           fsn_stream_t stream);
/* fsn_ray_batch / fsn_ray_patch_batch over a camera table: the same arguments plus K [k_rows, 4]; the same kernels
 * (a compile-time switch), the same rows but for the pinhole direction, which is the table's.  `focal` keeps feeding the
 * NDC constants: the NDC map is a fixed warp of space and does not follow the learned focal.
 * Errors: those of the two entry points; FSN_E_INVALID for a null K or k_rows not in {1, n_views}. */
int fsn_ray_batch_k(const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C, double focal,
                    const float* K, int64_t k_rows, int ndc, double near, int white_bkgd, int order, uint64_t seed,
                    int64_t epoch, const int64_t* indices, int64_t start, int64_t count, float* rays_o, float* rays_d,
                    float* rgb, int64_t* index, fsn_stream_t stream);
int fsn_ray_patch_batch_k(const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C, double focal,
                          const float* K, int64_t k_rows, int ndc, double near, int white_bkgd, int order, uint64_t seed,
                          int64_t epoch, const int64_t* anchors, int64_t start, int64_t count, int P, int dilation,
                          float* rays_o, float* rays_d, float* rgb, int64_t* index, fsn_stream_t stream);
/* ---- auxiliary planes behind the data layer (this package's own; DESIGN.md 7 "Data layer")       csrc/raydata.hip
 * Per-pixel float targets other than colour (sparse or sensor depth, masks, a monocular depth prior), served in the
 * batch's own launch: aux DEVICE float32 [n_views*H*W, aux_channels] (1 <= aux_channels <= 4; any bit pattern, NaN is
 * the documented "nothing known here"), aux_out DEVICE [count, aux_channels] ([count*P*P, aux_channels] for patches; may
 * be NULL = not wanted).  Row i of aux_out is aux[idx_i*aux_channels .. idx_i*aux_channels + aux_channels) for the flat
 * ray index idx_i of that row, copied bit for bit.  Every other argument and output is that of fsn_ray_batch_k /
 * fsn_ray_patch_batch_k, and K == NULL with k_rows == 0 means the stored intrinsics (fsn_ray_batch / fsn_ray_patch_batch):
 * the same kernels behind a second compile-time switch, the same rows.  An explicit index or anchor outside the range
 * leaves its aux row untouched like every other output (recorded for fsn_debug_report("raydata") in the debug build).
 * Errors (FSN_E_INVALID): aux_out without aux, aux_channels outside 1..4, and those of the underlying calls. */
int fsn_ray_batch_aux(const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C, double focal,
                      const float* K, int64_t k_rows, int ndc, double near, int white_bkgd, int order, uint64_t seed,
                      int64_t epoch, const int64_t* indices, int64_t start, int64_t count, float* rays_o, float* rays_d,
                      float* rgb, int64_t* index, const float* aux, int aux_channels, float* aux_out, fsn_stream_t stream);
int fsn_ray_patch_batch_aux(const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C, double focal,
                            const float* K, int64_t k_rows, int ndc, double near, int white_bkgd, int order, uint64_t seed,
                            int64_t epoch, const int64_t* anchors, int64_t start, int64_t count, int P, int dilation,
                            float* rays_o, float* rays_d, float* rgb, int64_t* index, const float* aux, int aux_channels,
                            float* aux_out, fsn_stream_t stream);
/* The backward of "flat ray index -> ray of the corrected pose under the camera table", reduced per view in ONE launch:
 * fsn_ray_pose_grad's walk (the other instantiation of its kernel template: one workgroup per view, no atomics, a fixed
 * summation order) with four more sums.
 * xi [n_views, 6] may be NULL = no correction (the rays were served over poses0).  Outputs, WRITTEN for every view and
 * exactly 0 for a view without a ray in the batch: grad_xi [n_views, 6] (may be NULL) - with the stored intrinsics in K
 * bit for bit fsn_ray_pose_grad's; grad_K_views [n_views, 4] = this view's rays' share of dL/d(fx, fy, cx, cy).
 * focal0 feeds the NDC constants only.  An index outside [0, n_views*H*W) contributes nothing (and, in the debug build,
 * is recorded for fsn_debug_report("pose_refine")).
 * Errors (FSN_E_INVALID): n_views < 0, H, W or focal0 <= 0, count < 0, null poses0 / K / grad_K_views, null index with
 * count > 0, k_rows not in {1, n_views}; FSN_E_UNSUPPORTED: H*W or n_views of 2^31 or more. */
int fsn_ray_camera_grad(const float* poses0, const float* xi, int64_t n_views, int H, int W, double focal0, const float* K,
                        int64_t k_rows, int ndc, double near, const int64_t* index, const float* grad_o,
                        const float* grad_d, int64_t count, float* grad_xi, float* grad_K_views, fsn_stream_t stream);
/* The chain K -> phi: grad_K_views [n_views, 4] -> grad_phi [m, 4] (WRITTEN), m = 1 or n_views:
 *   dL/dphi_0 = fx dL/dfx (+ fy dL/dfy with tie_focal, and then dL/dphi_1 = 0),  dL/dphi_1 = fy dL/dfy,
 *   dL/dphi_2 = W dL/dcx,  dL/dphi_3 = H dL/dcy.
 * m = 1 sums over the views first, in float64, in a fixed order inside one workgroup; m = n_views: one thread per view.
 * Errors (FSN_E_INVALID): n_views < 0, H, W or focal0 <= 0, m not in {1, n_views}, a null pointer. */
int fsn_intrinsics_grad(const float* phi, const float* grad_K_views, int64_t n_views, int64_t m, int H, int W,
                        double focal0, int tie_focal, float* grad_phi, fsn_stream_t stream);

/* ---- unseen views: random poses and their patch rays (this package's own, after RegNeRF's)
 *                                                                                              csrc/unseen_views.hip
 * Pose draw g of a distribution is a pure function of (dist, seed, g): no state on the device or the host, no
 * transcendental function, every operation a float32 +, -, *, / or sqrtf in the order of csrc/unseen_views.hip (the
 * library is built with -ffp-contract=off), so tests/unseen_ref.py restates it bit for bit in NumPy.
 *   bits(g, slot) = mix(mix(seed ^ mix(g)) + slot), mix = the splitmix64 finaliser of csrc/ray_perm.hpp;
 *   u(g, slot) = (bits >> 40) * 2^-24 in [0, 1).  Slots of a pose draw g: 0, 1, 2 origin; 3, 4, 5 target; 6 + 2k, 7 + 2k
 *   the k-th try (k < 16) of the azimuth's disc rejection.  Slots of a PATCH q: 38 anchor row, 39 anchor column.
 * mode FSN_UNSEEN_SHELL: z = min(z_lo + u0 (z_hi - z_lo), z_hi), r = min(r_lo + u1 (r_hi - r_lo), r_hi), (c, s) = (a, b) /
 *   sqrt(a^2 + b^2) of the first try (a, b) = (2 u - 1, 2 u' - 1) with 0 < a^2 + b^2 <= 1, (1, 0) after 16 failures;
 *   h = sqrt(1 - z z); origin = centre + r ((h c e1 + h s e2) + z up).  Needs -1 < z_lo <= z_hi < 1, 0 <= r_lo <= r_hi.
 * mode FSN_UNSEEN_BOX: origin_k = min(lo_k + u_k (hi_k - lo_k), hi_k), k = 0, 1, 2.  Needs lo <= hi.
 * Both: target_k = focus_k + jitter (2 u_{3+k} - 1); v = origin - target, zc = v / |v| (up when |v|^2 < 1e-20);
 *   x = up x zc (e1 x zc when |up x zc|^2 < 1e-8), xc = x / |x|, yc = zc x xc; the pose is rows [xc_k yc_k zc_k origin_k]:
 *   the camera looks down its own -z with y up, the convention of fsn_get_rays.  (e1, e2, up) is an orthonormal frame,
 *   which the caller provides; the entry points check the ranges above, finiteness and jitter >= 0. */
#define FSN_UNSEEN_SHELL 0
#define FSN_UNSEEN_BOX 1
typedef struct fsn_unseen_dist {
  int32_t mode;
  float jitter;
  float focus[3];
  float up[3];
  float e1[3];
  float e2[3];
  float centre[3]; /* shell */
  float r_lo, r_hi, z_lo, z_hi;
  float lo[3]; /* box */
  float hi[3];
} fsn_unseen_dist;
/* Pose draws [first_draw, first_draw + count) -> poses_out [count, 12] (DEVICE), one thread per pose.
 * Errors (FSN_E_INVALID): a null pointer, negative first_draw or count, a distribution outside the ranges above. */
int fsn_unseen_poses(const fsn_unseen_dist* dist_host, uint64_t seed, int64_t first_draw, int64_t count, float* poses_out,
                     fsn_stream_t stream);
/* `count` patches of P x P rays of freshly drawn poses in ONE launch, one thread per output row (b*P + i)*P + j: patch
 * q = first_patch + b is seen from pose draw g = q / patches_per_pose; its anchor (row0, col0) is uniform on the
 * AH x AW lattice, AH = H - ext + 1, AW = W - ext + 1, ext = (P-1)*dilation + 1: row0 = (hi32(bits(q, 38)) * AH) >> 32,
 * col0 = (hi32(bits(q, 39)) * AW) >> 32; the row is the ray of pixel (row0 + i*dilation, col0 + j*dilation) over that
 * pose - H, W, focal, ndc, near and the arithmetic are those of fsn_ray_patch_batch, whose rows over poses_out with the
 * explicit anchors b*AH*AW + anchors_out[b] these are bit for bit.  Every thread recomputes its patch's pose: no LDS, no
 * atomics, no index is read.  Outputs (DEVICE): rays_o, rays_d [count*P*P, 3] (either may be NULL, not both with the
 * other two), poses_out [count, 12] and anchors_out [count] int64 = row0*AW + col0 (each may be NULL).
 * Errors (FSN_E_INVALID): those of fsn_unseen_poses, P < 1, dilation < 1, patches_per_pose < 1, ext > H or ext > W, null
 * pointer for every output; FSN_E_UNSUPPORTED: more than 2^38 rows in one call. */
int fsn_unseen_patch_batch(const fsn_unseen_dist* dist_host, uint64_t seed, int64_t first_patch, int64_t count,
                           int64_t patches_per_pose, int H, int W, double focal, int P, int dilation, int ndc, double near,
                           float* rays_o, float* rays_d, float* poses_out, int64_t* anchors_out, fsn_stream_t stream);

/* ---- a4: PositionalEncoder.forward(x)                    src/core/models.py:43-50
 * x [n, d_in] -> out [n, d_in*(1+2*n_freqs)], block order x, sin f0, cos f0, sin f1, ...
 * freqs_host: n_freqs float32 values (models.py:31-34).  mask (device, [d_out]) may be NULL:
 * the build's frequency mask, multiplied onto the encoded features (mask==1 = reference). */
int fsn_posenc_fwd(const float* x, int64_t n, int d_in, int n_freqs, const float* freqs_host,
                   const float* mask, float* out, fsn_stream_t stream);

/* ---- a8: the `estimator.sampling` slot                   src/render/rendering.py:66-74
 * Fixed-count stratified sampler (build's definition): S+1 sorted interval
 * edges per ray, edges [R, S+1].  u_mode 0: u ignored, e_i = near + i*step;
 * 1: u [R], one shift per ray, e_i = near + (i+u_r)*step; 2: u [R, S+1], per-edge jitter. */
int fsn_stratified_edges(float near, float far, int S, int64_t R, const float* u, int u_mode,
                         float* edges, fsn_stream_t stream);
/* edges [R, S+1] -> packed (ray_indices int64 [R*S], t_starts [R*S], t_ends [R*S]) */
int fsn_edges_to_packed(const float* edges, int64_t R, int S, int64_t* ray_indices,
                        float* t_starts, float* t_ends, fsn_stream_t stream);
/* hierarchical "+n_imp" step: inverse-CDF samples of the piecewise-constant pdf given by the
 * coarse weights [R,S] over edges [R,S+1], merged with the coarse edges and sorted:
 * edges_out [R, S+1+n_imp].  u [R, n_imp] or NULL (deterministic linspace(0,1,n_imp)). */
int fsn_sample_pdf_merge(const float* edges, const float* weights, int64_t R, int S, int n_imp,
                         const float* u, float* edges_out, fsn_stream_t stream);

/* ---- a7: nerfacc.volrend.rendering arithmetic            call site src/render/rendering.py:89-96
 * Dense form: every ray has S samples; sigmas [R,S], rgbs [R,S,3], t_starts/t_ends [R,S].
 * colors [R,3], opacity [R], depth [R]; weights/alphas/trans [R,S] may be NULL.
 * bkgd_host: 3 floats (render_bkgd) or NULL (no background term). */
int fsn_composite_fwd(const float* sigmas, const float* rgbs, const float* t_starts,
                      const float* t_ends, int64_t R, int S, const float* bkgd_host,
                      float* colors, float* opacity, float* depth, float* weights,
                      float* alphas, float* trans, fsn_stream_t stream);
/* Packed (variable samples per ray) form with the reference's own contract: samples of a ray
 * are contiguous; ray_indices int64 [N] non-decreasing.  Rays with no sample get the
 * background colour, zero opacity and zero depth (reference fallback, rendering.py:97-103). */
int fsn_composite_packed_fwd(const float* sigmas, const float* rgbs, const float* t_starts,
                             const float* t_ends, const int64_t* ray_indices, int64_t N,
                             int64_t R, const float* bkgd_host, float* colors, float* opacity,
                             float* depth, float* weights, float* alphas, float* trans,
                             fsn_stream_t stream);

/* ---- a5: NeRF(d_pos,d_dir,n_layers,d_hidden,skip,...).forward(x, dirs)   src/core/models.py:53-143 */
typedef struct fsn_mlp_desc {
  int32_t n_layers;    /* hidden layers before the bottleneck (8)                 */
  int32_t d_hidden;    /* 256 or 128                                              */
  uint32_t skip_mask;  /* bit i set: x_in is concatenated after layer i (i < n_layers-1) */
  int32_t n_freqs_pos; /* <= 10 */
  int32_t n_freqs_dir; /* <= 4  */
  float freqs_pos[16]; /* models.py:31-34 values */
  float freqs_dir[16];
} fsn_mlp_desc;

/* Size in bytes of the packed-weights blob for (desc, prec); negative on error. */
int64_t fsn_mlp_blob_bytes(const fsn_mlp_desc* desc, int prec);
/* Pack a reference-format state_dict into the MFMA streaming layout (DESIGN.md "weight blob").
 * weights / biases: HOST arrays of n_layers+4 DEVICE pointers in the order
 *   layers.0 .. layers.{n_layers-1}, sigma, connection, branch, rgb
 * each weight row-major [out, in] exactly as in the state_dict (src/core/models.py:96-108). */
int fsn_mlp_pack(const fsn_mlp_desc* desc, int prec, const float* const* weights_host_of_dev,
                 const float* const* biases_host_of_dev, void* blob, fsn_stream_t stream);
/* fsn_mlp_pack of the SCALED network (round 4; any prec, meant for FSN_PREC_FP16X3U).  layer_exps_host: n_layers + 2
 * int32 exponents e_g, one per GEMM in kernel order (hidden layers 0 .. n_layers-1, connection, branch), or NULL = all
 * zero = fsn_mlp_pack.  With s_g = 2^e_g the blob holds the network whose GEMM g produces s_g times the reference's
 * activations: rows of W_g that multiply activations are scaled by s_g / s_(g-1) (the connection and the sigma head read
 * layer n_layers-1, the branch reads the connection), rows that multiply an encoding by s_g, biases by s_g, sigma.weight
 * by 1 / s_(n_layers-1), rgb.weight by 1 / s_branch.  Every factor is a power of two and ReLU commutes with it: in exact
 * arithmetic the outputs are the reference's (src/core/models.py:111-143); the point is that the 16-bit parts the
 * kernels form sit where fp16 is accurate whatever the network's own scale.  |e_g| <= 60. */
int fsn_mlp_pack_scaled(const fsn_mlp_desc* desc, int prec, const float* const* weights_host_of_dev,
                        const float* const* biases_host_of_dev, const int32_t* layer_exps_host, void* blob,
                        fsn_stream_t stream);
/* Calibration of those scales: NeRF.forward(x, dirs) on n probe samples (any blob / prec; FSN_PREC_BF16X3 on an
 * unscaled blob has float32's range) reporting, per GEMM in kernel order, the largest |output after its activation|
 * (ReLU layers, branch: max relu; connection: max |feat|) seen by any sample.  maxima: DEVICE float32 [n_layers + 2],
 * zeroed by the caller (the launch takes the maximum with what is there, so several probes may accumulate).  Values are
 * those of the blob's own scale (a blob packed with exponents e reports 2^e_g x the reference's).  No other output. */
int fsn_mlp_layer_maxima(const fsn_mlp_desc* desc, int prec, const void* blob, const float* x, const float* dirs,
                         const float* pos_mask, const float* dir_mask, int64_t n, float* maxima, fsn_stream_t stream);
/* Same packing on the CPU with HOST pointers and a HOST blob (format tests, no GPU needed). */
int fsn_mlp_pack_host(const fsn_mlp_desc* desc, int prec, const float* const* weights_host,
                      const float* const* biases_host, void* blob_host);
int fsn_mlp_pack_scaled_host(const fsn_mlp_desc* desc, int prec, const float* const* weights_host,
                             const float* const* biases_host, const int32_t* layer_exps_host, void* blob_host);
/* The two weight streams the training backward packs into its workspace, on their own (format tests; the backward calls
 * the same packer).  They have the blob's stream format - units of 1 KiB of 16-bit high parts and, in the x3 modes,
 * 1 KiB of low parts, lane-linear MFMA A fragments - and no header or aux region:
 *   FSN_WSTREAM_BWD         the dgrad chain's transposed weights: branch^T (first d_hidden input columns), connection^T,
 *                           layers n_layers-1 .. 1 (their d_hidden activation columns), padded with zeros to whole
 *                           16-KiB phases; want_x / want_dirs are not read
 *   FSN_WSTREAM_INPUT_GRAD  the encoding columns of layer 0 and the skip-fed layers (when want_x != 0), then of the
 *                           branch (when want_dirs != 0), transposed, rows in the encoder's slot order; no padding
 * prec: a training mode (FSN_PREC_BF16X3, _BF16, _FP16X3, _FP16), any other value is FSN_E_UNSUPPORTED.  An unknown
 * kind, a null pointer, or FSN_WSTREAM_INPUT_GRAD with both flags zero is FSN_E_INVALID; a descriptor fsn_mlp_blob_bytes
 * refuses is refused with the same code.  weights: n_layers+4 pointers in fsn_mlp_pack's order; those the stream does
 * not read (sigma, rgb, ...) are not dereferenced.
 * fsn_weight_stream_bytes: the stream's size in bytes (negative on error); dst / dst_host hold that many. */
#define FSN_WSTREAM_BWD 1
#define FSN_WSTREAM_INPUT_GRAD 2
int64_t fsn_weight_stream_bytes(const fsn_mlp_desc* desc, int prec, int kind, int want_x, int want_dirs);
int fsn_weight_stream_pack(const fsn_mlp_desc* desc, int prec, int kind, int want_x, int want_dirs,
                           const float* const* weights_host_of_dev, void* dst, fsn_stream_t stream);
int fsn_weight_stream_pack_host(const fsn_mlp_desc* desc, int prec, int kind, int want_x, int want_dirs,
                                const float* const* weights_host, void* dst_host);
/* x [n,3]; dirs [n,3] or NULL.  out [n,4]=[r,g,b,sigma] when dirs != NULL, else [n,1]=sigma.
 * pos_mask [3*(1+2*n_freqs_pos)] / dir_mask [3*(1+2*n_freqs_dir)] device pointers or NULL. */
int fsn_mlp_fwd(const fsn_mlp_desc* desc, int prec, const void* blob, const float* x,
                const float* dirs, const float* pos_mask, const float* dir_mask, int64_t n,
                float* out, uint32_t* status, fsn_stream_t stream);
/* fsn_mlp_fwd_rays: the same forward with the samples given as the reference's closures form them (sigma_fn /
 * rgb_sigma_fn, src/render/rendering.py:58-64, 76-84): sample s is the midpoint of [t_starts[s], t_ends[s]) on ray
 * ray_indices[s], x = o + d (t0 + t1) / 2 evaluated in the launch in the reference's operation order, dirs = d
 * (full != 0: [n,4] output, else [n,1]) - no [n,3] position / direction tensors in HBM. */
int fsn_mlp_fwd_rays(const fsn_mlp_desc* desc, int prec, const void* blob, const float* rays_o, const float* rays_d,
                     const int64_t* ray_indices, const float* t_starts, const float* t_ends, int full,
                     const float* pos_mask, const float* dir_mask, int64_t n, float* out, uint32_t* status,
                     fsn_stream_t stream);

/* ---- a6: render_rays(rays_o, rays_d, estimator, model, ...)   src/render/rendering.py:25-107
 * The whole path fused in one launch for the fixed-count sampler: stratified edges ->
 * [density pass of the coarse net -> weights -> sample_pdf -> sorted union] -> full pass of
 * the fine net -> volume integration.  n_imp == 0 renders the S coarse intervals with
 * `blob_fine` only (blob_coarse unused).  S_out = S + n_imp intervals per ray.
 *   u_mode/u as fsn_stratified_edges; u_fine [R,n_imp] or NULL (deterministic).
 *   rays_o / rays_d [R,3], or rays_o == NULL and the cam_* fields (rays generated in the launch);
 *   outputs: colors [R,3], opacity [R], depth [R]; optional (NULL to skip):
 *   weights, alphas, trans, sigmas [R,S_out], rgbs [R,S_out,3], edges_out [R,S_out+1],
 *   weights_coarse [R,S] (only written when n_imp > 0). */
typedef struct fsn_render_args {
  const float* rays_o; /* [R,3] */
  const float* rays_d; /* [R,3] */
  int64_t R;
  float near, far;
  int32_t S, n_imp;
  int32_t u_mode;
  const float* u;
  const float* u_fine;
  const float* pos_mask;
  const float* dir_mask;
  float bkgd[3];
  float* colors;
  float* opacity;
  float* depth;
  float* weights;
  float* alphas;
  float* trans;
  float* sigmas;
  float* rgbs;
  float* edges_out;
  float* weights_coarse;
  uint32_t* status; /* range guard of the fp16 modes (above), or NULL */
  /* f3: rays generated inside the launch.  When rays_o == NULL (rays_d ignored), ray r is pixel
   * (cam_row0 + r / cam_W, r % cam_W) of the cam_H x cam_W pinhole image of `cam_pose` (12 floats, rows 0..2 of the
   * camera-to-world matrix) with focal length cam_focal: the arithmetic of fsn_get_rays (utilities.py:57-80),
   * so a frame is ONE launch with no ray tensors in HBM.  R = number of pixels rendered. */
  float cam_pose[12];
  int32_t cam_H, cam_W, cam_row0;
  double cam_focal;
  /* Hierarchical launches over many rays run in two phases when `edges_out` is given (it doubles as the hand-over
   * buffer): every workgroup first runs the coarse pass + resampling of ALL its ray groups, then the fine pass of
   * all of them, so that an XCD's L2 holds ONE network's weight stream at a time (2.0 / 2.3 MB of the 4 MiB)
   * instead of both.  Results are identical.  two_phase: 0 = never, 1 = whenever edges_out != NULL and n_imp > 0,
   * 2 = SAMPLER ONLY: the launch stops after the coarse pass + resampling; edges_out [R,S+n_imp+1] (and
   * weights_coarse when given) are its results, the per-ray outputs are not written and may be NULL, blob_fine may be
   * NULL.  This is estimator.sampling of the hierarchical sampler (stratified edges -> density pass -> weights ->
   * inverse-CDF resampling -> sorted union) as ONE launch in front of the training forward. */
  int32_t two_phase;
  /* Measurement aid (bench.py, NULL = off): DEVICE uint64_t[2].  Wave 0 of workgroup 0 reads the shader clock counter
   * (s_memtime) and the constant 100 MHz counter (s_memrealtime) when it enters and when it leaves the kernel and ADDS
   * the two differences to clock_out[0] / clock_out[1]: their ratio x 0.1 is the clock in GHz the chip held during the
   * launch(es) - workgroup 0 lives as long as the persistent launch does. */
  uint64_t* clock_out;
} fsn_render_args;

int fsn_render_rays_fused(const fsn_mlp_desc* desc, int prec, const void* blob_coarse,
                          const void* blob_fine, const fsn_render_args* args_host,
                          fsn_stream_t stream);

/* Measurement aid (bench.py's `roofline.bare_stream`; not part of the path): the fused kernel's own MFMA stream with
 * nothing else in the kernel.  One persistent 512-thread workgroup per compute unit runs `layers` 256 -> 256 hidden
 * layers back to back through the SAME code as the render kernels (mlp_dev.hpp gemm_layer: the hand-scheduled GEMM-pair
 * blocks, the pair epilogues with ReLU / 16-bit split / range tracking, the weight stream's LDS-DMA ring with its
 * barriers) on fixed pseudo-random activations, the weight stream WALKING the hidden phases of a real packed blob
 * (d_hidden 256, x3 / x2 modes) like a density pass does - no encodings, heads, samplers, compositing or tile tails.
 * clock_out: DEVICE uint64_t[2 * 8 * n_workgroups] or NULL: per wave the s_memtime and s_memrealtime differences
 * around the loop.  Returns the number of workgroups launched (> 0) or an FSN_E_* code; per workgroup and layer the
 * stream issues 8 waves x 384 MFMAs (v_mfma_f32_16x16x32, 16,384 FLOP each) and fills 256 KiB from L2. */
int fsn_bench_bare_stream(const fsn_mlp_desc* desc, int prec, const void* blob, int layers, uint64_t* clock_out,
                          fsn_stream_t stream);

/* ---- a6 with the occupancy estimator in the `estimator` slot: the path the reference itself renders with
 * (render_rays, src/render/rendering.py:58-107; OccGridEstimator, src/run-nerf.py:96-98, 288-295) in ONE launch:
 * grid march -> density pass (sigma_fn) -> visibility cull -> full pass (rgb_sigma_fn) -> packed volume integration,
 * per batch of rays inside persistent workgroups, no host sync for the data-dependent sample count.  Same sampling
 * rule and arithmetic as fsn_occgrid_march + fsn_mlp_fwd + fsn_packed_visibility + fsn_mlp_fwd +
 * fsn_composite_packed_fwd (the results are the unfused sequence's).  Outputs per ray only: colors [R,3], opacity [R],
 * depth [R] (what render_frame consumes, rendering.py:169-171), optional sample counts per ray n_cand / n_kept [R]
 * (int32; NULL to skip); the per-sample extras of render_rays' full return contract in EXTRAS mode (below).
 *   aabb / res / levels / bits / near_plane / far_plane / step / u (one jitter value per ray or NULL) / max_steps as
 *   fsn_occgrid_march (max_steps <= 2048 here, else FSN_E_UNSUPPORTED); early_stop_eps / alpha_thre as
 *   fsn_packed_visibility (both <= 0: no density pass, every marched sample is kept);
 *   rays_o / rays_d [R,3], or rays_o == NULL and the cam_* fields as in fsn_render_args;
 *   work_counter: 8 bytes of DEVICE scratch (the launch zeroes it: the global ray-chunk queue);
 *   prec: FSN_PREC_BF16X3 .. FSN_PREC_FP16. */
typedef struct fsn_occ_render_args {
  const float* rays_o;
  const float* rays_d;
  int64_t R;
  float aabb[6];
  int32_t res, levels;
  const uint32_t* bits;
  float near_plane, far_plane, step;
  const float* u;
  int32_t max_steps;
  float early_stop_eps, alpha_thre;
  const float* pos_mask;
  const float* dir_mask;
  float bkgd[3];
  float* colors;
  float* opacity;
  float* depth;
  int32_t* n_cand;
  int32_t* n_kept;
  uint32_t* status;
  void* work_counter;
  float cam_pose[12];
  int32_t cam_H, cam_W, cam_row0;
  double cam_focal;
  /* SAMPLER mode (sample_t0 != NULL; estimator.sampling(..., sigma_fn) of a training step, rendering.py:58-74): every
   * batch stops after the visibility cull; per ray the kept count goes to n_kept (required) and the kept samples'
   * interval starts to sample_t0[ray * sample_cap + i] (sample_cap >= max_steps); colors / opacity / depth are not
   * written and may be NULL.  fsn_occ_gather_samples packs the slots behind an exclusive scan of n_kept. */
  float* sample_t0;
  int32_t sample_cap;
  /* EXTRAS mode (round 4; ex_weights != NULL, with sample_t0 / sample_cap / n_kept as above): render_rays' FULL return
   * contract (rendering.py:88-107: (rgb, opacity, depth, extras), ray_indices, t_vals) in the one launch, without
   * gradients.  The launch runs the full pass and the integration as usual (colors / opacity / depth are written) and
   * additionally leaves, in per-ray slot rows of sample_cap entries, the kept samples' weights / alphas / trans / sigmas
   * [R, sample_cap] and rgbs [R, sample_cap, 3] next to their interval starts in sample_t0; fsn_occ_gather_extras packs
   * them behind an exclusive scan of n_kept into nerfacc's packed [N] arrays. */
  float* ex_weights;
  float* ex_alphas;
  float* ex_trans;
  float* ex_sigmas;
  float* ex_rgbs;
} fsn_occ_render_args;

int fsn_render_rays_occgrid(const fsn_mlp_desc* desc, int prec, const void* blob, const fsn_occ_render_args* args_host,
                            fsn_stream_t stream);
/* fsn_render_rays_occgrid_ex: the same launch with the march of fsn_occgrid_march_ex - its definition below, per-ray
 * bounds and cone regime included, is the fused kernel's as well (one device function serves both kernels), so the
 * results stay the unfused sequence's with fsn_occgrid_march_ex in the first place.  fsn_render_rays_occgrid is this
 * entry point with cone_angle = 0 and NULL pointers: one kernel template serves both, instantiated without the extended
 * march for such a launch (the code of the plain lattice) and with it otherwise - the same results where both apply.
 *   cone_angle / t_min / t_max (DEVICE float [R] or NULL): as fsn_occgrid_march_ex; every candidate keeps the interval
 *   end the march gave it (no common width).  max_steps counts the cone march's intervals (<= 2048 here).
 *   sample_t1: DEVICE float [R, sample_cap] or NULL: in the sampler / extras mode the kept samples' interval ENDS, next
 *   to their starts in sample_t0; required there when cone_angle > 0 (an end is not start + step), ignored outside
 *   those modes.
 * FSN_E_INVALID (before any device work): cone_angle < 0; cone_angle > 0 with near_plane < 0; t_min / t_max with a
 * camera instead of ray arrays; cone_angle > 0 in the sampler / extras mode without sample_t1. */
int fsn_render_rays_occgrid_ex(const fsn_mlp_desc* desc, int prec, const void* blob, const fsn_occ_render_args* args_host,
                               float cone_angle, const float* t_min, const float* t_max, float* sample_t1,
                               fsn_stream_t stream);
/* Packed (ray_indices, t_starts, t_ends = t_start + step) from the sampler mode's per-ray slots: offsets = exclusive
 * scan of n_kept (int64 [R]); the outputs hold sum(n_kept) entries, sorted by ray then t - what fsn_occgrid_march +
 * fsn_packed_visibility + a compaction produce, bit for bit. */
int fsn_occ_gather_samples(const int32_t* n_kept, const int64_t* offsets, const float* sample_t0, int sample_cap,
                           int64_t R, float step, int64_t* ray_indices, float* t_starts, float* t_ends,
                           fsn_stream_t stream);
/* fsn_occ_gather_samples plus the EXTRAS mode's slot rows -> packed weights / alphas / trans / sigmas [N], rgbs [N,3]
 * (slots / outputs in that order: HOST arrays of 5 DEVICE pointers). */
int fsn_occ_gather_extras(const int32_t* n_kept, const int64_t* offsets, const float* sample_t0, int sample_cap, int64_t R,
                          float step, int64_t* ray_indices, float* t_starts, float* t_ends,
                          const float* const* slots_host_of_dev, float* const* out_host_of_dev, fsn_stream_t stream);
/* Both gathers with optional end rows: sample_t1 (fsn_render_rays_occgrid_ex) != NULL: t_ends are copied from it; NULL:
 * t_start + step.  slots / outputs both NULL: samples only.  The two entry points above are this one with
 * sample_t1 = NULL. */
int fsn_occ_gather_ex(const int32_t* n_kept, const int64_t* offsets, const float* sample_t0, const float* sample_t1,
                      int sample_cap, int64_t R, float step, int64_t* ray_indices, float* t_starts, float* t_ends,
                      const float* const* slots_host_of_dev, float* const* out_host_of_dev, fsn_stream_t stream);

/* ---- "next" rows ------------------------------------------------------------------ */

/* f4: OcclusionRegularizer.__call__(sigmas, t_vals, ray_idxs)          src/core/loss.py:26-60
 * mean over the rays that own at least one sample of  sum_i w(t_i) sigma_i,  w = -a t + b (func 0,
 * 'linear') or a exp(-b t) (func 1, 'exp').  ray_idxs int64 [N] non-decreasing, n_rays > max index.
 * ray_sums [n_rays] is caller-provided workspace; out is one float. */
int fsn_occlusion_reg_fwd(const float* sigmas, const float* t_vals, const int64_t* ray_idxs, int64_t N,
                          int64_t n_rays, float a, float b, int func, float* ray_sums, float* out,
                          fsn_stream_t stream);

/* backward of fsn_occlusion_reg_fwd w.r.t. sigmas: d_sigmas[i] = *d_out * w(t_i) / #rays with samples.  ray_sums is
 * the forward's workspace (NaN marks rays without samples); count_ws: one int32 of device scratch. */
int fsn_occlusion_reg_bwd(const float* t_vals, int64_t N, const float* ray_sums, int64_t n_rays, float a, float b,
                          int func, const float* d_out, int32_t* count_ws, float* d_sigmas, fsn_stream_t stream);

/* f1: the training step around the path.                         src/run-nerf.py:243-285, models.py:111-143
 * NeRF.forward keeping what its backward needs in a caller-provided workspace, and that backward (gradients of
 * every parameter; fsn_nerf_train_bwd_inputs adds those of the sample positions / directions).
 *   prec 0..3 (FSN_PREC_*).  Forward = the inference kernel with fp32 activations saved in tiles of
 *     128 samples; backward = register-resident dgrad chain on transposed weights + split-K wgrad GEMMs over all
 *     samples (csrc/train_fused.hip).  grad_scale: DEVICE pointer to one float, a power of two that d_out is
 *     multiplied by on entry (results are divided by it again) so that fp16 parts keep small gradients; null = 1.
 *   weights / biases / d_weights / d_biases: HOST arrays of n_layers+4 DEVICE pointers in state_dict order
 *   (layers.0.., sigma, connection, branch, rgb); gradients are overwritten, not accumulated.
 *   workspace: fsn_nerf_train_workspace_floats(desc, prec, n) floats, written by _fwd, consumed (and scribbled on)
 *   by _bwd with the same desc / prec / n; out / d_out [n,4] = [rgb, sigma].
 *   status: the range-guard word OF THIS STEP AND THIS NETWORK (device, or NULL): the caller zeroes it before _fwd
 *   and hands the same word to _bwd.  In the fp16 modes _bwd writes this call's gradients as ZEROS when bit 0
 *   (FSN_STATUS_FP16_RANGE) was raised by either launch (the sums are inf / NaN then); the bf16 modes never consult
 *   it.  It is NOT a sticky shared word: a flag raised by another network or by an inference launch must not zero
 *   this network's gradients.  Hand it to fsn_adam_step(skip_word) to skip the update of a flagged step. */
int64_t fsn_nerf_train_workspace_floats(const fsn_mlp_desc* desc, int prec, int64_t n);
int fsn_nerf_train_fwd(const fsn_mlp_desc* desc, int prec, const float* const* weights, const float* const* biases,
                       const float* x, const float* dirs, const float* pos_mask, const float* dir_mask,
                       int64_t n, float* workspace, float* out, uint32_t* status, fsn_stream_t stream);
/* fsn_nerf_train_fwd with the samples in ray form (as fsn_mlp_fwd_rays): the training step's forward reads the rays and
 * the packed intervals, never a gathered [n,3] tensor (run-nerf.py:243-252 -> rendering.py:76-84). */
int fsn_nerf_train_fwd_rays(const fsn_mlp_desc* desc, int prec, const float* const* weights, const float* const* biases,
                            const float* rays_o, const float* rays_d, const int64_t* ray_indices, const float* t_starts,
                            const float* t_ends, const float* pos_mask, const float* dir_mask, int64_t n,
                            float* workspace, float* out, uint32_t* status, fsn_stream_t stream);
/* accumulate != 0: the gradients are ADDED to d_weights / d_biases (the caller's .grad buffers: what autograd's
 * AccumulateGrad would do with a returned tensor, without the temporaries and the 24 add launches per step);
 * 0: they are overwritten.  A flagged call (bit 0 of *status) contributes zeros either way.
 * stage_scales / stage_amax (both or neither; fp16 modes): n_layers + 2 device floats, initially 1.0, and as many zeroed
 * device words - the backward chain's per-stage power-of-two factors on top of grad_scale and the maxima they are
 * steered by.  The call uses the factors it finds and leaves the ones for the NEXT call (delayed scaling): a network
 * whose layer gradients span more than fp16's range (weight-norm regularised ones do) keeps float32-grade weight
 * gradients from the second call on; run one throw-away call to calibrate a fresh pair of arrays. */
int fsn_nerf_train_bwd(const fsn_mlp_desc* desc, int prec, const float* const* weights, int64_t n, float* workspace,
                       const float* out, const float* d_out, const float* grad_scale, float* const* d_weights,
                       float* const* d_biases, int accumulate, float* stage_scales, uint32_t* stage_amax,
                       uint32_t* status, fsn_stream_t stream);
/* fsn_nerf_train_bwd plus the gradients of the network's INPUTS (csrc/input_grad.hip): d_x [n,3] = dL/d(sample
 * positions), d_dirs [n,3] = dL/d(directions), float32, either may be NULL.  The inputs of the forward are handed in
 * again - x and dirs (point form), or rays_o, rays_d, ray_indices, t_starts, t_ends (ray form, all five; x and dirs NULL:
 * d_x / d_dirs are then per SAMPLE, fsn_ray_grad_reduce sums them per ray) - with the forward's pos_mask / dir_mask.
 *   d_weights == NULL && d_biases == NULL: the dgrad chain and the input gradient only, no weight-gradient launches
 *   (frozen networks: normals, pose-only optimisation).  Otherwise the parameter gradients are bit for bit those of
 *   fsn_nerf_train_bwd.  The workspace size is unchanged (the packed weight slices reuse the chain's transposed-weight
 *   stream, dead by then); the stage arrays advance exactly once per call, and the input gradient is formed with the
 *   factors this call's chain used.  fp16 modes: a flagged call (FSN_STATUS_FP16_RANGE or FSN_STATUS_GRAD_RANGE in
 *   *status) writes d_x / d_dirs as zeros, like the weight gradients.  n == 0: nothing is launched, FSN_OK. */
int fsn_nerf_train_bwd_inputs(const fsn_mlp_desc* desc, int prec, const float* const* weights, int64_t n, float* workspace,
                              const float* out, const float* d_out, const float* grad_scale, float* const* d_weights,
                              float* const* d_biases, int accumulate, float* stage_scales, uint32_t* stage_amax,
                              uint32_t* status, const float* x, const float* dirs, const float* rays_o,
                              const float* rays_d, const int64_t* ray_indices, const float* t_starts, const float* t_ends,
                              const float* pos_mask, const float* dir_mask, float* d_x, float* d_dirs, fsn_stream_t stream);
/* The ray form's reduction of per-sample input gradients: d_rays_o[r] = sum_i d_x[i], d_rays_d[r] = sum_i (m_i d_x[i] +
 * d_dirs[i]) over ray r's samples (ray_indices sorted), m_i = (t_starts[i] + t_ends[i]) / 2.  d_x, d_dirs [N,3] (either
 * may be NULL: that term is absent), outputs [R,3] (either may be NULL).  One wave per ray, fixed summation order, no
 * atomics: deterministic; a ray without samples gets zeros.  No gradient goes to t_starts / t_ends. */
int fsn_ray_grad_reduce(const float* d_x, const float* d_dirs, const int64_t* ray_indices, const float* t_starts,
                        const float* t_ends, int64_t N, int64_t R, float* d_rays_o, float* d_rays_d, fsn_stream_t stream);
/* The power-of-two `grad_scale` of the fp16 modes' backward in one launch: 2^floor(log2(1024 / max|d_out|)), exponent
 * clamped to [-40, 60], 1 when the maximum is 0 / inf / NaN (the arithmetic of ops.grad_scale_for, which took nine
 * elementwise / reduction launches).  buf: 4 device floats, ZEROED by the caller; buf[0] receives the scale (buf[1..2]
 * are the launch's reduction words). */
int fsn_grad_scale(const float* d_out, int64_t n, float* buf, fsn_stream_t stream);
/* backward of fsn_composite_packed_fwd with respect to sigmas and rgbs, given dL/dcolors [R,3] and
 * (optional) dL/dopacity [R]; dL/ddepth is not propagated (the lean backward of the default training step: a call of
 * fsn_composite_packed_bwd_full's kernel with the other cotangents NULL; here d_colors is required). */
int fsn_composite_packed_bwd(const float* sigmas, const float* rgbs, const float* t_starts, const float* t_ends,
                             const int64_t* ray_indices, int64_t N, int64_t R, const float* bkgd_host,
                             const float* d_colors, const float* d_opacity, float* d_sigmas, float* d_rgbs,
                             fsn_stream_t stream);
/* The FULL backward of fsn_composite_packed_fwd: every output carries a cotangent.  Arguments of
 * fsn_composite_packed_bwd plus, all DEVICE pointers:
 *   opacity, depth [R]                 the forward's outputs; required when d_depth is given
 *   d_depth [R]                        optional dL/ddepth
 *   d_weights, d_alphas, d_trans [N]   optional dL/dweights, dL/dalphas, dL/dtrans
 * Any optional pointer may be NULL, and here d_colors as well (that term is absent; nothing is loaded through it: a
 * loss on depth alone has no colour cotangent).  With only d_colors / d_opacity given this IS fsn_composite_packed_bwd:
 * one kernel serves both entry points.  The depth term follows
 * depth = sum w m / max(opacity, eps): d depth / d w_i = (m_i - depth) / opacity for opacity >= eps, m_i / eps below.
 * No gradient goes to t_starts / t_ends.  One wave per ray, no atomics: deterministic. */
int fsn_composite_packed_bwd_full(const float* sigmas, const float* rgbs, const float* t_starts, const float* t_ends,
                                  const int64_t* ray_indices, int64_t N, int64_t R, const float* bkgd_host,
                                  const float* d_colors, const float* d_opacity, const float* opacity,
                                  const float* depth, const float* d_depth, const float* d_weights,
                                  const float* d_alphas, const float* d_trans, float* d_sigmas, float* d_rgbs,
                                  fsn_stream_t stream);

/* Distortion loss of the compositor's weights (mip-NeRF 360, interval form; this package's own definition), per ray:
 *   out[r] = sum_i [ 2 w_i (m_i W_i - V_i) + w_i^2 dt_i / 3 ],  W_i = sum_{j<i} w_j,  V_i = sum_{j<i} w_j m_j,
 * m = (t_starts + t_ends)/2, dt = t_ends - t_starts, samples of a ray contiguous and sorted (ray_indices int64 [N]
 * non-decreasing).  out [n_rays]; a ray without samples gives 0 (N == 0: out, when given, is zeroed).  One wave per
 * ray, two scans, no atomics: deterministic. */
int fsn_distortion_fwd(const float* weights, const float* t_starts, const float* t_ends, const int64_t* ray_indices,
                       int64_t N, int64_t n_rays, float* out, fsn_stream_t stream);
/* backward of fsn_distortion_fwd w.r.t. weights: d_weights[k] = d_out[ray of k] *
 *   ( 2 (m_k W_k - V_k + V'_k - m_k W'_k) + 2 w_k dt_k / 3 ),  W'_k / V'_k the sums over j > k.  d_out [n_rays]. */
int fsn_distortion_bwd(const float* weights, const float* t_starts, const float* t_ends, const int64_t* ray_indices,
                       int64_t N, int64_t n_rays, const float* d_out, float* d_weights, fsn_stream_t stream);

/* Few-shot geometry losses (csrc/ray_losses.hip; this package's own definitions of InfoNeRF's ray entropy, DS-NeRF's
 * depth KL term and RegNeRF's patch depth smoothness - DESIGN.md 6.1).  The two ray losses take sorted ray_indices
 * int64 [N] and write out [n_rays]; a ray without samples gives 0 (N == 0: out, when given, is zeroed); N == 0 or
 * n_rays == 0 returns FSN_OK without a launch; null pointers and negative sizes are FSN_E_INVALID.  One wave per ray, no
 * LDS, no atomics, every sum in a fixed order: deterministic.  Each backward zeroes its output first.
 * fsn_ray_entropy_fwd: with u_i = max(values_i, 0), s = sum u_i, p_i = u_i / (s + eps):
 *     out[r] = -scale c_r sum_i p_i log(p_i + eps)
 *   (scale 1: nats, 1/ln 2: bits).  ray_weight [n_rays] = c_r is optional (NULL: 1) and not differentiated; a ray with
 *   c_r == 0 is skipped (value 0, gradient exactly 0). */
int fsn_ray_entropy_fwd(const float* values, const int64_t* ray_indices, int64_t N, int64_t n_rays,
                        const float* ray_weight, float eps, float scale, float* out, fsn_stream_t stream);
/* backward of fsn_ray_entropy_fwd w.r.t. values: with f'(p) = -log(p + eps) - p / (p + eps),
 *   d_values[k] = d_out[r] scale c_r ( f'(p_k) - sum_i p_i f'(p_i) ) / (s + eps)  where values_k >= 0,  0 below
 * (torch.clamp(min=0)'s rule).  d_out [n_rays]. */
int fsn_ray_entropy_bwd(const float* values, const int64_t* ray_indices, int64_t N, int64_t n_rays,
                        const float* ray_weight, float eps, float scale, const float* d_out, float* d_values,
                        fsn_stream_t stream);
/* fsn_depth_kl_fwd: with m = (t_starts + t_ends)/2, dt = t_ends - t_starts and per-ray depth, var [n_rays]:
 *     out[r] = sum_i -log(max(w_i, 0) + eps) exp(-(m_i - depth_r)^2 / (2 var_r)) dt_i
 *   for a supervised ray (depth_r and var_r both finite and > 0); any other ray gives 0 and gradient exactly 0. */
int fsn_depth_kl_fwd(const float* weights, const float* t_starts, const float* t_ends, const int64_t* ray_indices,
                     int64_t N, int64_t n_rays, const float* depth, const float* var, float eps, float* out,
                     fsn_stream_t stream);
/* backward of fsn_depth_kl_fwd w.r.t. weights:
 *   d_weights[k] = -d_out[r] exp(-(m_k - depth_r)^2 / (2 var_r)) dt_k / (w_k + eps)  where w_k >= 0,  0 below. */
int fsn_depth_kl_bwd(const float* weights, const float* t_starts, const float* t_ends, const int64_t* ray_indices,
                     int64_t N, int64_t n_rays, const float* depth, const float* var, float eps, const float* d_out,
                     float* d_weights, fsn_stream_t stream);
/* fsn_patch_tv_fwd: depth [B, P, Q] contiguous -> out [B],
 *     out[b] = sum_{i < P-1, j < Q-1} (d[i,j] - d[i,j+1])^2 + (d[i,j] - d[i+1,j])^2       (0 when P or Q is 1).
 *   One wave per patch, the lanes striding over the anchors (i, j).  B == 0 returns FSN_OK; P, Q >= 1. */
int fsn_patch_tv_fwd(const float* depth, int64_t B, int P, int Q, float* out, fsn_stream_t stream);
/* backward of fsn_patch_tv_fwd: d_depth [B, P, Q], one thread per pixel, which sums the up-to-four differences it
 * appears in (as the anchor, as an anchor's right and lower neighbour) times d_out[b].  No atomics. */
int fsn_patch_tv_bwd(const float* depth, int64_t B, int P, int Q, const float* d_out, float* d_depth,
                     fsn_stream_t stream);

/* Neighbouring-ray KL (csrc/ray_hist.hip; this package's own definition of InfoNeRF's second term, the KL divergence
 * between the termination distributions of neighbouring rays - DESIGN.md 6.1): packed rays have differing sample
 * counts, so each ray's samples are first binned into a histogram over fixed bins of [t_min, t_max], and neighbouring
 * pixels of a rendered patch are compared bin by bin.  No LDS, no atomics, every sum in a fixed order: deterministic.
 * Each backward zeroes its output first.
 *
 * The axis, float32, in exactly this order: h = (t_max - t_min) / (float)bins, edge e_b = t_min + (float)b h for
 * b = 0 ... bins.  Those float32 values ARE the edges.  t_min < t_max, both finite, and 1 <= bins <= 4096, else
 * FSN_E_INVALID.  fsn_ray_hist_edges writes the bins + 1 edges to host memory (no GPU is touched). */
int fsn_ray_hist_edges(int bins, float t_min, float t_max, float* edges_host);
/* fsn_ray_hist_fwd: sorted ray_indices int64 [N]; out [n_rows, bins], row q = ray first_ray + q (the rows are a
 * subset of the rays: 0 <= first_ray, first_ray + n_rows <= n_rays).  Sample i of ray r, a = t_starts_i, c = t_ends_i:
 *     ok_i = a, c finite and c - a > 0;   u_i = ok_i ? max(values_i, 0) : 0
 *     f_ib = max(min(c, e_{b+1}) - max(a, e_b), 0) / (c - a)
 *     H_rb = sum_i u_i f_ib     in ascending sample order, from +0 (one sequential float32 sum per bin: the lanes own the
 *                               bins and every lane walks all of the ray's samples; the samples need not be sorted)
 *     out  = H                                   (normalize == 0)
 *     out  = P,  P_rb = H_rb / (s_r + eps),  s_r = sum_i u_i             (normalize != 0)
 *   Mass outside [t_min, t_max] is dropped (sum_b P_rb <= 1); a ray without samples gives a row of zeros (N == 0: out is
 *   zeroed); n_rows == 0 returns FSN_OK without a launch.  One wave per ray. */
int fsn_ray_hist_fwd(const float* values, const float* t_starts, const float* t_ends, const int64_t* ray_indices,
                     int64_t N, int64_t n_rays, int64_t first_ray, int64_t n_rows, int bins, float t_min, float t_max,
                     int normalize, float eps, float* out, fsn_stream_t stream);
/* backward of fsn_ray_hist_fwd w.r.t. values, G = d_out [n_rows, bins], hist = the forward's output (read only when
 * normalize != 0; may be NULL otherwise):
 *     d u_i = sum_b G_rb f_ib                                             (normalize == 0)
 *     d u_i = ( sum_b G_rb f_ib - sum_b G_rb P_rb ) / (s_r + eps)          (normalize != 0)
 *     d_values[i] = d u_i  where ok_i and values_i >= 0 (torch.clamp(min=0)'s rule),  0 elsewhere
 *   d_values [N] is zeroed first, so the samples of the rays outside the rows get exactly 0.  One wave per ray, the lanes
 *   striding over the samples; each sums over the bins its interval can touch, in ascending order. */
int fsn_ray_hist_bwd(const float* values, const float* t_starts, const float* t_ends, const int64_t* ray_indices,
                     int64_t N, int64_t n_rays, int64_t first_ray, int64_t n_rows, int bins, float t_min, float t_max,
                     int normalize, float eps, const float* hist, const float* d_out, float* d_values,
                     fsn_stream_t stream);
/* fsn_patch_nkl_fwd: P [B, Ph, Pw, bins] contiguous -> out [B, Ph, Pw].  With
 *     D(p, q) = sum_b p_b ( log(p_b + eps) - log(q_b + eps) ),
 *     out[i,j] = D(P_ij, P_i,j+1)  (j < Pw-1, the pair counted)  +  D(P_ij, P_i+1,j)  (i < Ph-1, the pair counted):
 *   every horizontally and every vertically adjacent pair appears once, owned by its left or upper pixel.  pair_weight
 *   [B, Ph, Pw] = c is a 0/1 mask (NULL: all ones), not differentiated; a pair is counted iff both of its pixels have
 *   c != 0, any other pair is skipped: value 0 and gradient exactly 0.  B == 0 returns FSN_OK; Ph, Pw >= 1,
 *   1 <= bins <= 4096, eps > 0.  One wave per pixel, the lanes striding over the bins. */
int fsn_patch_nkl_fwd(const float* P, const float* pair_weight, int64_t B, int Ph, int Pw, int bins, float eps,
                      float* out, fsn_stream_t stream);
/* backward of fsn_patch_nkl_fwd w.r.t. P: d_P [B, Ph, Pw, bins], d_out [B, Ph, Pw]; with
 *     dD/dp_b = log(p_b + eps) - log(q_b + eps) + p_b / (p_b + eps),   dD/dq_b = -p_b / (q_b + eps)
 *   bin b of pixel (i, j) adds, in this order, its own right pair, its own down pair, the left neighbour's right pair
 *   and the upper neighbour's down pair.  One wave per pixel, each lane writes its bins once.  No atomics. */
int fsn_patch_nkl_bwd(const float* P, const float* pair_weight, int64_t B, int Ph, int Pw, int bins, float eps,
                      const float* d_out, float* d_P, fsn_stream_t stream);
/* the number of adjacent pairs of B patches of Ph x Pw pixels, B (Ph (Pw-1) + (Ph-1) Pw): what an unmasked
 * fsn_patch_nkl_fwd counts (host arithmetic; negative: FSN_E_INVALID) */
int64_t fsn_patch_nkl_pairs(int64_t B, int Ph, int Pw);

/* Monocular depth priors (csrc/depth_prior.hip; this package's own definitions of the scale-and-shift-invariant depth
 * term of MonoSDF / MiDaS and of SparseNeRF's ordinal ranking term - DESIGN.md 6.1; parity with either is unpinned).
 * depth (the renderer's), prior and the optional weight (NULL: 1; a confidence or a mask) are [B, P, Q] float32,
 * contiguous, 1 <= P * Q <= 4096 (larger: FSN_E_UNSUPPORTED); B == 0 returns FSN_OK without a launch; null pointers and
 * negative sizes are FSN_E_INVALID.  A pixel is VALID iff prior and depth are finite and weight > 0; an invalid pixel
 * contributes nothing and gets a gradient of exactly 0.  No LDS, no atomics, every sum in a fixed order: deterministic.
 * Gradients go to depth only; each backward writes every entry of d_depth once.
 * fsn_ssi_depth_fwd: per patch, x = depth (inverse == 0) or x = 1 / max(depth, z_min) (inverse != 0; z_min > 0), w the
 *   weight of a valid pixel and 0 otherwise, every sum in float64:
 *     M = sum w,  mx = sum w x / M,  mp = sum w p / M
 *     vx = sum w (x - mx)^2 / M,  cxp = sum w (x - mx)(p - mp) / M          (a second, centred pass)
 *     s = cxp / vx,  t = mp - s mx,   out[b] = L_b = sum w (s x + t - p)^2 / M
 *   A patch is DEGENERATE with fewer than two valid pixels, M <= 0 or vx <= rel_eps mx^2: out[b] = 0, gradient exactly 0.
 *   fit [B, 4] = (s, t, M, degenerate ? 1 : 0) as float32 (s, t = 0 when degenerate); s may be negative, it is not
 *   clamped.  fit64 [B, 4] float64: the same four values unrounded, for the backward.  One wave per patch, four per
 *   workgroup. */
int fsn_ssi_depth_fwd(const float* depth, const float* prior, const float* weight, int64_t B, int P, int Q, int inverse,
                      float z_min, float rel_eps, float* out, float* fit, double* fit64, fsn_stream_t stream);
/* backward of fsn_ssi_depth_fwd w.r.t. depth.  (s, t) minimise L_b, so its total derivative is the partial at fixed
 * (s, t):  dL_b/dx_k = 2 w_k s (s x_k + t - p_k) / M, the residual formed again (float64) from `fit64`, the forward's -
 * near a perfect fit it cancels to nothing, and (s, t) rounded to float32 would leave it an error of 2^-24 |s x|;
 * with inverse, times dx/ddepth = -1 / depth^2, and 0 where depth < z_min.  d_out [B]; one thread per pixel. */
int fsn_ssi_depth_bwd(const float* depth, const float* prior, const float* weight, const double* fit64, int64_t B, int P,
                      int Q, int inverse, float z_min, const float* d_out, float* d_depth, fsn_stream_t stream);
/* fsn_depth_rank_fwd: ALL ordered pairs (i, j) of valid pixels of a patch instead of random draws.  The prior puts i
 *   nearer iff p_i < p_j - prior_gap (prior_is_disparity: p_i > p_j + prior_gap), prior_gap >= 0; such a pair adds
 *     max(0, (d_i - d_j) + margin)            (float32, in that order)
 *   to out[b] and 1 to pairs[b] (int64 [B]).  weight acts as a mask here.  Summation: per i a float32 sum over ascending
 *   j from +0, the rows added in float64, rounded once to out[b].  One wave per patch: the lanes stride over i and every
 *   lane walks all j (P * Q = 4096: 16.8 M pair tests per patch). */
int fsn_depth_rank_fwd(const float* depth, const float* prior, const float* weight, int64_t B, int P, int Q, float margin,
                       float prior_gap, int prior_is_disparity, float* out, int64_t* pairs, fsn_stream_t stream);
/* backward of fsn_depth_rank_fwd w.r.t. depth, gather form: pixel k walks all partners of its patch and counts +1 for
 * every active pair (hinge > 0) in which it is the nearer pixel and -1 for every active pair in which it is the farther;
 * d_depth[k] = d_out[b] * (float)count.  One thread per pixel. */
int fsn_depth_rank_bwd(const float* depth, const float* prior, const float* weight, int64_t B, int P, int Q, float margin,
                       float prior_gap, int prior_is_disparity, const float* d_out, float* d_depth, fsn_stream_t stream);

/* ---- depth-warp sampling: a rendered ray and its depth -> the colour a training photograph shows at that 3-D point
 *                                                     (this package's own; DESIGN.md 6.1 "Depth-warp consistency")
 *                                                                                                     csrc/warp.hip
 * The operator under the cross-view reprojection losses (GeCoNeRF, SPARF, ConsistentNeRF): ONE launch, one thread per
 * row, no LDS, no atomics, no workspace; rows are independent, so every output is bitwise reproducible.  The library is
 * built with -ffp-contract=off and every step is a float32 operation in the order written, so tests/warp_ref.py
 * restates the forward bit for bit in NumPy.  Row r, with (o, d) = (rays_o_r, rays_d_r), t = depth_r, s = src_view_r,
 * M = poses[s] ([3][4]: rotation columns and centre c, as fsn_ray_batch reads it), (fx, fy, cx, cy) = row s of
 * K [m, 4] (row 0 when m == 1; the stored intrinsics are (focal, focal, W/2, H/2)):
 *   X_k = o_k + t d_k,  p_k = X_k - c_k;
 *   xc = (M[0] p0 + M[4] p1) + M[8] p2, yc and zc likewise with columns 1 and 2 (R^T p);  z = -zc (the camera looks
 *   down its own -z);
 *   u = cx + fx (xc / z),  v = cy - fy (yc / z)      (the pixel index w of fsn_ray_batch is the coordinate u = w);
 *   valid iff 0 <= s < n_views, t finite and > 0, z >= z_min, border <= u <= (W-1) - border and
 *   border <= v <= (H-1) - border (a NaN anywhere makes the row invalid);
 *   x0 = min((int)floorf(u), W-2), fu = u - x0; y0 = min((int)floorf(v), H-2), fv = v - y0; the taps c00 at (y0, x0),
 *   c10 at (y0, x0+1), c01 at (y0+1, x0), c11 at (y0+1, x0+1) of images [n_views, H, W, C] uint8, each converted as
 *   fsn_ray_batch converts its pixel (byte / 255; with white_bkgd c a + (1 - a) in three float32 operations);
 *   top = c00 + fu (c10 - c00), bot = c01 + fu (c11 - c01), colour = top + fv (bot - top).
 * Outputs: colour [n,3]; valid [n] uint8 (0 / 1); uvz [n,3] = (u, v, z) (may be NULL) for every row whose s is in range,
 * valid or not (a NaN is stored as the canonical quiet NaN), zeros otherwise - for a caller that holds source depths and
 * builds an occlusion mask; not differentiable.  An invalid row gets colour = 0 and valid = 0 and reads no byte of
 * `images`.  s = -1 is the documented "no source view"; any other s outside [0, n_views) is invalid too (and, in the
 * debug build, recorded for fsn_debug_report("warp"), as is a tap offset outside the images).
 * n == 0 returns FSN_OK without a launch.  Errors (FSN_E_INVALID): n or n_views negative, null pointers, C not in
 * {3, 4}, white_bkgd with C = 3, H < 2 or W < 2, m not in {1, n_views}, z_min <= 0, border < 0 (or either not finite). */
int fsn_warp_sample_fwd(const float* rays_o, const float* rays_d, const float* depth, const int64_t* src_view, int64_t n,
                        const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C, int white_bkgd,
                        const float* K, int64_t m, float z_min, float border, float* colour, uint8_t* valid, float* uvz,
                        fsn_stream_t stream);
/* backward of fsn_warp_sample_fwd w.r.t. depth and the ray (each of d_depth [n], d_rays_o [n,3], d_rays_d [n,3] may be
 * NULL = not wanted): ONE launch that recomputes the projection and the four taps from the inputs - nothing is saved.
 * For a valid row, with g = d_colour_r and per channel dcu = (c10 - c00) + fv ((c11 - c01) - (c10 - c00)),
 * dcv = bot - top:  gu = sum_c g_c dcu_c,  gv = sum_c g_c dcv_c;
 *   g_xc = gu fx / z,  g_yc = -gv fy / z,  g_z = (-gu fx xc + gv fy yc) / (z z),  g_zc = -g_z;  gp = R (g_xc, g_yc, g_zc);
 *   d_rays_o = gp,  d_rays_d = t gp,  d_depth = gp . d.
 * The cell (x0, y0) is a constant of the backward (as for grid_sample); every gradient of an invalid row is written as
 * exactly 0.  No gradient to the images, to the source pose or to K. */
int fsn_warp_sample_bwd(const float* rays_o, const float* rays_d, const float* depth, const int64_t* src_view, int64_t n,
                        const float* poses, int64_t n_views, const uint8_t* images, int H, int W, int C, int white_bkgd,
                        const float* K, int64_t m, float z_min, float border, const float* d_colour, float* d_depth,
                        float* d_rays_o, float* d_rays_d, fsn_stream_t stream);

/* Packed volume-rendering primitives (csrc/packed_scan.hip; render/volrend.py is their Python surface, named after
 * nerfacc's volrend / scan / pack modules - this package's own definitions of nerfacc's documented semantics).
 * Every entry point below finds the samples [beg, beg + S) of ray r in ONE of three ways ("span" arguments):
 *   ray_indices  int64 [N], sorted (non-decreasing): a binary search per ray;
 *   packed_info  int64 [R,2] = (start, count) per ray, as fsn_pack_info writes it: no search (entries are clamped into
 *                [0, N]); samples no ray owns get 0 in every gradient / keep output;
 *   dense_S > 0  dense rows: ray r owns [r dense_S, (r+1) dense_S), N == R * dense_S.
 * Exactly one of the three is given (the other pointers NULL, dense_S 0); anything else is FSN_E_INVALID, as are
 * negative sizes and null data pointers; N == 0 or R == 0 returns FSN_OK without a launch.  One wave per ray, lane l
 * owns the contiguous samples [l per, (l+1) per), per = ceil(S/64); no LDS, no atomics, every sum in a fixed order;
 * float32.
 * fsn_pack_info: packed_info[r] = (first index i with ray_indices[i] >= r, number of samples of ray r) - a ray
 *   without samples has count 0 and the start where its samples would be.  N == 0: all zeros.
 * fsn_packed_scan_fwd: out[k] = sum (op FSN_SCAN_SUM) or product (FSN_SCAN_PROD) of x[j] over the ray's samples j < k
 *   (exclusive != 0) or j <= k.
 * fsn_packed_scan_bwd: d_x from d_out.  Sum: the reverse scan of d_out (x may be NULL).  Product: division-free, so
 *   that x[k] == 0 has a finite, correct gradient - with P_k = prod_{j<k} x_j:  d_x[k] = P_k S_k,
 *   S_k = d_out[k+1] + x[k+1] S_{k+1} (exclusive)  or  S_k = d_out[k] + x[k+1] S_{k+1} (inclusive), S = 0 past the end.
 * fsn_packed_weights_fwd: from_alpha == 0: v = sigmas, alpha = 1 - exp(-sigma (t_ends - t_starts)), T = exp(-exclusive
 *   sum of sigma dt) - the operation sequence of fsn_composite_packed_fwd, whose weights / trans / alphas these are bit
 *   for bit; from_alpha != 0: v = alphas (t_starts / t_ends unused, may be NULL), T = exclusive product of 1 - alpha.
 *   trans = T * prefix_trans[i] when prefix_trans [N] is given, weights = trans * alpha.  Any output may be NULL.
 * fsn_packed_weights_bwd: d_v (d_sigmas or d_alphas) [N] from the optional cotangents d_weights (u), d_trans (tau),
 *   d_alphas (a), with p = prefix_trans or 1:
 *     density: d_sigma_i = dt_i ( (u_i T_i p_i + a_i) e_i - sum_{j>i} (u_j alpha_j + tau_j) p_j T_j ),  e = exp(-sigma dt)
 *     alpha:   d_alpha_k = u_k T_k p_k + a_k - T_k S_k,  S_k = g_{k+1} + (1 - alpha_{k+1}) S_{k+1},
 *              g_i = (u_i alpha_i + tau_i) p_i   (division-free: alpha == 1 is fine)
 *   No gradient goes to t_starts / t_ends / prefix_trans.
 * fsn_packed_visibility_alpha: fsn_packed_visibility's rule on alphas: keep[i] = (T_i >= early_stop_eps &&
 *   alpha_i >= alpha_thre), T = exclusive product of 1 - alpha.
 * fsn_accumulate_fwd: out[r,c] = sum_i weights[i] values[i,c] over the ray's samples, values [N,C], out [R,C];
 *   values == NULL: out[r,0] = sum_i weights[i] (C must be 1).  A ray without samples gives 0 (N == 0: out zeroed).
 * fsn_accumulate_bwd: d_weights[i] = sum_c d_out[r,c] values[i,c] (values NULL: d_out[r,0]),
 *   d_values[i,c] = weights[i] d_out[r,c]; either output may be NULL (not both). */
#define FSN_SCAN_SUM 0
#define FSN_SCAN_PROD 1
int fsn_pack_info(const int64_t* ray_indices, int64_t N, int64_t R, int64_t* packed_info, fsn_stream_t stream);
int fsn_packed_scan_fwd(const float* x, const int64_t* ray_indices, const int64_t* packed_info, int64_t N, int64_t R,
                        int dense_S, int op, int exclusive, float* out, fsn_stream_t stream);
int fsn_packed_scan_bwd(const float* x, const float* d_out, const int64_t* ray_indices, const int64_t* packed_info,
                        int64_t N, int64_t R, int dense_S, int op, int exclusive, float* d_x, fsn_stream_t stream);
int fsn_packed_weights_fwd(const float* v, const float* t_starts, const float* t_ends, const int64_t* ray_indices,
                           const int64_t* packed_info, int64_t N, int64_t R, int dense_S, int from_alpha,
                           const float* prefix_trans, float* weights, float* trans, float* alphas, fsn_stream_t stream);
int fsn_packed_weights_bwd(const float* v, const float* t_starts, const float* t_ends, const int64_t* ray_indices,
                           const int64_t* packed_info, int64_t N, int64_t R, int dense_S, int from_alpha,
                           const float* prefix_trans, const float* d_weights, const float* d_trans, const float* d_alphas,
                           float* d_v, fsn_stream_t stream);
int fsn_packed_visibility_alpha(const float* alphas, const int64_t* ray_indices, const int64_t* packed_info, int64_t N,
                                int64_t R, int dense_S, float early_stop_eps, float alpha_thre, uint8_t* keep,
                                fsn_stream_t stream);
int fsn_accumulate_fwd(const float* weights, const float* values, int C, const int64_t* ray_indices,
                       const int64_t* packed_info, int64_t N, int64_t R, int dense_S, float* out, fsn_stream_t stream);
int fsn_accumulate_bwd(const float* d_out, const float* weights, const float* values, int C, const int64_t* ray_indices,
                       const int64_t* packed_info, int64_t N, int64_t R, int dense_S, float* d_weights, float* d_values,
                       fsn_stream_t stream);

/* Proposal-network sampler (csrc/propnet.hip; render/pdf.py and render/propnet.py are the Python surface, named after
 * nerfacc's pdf module and PropNetEstimator - this package's own definitions of nerfacc's documented semantics, see
 * DESIGN.md "Proposal-network estimator").  Dense rows only: every array is [R, .] float32 on the DEVICE, one wave per
 * ray, no atomics, every sum in a fixed order.  A ray's histogram is S intervals: edges v[0..S] (non-decreasing) and cdf
 * c[0..S] (non-decreasing, c[0] = 0, c[S] = 1).
 * fsn_importance_sample: n intervals per ray from the inverse cdf.  Centre i: u = (i + b) / n (one float32 add, one
 *   divide), b = 0.5 (b == NULL) or b[r] (DEVICE [R]: one jitter per ray, in [0, 1)); k = clamp(#{c <= u} - 1, 0, S-1),
 *   frac = c[k+1] > c[k] ? clamp((u - c[k]) / (c[k+1] - c[k]), 0, 1) : 0, x_i = v[k] + frac (v[k+1] - v[k]).  Edges:
 *   e_j = (x_{j-1} + x_j) / 2 inside, e_0 = max(2 x_0 - e_1, v[0]), e_n = min(2 x_{n-1} - e_{n-1}, v[S]); n == 1:
 *   (v[0], v[S]).  s_edges [R, n+1]; centres [R, n] (may be NULL); with transform FSN_STOT_UNIFORM, t = s far +
 *   (1 - s) near, or FSN_STOT_LINDISP, t = 1 / (s (1/far) + (1 - s) (1/near)), t_edges [R, n+1] = the transformed
 *   s_edges (FSN_STOT_NONE: t_edges is not written).  A cdf that is not monotone is outside the contract: the kernel
 *   still reads and writes its own rows only and returns finite values inside [v[0], v[S]], not necessarily sorted.
 * fsn_prop_resample: the step between two proposal evaluations in one launch: cdfs [R, S+1] = 1 - (T_0 .. T_{S-1}, 0),
 *   T the transmittance of sigmas [R, S] on the intervals t_edges [R, S+1] (the values of fsn_packed_weights_fwd on
 *   t_starts = t_edges[:, :-1], t_ends = t_edges[:, 1:], bit for bit), then fsn_importance_sample on (s_edges, cdfs),
 *   bit for bit.
 * fsn_searchsorted_dense: keys [R, K] sorted per row, values [R, Q]; with h = #{key <= q}: ids_left = max(h - 1, 0),
 *   ids_right = min(h, K - 1), int64 [R, Q] (inside the range key[ids_left] <= q < key[ids_right]; below the first key
 *   both 0, at or beyond the last both K - 1).
 * fsn_prop_loss_fwd: the interlevel loss of query intervals q_edges / q_cdfs [R, n+1] against a proposal's k_edges /
 *   k_cdfs [R, S+1] (both in s-space, sorted): w_i = cq[i+1] - cq[i], wo_i = ck[ids_right(q[i+1])] - ck[ids_left(q[i])],
 *   loss [R, n] = max(w_i - wo_i, 0)^2 / (w_i + 1e-7) where w_i > 0, else 0.
 * fsn_prop_loss_bwd: d_k_cdfs [R, S+1] from d_loss [R, n] (the query side carries no gradient): coef_i =
 *   -2 max(w_i - wo_i, 0) / (w_i + 1e-7) d_loss_i, d_ck[m] = sum of coef_i over ids_right(q[i+1]) == m minus the sum over
 *   ids_left(q[i]) == m, each one run of the sorted queries, summed in ascending i.
 * FSN_E_INVALID: null pointers, S < 1, n < 1, K < 1, near <= 0 or far <= 0 with FSN_STOT_LINDISP.  FSN_E_UNSUPPORTED:
 *   the sampler and loss kernels hold a ray's rows in LDS, S and n <= FSN_PROP_MAX_ROW each.  R == 0: FSN_OK, no launch. */
#define FSN_PROP_MAX_ROW 1024
#define FSN_STOT_NONE 0
#define FSN_STOT_UNIFORM 1
#define FSN_STOT_LINDISP 2
int fsn_importance_sample(const float* vals, const float* cdfs, int64_t R, int S, int n, const float* b, int transform,
                          float near, float far, float* s_edges, float* centres, float* t_edges, fsn_stream_t stream);
int fsn_prop_resample(const float* s_edges, const float* t_edges, const float* sigmas, int64_t R, int S, int n,
                      const float* b, int transform, float near, float far, float* cdfs, float* s_out, float* centres,
                      float* t_out, fsn_stream_t stream);
int fsn_searchsorted_dense(const float* keys, const float* values, int64_t R, int K, int Q, int64_t* ids_left,
                           int64_t* ids_right, fsn_stream_t stream);
int fsn_prop_loss_fwd(const float* q_edges, const float* q_cdfs, const float* k_edges, const float* k_cdfs, int64_t R,
                      int n, int S, float* loss, fsn_stream_t stream);
int fsn_prop_loss_bwd(const float* q_edges, const float* q_cdfs, const float* k_edges, const float* k_cdfs,
                      const float* d_loss, int64_t R, int n, int S, float* d_k_cdfs, fsn_stream_t stream);

/* f1: optimizer side of the training step on ONE flat float32 parameter arena (run-nerf.py:217, 266-285).
 * fsn_adam_step: torch.optim.Adam's update (no amsgrad), operation for operation in float32, one launch over the
 *   arena: params / grads / exp_avg / exp_avg_sq [n]; `step` = 1, 2, ... (bias corrections are formed in double on
 *   the host); grad_div divides the gradient first (pass the number of ranks when `grads` holds an all-reduced SUM).
 *   skip_word / skip_count (DEVICE pointers or NULL): the launch leaves parameters and moments untouched when
 *   FSN_STATUS_FP16_RANGE or FSN_STATUS_GRAD_RANGE is set in *skip_word or *skip_count > 0 - the per-step status word of fsn_nerf_train_fwd/_bwd (fp16 overflow in
 *   this step) and the flag slot of an all-reduced gradient bucket; decided on the device, no host sync.
 * fsn_weight_norm_*: the weight-norm "frequency" regulariser of run-nerf.py:266-279: out = sum over the selected
 *   tensors (segments [off, off+len) of the arena, HOST tables, <= 40) of |w|_1 (l2 = 0) or |w|_2 (l2 = 1).
 *   workspace: fsn_weight_norm_workspace_floats(...) floats, written by _fwd and read by _bwd (per-tensor norms);
 *   _bwd ACCUMULATES d_out[0] * d(out)/dw into grad_arena (same layout as the arena).  No atomics: sums are taken
 *   in a fixed order. */
int fsn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int step,
                  double lr, double beta1, double beta2, double eps, double weight_decay, double grad_div,
                  const uint32_t* skip_word, const float* skip_count, fsn_stream_t stream);
/* fsn_adam_step with the step counter ON THE DEVICE (round 4): step_count (DEVICE int32[1]) holds the number of updates
 * applied so far; a first one-thread launch looks at skip_word / skip_count, and only when the step runs advances the
 * counter and forms the bias-correction constants (double precision, torch's expressions) into tick (DEVICE float[4],
 * scratch); the update launch reads them.  A skipped step therefore does not advance the bias corrections - as with
 * torch's GradScaler, which does not call optimizer.step() on an overflowing step - and the host never needs the count. */
int fsn_adam_step_dev(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t* step_count,
                      float* tick, double lr, double beta1, double beta2, double eps, double weight_decay, double grad_div,
                      const uint32_t* skip_word, const float* skip_count, fsn_stream_t stream);
int64_t fsn_weight_norm_workspace_floats(int n_seg, const int64_t* seg_len_host);
int fsn_weight_norm_fwd(const float* arena, int n_seg, const int64_t* seg_off_host, const int64_t* seg_len_host, int l2,
                        float* workspace, float* out, fsn_stream_t stream);
int fsn_weight_norm_bwd(const float* arena, int n_seg, const int64_t* seg_off_host, const int64_t* seg_len_host, int l2,
                        const float* workspace, const float* d_out, float* grad_arena, fsn_stream_t stream);

/* f2: occupancy-grid sampler for the `estimator` slot (nerfacc OccGridEstimator; call sites
 * src/render/rendering.py:66-74, src/run-nerf.py:96-98, 288-295).  nerfacc is not part of the reference: the
 * arithmetic is this build's definition of the contract, mirrored by oracle/fsnerf_oracle.py.
 *   grid: `levels` nested boxes (level l = roi aabb scaled by 2^l about its centre), res^3 cells each, cell index
 *   (ix*res + iy)*res + iz (+ l*res^3); `bits` = one bit per cell (word c>>5, bit c&31), `occs` fp32 per cell.
 * fsn_occgrid_march: per ray the lattice t_k = near_r + k*step, near_r = near_plane + (u ? u[r]*step : 0); interval
 *   [t_k, t_k+step) is a sample iff t_k lies in [max(t_enter, near_r), min(t_exit, far_plane)) of the outermost box
 *   and the cell of its midpoint (finest level containing it) is occupied; at most max_steps lattice points per ray.
 *   Two passes: offsets == NULL -> counts[R] (int64); else fill ray_indices / t_starts / t_ends at offsets[r]
 *   (exclusive scan of the counts, by the caller).  It is fsn_occgrid_march_ex with t_min = t_max = NULL and
 *   cone_angle = 0: one kernel serves both entry points.
 * fsn_packed_visibility: keep[i] = (T_i >= early_stop_eps && alpha_i >= alpha_thre), T = exp(-exclusive sum of
 *   sigma*dt) per ray, samples packed and sorted by ray.
 * fsn_occgrid_update: occs[cells[i]] = max(occs[cells[i]]*decay, vals[i]) (cells must be unique), then, when
 *   threshold_dev != NULL (device pointer to one float), bits = (occs > *threshold_dev). n_cells % 64 == 0. */
int fsn_occgrid_march(const float* rays_o, const float* rays_d, int64_t R, const float* aabb_host, int res, int levels,
                      const uint32_t* bits, float near_plane, float far_plane, float step, const float* u,
                      int max_steps, int64_t* counts, const int64_t* offsets, int64_t* ray_indices, float* t_starts,
                      float* t_ends, fsn_stream_t stream);
/* fsn_occgrid_march_ex: fsn_occgrid_march with per-ray bounds and a step that grows with distance (nerfacc's `t_min` /
 * `t_max` / `cone_angle` keywords; nerfacc's source is absent, so this is the build's own definition, float32 with plain
 * operations throughout - tests/occ_cone_ref.py restates it in NumPy, bit for bit).
 *   bounds: t_min / t_max = DEVICE float [R] or NULL; t_lo = max(t_enter, near_r, t_min[r]), t_hi = min(t_exit,
 *   far_plane, t_max[r]) (fmaxf / fminf in that order); +-inf allowed, t_max <= t_min: no samples.
 *   cone_angle == 0: fsn_occgrid_march's lattice t_k = near_r + k*step (anchored at the near plane) inside [t_lo, t_hi).
 *   cone_angle > 0 (needs near_plane >= 0; near_r = near_plane): dt(t) = fmaxf(t * cone_angle, step); the first block
 *   starts at t_0 = t_lo + (u ? u[r] * dt(t_lo) : 0); block b holds 64 intervals of ONE width dt_b = dt(t_b):
 *   ts_j = t_b + (float)j * dt_b, te_j = t_b + (float)(j+1) * dt_b (te_j is bitwise ts_{j+1}), t_{b+1} = t_b + 64 dt_b.
 *   Interval j of block b is a sample iff 64 b + j < max_steps, ts_j < t_hi and the cell of its midpoint
 *   (ts_j + te_j) / 2 (finest level containing it) is occupied; the march ends after the block with !(t_{b+1} < t_hi).
 *   A sample is never wider than clamp(t * cone_angle, step, inf) at its own start, and at most 1 + 64 cone_angle
 *   times narrower.  Passes, outputs and scan as fsn_occgrid_march.  FSN_E_INVALID: null pointers, step <= 0,
 *   cone_angle < 0, cone_angle > 0 with near_plane < 0.
 * fsn_ray_aabb_intersect: rays [R] against boxes aabbs (DEVICE float [M,6]: xmin ymin zmin xmax ymax zmax) with the
 *   march's slab arithmetic (division form; a zero direction component tests the origin against the slab):
 *   hit = !miss && min(t_exit, far_plane) > max(t_enter, near_plane); t_mins / t_maxs [R,M] hold those two clipped
 *   values for a hit and miss_value for a miss; hits: uint8 [R,M]. */
int fsn_occgrid_march_ex(const float* rays_o, const float* rays_d, int64_t R, const float* aabb_host, int res, int levels,
                         const uint32_t* bits, float near_plane, float far_plane, float step, const float* u,
                         int max_steps, const float* t_min, const float* t_max, float cone_angle, int64_t* counts,
                         const int64_t* offsets, int64_t* ray_indices, float* t_starts, float* t_ends,
                         fsn_stream_t stream);
int fsn_ray_aabb_intersect(const float* rays_o, const float* rays_d, int64_t R, const float* aabbs, int M,
                           float near_plane, float far_plane, float miss_value, float* t_mins, float* t_maxs,
                           uint8_t* hits, fsn_stream_t stream);
int fsn_packed_visibility(const float* sigmas, const float* t_starts, const float* t_ends, const int64_t* ray_indices,
                          int64_t N, int64_t R, float early_stop_eps, float alpha_thre, uint8_t* keep,
                          fsn_stream_t stream);
int fsn_occgrid_update(float* occs, int64_t n_cells, const int64_t* cells, const float* vals, int64_t n, float decay,
                       const float* threshold_dev, uint32_t* bits, fsn_stream_t stream);
/* update_every_n_steps on the device (round 4; run-nerf.py:288-295): which cells of level `lvl` an update re-evaluates,
 * and where.  all_cells != 0 (warm-up): draw i is cell i, n = res^3.  Else n = n_uniform + n_occupied draws: the first
 * n_uniform uniform over the level's cells, with replacement; the rest from its OCCUPIED cells, read straight from the
 * bit field (popcount prefix over its words in prefix_scratch, DEVICE int32 [res^3/32 + 1]).  A level with m <= n_occupied
 * occupied cells gives each of them exactly once (draw n_uniform + q -> the q-th occupied cell in index order) and the
 * sentinel cell -1 to the draws q >= m; with m > n_occupied the draws are uniform over the occupied cells, with
 * replacement.  Each draw gets a point uniform inside its cell of the level's box (a sentinel draw: inside its uniform
 * cell).  Randomness: the counter-based hash of csrc/occgrid.hip (occ_rand) of (seed, draw index) - no generator state,
 * no host sync, restated by the oracle.  cells: int64 [n] (global cell index, + lvl res^3, or -1), x: [n,3].
 * fsn_occgrid_update and fsn_occgrid_update_multi skip the cells < 0.
 * fsn_occgrid_update_multi: fsn_occgrid_update's EMA for draws that may repeat a cell: occs[c] = max(occs[c] * decay,
 * max of the vals drawn for c) - the maximum is taken first (pending: DEVICE uint32 [n_cells], all zero between calls),
 * so the result does not depend on the order of the draws. */
int fsn_occgrid_select(const uint32_t* bits, int res, int levels, int lvl, const float* aabb_host, int all_cells,
                       int64_t n_uniform, int64_t n_occupied, uint64_t seed, int32_t* prefix_scratch, int64_t* cells,
                       float* x, fsn_stream_t stream);
int fsn_occgrid_update_multi(float* occs, int64_t n_cells, uint32_t* pending, const int64_t* cells, const float* vals,
                             int64_t n, float decay, fsn_stream_t stream);
/* update_every_n_steps in ONE launch for all levels, the density pass in a single-pass mode (csrc/occ_refresh.hip): per
 * draw (lvl, i), i < n = res^3 (all_cells) or n_uniform + n_occupied, the cell and the point of fsn_occgrid_select (same
 * rule, counters and operation order; seeds_host: HOST uint64 [levels], level l's seed), the density of the packed
 * network `blob` (fsn_mlp_pack in `prec`; FSN_PREC_FP16 or FSN_PREC_BF16, any other mode: FSN_E_UNSUPPORTED) at that
 * point with pos_mask as in fsn_mlp_fwd, occ = sigma * step in float32, and pending[cell] = max(pending[cell], key(occ))
 * as fsn_occgrid_update_multi forms it (NaN and the sentinel cell -1 skipped).  Points, cells and densities are not
 * written anywhere.  prefix_scratch: DEVICE int32 [levels * (res^3/32 + 1)] (needed when n_occupied > 0 and not
 * all_cells); pending: DEVICE uint32 [levels * res^3], all zero before the call; status: the range word of fsn_mlp_fwd.
 * levels * res^3 and levels * n must be below 2^31.
 * fsn_occgrid_apply_pending: the second half of fsn_occgrid_update_multi on its own - occs[c] = max(occs[c] * decay,
 * pending[c]) for the touched cells, pending cleared.  (Apart, so that a caller can look at the status word - or zero
 * `pending` and repeat the refresh in FSN_PREC_BF16 - before the grid changes.) */
int fsn_occgrid_refresh(const fsn_mlp_desc* desc, int prec, const void* blob, const float* pos_mask, const uint32_t* bits,
                        int res, int levels, const float* aabb_host, int all_cells, int64_t n_uniform, int64_t n_occupied,
                        const uint64_t* seeds_host, float step, int32_t* prefix_scratch, uint32_t* pending,
                        uint32_t* status, fsn_stream_t stream);
int fsn_occgrid_apply_pending(float* occs, int64_t n_cells, uint32_t* pending, float decay, fsn_stream_t stream);
/* OccGridEstimator.mark_invisible_cells (csrc/occ_invisible.hip): which cells any training camera can see.  nerfacc
 * tests one lattice point per cell; this rule is a conservative frustum / box test instead (a removed cell is a permanent
 * hole), and it is this build's definition - tests/occ_invisible_ref.py restates it in float32, bit for bit.
 *   cell box: level l's box [lo, hi] (roi scaled by 2^l about its centre, in double, rounded once), w = (hi - lo) / res
 *   per axis, cell (ix, iy, iz) = [lo + i w, lo + (i + 1) w]; centre = mean of the two ends per axis.
 *   cams: DEVICE float [n_cams,16] = world -> camera map [3,4] row major (camera x right, y down, z = depth forward),
 *   then fx, fy, cx, cy.  Camera-space point (X, Y, D), each ((m0 x + m1 y) + m2 z) + m3, has the margins D - near_plane,
 *   fx X + cx D, (width - cx) D - fx X, fy Y + cy D, (height - cy) D - fy Y.
 *   A camera covers a cell unless all 8 corners are negative in one of the five margins; a cell is too near a camera
 *   when its centre has the four side margins >= 0 and 0 <= D < near_plane (a depth along the optical axis, not a ray
 *   parameter).  visible = covered by at least min_views cameras and too near to none.
 *   ndc != 0: the grid lives in the NDC space of to_ndc with near = ndc_near; the box is clipped to z' <= 1 - 1e-6 (a
 *   cell with nothing left is invisible) and its corners and centre are mapped back first: z = 2 ndc_near / (z' - 1),
 *   x = ((-x') z) ndc_wf, y = ((-y') z) ndc_hf, with ndc_wf = W / (2 focal), ndc_hf = H / (2 focal).
 *   visible: DEVICE uint32 [levels res^3 / 32], word / bit layout of `bits`; levels * res^3 % 64 == 0.  Any n_cams >= 1.
 *   FSN_E_INVALID: null pointers, n_cams < 1, min_views < 1, near_plane < 0, width or height <= 0.
 * fsn_occgrid_update_masked: the end of an update on a marked grid, two launches, no host synchronisation:
 *   occs = -1 at the invisible cells (revive != 0: a visible cell holding -1 becomes 0 first - a mask that was replaced),
 *   threshold = min(mean of occs over the visible cells, occ_thre) (sum in double, fixed order; no visible cell:
 *   occ_thre), bits = (occs > threshold) & visible (bits == NULL: the first launch only, occs alone).  scratch: DEVICE
 *   double [2048].  n_cells % 64 == 0. */
int fsn_occgrid_visibility(const float* aabb_host, int res, int levels, const float* cams, int n_cams, int width,
                           int height, float near_plane, int min_views, int ndc, float ndc_wf, float ndc_hf,
                           float ndc_near, uint32_t* visible, fsn_stream_t stream);
int fsn_occgrid_update_masked(float* occs, int64_t n_cells, const uint32_t* visible, float occ_thre, int revive,
                              double* scratch, uint32_t* bits, fsn_stream_t stream);

/* f3: to8b(x) = (255 * clip(x, 0, 1)).astype(uint8)                    src/render/rendering.py:21 */
int fsn_to8b(const float* x, int64_t n, uint8_t* out, fsn_stream_t stream);
/* f3: render_video(frames, d_frames, cmap)                             src/render/rendering.py:240-266
 * fsn_to8b_nchw: frames [N,HW,3] float -> uint8 [N,3,HW] = transpose(to8b(frames), (0,3,1,2)).
 * fsn_depth_colormap: depth [N,HW] -> uint8 [N,3,HW]: matplotlib's Normalize(vmin, vmax) (float32; vmin == vmax
 *   maps to 0) and ScalarMappable lookup, index = int(x * 256) (x == 1 -> 255, out of range -> first / last entry),
 *   in lut_rgb8 = to8b of the colormap's 256 RGB entries (uint8 [256][3], device).  vmin_vmax: 2 floats (device). */
int fsn_to8b_nchw(const float* frames, int64_t n_frames, int64_t hw, uint8_t* out, fsn_stream_t stream);
int fsn_depth_colormap(const float* depth, int64_t n_frames, int64_t hw, const float* vmin_vmax,
                       const uint8_t* lut_rgb8, uint8_t* out, fsn_stream_t stream);

/* Evaluation metrics of the reference's evaluation() (src/run-nerf.py:108-191), on N image pairs x, y (float32,
 * DEVICE) of C channels and H x W pixels.  Element (n, c, h, w) of an image is at ptr[n*s[0] + c*s[1] + h*s[2] + w*s[3]]
 * with the strides (in elements) of a HOST int64 array s[4]: NHWC, NCHW and permuted views need no copy.  Sums are
 * taken in float64 in a fixed order (no atomics): the results are bitwise reproducible.  N = 0 is a no-op.
 * fsn_ssim: skimage.metrics.structural_similarity (scikit-image 0.22) per image, each channel on its own:
 *   window FSN_SSIM_GAUSSIAN (gaussian_weights=True: sigma 1.5, truncate 3.5, 11 taps) or FSN_SSIM_UNIFORM (7 x 7 box),
 *   separable, scipy's mode='reflect' edges; moments ux, uy, uxx, uyy, uxy; v = cn (uxx - ux^2) ...,
 *   cn = NP / (NP - 1) with NP = win^2 when use_sample_covariance, else 1; C1 = (K1 data_range)^2, C2 = (K2 data_range)^2;
 *   S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)).  out: N + 1 doubles = the mean of S over the
 *   interior (the map cropped by the window radius) and the channels of each image, then the mean over the N images.
 *   smap (optional, with smap_strides_host): the uncropped S map in float32.  H and W must be at least the window width.
 *   workspace: fsn_ssim_workspace_doubles(N, C, H, W) doubles.
 * fsn_psnr: out: N + 1 floats = -10 log10(MSE) of each image, then of the whole stack (one MSE over every element).
 *   workspace: fsn_psnr_workspace_doubles(N, C, H, W) doubles. */
#define FSN_SSIM_GAUSSIAN 0
#define FSN_SSIM_UNIFORM 1
int64_t fsn_ssim_workspace_doubles(int64_t N, int C, int H, int W);
int fsn_ssim(const float* x, const float* y, int64_t N, int C, int H, int W, const int64_t* x_strides_host,
             const int64_t* y_strides_host, int window, int use_sample_covariance, double data_range, double K1, double K2,
             double* workspace, double* out, float* smap, const int64_t* smap_strides_host, fsn_stream_t stream);
int64_t fsn_psnr_workspace_doubles(int64_t N, int C, int H, int W);
int fsn_psnr(const float* x, const float* y, int64_t N, int C, int H, int W, const int64_t* x_strides_host,
             const int64_t* y_strides_host, double* workspace, float* out, fsn_stream_t stream);

/* The backward of the SSIM above (csrc/ssim_grad.hip): the gradient of sum_n upstream[n] * ssim_n, ssim_n = out[n] of
 * the forward (the mean of S over the interior and the channels of image n), with respect to x and y.  With the
 * forward's taps w, radius r, cn, C1, C2 and moments, A1 = 2 ux uy + C1, A2 = 2 cn (uxy - ux uy) + C2,
 * B1 = ux^2 + uy^2 + C1, B2 = cn (uxx - ux^2 + uyy - uy^2) + C2, S = A1 A2 / (B1 B2); on the interior, zero elsewhere,
 * with g = upstream[n] / (C (H-2r) (W-2r)):
 *   Suxy = 2 cn A1 / (B1 B2),   Suxx = Suyy = -S cn / B2,
 *   Sux  = (2 uy A2 - 2 cn uy A1) / (B1 B2) - 2 S ux / B1 + 2 S cn ux / B2,   Suy: x and y swapped;
 *   dx(p) = F[g Sux](p) + 2 x(p) F[g Suxx](p) + y(p) F[g Suxy](p),  F[m](p) = sum_q w(q - p) m(q),  dy: x and y swapped.
 * The reflect edges play no part: an interior window never leaves the image.  Float64 throughout, one rounding to the
 * float32 outputs; every output pixel sums over its own window in a fixed order (no atomics): bitwise reproducible, and
 * an image's gradient does not depend on the rest of the batch.
 * x, y, strides, window, use_sample_covariance, data_range, K1, K2: as in the forward, validated alike.  upstream:
 * DEVICE double [N] = dL/d ssim_n.  dx, dy: DEVICE float32 with their own HOST strides, every element written; one of
 * them may be NULL, not both.  workspace: the workspace query below, in doubles.  N = 0 is a no-op. */
int64_t fsn_ssim_grad_workspace_doubles(int64_t N, int C, int H, int W);
int fsn_ssim_grad(const float* x, const float* y, int64_t N, int C, int H, int W, const int64_t* x_strides_host,
                  const int64_t* y_strides_host, int window, int use_sample_covariance, double data_range, double K1,
                  double K2, const double* upstream, double* workspace, float* dx, const int64_t* dx_strides_host,
                  float* dy, const int64_t* dy_strides_host, fsn_stream_t stream);

/* LPIPS v0.1, VGG16 backbone (the `lpips` package's LPIPS(net="vgg")), of N image pairs x, y (float32, DEVICE, 3
 * channels, H x W >= 16 x 16), read through their element strides (n, c, h, w) as the metrics above.  Per pair: the
 * optional 2x - 1 (normalize != 0), the scaling layer (x - shift) / scale, the 13 convolutions of VGG16's `features`
 * (3x3, padding 1, bias, ReLU; 2x2 stride-2 max-pools, floor on odd sizes) on the f32 MFMA, and at relu1_2, relu2_2,
 * relu3_3, relu4_3, relu5_3: each pixel's channel vector over (its norm + 1e-10), the squared difference, the 1x1 lin
 * weights, the spatial mean; their sum.  Head sums in float64 in a fixed order: bitwise reproducible.
 * fsn_lpips_pack: the weights (DEVICE float32, contiguous) into `packed` (fsn_lpips_pack_bytes() bytes, device):
 *   conv_w_host / conv_b_host: HOST arrays of 13 device pointers ([Cout][Cin][3][3] and [Cout], VGG16 order),
 *   lin_w_host: HOST array of 5 device pointers ([C] = the [1][C][1][1] lin weights), shift / scale: 3 floats each.
 * fsn_lpips_vgg: out: N floats (one per pair); per_layer (optional): [5][N] floats, the five taps' values.
 *   workspace: fsn_lpips_workspace_floats(H, W) floats (device), independent of N: the pairs run one after another.
 *   N = 0 is a no-op. */
int64_t fsn_lpips_pack_bytes(void);
int fsn_lpips_pack(const float* const* conv_w_host, const float* const* conv_b_host, const float* const* lin_w_host,
                   const float* shift, const float* scale, void* packed, fsn_stream_t stream);
int64_t fsn_lpips_workspace_floats(int H, int W);
int fsn_lpips_vgg(const void* packed, const float* x, const float* y, int64_t N, int H, int W,
                  const int64_t* x_strides_host, const int64_t* y_strides_host, int normalize, float* out,
                  float* per_layer, float* workspace, fsn_stream_t stream);
/* LPIPS-VGG as a loss: the gradient of sum_b upstream[b] * lpips_b with respect to the images (the VGG and lin
 * weights are frozen).  B pairs go through the network together, the x images and then the y images on blockIdx.z.
 * fsn_lpips_vgg_fwd_save: fsn_lpips_vgg's values (out: B floats, per_layer (optional): [5][B]), bit for bit, and every
 *   layer's post-ReLU activation of the images that need a gradient kept in `workspace` (of the other image: the five
 *   taps only).  want_dx / want_dy: which image of a pair needs a gradient, not both zero.  1 <= B <= 32767.
 * fsn_lpips_vgg_bwd: on the workspace fsn_lpips_vgg_fwd_save left (same B, H, W, normalize, want_dx, want_dy):
 *   tap backward in float64 - with s = |f|, u = f / (s + 1e-10), g_c = 2 lin_c (ux_c - uy_c) upstream[b] / HW the x
 *   image gets g_k / (s + eps) - f_k (g . f) / (s (s + eps)^2), the y image the same with -g; a pixel whose tap
 *   vector is all zero gets 0 (autograd gives NaN there); plus the gradient arriving through the 2x2 max-pool, which
 *   goes to the FIRST maximum of its window in row-major order (an odd last row or column lies in no window); times
 *   the ReLU mask f > 0.  Convolution data gradients: the forward's MFMA kernel with Cin and Cout exchanged, on the
 *   weights of fsn_lpips_grad_pack ([Cin][9 Cout], taps flipped).  conv1_1 and the scaling layer: one direct kernel
 *   that writes dx / dy (DEVICE float32, HOST element strides (n, c, h, w), every element written; NULL for a
 *   gradient not wanted).  upstream: DEVICE double [B].  No atomics, fixed summation orders: bitwise reproducible,
 *   and a pair's gradient does not depend on the rest of the batch.
 * fsn_lpips_grad_pack: conv_w_host as in fsn_lpips_pack -> packed_grad (fsn_lpips_grad_pack_bytes() bytes, device).
 * fsn_lpips_train_workspace_floats: the workspace of the pair of calls, in floats (about 270 H W per back-propagated
 *   image for the activations, 128 H W for the gradients); validates as fsn_lpips_workspace_floats. */
int64_t fsn_lpips_grad_pack_bytes(void);
int fsn_lpips_grad_pack(const float* const* conv_w_host, void* packed_grad, fsn_stream_t stream);
int64_t fsn_lpips_train_workspace_floats(int64_t B, int H, int W, int want_dx, int want_dy);
int fsn_lpips_vgg_fwd_save(const void* packed, const float* x, const float* y, int64_t B, int H, int W,
                           const int64_t* x_strides_host, const int64_t* y_strides_host, int normalize, int want_dx,
                           int want_dy, float* out, float* per_layer, float* workspace, fsn_stream_t stream);
int fsn_lpips_vgg_bwd(const void* packed, const void* packed_grad, int64_t B, int H, int W, int normalize, int want_dx,
                      int want_dy, const double* upstream, float* workspace, float* dx, const int64_t* dx_strides_host,
                      float* dy, const int64_t* dy_strides_host, fsn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FSNERF_HIP_H */
