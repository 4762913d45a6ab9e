// train_internal.hpp — entry points of the fused (MFMA) training path, called from the C-ABI in train.hip and
// input_grad.hip.
#pragma once
#include "common.hpp"

namespace fsn {

struct TrainRays {  // ray form of the forward's inputs: sample s = midpoint of [t0[s], t1[s]) on ray ri[s]
  const float *rays_o, *rays_d, *t0, *t1;
  const int64_t* ri;
};

struct InputGradReq {  // gradients to the network's inputs (fsn_nerf_train_bwd_inputs): the forward's inputs again
  const float *x, *dirs;     // point form, or null with `rays`
  const TrainRays* rays;
  const float *pos_mask, *dir_mask;
  float *d_x, *d_dirs;       // [n,3] each, either may be null
};

int64_t fused_train_workspace_floats(const fsn_mlp_desc& d, int prec, int64_t n);
int fused_train_fwd(const fsn_mlp_desc* d, int prec, const float* const* W, const float* const* b, const float* x,
                    const float* dirs, const float* pos_mask, const float* dir_mask, int64_t n, float* ws, float* out,
                    uint32_t* status, hipStream_t s, const TrainRays* rays = nullptr);
int fused_train_bwd(const fsn_mlp_desc* d, int prec, const float* const* W, int64_t n, float* ws, const float* out,
                    const float* d_out, const float* grad_scale_dev, float* const* dW, float* const* db,
                    bool accumulate, float* bscale, uint32_t* bamax, uint32_t* status, hipStream_t s,
                    const InputGradReq* ig = nullptr);

// train.hip: the descriptor check of the training path, and the validated body shared by fsn_nerf_train_bwd (rq null)
// and fsn_nerf_train_bwd_inputs (`who` prefixes the messages).
int check_desc(const fsn_mlp_desc* d);
int train_bwd_checked(const char* who, const fsn_mlp_desc* desc, int prec, const float* const* W, int64_t n, float* ws,
                      const float* out, const float* d_out, const float* grad_scale, float* const* dW, float* const* db,
                      int accumulate, float* stage_scales, uint32_t* stage_amax, uint32_t* status, fsn_stream_t stream,
                      const InputGradReq* rq);

// k_input_grad (input_grad.hip), launched by fused_train_bwd between the dgrad chain and k_bwd_rescale.  The packed
// weight slices go where the chain's transposed-weight stream lay (dead once the chain has run; the workspace layout
// sizes that area for the larger of the two streams).
struct InputGradWs {
  int64_t blob;                   // float offsets into the workspace: the backward stream's area
  int64_t dp, h_stride, dbo;      // dPre_0 (stage l at dp + l h_stride), dBo
};
int input_grad_launch(const fsn_mlp_desc& d, int prec, const float* const* W, int64_t n, float* ws, const InputGradWs& o,
                      const float* grad_scale_dev, const float* bscale, const uint32_t* status, const InputGradReq& rq,
                      hipStream_t s);

}  // namespace fsn
