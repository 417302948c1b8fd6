// Shared launcher declarations between the .hip kernel TUs and the
// torch-extension bindings TU. Streams are passed as the raw HIP stream
// pointer (forward-declared so the bindings TU needs no HIP headers).
#pragma once

#include <cstdint>

struct ihipStream_t;
using tft_stream = ihipStream_t*;

namespace torchft_amd {

// fp8_quant.hip ------------------------------------------------------------
// dtype_code: 0 = bf16, 1 = fp16, 2 = fp32
void launch_quantize_dtype(int dtype_code, const int64_t* ptrs,
                           const int64_t* block_prefix, const int64_t* numels,
                           int n_tensors, int64_t total_blocks,
                           int64_t padded_blocks, int64_t blocks_per_rank,
                           int64_t slice_bytes, uint8_t* pack, tft_stream stream);

void launch_dequantize_dtype(int dtype_code, const int64_t* ptrs,
                             const int64_t* block_prefix, const int64_t* numels,
                             int n_tensors, int64_t total_blocks,
                             int64_t padded_blocks, int64_t blocks_per_rank,
                             int64_t slice_bytes, const uint8_t* pack,
                             tft_stream stream);

void launch_reduce(const uint8_t* in, uint8_t* out, int world,
                   int64_t blocks_per_rank, int64_t slice_bytes, bool avg,
                   tft_stream stream);

// fused_model_ops.hip ------------------------------------------------------
void launch_rmsnorm_fwd(const void* x, const void* w, void* y, float* invrms,
                        int64_t rows, int H, float eps, tft_stream stream);
void launch_rmsnorm_bwd(const void* dy, const void* x, const void* w,
                        const float* invrms, void* dx, float* dw, int64_t rows,
                        int H, tft_stream stream);
void launch_rope(const void* x, void* out, const float* cos_tab,
                 const float* sin_tab, int64_t total_pairs, int S, int Hh, int D,
                 bool backward, tft_stream stream);
void launch_swiglu_fwd(const void* a, const void* b, void* out, int64_t n,
                       tft_stream stream);
void launch_swiglu_glu_fwd(const void* gu, void* out, int64_t rows, int64_t f,
                           tft_stream stream);
void launch_swiglu_glu_bwd(const void* dy, const void* gu, void* dgu,
                           int64_t rows, int64_t f, tft_stream stream);
void launch_swiglu_bwd(const void* dy, const void* a, const void* b, void* da,
                       void* db, int64_t n, tft_stream stream);

// fused_adamw.hip ----------------------------------------------------------
void launch_adamw(const int64_t* param_ptrs, const int64_t* grad_ptrs,
                  const int64_t* m_ptrs, const int64_t* v_ptrs,
                  const int64_t* numels, const int64_t* block_prefix,
                  int n_tensors, int64_t total_blocks, float lr, float beta1,
                  float beta2, float eps, float weight_decay,
                  float bias_correction1, float bias_correction2,
                  tft_stream stream);
// clip mode: coefficient from stats[0] (global sum of squared gradients),
// bias corrections from the per-tensor device int32 step counts; a
// non-finite norm stores nothing
void launch_adamw_clip(const int64_t* param_ptrs, const int64_t* grad_ptrs,
                       const int64_t* m_ptrs, const int64_t* v_ptrs,
                       const int64_t* numels, const int64_t* block_prefix,
                       const int64_t* step_ptrs, int n_tensors,
                       int64_t total_blocks, float lr, float beta1, float beta2,
                       float eps, float weight_decay, const float* stats,
                       float max_norm, tft_stream stream);
// finite norm: ++*step[t] for every tensor; else ++*skipped. norm_out[0] = norm
void launch_adamw_bump_steps(const int64_t* step_ptrs, int n_tensors,
                             const float* stats, int32_t* skipped, float* norm_out,
                             tft_stream stream);

// grad_norm.hip ------------------------------------------------------------
// dtype_code as above. `grid` workgroups grid-stride over total_blocks logical
// blocks and write partials[0..grid); finalize sums n_partials of them in
// double into stats[0] (the sum of squares, fp32).
void launch_grad_sumsq_partial(int dtype_code, const int64_t* ptrs,
                               const int64_t* numels, const int64_t* block_prefix,
                               int n_tensors, int64_t total_blocks, int grid,
                               float* partials, tft_stream stream);
void launch_grad_sumsq_finalize(const float* partials, int n_partials, float* stats,
                                tft_stream stream);
// in place g *= min(1, max_norm / (sqrt(stats[0]) + 1e-6)); no-op if non-finite
void launch_grad_scale(int dtype_code, const int64_t* ptrs, const int64_t* numels,
                       const int64_t* block_prefix, int n_tensors,
                       int64_t total_blocks, const float* stats, float max_norm,
                       tft_stream stream);

}  // namespace torchft_amd

namespace torchft_amd {

// flash_attn_bwd.hip --------------------------------------------------------
void launch_fa_fwd(const void* q, const void* k, const void* v, void* out,
                   float* lse, int B, int Hq, int Hkv, int S, float scale,
                   bool causal, bool bshd, tft_stream stream);
void launch_fa_delta(const void* dout, const void* o, float* delta,
                     int64_t rows, int Hq, int S, bool bshd, tft_stream stream);
void launch_fa_bwd(const void* q, const void* k, const void* v, const void* dout,
                   const float* lse, const float* delta, void* dq, void* dk,
                   void* dv, int B, int Hq, int Hkv, int S, float scale,
                   bool causal, bool bshd, tft_stream stream);

// fused_cross_entropy.hip ---------------------------------------------------
// logits: bf16 [rows, V] contiguous, overwritten with the gradient when
// write_grad; grad_scale: one fp32 on the device.
void launch_cross_entropy(void* logits, const int64_t* targets, float* row_loss,
                          const float* grad_scale, int64_t rows, int V,
                          int64_t ignore_index, float z_loss, bool write_grad,
                          tft_stream stream);

// diloco_sync.hip -----------------------------------------------------------
// dtype_code as above; every tensor of one call has that dtype.
// out[t] = a[t] - b[t], one rounding
void launch_pseudograd(int dtype_code, const int64_t* out_ptrs, const int64_t* a_ptrs,
                       const int64_t* b_ptrs, const int64_t* numels,
                       const int64_t* block_prefix, int n_tensors,
                       int64_t total_blocks, tft_stream stream);
// outer SGD on the snapshots g from the pseudo-gradients d (momentum buffers m
// read only when has_momentum), then l <- lerp(new g, l, alpha); g, m, l in place
void launch_outer_sgd(int dtype_code, bool has_momentum, const int64_t* g_ptrs,
                      const int64_t* l_ptrs, const int64_t* d_ptrs,
                      const int64_t* m_ptrs, const int64_t* numels,
                      const int64_t* block_prefix, int n_tensors,
                      int64_t total_blocks, float lr, float mu, bool nesterov,
                      float alpha, tft_stream stream);

// mfma_probe.hip ------------------------------------------------------------
void launch_mfma_probe(const void* A, const void* B, float* D, tft_stream s);

}  // namespace torchft_amd
