// Shared launcher declarations between the .hip kernel TUs and the
// torch-extension bindings TU. Streams are passed as the raw HIP stream
// pointer (forward-declared so the bindings TU needs no HIP headers).
#pragma once

#include <cstdint>

struct ihipStream_t;
using tft_stream = ihipStream_t*;

// callable from kernels when a HIP compiler reads this header
#if defined(__HIP__)
#define TFT_HD __host__ __device__
#else
#define TFT_HD
#endif

namespace torchft_amd {

// Multi-tensor addressing (docs/KERNELS.md, "Shared conventions") -----------
// Tensors are cut into logical blocks of kMtBlock elements; a workgroup of
// kMtThreads lanes handles one block, kMtEpt elements per lane.
constexpr int kMtBlock = 2048;
constexpr int kMtThreads = 256;
constexpr int kMtEpt = 8;
static_assert(kMtBlock == kMtThreads * kMtEpt, "one lane per kMtEpt elements");

enum DtypeCode : int { kBF16 = 0, kF16 = 1, kF32 = 2 };

// View of one device table of n tensors (rows) and n_cols pointer columns:
//   [col 0 | ... | col n_cols-1 | numels | block_prefix (n+1)]
// every column n int64 entries; tensor t owns the logical blocks
// [prefix()[t], prefix()[t+1]). Passed to launchers and kernels by value.
struct MultiTensorTable {
  const int64_t* base;
  int n;
  int n_cols;
  int64_t total_blocks;

  TFT_HD const int64_t* col(int j) const { return base + (int64_t)j * n; }
  TFT_HD const int64_t* numels() const { return col(n_cols); }
  TFT_HD const int64_t* prefix() const { return col(n_cols + 1); }
};

// fp8_quant.hip ------------------------------------------------------------
// table: col 0 = the tensors, every one 16 B-aligned (the bindings check).
// The grid is padded_blocks workgroups; blocks at or past tb.total_blocks are
// padding slots of the pack.
void launch_quantize_dtype(int dtype_code, MultiTensorTable tb,
                           int64_t padded_blocks, int64_t blocks_per_rank,
                           int64_t slice_bytes, uint8_t* pack, tft_stream stream);
void launch_dequantize_dtype(int dtype_code, MultiTensorTable tb,
                             int64_t padded_blocks, int64_t blocks_per_rank,
                             int64_t slice_bytes, const uint8_t* pack,
                             tft_stream stream);
void launch_reduce(const uint8_t* in, uint8_t* out, int world,
                   int64_t blocks_per_rank, int64_t slice_bytes, bool avg,
                   tft_stream stream);

// fused_model_ops.hip ------------------------------------------------------
// bf16 activations, weights and gradients, fp32 invrms and rotary tables, all
// contiguous and 16 B-aligned (the bindings see to both); H % 8 == 0,
// D % 8 == 0, n % 8 == 0, f % 8 == 0. No rows or no elements: no launch.
void launch_rmsnorm_fwd(const void* x, const void* w, void* y, float* invrms,
                        int64_t rows, int H, float eps, tft_stream stream);
// a workgroup keeps its fp32 dw[H] in dynamic LDS next to the static LDS of
// block_reduce_sum<256> (one float per wave; the .hip file asserts the size):
// H * 4 + kRmsnormBwdStaticLdsBytes <= kRmsnormBwdMaxLdsBytes, so H <= 40952.
// dw must be zeros. Returns the launch's HIP status, 0 for success.
constexpr int64_t kRmsnormBwdMaxLdsBytes = 160 * 1024;
constexpr int64_t kRmsnormBwdStaticLdsBytes = 16;
int launch_rmsnorm_bwd(const void* dy, const void* x, const void* w,
                        const float* invrms, void* dx, float* dw, int64_t rows,
                        int H, tft_stream stream);
// The launchers below give every lane `per_lane` items (4 pairs, 8
// elements) and a workgroup kElemThreads lanes. The grid must stay below 2^31.
constexpr int kElemThreads = 256;
constexpr int64_t elementwise_grid(int64_t items, int per_lane) {
  return (items + per_lane * kElemThreads - 1) / (per_lane * kElemThreads);
}
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

// qkv_rope.hip ---------------------------------------------------------------
// Fused split + rotary of the QKV projection (qkv_layout.h has the map).
// qkv / dqkv: bf16 [tokens, (Hq + 2*Hkv) * D]; q / dq: [tokens, Hq, D]; k, v /
// dk, dv: [tokens, Hkv, D]; tokens = B * S. All contiguous and 16 B-aligned,
// D % 16 == 0. cos / sin: fp32 [table_rows, D/2], table_rows >= 1. positions:
// int32 [tokens] on the device, or null for position s = token % S (then
// table_rows >= S). One lane per 16 elements, elementwise_grid(items, 1)
// workgroups (below 2^31); no tokens, no launch. The backward writes every
// element of dqkv.
void launch_qkv_rope_fwd(const void* qkv, void* q, void* k, void* v,
                         const float* cos_tab, const float* sin_tab,
                         const int* positions, int table_rows, int64_t tokens, int S,
                         int Hq, int Hkv, int D, tft_stream stream);
void launch_qkv_rope_bwd(const void* dq, const void* dk, const void* dv, void* dqkv,
                         const float* cos_tab, const float* sin_tab,
                         const int* positions, int table_rows, int64_t tokens, int S,
                         int Hq, int Hkv, int D, tft_stream stream);

// fused_adamw.hip ----------------------------------------------------------
// table: cols 0..3 = param, grad, exp_avg, exp_avg_sq (bf16, bf16, fp32, fp32)
void launch_adamw(MultiTensorTable tb, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float bias_correction1,
                  float bias_correction2, tft_stream stream);
// clip mode: col 4 = the per-tensor device int32 step counts the bias
// corrections come from; coefficient from stats[0] (global sum of squared
// gradients); a non-finite norm stores nothing
void launch_adamw_clip(MultiTensorTable tb, float lr, float beta1, float beta2,
                       float eps, float weight_decay, const float* stats,
                       float max_norm, tft_stream stream);
// finite norm: ++*step[t] for every tensor; else ++*skipped. norm_out[0] = norm
void launch_adamw_bump_steps(const int64_t* step_ptrs, int n_tensors,
                             const float* stats, int32_t* skipped, float* norm_out,
                             tft_stream stream);

// grad_norm.hip ------------------------------------------------------------
// table: col 0 = the gradients. `grid` workgroups grid-stride over the
// logical blocks and write partials[0..grid); finalize sums n_partials of
// them in double into stats[0] (the sum of squares, fp32).
void launch_grad_sumsq_partial(int dtype_code, MultiTensorTable tb, int grid,
                               float* partials, tft_stream stream);
void launch_grad_sumsq_finalize(const float* partials, int n_partials, float* stats,
                                tft_stream stream);
// in place g *= min(1, max_norm / (sqrt(stats[0]) + 1e-6)); no-op if non-finite
void launch_grad_scale(int dtype_code, MultiTensorTable tb, const float* stats,
                       float max_norm, tft_stream stream);

// diloco_sync.hip -----------------------------------------------------------
// every tensor of one call has the dtype of dtype_code.
// cols 0..2 = out, a, b: out[t] = a[t] - b[t], one rounding
void launch_pseudograd(int dtype_code, MultiTensorTable tb, tft_stream stream);
// cols 0..2 = g, l, d (col 3 = m when has_momentum): outer SGD on the
// snapshots g from the pseudo-gradients d, then l <- lerp(new g, l, alpha);
// g, m, l in place
void launch_outer_sgd(int dtype_code, bool has_momentum, MultiTensorTable tb,
                      float lr, float mu, bool nesterov, float alpha,
                      tft_stream stream);

// flash_attn_fwd.hip --------------------------------------------------------
// q / k / v / out: bf16, logical [B,H,S,128]; bshd = the storage is
// [B,S,H,128] (fa_layout.h, row_off). lse: dense fp32 [B,Hq,S]. S % 256 == 0.
// doc_start / doc_end: the document mask (fa_layout.h), dense int32 [B,S]
// device arrays, both null for no mask and given only with causal.
void launch_fa_fwd(const void* q, const void* k, const void* v, void* out,
                   float* lse, int B, int Hq, int Hkv, int S, float scale,
                   bool causal, bool bshd, const int* doc_start, const int* doc_end,
                   tft_stream stream);

// flash_attn_bwd.hip --------------------------------------------------------
// tensors and layouts as in the forward; delta: dense fp32 [B,Hq,S], the row
// sums of dout * o. launch_fa_bwd needs S % 128 == 0.
void launch_fa_delta(const void* dout, const void* o, float* delta,
                     int64_t rows, int Hq, int S, bool bshd, tft_stream stream);
void launch_fa_bwd(const void* q, const void* k, const void* v, const void* dout,
                   const float* lse, const float* delta, void* dq, void* dk,
                   void* dv, int B, int Hq, int Hkv, int S, float scale,
                   bool causal, bool bshd, const int* doc_start, const int* doc_end,
                   tft_stream stream);

// fused_cross_entropy.hip ---------------------------------------------------
// logits: bf16 [rows, V] contiguous, overwritten with the gradient when
// write_grad; grad_scale: one fp32 on the device.
void launch_cross_entropy(void* logits, const int64_t* targets, float* row_loss,
                          const float* grad_scale, int64_t rows, int V,
                          int64_t ignore_index, float z_loss, bool write_grad,
                          tft_stream stream);

// mfma_probe.hip ------------------------------------------------------------
void launch_mfma_probe(const void* A, const void* B, float* D, tft_stream s);

}  // namespace torchft_amd
