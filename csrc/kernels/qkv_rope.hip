// Fused QKV split + rotary embedding for the Llama attention block, CDNA4
// (gfx950) native.
//
// Forward: reads the fused projection qkv [B, S, (Hq + 2*Hkv) * D] once and
// writes contiguous q [B,S,Hq,D], k and v [B,S,Hkv,D]; q and k are rotated
// (rotate-half pairing, the arithmetic of rope_kernel in fused_model_ops.hip),
// v is copied. Backward: reads dq, dk, dv once and writes every element of
// dqkv (the rotation transpose on the q and k heads). The optional
// `positions` gives every token its own row of the tables (document position
// reset for packed rows); without it a token reads row s.
//
// One lane per item of 16 elements (qkv_layout.h): two 16 B accesses on each
// side, two float4 each of cos and sin.

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "qkv_layout.h"
#include "vec8.h"

namespace torchft_amd {

using bf16 = __hip_bfloat16;

namespace {

// What a lane works on: item `it` of token `token`.
struct QkvItemAddr {
  int cls;             // kQkvQ / kQkvK / kQkvV
  int col;             // first column of the lower half inside the head
  int64_t token;       // b * S + s
  int64_t packed_off;  // lower half in qkv / dqkv
  int64_t split_off;   // lower half in q / k / v (dq / dk / dv)
};

__device__ inline bool qkv_item(int64_t total_items, int Hq, int Hkv, int D,
                                QkvItemAddr& a) {
  const int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= total_items) return false;
  const int ipt = qkv_items_per_token(Hq, Hkv, D);
  a.token = item / ipt;
  const int it = (int)(item % ipt);
  a.cls = qkv_slot_class(qkv_item_slot(it, D), Hq, Hkv);
  a.col = qkv_item_col(it, D);
  a.packed_off = qkv_packed_off(a.token, it, Hq, Hkv, D);
  a.split_off = qkv_split_off(a.token, it, Hq, Hkv, D);
  return true;
}

// Rotates the lane's eight pairs in place: x1 = columns col .. col+7, x2 the
// same columns of the upper half. The expression of rope_kernel, with `sign`
// (+1 forward, -1 backward: the rotation transpose) a kernel argument as it
// is there, so that the compiler contracts the same terms in both files and
// the results agree bit for bit (docs/KERNELS.md, "qkv_rope.hip").
__device__ inline void rotate8(float (&x1)[8], float (&x2)[8],
                               const float* __restrict__ cos_tab,
                               const float* __restrict__ sin_tab,
                               const int* __restrict__ positions, int table_rows,
                               int S, int D, const QkvItemAddr& a, float sign) {
  const int pos = positions ? positions[a.token] : (int)(a.token % S);
  const int64_t t = (int64_t)rope_pos_row(pos, table_rows) * (D / 2) + a.col;
  float cc[8], ssn[8];
  load8(cos_tab + t, cc);
  load8(sin_tab + t, ssn);
#pragma unroll
  for (int k = 0; k < 8; k++) ssn[k] = ssn[k] * sign;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const float o1 = x1[k] * cc[k] - x2[k] * ssn[k];
    const float o2 = x2[k] * cc[k] + x1[k] * ssn[k];
    x1[k] = o1;
    x2[k] = o2;
  }
}

}  // namespace

// qkv: [B*S, (Hq + 2*Hkv) * D]; q: [B*S, Hq, D]; k, v: [B*S, Hkv, D];
// cos / sin: [table_rows, D/2] fp32; positions: [B*S] int32 or null.
__global__ void qkv_rope_fwd_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ q,
                                    bf16* __restrict__ k, bf16* __restrict__ v,
                                    const float* __restrict__ cos_tab,
                                    const float* __restrict__ sin_tab,
                                    const int* __restrict__ positions, int table_rows,
                                    int64_t total_items, int S, int Hq, int Hkv, int D,
                                    float sign) {
  QkvItemAddr a;
  if (!qkv_item(total_items, Hq, Hkv, D, a)) return;
  float x1[8], x2[8];
  load8(qkv + a.packed_off, x1);
  load8(qkv + a.packed_off + D / 2, x2);
  if (a.cls != kQkvV)
    rotate8(x1, x2, cos_tab, sin_tab, positions, table_rows, S, D, a, sign);
  bf16* out = (a.cls == kQkvQ ? q : (a.cls == kQkvK ? k : v)) + a.split_off;
  store8(out, x1);
  store8(out + D / 2, x2);
}

// The transpose: dq, dk, dv in, every element of dqkv out.
__global__ void qkv_rope_bwd_kernel(const bf16* __restrict__ dq,
                                    const bf16* __restrict__ dk,
                                    const bf16* __restrict__ dv, bf16* __restrict__ dqkv,
                                    const float* __restrict__ cos_tab,
                                    const float* __restrict__ sin_tab,
                                    const int* __restrict__ positions, int table_rows,
                                    int64_t total_items, int S, int Hq, int Hkv, int D,
                                    float sign) {
  QkvItemAddr a;
  if (!qkv_item(total_items, Hq, Hkv, D, a)) return;
  const bf16* in = (a.cls == kQkvQ ? dq : (a.cls == kQkvK ? dk : dv)) + a.split_off;
  float x1[8], x2[8];
  load8(in, x1);
  load8(in + D / 2, x2);
  if (a.cls != kQkvV)
    rotate8(x1, x2, cos_tab, sin_tab, positions, table_rows, S, D, a, sign);
  store8(dqkv + a.packed_off, x1);
  store8(dqkv + a.packed_off + D / 2, x2);
}

// ---------------------------------------------------------------- launchers

void launch_qkv_rope_fwd(const void* qkv, void* q, void* k, void* v,
                         const float* cos_tab, const float* sin_tab,
                         const int* positions, int table_rows, int64_t tokens, int S,
                         int Hq, int Hkv, int D, hipStream_t stream) {
  const int64_t items = tokens * qkv_items_per_token(Hq, Hkv, D);
  const int64_t grid = elementwise_grid(items, 1);
  if (grid == 0) return;
  hipLaunchKernelGGL(qkv_rope_fwd_kernel, dim3((uint32_t)grid), dim3(kElemThreads), 0,
                     stream, (const bf16*)qkv, (bf16*)q, (bf16*)k, (bf16*)v, cos_tab,
                     sin_tab, positions, table_rows, items, S, Hq, Hkv, D, 1.0f);
}

void launch_qkv_rope_bwd(const void* dq, const void* dk, const void* dv, void* dqkv,
                         const float* cos_tab, const float* sin_tab,
                         const int* positions, int table_rows, int64_t tokens, int S,
                         int Hq, int Hkv, int D, hipStream_t stream) {
  const int64_t items = tokens * qkv_items_per_token(Hq, Hkv, D);
  const int64_t grid = elementwise_grid(items, 1);
  if (grid == 0) return;
  hipLaunchKernelGGL(qkv_rope_bwd_kernel, dim3((uint32_t)grid), dim3(kElemThreads), 0,
                     stream, (const bf16*)dq, (const bf16*)dk, (const bf16*)dv,
                     (bf16*)dqkv, cos_tab, sin_tab, positions, table_rows, items, S, Hq,
                     Hkv, D, -1.0f);
}

}  // namespace torchft_amd
