// Device side of the multi-tensor addressing shared by fp8_quant.hip,
// fused_adamw.hip, grad_norm.hip and diloco_sync.hip (docs/KERNELS.md,
// "Shared conventions"): the block -> tensor search, the 8-element
// accessors, the per-lane block cursor and the dtype dispatch. The table
// itself (MultiTensorTable) and the block constants live in kernels.h. The
// fp8 kernels use everything but the cursor (see fp8_quant.hip for why).
#pragma once

#include "kernels.h"

namespace torchft_amd {

// block_prefix has n+1 entries: tensor t owns blocks
// [block_prefix[t], block_prefix[t+1]). Returns the last t whose range
// starts at or before `block`, so repeated entries (empty tensors) are
// skipped. Wave-uniform on the device: every operand is scalar.
TFT_HD inline int find_tensor(const int64_t* block_prefix, int n, int64_t block) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (block_prefix[mid] <= block)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

}  // namespace torchft_amd

#if defined(__HIP__)

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

namespace torchft_amd {

// scalar conversions (torch extensions build with __HIP_NO_HALF_CONVERSIONS__)
__device__ inline float to_f32(__hip_bfloat16 v) { return __bfloat162float(v); }
__device__ inline float to_f32(__half v) { return __half2float(v); }
__device__ inline float to_f32(float v) { return v; }
__device__ inline void from_f32(__hip_bfloat16* d, float v) { *d = __float2bfloat16(v); }
__device__ inline void from_f32(__half* d, float v) { *d = __float2half(v); }
__device__ inline void from_f32(float* d, float v) { *d = v; }

// fp32 value of v after the round trip through T (what a store of v holds)
__device__ inline float d_round(__hip_bfloat16*, float v) {
  return __bfloat162float(__float2bfloat16(v));
}
__device__ inline float d_round(__half*, float v) { return __half2float(__float2half(v)); }
__device__ inline float d_round(float*, float v) { return v; }

// 8 elements per lane: one 16 B access for bf16/fp16, two for fp32. The
// address must be 16 B-aligned (MtCursor::vec_ok).
__device__ inline void load8(const __hip_bfloat16* p, float (&v)[kMtEpt]) {
  const uint4 raw = *reinterpret_cast<const uint4*>(p);
  const __hip_bfloat162* h = reinterpret_cast<const __hip_bfloat162*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float2 f = __bfloat1622float2(h[i]);
    v[2 * i] = f.x;
    v[2 * i + 1] = f.y;
  }
}
__device__ inline void load8(const __half* p, float (&v)[kMtEpt]) {
  const uint4 raw = *reinterpret_cast<const uint4*>(p);
  const __half2* h = reinterpret_cast<const __half2*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float2 f = __half22float2(h[i]);
    v[2 * i] = f.x;
    v[2 * i + 1] = f.y;
  }
}
__device__ inline void load8(const float* p, float (&v)[kMtEpt]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ inline void store8(__hip_bfloat16* p, const float (&v)[kMtEpt]) {
  uint4 raw;
  __hip_bfloat162* h = reinterpret_cast<__hip_bfloat162*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++)
    h[i] = __float22bfloat162_rn(make_float2(v[2 * i], v[2 * i + 1]));
  *reinterpret_cast<uint4*>(p) = raw;
}
__device__ inline void store8(__half* p, const float (&v)[kMtEpt]) {
  uint4 raw;
  __half2* h = reinterpret_cast<__half2*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++)
    h[i] = __float22half2_rn(make_float2(v[2 * i], v[2 * i + 1]));
  *reinterpret_cast<uint4*>(p) = raw;
}
__device__ inline void store8(float* p, const float (&v)[kMtEpt]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// Where lane `tid` of the workgroup handling logical block `block` works:
// tensor t, elements [off, off + cnt) of it. cnt is 0 for a lane past the
// tensor's end, kMtEpt everywhere but in the tensor's last vector.
struct MtCursor {
  int t;
  int64_t off;
  int cnt;

  __device__ MtCursor(const MultiTensorTable& tb, int64_t block, int tid) {
    const int64_t* prefix = tb.prefix();
    t = find_tensor(prefix, tb.n, block);
    off = (block - prefix[t]) * kMtBlock + tid * kMtEpt;
    const int64_t left = tb.numels()[t] - off;
    cnt = left >= kMtEpt ? kMtEpt : left > 0 ? (int)left : 0;
  }

  // address of this tensor in pointer column j, as the table holds it
  __device__ int64_t addr(const MultiTensorTable& tb, int j) const { return tb.col(j)[t]; }

  // this lane's first element of a tensor at address `a`
  template <typename T>
  __device__ T* at(int64_t a) const {
    return reinterpret_cast<T*>(a) + off;
  }

  // May this lane use load8/store8? `addrs` is the OR of every tensor
  // address it will access: all eight elements in range and every tensor
  // 16 B-aligned (off * sizeof(T) is a multiple of 16). Anything else, a view
  // such as buf[1:] or a tensor's last partial vector, goes element by element.
  __device__ bool vec_ok(int64_t addrs) const {
    return cnt == kMtEpt && (addrs & 15) == 0;
  }
};

// f(TypeTag<T>{}) with the element type of dtype_code
template <typename T>
struct TypeTag {
  using type = T;
};

template <typename F>
void dispatch_dtype(int dtype_code, F&& f) {
  switch (dtype_code) {
    case kBF16:
      f(TypeTag<__hip_bfloat16>{});
      break;
    case kF16:
      f(TypeTag<__half>{});
      break;
    default:
      f(TypeTag<float>{});
      break;
  }
}

}  // namespace torchft_amd

#endif  // __HIP__
