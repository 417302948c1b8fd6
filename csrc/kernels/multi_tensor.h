// Device side of the multi-tensor addressing shared by fp8_quant.hip,
// fused_adamw.hip, grad_norm.hip and diloco_sync.hip (docs/KERNELS.md,
// "Shared conventions"): the block -> tensor search, the per-lane block
// cursor and the dtype dispatch. The 8-element accessors are vec8.h's; the
// table itself (MultiTensorTable) and the block constants live in kernels.h.
// The fp8 kernels use everything but the cursor (see fp8_quant.hip for why).
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

#include <hip/hip_runtime.h>

#include "vec8.h"

namespace torchft_amd {

static_assert(kMtEpt == 8, "a lane's elements are one load8 / store8 of vec8.h");

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
