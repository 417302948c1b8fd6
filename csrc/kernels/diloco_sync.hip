// Fused DiLoCo outer sync — CDNA4 (gfx950) native.
//
// Two multi-tensor kernels replace the per-parameter torch ops of the
// Streaming DiLoCo outer sync (torchft_amd/local_sgd.py, fused_sync=True):
//
//   pseudograd_kernel   out = a - b for a whole fragment in one launch; the
//                       outputs are views into the flat allreduce buckets, so
//                       no flatten copy follows
//   outer_sgd_kernel    SGD (momentum / Nesterov) on the global snapshot from
//                       the averaged pseudo-gradient, re-snapshot, and the
//                       lerp of local progress back into the parameter — one
//                       launch per param group
//
// Addressing is the one of fused_adamw.hip / grad_norm.hip: pointer / numel /
// block_prefix tables, 2048-element logical blocks, a wave-uniform binary
// search per block, 8 elements (16 B for bf16/fp16, 2 x 16 B for fp32) per
// lane. A tensor with any pointer off a 16 B boundary, and the partial last
// vector of every tensor, take the element-wise path. All math is fp32; every
// thread reads its elements before it writes them, and no two threads touch
// the same element, so the in-place parameter update needs no atomics.

#include <hip/hip_runtime.h>

#include "multi_tensor.h"

namespace torchft_amd {

// out[i] = T(float(a[i]) - float(b[i])): one rounding, torch's `a - b`.
template <typename T>
__global__ void __launch_bounds__(kMtThreads) pseudograd_kernel(MultiTensorTable tb) {
  const MtCursor c(tb, blockIdx.x, threadIdx.x);
  if (c.cnt == 0) return;
  const int64_t po = c.addr(tb, 0), pa = c.addr(tb, 1), pb = c.addr(tb, 2);
  T* out = c.at<T>(po);
  const T* a = c.at<const T>(pa);
  const T* b = c.at<const T>(pb);
  if (c.vec_ok(po | pa | pb)) {
    float av[kMtEpt], bv[kMtEpt];
    load8(a, av);
    load8(b, bv);
#pragma unroll
    for (int i = 0; i < kMtEpt; i++) av[i] -= bv[i];
    store8(out, av);
  } else {
    for (int i = 0; i < c.cnt; i++) from_f32(out + i, to_f32(a[i]) - to_f32(b[i]));
  }
}

// Per element, in fp32 (g snapshot, d averaged pseudo-gradient, m momentum,
// l local parameter; l and the stored parameter are the same memory):
//   m' = mu*m + d                     (no momentum: u = d)
//   u  = nesterov ? d + mu*m' : m'
//   g' = g - lr*u
//   m <- T(m'),  g <- T(g'),  gs = float(T(g'))
//   p  = alpha < 0.5 ? gs + alpha*(l - gs) : l - (l - gs)*(1 - alpha)
//   l <- T(p)
// alpha == 0 gives p == gs and alpha == 1 gives p == l exactly, with or
// without fma contraction: the product is an exact zero either way.
template <typename T, bool HAS_MOMENTUM>
__device__ inline void outer_sgd_elem(float& g, float d, float& m, float& l, float lr,
                                      float mu, bool nesterov, float alpha) {
  float u = d;
  if constexpr (HAS_MOMENTUM) {
    m = mu * m + d;
    u = nesterov ? d + mu * m : m;
  }
  g = g - lr * u;
  const float gs = d_round((T*)nullptr, g);
  const float diff = l - gs;
  l = alpha < 0.5f ? gs + alpha * diff : l - diff * (1.f - alpha);
}

template <typename T, bool HAS_MOMENTUM>
__global__ void __launch_bounds__(kMtThreads)
outer_sgd_kernel(MultiTensorTable tb, float lr, float mu, int nesterov, float alpha) {
  const MtCursor c(tb, blockIdx.x, threadIdx.x);
  if (c.cnt == 0) return;
  const int64_t pg = c.addr(tb, 0), pl = c.addr(tb, 1), pd = c.addr(tb, 2);
  int64_t pm = 0;
  if constexpr (HAS_MOMENTUM) pm = c.addr(tb, 3);
  T* g = c.at<T>(pg);
  T* l = c.at<T>(pl);
  const T* d = c.at<const T>(pd);
  T* m = nullptr;
  if constexpr (HAS_MOMENTUM) m = c.at<T>(pm);
  const bool nes = nesterov != 0;

  if (c.vec_ok(pg | pl | pd | pm)) {
    float gv[kMtEpt], lv[kMtEpt], dv[kMtEpt], mv[kMtEpt] = {};
    load8(g, gv);
    load8(l, lv);
    load8(d, dv);
    if constexpr (HAS_MOMENTUM) load8(m, mv);
#pragma unroll
    for (int i = 0; i < kMtEpt; i++)
      outer_sgd_elem<T, HAS_MOMENTUM>(gv[i], dv[i], mv[i], lv[i], lr, mu, nes, alpha);
    if constexpr (HAS_MOMENTUM) store8(m, mv);
    store8(g, gv);
    store8(l, lv);
  } else {
    for (int i = 0; i < c.cnt; i++) {
      float gf = to_f32(g[i]), lf = to_f32(l[i]), mf = 0.f;
      const float df = to_f32(d[i]);
      if constexpr (HAS_MOMENTUM) mf = to_f32(m[i]);
      outer_sgd_elem<T, HAS_MOMENTUM>(gf, df, mf, lf, lr, mu, nes, alpha);
      if constexpr (HAS_MOMENTUM) from_f32(m + i, mf);
      from_f32(g + i, gf);
      from_f32(l + i, lf);
    }
  }
}

void launch_pseudograd(int dtype_code, MultiTensorTable tb, hipStream_t stream) {
  if (tb.total_blocks <= 0) return;
  dispatch_dtype(dtype_code, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(pseudograd_kernel<T>, dim3((uint32_t)tb.total_blocks),
                       dim3(kMtThreads), 0, stream, tb);
  });
}

void launch_outer_sgd(int dtype_code, bool has_momentum, MultiTensorTable tb,
                      float lr, float mu, bool nesterov, float alpha,
                      hipStream_t stream) {
  if (tb.total_blocks <= 0) return;
  const dim3 grid((uint32_t)tb.total_blocks);
  const int nes = nesterov ? 1 : 0;
  dispatch_dtype(dtype_code, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (has_momentum)
      hipLaunchKernelGGL((outer_sgd_kernel<T, true>), grid, dim3(kMtThreads), 0, stream,
                         tb, lr, mu, nes, alpha);
    else
      hipLaunchKernelGGL((outer_sgd_kernel<T, false>), grid, dim3(kMtThreads), 0, stream,
                         tb, lr, mu, nes, alpha);
  });
}

}  // namespace torchft_amd
