// Multi-tensor global gradient norm and in-place clip — CDNA4 (gfx950) native.
//
// The L2 norm of a whole gradient zoo in two launches, with no atomics:
//
//   grad_sumsq_partial_kernel   capped grid, grid-stride over the 2048-element
//                               logical blocks of the multi-tensor table
//                               (same addressing as fused_adamw.hip); each
//                               workgroup writes ONE fp32 partial
//   grad_sumsq_finalize_kernel  one workgroup sums the partials in double and
//                               writes sumsq (fp32) to stats[0]
//
// Every addition happens in an order fixed by (table, grid size) alone, so
// the result is bitwise reproducible for a given max_blocks. The sum of
// squares (not the norm) is what is published: sharded callers all-reduce it
// before anything takes the square root.
//
// grad_scale_kernel is the stand-alone clip: g *= min(1, max_norm/(norm+1e-6)),
// a no-op when the norm is non-finite. FusedAdamW's clip mode folds the same
// coefficient into its gradient read instead (fused_adamw.hip).

#include <hip/hip_runtime.h>

#include "multi_tensor.h"

namespace torchft_amd {

// Longest fp32 addition chain: 8 per logical block a workgroup visits
// (ceil(total_blocks / gridDim.x) of them), 6 shuffle steps, 3 wave adds.
template <typename T>
__global__ void __launch_bounds__(kMtThreads)
grad_sumsq_partial_kernel(MultiTensorTable tb, float* __restrict__ partials) {
  float acc = 0.f;
  for (int64_t b = blockIdx.x; b < tb.total_blocks; b += gridDim.x) {
    const MtCursor c(tb, b, threadIdx.x);
    if (c.cnt == 0) continue;
    const int64_t a = c.addr(tb, 0);
    const T* g = c.at<const T>(a);
    if (c.vec_ok(a)) {
      float gv[kMtEpt];
      load8(g, gv);
#pragma unroll
      for (int i = 0; i < kMtEpt; i++) acc = fmaf(gv[i], gv[i], acc);
    } else {
      for (int i = 0; i < c.cnt; i++) {
        const float x = to_f32(g[i]);
        acc = fmaf(x, x, acc);
      }
    }
  }

  // wave64 shuffle tree, then the four wave sums in index order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  __shared__ float wave_sum[kMtThreads / 64];
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

__global__ void __launch_bounds__(kMtThreads)
grad_sumsq_finalize_kernel(const float* __restrict__ partials, int n_partials,
                           float* __restrict__ stats) {
  __shared__ double red[kMtThreads];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += kMtThreads) s += (double)partials[i];
  red[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int w = kMtThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) stats[0] = (float)red[0];
}

template <typename T>
__global__ void __launch_bounds__(kMtThreads)
grad_scale_kernel(MultiTensorTable tb, const float* __restrict__ stats, float max_norm) {
  const float norm = sqrtf(stats[0]);
  if (!isfinite(norm)) return;
  const float coef = fminf(1.f, max_norm / (norm + 1e-6f));
  if (coef == 1.f) return;  // g * 1.0f changes no bit

  const MtCursor c(tb, blockIdx.x, threadIdx.x);
  if (c.cnt == 0) return;
  const int64_t a = c.addr(tb, 0);
  T* g = c.at<T>(a);
  if (c.vec_ok(a)) {
    float gv[kMtEpt];
    load8(g, gv);
#pragma unroll
    for (int i = 0; i < kMtEpt; i++) gv[i] *= coef;
    store8(g, gv);
  } else {
    for (int i = 0; i < c.cnt; i++) from_f32(g + i, to_f32(g[i]) * coef);
  }
}

void launch_grad_sumsq_partial(int dtype_code, MultiTensorTable tb, int grid,
                               float* partials, hipStream_t stream) {
  if (tb.total_blocks <= 0 || grid <= 0) return;
  dispatch_dtype(dtype_code, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(grad_sumsq_partial_kernel<T>, dim3(grid), dim3(kMtThreads), 0,
                       stream, tb, partials);
  });
}

void launch_grad_sumsq_finalize(const float* partials, int n_partials, float* stats,
                                hipStream_t stream) {
  hipLaunchKernelGGL(grad_sumsq_finalize_kernel, dim3(1), dim3(kMtThreads), 0, stream,
                     partials, n_partials, stats);
}

void launch_grad_scale(int dtype_code, MultiTensorTable tb, const float* stats,
                       float max_norm, hipStream_t stream) {
  if (tb.total_blocks <= 0) return;
  dispatch_dtype(dtype_code, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(grad_scale_kernel<T>, dim3((uint32_t)tb.total_blocks),
                       dim3(kMtThreads), 0, stream, tb, stats, max_norm);
  });
}

}  // namespace torchft_amd
