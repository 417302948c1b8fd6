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

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdint>

namespace torchft_amd {

#define GBLOCK 2048
#define GTHREADS 256
#define GEPT 8  // elements per thread per logical block

namespace {

__device__ inline float g_to_f32(__hip_bfloat16 v) { return __bfloat162float(v); }
__device__ inline float g_to_f32(__half v) { return __half2float(v); }
__device__ inline float g_to_f32(float v) { return v; }
__device__ inline void g_from_f32(__hip_bfloat16* d, float v) { *d = __float2bfloat16(v); }
__device__ inline void g_from_f32(__half* d, float v) { *d = __float2half(v); }
__device__ inline void g_from_f32(float* d, float v) { *d = v; }

// 8 elements per lane: one 16 B access for bf16/fp16, two for fp32.
__device__ inline void g_load8(const __hip_bfloat16* p, float (&v)[GEPT]) {
  const uint4 raw = *reinterpret_cast<const uint4*>(p);
  const __hip_bfloat162* h = reinterpret_cast<const __hip_bfloat162*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float2 f = __bfloat1622float2(h[i]);
    v[2 * i] = f.x;
    v[2 * i + 1] = f.y;
  }
}
__device__ inline void g_load8(const __half* p, float (&v)[GEPT]) {
  const uint4 raw = *reinterpret_cast<const uint4*>(p);
  const __half2* h = reinterpret_cast<const __half2*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float2 f = __half22float2(h[i]);
    v[2 * i] = f.x;
    v[2 * i + 1] = f.y;
  }
}
__device__ inline void g_load8(const float* p, float (&v)[GEPT]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ inline void g_store8(__hip_bfloat16* p, const float (&v)[GEPT]) {
  uint4 raw;
  __hip_bfloat162* h = reinterpret_cast<__hip_bfloat162*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++)
    h[i] = __float22bfloat162_rn(make_float2(v[2 * i], v[2 * i + 1]));
  *reinterpret_cast<uint4*>(p) = raw;
}
__device__ inline void g_store8(__half* p, const float (&v)[GEPT]) {
  uint4 raw;
  __half2* h = reinterpret_cast<__half2*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++)
    h[i] = __float22half2_rn(make_float2(v[2 * i], v[2 * i + 1]));
  *reinterpret_cast<uint4*>(p) = raw;
}
__device__ inline void g_store8(float* p, const float (&v)[GEPT]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// same search as find_tensor_a in fused_adamw.hip
__device__ inline int find_tensor_g(const int64_t* block_prefix, int n, int64_t b) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (block_prefix[mid] <= b)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

}  // namespace

// Longest fp32 addition chain: 8 per logical block a workgroup visits
// (ceil(total_blocks / gridDim.x) of them), 6 shuffle steps, 3 wave adds.
template <typename T>
__global__ void __launch_bounds__(GTHREADS)
grad_sumsq_partial_kernel(const int64_t* __restrict__ ptrs,
                          const int64_t* __restrict__ numels,
                          const int64_t* __restrict__ block_prefix, int n_tensors,
                          int64_t total_blocks, float* __restrict__ partials) {
  float acc = 0.f;
  for (int64_t b = blockIdx.x; b < total_blocks; b += gridDim.x) {
    const int t = find_tensor_g(block_prefix, n_tensors, b);
    const int64_t off = (b - block_prefix[t]) * GBLOCK + threadIdx.x * GEPT;
    const int64_t numel = numels[t];
    if (off >= numel) continue;
    const int64_t base = ptrs[t];
    const T* g = reinterpret_cast<const T*>(base) + off;
    // a view such as buf[1:] has a base that no 16 B load may start from
    if ((base & 15) == 0 && off + GEPT <= numel) {
      float gv[GEPT];
      g_load8(g, gv);
#pragma unroll
      for (int i = 0; i < GEPT; i++) acc = fmaf(gv[i], gv[i], acc);
    } else {
      const int cnt = numel - off < GEPT ? (int)(numel - off) : GEPT;
      for (int i = 0; i < cnt; i++) {
        const float x = g_to_f32(g[i]);
        acc = fmaf(x, x, acc);
      }
    }
  }

  // wave64 shuffle tree, then the four wave sums in index order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  __shared__ float wave_sum[GTHREADS / 64];
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

__global__ void __launch_bounds__(GTHREADS)
grad_sumsq_finalize_kernel(const float* __restrict__ partials, int n_partials,
                           float* __restrict__ stats) {
  __shared__ double red[GTHREADS];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += GTHREADS) s += (double)partials[i];
  red[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int w = GTHREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) stats[0] = (float)red[0];
}

template <typename T>
__global__ void __launch_bounds__(GTHREADS)
grad_scale_kernel(const int64_t* __restrict__ ptrs,
                  const int64_t* __restrict__ numels,
                  const int64_t* __restrict__ block_prefix, int n_tensors,
                  const float* __restrict__ stats, float max_norm) {
  const float norm = sqrtf(stats[0]);
  if (!isfinite(norm)) return;
  const float coef = fminf(1.f, max_norm / (norm + 1e-6f));
  if (coef == 1.f) return;  // g * 1.0f changes no bit

  const int64_t b = blockIdx.x;
  const int t = find_tensor_g(block_prefix, n_tensors, b);
  const int64_t off = (b - block_prefix[t]) * GBLOCK + threadIdx.x * GEPT;
  const int64_t numel = numels[t];
  if (off >= numel) return;
  const int64_t base = ptrs[t];
  T* g = reinterpret_cast<T*>(base) + off;
  if ((base & 15) == 0 && off + GEPT <= numel) {
    float gv[GEPT];
    g_load8(g, gv);
#pragma unroll
    for (int i = 0; i < GEPT; i++) gv[i] *= coef;
    g_store8(g, gv);
  } else {
    const int cnt = numel - off < GEPT ? (int)(numel - off) : GEPT;
    for (int i = 0; i < cnt; i++) g_from_f32(g + i, g_to_f32(g[i]) * coef);
  }
}

// dtype_code: 0 = bf16, 1 = fp16, 2 = fp32 (matches kernels.h)
void launch_grad_sumsq_partial(int dtype_code, const int64_t* ptrs,
                               const int64_t* numels, const int64_t* block_prefix,
                               int n_tensors, int64_t total_blocks, int grid,
                               float* partials, hipStream_t stream) {
  if (total_blocks <= 0 || grid <= 0) return;
  switch (dtype_code) {
    case 0:
      hipLaunchKernelGGL(grad_sumsq_partial_kernel<__hip_bfloat16>, dim3(grid),
                         dim3(GTHREADS), 0, stream, ptrs, numels, block_prefix,
                         n_tensors, total_blocks, partials);
      break;
    case 1:
      hipLaunchKernelGGL(grad_sumsq_partial_kernel<__half>, dim3(grid),
                         dim3(GTHREADS), 0, stream, ptrs, numels, block_prefix,
                         n_tensors, total_blocks, partials);
      break;
    default:
      hipLaunchKernelGGL(grad_sumsq_partial_kernel<float>, dim3(grid),
                         dim3(GTHREADS), 0, stream, ptrs, numels, block_prefix,
                         n_tensors, total_blocks, partials);
      break;
  }
}

void launch_grad_sumsq_finalize(const float* partials, int n_partials, float* stats,
                                hipStream_t stream) {
  hipLaunchKernelGGL(grad_sumsq_finalize_kernel, dim3(1), dim3(GTHREADS), 0, stream,
                     partials, n_partials, stats);
}

void launch_grad_scale(int dtype_code, const int64_t* ptrs, const int64_t* numels,
                       const int64_t* block_prefix, int n_tensors,
                       int64_t total_blocks, const float* stats, float max_norm,
                       hipStream_t stream) {
  if (total_blocks <= 0) return;
  const dim3 grid((uint32_t)total_blocks);
  switch (dtype_code) {
    case 0:
      hipLaunchKernelGGL(grad_scale_kernel<__hip_bfloat16>, grid, dim3(GTHREADS), 0,
                         stream, ptrs, numels, block_prefix, n_tensors, stats,
                         max_norm);
      break;
    case 1:
      hipLaunchKernelGGL(grad_scale_kernel<__half>, grid, dim3(GTHREADS), 0, stream,
                         ptrs, numels, block_prefix, n_tensors, stats, max_norm);
      break;
    default:
      hipLaunchKernelGGL(grad_scale_kernel<float>, grid, dim3(GTHREADS), 0, stream,
                         ptrs, numels, block_prefix, n_tensors, stats, max_norm);
      break;
  }
}

}  // namespace torchft_amd
