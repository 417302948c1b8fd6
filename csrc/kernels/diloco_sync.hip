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

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdint>

namespace torchft_amd {

#define DBLOCK 2048
#define DTHREADS 256
#define DEPT 8  // elements per thread per logical block

namespace {

__device__ inline float d_to_f32(__hip_bfloat16 v) { return __bfloat162float(v); }
__device__ inline float d_to_f32(__half v) { return __half2float(v); }
__device__ inline float d_to_f32(float v) { return v; }
__device__ inline void d_from_f32(__hip_bfloat16* d, float v) { *d = __float2bfloat16(v); }
__device__ inline void d_from_f32(__half* d, float v) { *d = __float2half(v); }
__device__ inline void d_from_f32(float* d, float v) { *d = v; }

// fp32 value of v after the round trip through T (what a store of v holds)
__device__ inline float d_round(__hip_bfloat16*, float v) {
  return __bfloat162float(__float2bfloat16(v));
}
__device__ inline float d_round(__half*, float v) { return __half2float(__float2half(v)); }
__device__ inline float d_round(float*, float v) { return v; }

// same 8-element accessors as grad_norm.hip
__device__ inline void d_load8(const __hip_bfloat16* p, float (&v)[DEPT]) {
  const uint4 raw = *reinterpret_cast<const uint4*>(p);
  const __hip_bfloat162* h = reinterpret_cast<const __hip_bfloat162*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float2 f = __bfloat1622float2(h[i]);
    v[2 * i] = f.x;
    v[2 * i + 1] = f.y;
  }
}
__device__ inline void d_load8(const __half* p, float (&v)[DEPT]) {
  const uint4 raw = *reinterpret_cast<const uint4*>(p);
  const __half2* h = reinterpret_cast<const __half2*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float2 f = __half22float2(h[i]);
    v[2 * i] = f.x;
    v[2 * i + 1] = f.y;
  }
}
__device__ inline void d_load8(const float* p, float (&v)[DEPT]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ inline void d_store8(__hip_bfloat16* p, const float (&v)[DEPT]) {
  uint4 raw;
  __hip_bfloat162* h = reinterpret_cast<__hip_bfloat162*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++)
    h[i] = __float22bfloat162_rn(make_float2(v[2 * i], v[2 * i + 1]));
  *reinterpret_cast<uint4*>(p) = raw;
}
__device__ inline void d_store8(__half* p, const float (&v)[DEPT]) {
  uint4 raw;
  __half2* h = reinterpret_cast<__half2*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++)
    h[i] = __float22half2_rn(make_float2(v[2 * i], v[2 * i + 1]));
  *reinterpret_cast<uint4*>(p) = raw;
}
__device__ inline void d_store8(float* p, const float (&v)[DEPT]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// same search as find_tensor_a in fused_adamw.hip
__device__ inline int find_tensor_d(const int64_t* block_prefix, int n, int64_t b) {
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

// out[i] = T(float(a[i]) - float(b[i])): one rounding, torch's `a - b`.
template <typename T>
__global__ void __launch_bounds__(DTHREADS)
pseudograd_kernel(const int64_t* __restrict__ out_ptrs,
                  const int64_t* __restrict__ a_ptrs,
                  const int64_t* __restrict__ b_ptrs,
                  const int64_t* __restrict__ numels,
                  const int64_t* __restrict__ block_prefix, int n_tensors) {
  const int64_t blk = blockIdx.x;
  const int t = find_tensor_d(block_prefix, n_tensors, blk);
  const int64_t off = (blk - block_prefix[t]) * DBLOCK + threadIdx.x * DEPT;
  const int64_t numel = numels[t];
  if (off >= numel) return;
  const int64_t po = out_ptrs[t], pa = a_ptrs[t], pb = b_ptrs[t];
  T* out = reinterpret_cast<T*>(po) + off;
  const T* a = reinterpret_cast<const T*>(pa) + off;
  const T* b = reinterpret_cast<const T*>(pb) + off;
  if (((po | pa | pb) & 15) == 0 && off + DEPT <= numel) {
    float av[DEPT], bv[DEPT];
    d_load8(a, av);
    d_load8(b, bv);
#pragma unroll
    for (int i = 0; i < DEPT; i++) av[i] -= bv[i];
    d_store8(out, av);
  } else {
    const int cnt = numel - off < DEPT ? (int)(numel - off) : DEPT;
    for (int i = 0; i < cnt; i++) d_from_f32(out + i, d_to_f32(a[i]) - d_to_f32(b[i]));
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
__global__ void __launch_bounds__(DTHREADS)
outer_sgd_kernel(const int64_t* __restrict__ g_ptrs, const int64_t* __restrict__ l_ptrs,
                 const int64_t* __restrict__ d_ptrs, const int64_t* __restrict__ m_ptrs,
                 const int64_t* __restrict__ numels,
                 const int64_t* __restrict__ block_prefix, int n_tensors, float lr,
                 float mu, int nesterov, float alpha) {
  const int64_t blk = blockIdx.x;
  const int t = find_tensor_d(block_prefix, n_tensors, blk);
  const int64_t off = (blk - block_prefix[t]) * DBLOCK + threadIdx.x * DEPT;
  const int64_t numel = numels[t];
  if (off >= numel) return;
  const int64_t pg = g_ptrs[t], pl = l_ptrs[t], pd = d_ptrs[t];
  int64_t pm = 0;
  if constexpr (HAS_MOMENTUM) pm = m_ptrs[t];
  T* g = reinterpret_cast<T*>(pg) + off;
  T* l = reinterpret_cast<T*>(pl) + off;
  const T* d = reinterpret_cast<const T*>(pd) + off;
  T* m = nullptr;
  if constexpr (HAS_MOMENTUM) m = reinterpret_cast<T*>(pm) + off;
  const bool nes = nesterov != 0;

  if (((pg | pl | pd | pm) & 15) == 0 && off + DEPT <= numel) {
    float gv[DEPT], lv[DEPT], dv[DEPT], mv[DEPT] = {};
    d_load8(g, gv);
    d_load8(l, lv);
    d_load8(d, dv);
    if constexpr (HAS_MOMENTUM) d_load8(m, mv);
#pragma unroll
    for (int i = 0; i < DEPT; i++)
      outer_sgd_elem<T, HAS_MOMENTUM>(gv[i], dv[i], mv[i], lv[i], lr, mu, nes, alpha);
    if constexpr (HAS_MOMENTUM) d_store8(m, mv);
    d_store8(g, gv);
    d_store8(l, lv);
  } else {
    const int cnt = numel - off < DEPT ? (int)(numel - off) : DEPT;
    for (int i = 0; i < cnt; i++) {
      float gf = d_to_f32(g[i]), lf = d_to_f32(l[i]), mf = 0.f;
      const float df = d_to_f32(d[i]);
      if constexpr (HAS_MOMENTUM) mf = d_to_f32(m[i]);
      outer_sgd_elem<T, HAS_MOMENTUM>(gf, df, mf, lf, lr, mu, nes, alpha);
      if constexpr (HAS_MOMENTUM) d_from_f32(m + i, mf);
      d_from_f32(g + i, gf);
      d_from_f32(l + i, lf);
    }
  }
}

// dtype_code: 0 = bf16, 1 = fp16, 2 = fp32 (matches kernels.h)
void launch_pseudograd(int dtype_code, const int64_t* out_ptrs, const int64_t* a_ptrs,
                       const int64_t* b_ptrs, const int64_t* numels,
                       const int64_t* block_prefix, int n_tensors,
                       int64_t total_blocks, hipStream_t stream) {
  if (total_blocks <= 0) return;
  const dim3 grid((uint32_t)total_blocks);
  switch (dtype_code) {
    case 0:
      hipLaunchKernelGGL(pseudograd_kernel<__hip_bfloat16>, grid, dim3(DTHREADS), 0,
                         stream, out_ptrs, a_ptrs, b_ptrs, numels, block_prefix,
                         n_tensors);
      break;
    case 1:
      hipLaunchKernelGGL(pseudograd_kernel<__half>, grid, dim3(DTHREADS), 0, stream,
                         out_ptrs, a_ptrs, b_ptrs, numels, block_prefix, n_tensors);
      break;
    default:
      hipLaunchKernelGGL(pseudograd_kernel<float>, grid, dim3(DTHREADS), 0, stream,
                         out_ptrs, a_ptrs, b_ptrs, numels, block_prefix, n_tensors);
      break;
  }
}

namespace {

template <typename T>
void launch_outer_sgd_t(bool has_momentum, dim3 grid, hipStream_t stream,
                        const int64_t* g_ptrs, const int64_t* l_ptrs,
                        const int64_t* d_ptrs, const int64_t* m_ptrs,
                        const int64_t* numels, const int64_t* block_prefix,
                        int n_tensors, float lr, float mu, int nesterov, float alpha) {
  if (has_momentum)
    hipLaunchKernelGGL((outer_sgd_kernel<T, true>), grid, dim3(DTHREADS), 0, stream,
                       g_ptrs, l_ptrs, d_ptrs, m_ptrs, numels, block_prefix, n_tensors,
                       lr, mu, nesterov, alpha);
  else
    hipLaunchKernelGGL((outer_sgd_kernel<T, false>), grid, dim3(DTHREADS), 0, stream,
                       g_ptrs, l_ptrs, d_ptrs, m_ptrs, numels, block_prefix, n_tensors,
                       lr, mu, nesterov, alpha);
}

}  // namespace

void launch_outer_sgd(int dtype_code, bool has_momentum, const int64_t* g_ptrs,
                      const int64_t* l_ptrs, const int64_t* d_ptrs,
                      const int64_t* m_ptrs, const int64_t* numels,
                      const int64_t* block_prefix, int n_tensors,
                      int64_t total_blocks, float lr, float mu, bool nesterov,
                      float alpha, hipStream_t stream) {
  if (total_blocks <= 0) return;
  const dim3 grid((uint32_t)total_blocks);
  const int nes = nesterov ? 1 : 0;
  switch (dtype_code) {
    case 0:
      launch_outer_sgd_t<__hip_bfloat16>(has_momentum, grid, stream, g_ptrs, l_ptrs,
                                         d_ptrs, m_ptrs, numels, block_prefix,
                                         n_tensors, lr, mu, nes, alpha);
      break;
    case 1:
      launch_outer_sgd_t<__half>(has_momentum, grid, stream, g_ptrs, l_ptrs, d_ptrs,
                                 m_ptrs, numels, block_prefix, n_tensors, lr, mu, nes,
                                 alpha);
      break;
    default:
      launch_outer_sgd_t<float>(has_momentum, grid, stream, g_ptrs, l_ptrs, d_ptrs,
                                m_ptrs, numels, block_prefix, n_tensors, lr, mu, nes,
                                alpha);
      break;
  }
}

}  // namespace torchft_amd
