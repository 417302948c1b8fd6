// Fused model ops for the Llama training path — CDNA4 (gfx950) native.
//
// These are the HBM-bound elementwise/normalization ops that must be fused
// into single kernels to hit MI355X's ~8 TB/s roofline (the unfused torch
// graphs re-read activations 2-4x): RMSNorm fwd/bwd, rotary embedding
// fwd/bwd, SwiGLU fwd/bwd. All loads/stores are 16 B/lane vectorized
// (bf16x8); reductions are fp32 with wave64 shuffles + LDS cross-wave.
//
// New scope vs the reference (torchft delegates model compute to the user
// stack); these back torchft_amd.models.llama for the flagship benchmark.

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "kernels.h"
#include "vec8.h"

namespace torchft_amd {

using bf16 = __hip_bfloat16;
using bf16x2 = __hip_bfloat162;

// ---------------------------------------------------------------- helpers

template <int THREADS>
__device__ inline float block_reduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  __shared__ float wsum[THREADS / 64];
  static_assert(THREADS != 256 || sizeof(wsum) == kRmsnormBwdStaticLdsBytes,
                "rmsnorm_bwd's H limit counts this array");
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (lane == 0) wsum[wave] = v;
  __syncthreads();
  float s = wsum[0];
#pragma unroll
  for (int w = 1; w < THREADS / 64; w++) s += wsum[w];
  __syncthreads();  // allow reuse of wsum next iteration
  return s;
}

// ---------------------------------------------------------------- RMSNorm

// One 256-thread workgroup per row; H must be a multiple of 8.
// y = x * rsqrt(mean(x^2)+eps) * w ; saves invrms (fp32) for backward.
template <int THREADS>
__global__ void rmsnorm_fwd_kernel(const bf16* __restrict__ x,
                                   const bf16* __restrict__ w,
                                   bf16* __restrict__ y,
                                   float* __restrict__ invrms, int64_t rows,
                                   int H, float eps) {
  const int64_t row = blockIdx.x;
  if (row >= rows) return;
  const bf16* xr = x + row * H;
  bf16* yr = y + row * H;

  float ss = 0.f;
  for (int base = threadIdx.x * 8; base < H; base += THREADS * 8) {
    float v[8];
    load8(xr + base, v);
#pragma unroll
    for (int i = 0; i < 8; i++) ss += v[i] * v[i];
  }
  ss = block_reduce_sum<THREADS>(ss);
  const float inv = rsqrtf(ss / H + eps);
  if (threadIdx.x == 0) invrms[row] = inv;

  for (int base = threadIdx.x * 8; base < H; base += THREADS * 8) {
    float v[8], g[8];
    load8(xr + base, v);
    load8(w + base, g);
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = v[i] * inv * g[i];
    store8(yr + base, v);
  }
}

// Grid-strided rows; per-block dw accumulated in LDS (fp32), one atomicAdd
// sweep per block at the end. dw_out must be fp32 zeros [H].
// dx = invrms * w * dy - (invrms^3 / H) * x * sum(dy*w*x)
// LDS: dw[H] (dynamic) + block_reduce_sum's static array.
template <int THREADS>
__global__ void rmsnorm_bwd_kernel(const bf16* __restrict__ dy,
                                   const bf16* __restrict__ x,
                                   const bf16* __restrict__ w,
                                   const float* __restrict__ invrms,
                                   bf16* __restrict__ dx,
                                   float* __restrict__ dw_out, int64_t rows,
                                   int H) {
  extern __shared__ float dw_lds[];  // [H] fp32
  for (int i = threadIdx.x; i < H; i += THREADS) dw_lds[i] = 0.f;
  __syncthreads();

  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const bf16* dyr = dy + row * H;
    const bf16* xr = x + row * H;
    bf16* dxr = dx + row * H;
    const float inv = invrms[row];

    float s = 0.f;
    for (int base = threadIdx.x * 8; base < H; base += THREADS * 8) {
      float d[8], v[8], g[8];
      load8(dyr + base, d);
      load8(xr + base, v);
      load8(w + base, g);
#pragma unroll
      for (int i = 0; i < 8; i++) s += d[i] * g[i] * v[i];
    }
    s = block_reduce_sum<THREADS>(s);
    // inv^3 leaves the fp32 normal range for rows of |x| ~ 2^42 and beyond;
    // those take inv * s first, which is of the order of H * dy * w at any
    // scale. Every other row keeps the order, and the bits, it always had.
    const float inv3 = inv * inv * inv;
    const float k = inv3 >= FLT_MIN ? inv3 * s / H : inv * s / H * inv * inv;

    for (int base = threadIdx.x * 8; base < H; base += THREADS * 8) {
      float d[8], v[8], g[8], o[8];
      load8(dyr + base, d);
      load8(xr + base, v);
      load8(w + base, g);
#pragma unroll
      for (int i = 0; i < 8; i++) {
        o[i] = inv * g[i] * d[i] - k * v[i];
        dw_lds[base + i] += d[i] * v[i] * inv;
      }
      store8(dxr + base, o);
    }
    __syncthreads();  // dw_lds writes settle before next row reuses reduce LDS
  }

  for (int i = threadIdx.x; i < H; i += THREADS) {
    atomicAdd(&dw_out[i], dw_lds[i]);
  }
}

// ---------------------------------------------------------------- RoPE

// x: [B*S*Hh, D] rows conceptually; rotate-half pairing (i, i+D/2).
// cos/sin: [S, D/2] fp32. Thread handles 4 pairs.
// sign=+1 forward, -1 backward (rotation transpose).
__global__ void rope_kernel(const bf16* __restrict__ x, bf16* __restrict__ out,
                            const float* __restrict__ cos_tab,
                            const float* __restrict__ sin_tab, int64_t total_pairs,
                            int S, int Hh, int D, float sign) {
  const int64_t idx4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (idx4 >= total_pairs) return;
  const int halfD = D / 2;
  // flat pair index -> (b, s, h, i); pairs contiguous in i
  const int64_t i = idx4 % halfD;
  const int64_t rest = idx4 / halfD;  // b*S*Hh + s*Hh + h
  const int64_t h = rest % Hh;
  const int64_t s = (rest / Hh) % S;

  const int64_t base = rest * (int64_t)D + i;  // x1 at base, x2 at base+halfD
  const float* c = cos_tab + s * halfD + i;
  const float* sn = sin_tab + s * halfD + i;

  // 4 pairs; i+3 < halfD guaranteed when halfD % 4 == 0 (D % 8 == 0)
  float x1[4], x2[4], o1[4], o2[4];
  ushort4 raw1 = *reinterpret_cast<const ushort4*>(x + base);
  ushort4 raw2 = *reinterpret_cast<const ushort4*>(x + base + halfD);
  const bf16x2* h1 = reinterpret_cast<const bf16x2*>(&raw1);
  const bf16x2* h2 = reinterpret_cast<const bf16x2*>(&raw2);
#pragma unroll
  for (int k = 0; k < 2; k++) {
    float2 f1 = __bfloat1622float2(h1[k]);
    float2 f2 = __bfloat1622float2(h2[k]);
    x1[2 * k] = f1.x; x1[2 * k + 1] = f1.y;
    x2[2 * k] = f2.x; x2[2 * k + 1] = f2.y;
  }
  const float4 cv = *reinterpret_cast<const float4*>(c);
  const float4 sv = *reinterpret_cast<const float4*>(sn);
  const float cc[4] = {cv.x, cv.y, cv.z, cv.w};
  const float ssn[4] = {sv.x * sign, sv.y * sign, sv.z * sign, sv.w * sign};
#pragma unroll
  for (int k = 0; k < 4; k++) {
    o1[k] = x1[k] * cc[k] - x2[k] * ssn[k];
    o2[k] = x2[k] * cc[k] + x1[k] * ssn[k];
  }
  ushort4 r1, r2;
  bf16x2* p1 = reinterpret_cast<bf16x2*>(&r1);
  bf16x2* p2 = reinterpret_cast<bf16x2*>(&r2);
#pragma unroll
  for (int k = 0; k < 2; k++) {
    p1[k] = __float22bfloat162_rn(make_float2(o1[2 * k], o1[2 * k + 1]));
    p2[k] = __float22bfloat162_rn(make_float2(o2[2 * k], o2[2 * k + 1]));
  }
  *reinterpret_cast<ushort4*>(out + base) = r1;
  *reinterpret_cast<ushort4*>(out + base + halfD) = r2;
}

// ---------------------------------------------------------------- SwiGLU

// The element math, once for the plain and the packed kernels.
// o = silu(a) * b
__device__ inline void swiglu_fwd8(const float (&a)[8], const float (&b)[8],
                                   float (&o)[8]) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const float sig = 1.f / (1.f + __expf(-a[i]));
    o[i] = a[i] * sig * b[i];
  }
}

// da = dy * b * sig(a) * (1 + a*(1-sig(a))) ; db = dy * a * sig(a). One
// element: the kernels unroll it themselves (docs/KERNELS.md has why).
__device__ inline void swiglu_bwd1(float dy, float a, float b, float& da, float& db) {
  const float sig = 1.f / (1.f + __expf(-a));
  const float silu = a * sig;
  da = dy * b * sig * (1.f + a * (1.f - sig));
  db = dy * silu;
}

// out = silu(a) * b ; elementwise, bf16x8.
__global__ void swiglu_fwd_kernel(const bf16* __restrict__ a,
                                  const bf16* __restrict__ b,
                                  bf16* __restrict__ out, int64_t n) {
  const int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (base >= n) return;
  float va[8], vb[8], vo[8];
  load8(a + base, va);
  load8(b + base, vb);
  swiglu_fwd8(va, vb, vo);
  store8(out + base, vo);
}

__global__ void swiglu_bwd_kernel(const bf16* __restrict__ dy,
                                  const bf16* __restrict__ a,
                                  const bf16* __restrict__ b,
                                  bf16* __restrict__ da, bf16* __restrict__ db,
                                  int64_t n) {
  const int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (base >= n) return;
  float vdy[8], va[8], vb[8], vda[8], vdb[8];
  load8(dy + base, vdy);
  load8(a + base, va);
  load8(b + base, vb);
#pragma unroll
  for (int i = 0; i < 8; i++) swiglu_bwd1(vdy[i], va[i], vb[i], vda[i], vdb[i]);
  store8(da + base, vda);
  store8(db + base, vdb);
}

// Packed-GLU variants: gu = [rows][2f] with gate = gu[:, :f], up = gu[:, f:]
// (the fused w13 projection's natural layout — no contiguous() copies).
// out = silu(gate) * up, [rows][f].
__global__ void swiglu_glu_fwd_kernel(const bf16* __restrict__ gu,
                                      bf16* __restrict__ out, int64_t rows,
                                      int64_t f) {
  const int64_t idx = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (idx >= rows * f) return;
  const int64_t r = idx / f;
  const int64_t c = idx % f;
  float va[8], vb[8], vo[8];
  load8(gu + r * 2 * f + c, va);
  load8(gu + r * 2 * f + f + c, vb);
  swiglu_fwd8(va, vb, vo);
  store8(out + idx, vo);
}

// dgu (packed): dgate into gu's gate half, dup into its up half
__global__ void swiglu_glu_bwd_kernel(const bf16* __restrict__ dy,
                                      const bf16* __restrict__ gu,
                                      bf16* __restrict__ dgu, int64_t rows,
                                      int64_t f) {
  const int64_t idx = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (idx >= rows * f) return;
  const int64_t r = idx / f;
  const int64_t c = idx % f;
  float vdy[8], va[8], vb[8], vda[8], vdb[8];
  load8(dy + idx, vdy);
  load8(gu + r * 2 * f + c, va);
  load8(gu + r * 2 * f + f + c, vb);
#pragma unroll
  for (int i = 0; i < 8; i++) swiglu_bwd1(vdy[i], va[i], vb[i], vda[i], vdb[i]);
  store8(dgu + r * 2 * f + c, vda);
  store8(dgu + r * 2 * f + f + c, vdb);
}

// ---------------------------------------------------------------- launchers

void launch_rmsnorm_fwd(const void* x, const void* w, void* y, float* invrms,
                        int64_t rows, int H, float eps, hipStream_t stream) {
  if (rows == 0) return;
  hipLaunchKernelGGL((rmsnorm_fwd_kernel<256>), dim3((uint32_t)rows), dim3(256), 0,
                     stream, (const bf16*)x, (const bf16*)w, (bf16*)y, invrms,
                     rows, H, eps);
}

int launch_rmsnorm_bwd(const void* dy, const void* x, const void* w,
                       const float* invrms, void* dx, float* dw, int64_t rows,
                       int H, hipStream_t stream) {
  if (rows == 0) return 0;
  // grid: enough blocks to fill 256 CUs x ~4, capped so atomics stay cheap
  int grid = (int)(rows < 2048 ? rows : 2048);
  // + kRmsnormBwdStaticLdsBytes <= kRmsnormBwdMaxLdsBytes
  size_t lds = (size_t)H * sizeof(float);
  (void)hipGetLastError();  // an earlier call's error is not this launch's
  hipLaunchKernelGGL((rmsnorm_bwd_kernel<256>), dim3(grid), dim3(256), lds, stream,
                     (const bf16*)dy, (const bf16*)x, (const bf16*)w, invrms,
                     (bf16*)dx, dw, rows, H);
  return (int)hipGetLastError();
}

// One lane per `per_lane` items, elementwise_grid workgroups of kElemThreads;
// nothing to do, no launch.
template <typename... P, typename... A>
static void launch_elementwise(void (*kernel)(P...), int64_t items, int per_lane,
                               hipStream_t stream, A... args) {
  const int64_t grid = elementwise_grid(items, per_lane);
  if (grid == 0) return;
  hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(kElemThreads), 0, stream,
                     args...);
}

void launch_rope(const void* x, void* out, const float* cos_tab,
                 const float* sin_tab, int64_t total_pairs, int S, int Hh, int D,
                 bool backward, hipStream_t stream) {
  launch_elementwise(rope_kernel, total_pairs, 4, stream, (const bf16*)x, (bf16*)out,
                     cos_tab, sin_tab, total_pairs, S, Hh, D, backward ? -1.0f : 1.0f);
}

void launch_swiglu_fwd(const void* a, const void* b, void* out, int64_t n,
                       hipStream_t stream) {
  launch_elementwise(swiglu_fwd_kernel, n, 8, stream, (const bf16*)a, (const bf16*)b,
                     (bf16*)out, n);
}

void launch_swiglu_bwd(const void* dy, const void* a, const void* b, void* da,
                       void* db, int64_t n, hipStream_t stream) {
  launch_elementwise(swiglu_bwd_kernel, n, 8, stream, (const bf16*)dy, (const bf16*)a,
                     (const bf16*)b, (bf16*)da, (bf16*)db, n);
}

void launch_swiglu_glu_fwd(const void* gu, void* out, int64_t rows, int64_t f,
                           hipStream_t stream) {
  launch_elementwise(swiglu_glu_fwd_kernel, rows * f, 8, stream, (const bf16*)gu,
                     (bf16*)out, rows, f);
}

void launch_swiglu_glu_bwd(const void* dy, const void* gu, void* dgu,
                           int64_t rows, int64_t f, hipStream_t stream) {
  launch_elementwise(swiglu_glu_bwd_kernel, rows * f, 8, stream, (const bf16*)dy,
                     (const bf16*)gu, (bf16*)dgu, rows, f);
}

}  // namespace torchft_amd
