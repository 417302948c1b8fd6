// The 8-element accessors every elementwise kernel shares (docs/KERNELS.md,
// "Shared conventions"): scalar conversions between a storage type and fp32,
// and load8 / store8, which move 8 elements per lane as fp32 values. Device
// code only; a .hip file includes <hip/hip_runtime.h> itself before this.
#pragma once

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
// address must be 16 B-aligned.
__device__ inline void load8(const __hip_bfloat16* p, float (&v)[8]) {
  const uint4 raw = *reinterpret_cast<const uint4*>(p);
  const __hip_bfloat162* h = reinterpret_cast<const __hip_bfloat162*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float2 f = __bfloat1622float2(h[i]);
    v[2 * i] = f.x;
    v[2 * i + 1] = f.y;
  }
}
__device__ inline void load8(const __half* p, float (&v)[8]) {
  const uint4 raw = *reinterpret_cast<const uint4*>(p);
  const __half2* h = reinterpret_cast<const __half2*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const float2 f = __half22float2(h[i]);
    v[2 * i] = f.x;
    v[2 * i + 1] = f.y;
  }
}
__device__ inline void load8(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ inline void store8(__hip_bfloat16* p, const float (&v)[8]) {
  uint4 raw;
  __hip_bfloat162* h = reinterpret_cast<__hip_bfloat162*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++)
    h[i] = __float22bfloat162_rn(make_float2(v[2 * i], v[2 * i + 1]));
  *reinterpret_cast<uint4*>(p) = raw;
}
__device__ inline void store8(__half* p, const float (&v)[8]) {
  uint4 raw;
  __half2* h = reinterpret_cast<__half2*>(&raw);
#pragma unroll
  for (int i = 0; i < 4; i++)
    h[i] = __float22half2_rn(make_float2(v[2 * i], v[2 * i + 1]));
  *reinterpret_cast<uint4*>(p) = raw;
}
__device__ inline void store8(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

}  // namespace torchft_amd
