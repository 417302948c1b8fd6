// Block math of the fp8 wire pack, shared by fp8_quant.hip and the pack
// kernels of diloco_sync.hip: the workgroup maximum and the two block scales.
// Device code only; a .hip file includes <hip/hip_runtime.h> itself first.
#pragma once

#include <hip/hip_fp8.h>
#include <hip/hip_runtime.h>

#include "kernels.h"

#define FP8_MAX 448.0f

namespace torchft_amd {

using fp8_t = __hip_fp8_e4m3;  // OCP e4m3fn (gfx950); NOT the MI300X fnuz type

// ---- block reduce (max) across the 4 waves of a 256-thread workgroup ------

__device__ inline float block_reduce_max(float v) {
  // wave64 reduce
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    v = fmaxf(v, __shfl_down(v, off, 64));
  }
  __shared__ float warp_max[kMtThreads / 64];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  if (lane == 0) warp_max[wave] = v;
  __syncthreads();
  float m = warp_max[0];
#pragma unroll
  for (int w = 1; w < kMtThreads / 64; w++) m = fmaxf(m, warp_max[w]);
  return m;  // every thread gets the block max
}

// ---- block scales ----------------------------------------------------------

// q = 448/amax maps the block onto the e4m3 range, dq = amax/448 is what goes
// on the wire. A block of zeros gets 0 / 0. So does a block whose amax is
// below 448/FLT_MAX (1.3e-36, every fp32 subnormal included): 448/amax
// overflows to +inf there, and inf times the block's values would be inf or,
// for its zeros, NaN, so finite input would leave the wire as NaN. Such a
// block is flushed to zero instead. amax = +inf (an Inf element) keeps q = 0,
// dq = inf: the block decodes to NaN everywhere. A NaN element never enters
// amax (fmaxf returns the other operand) and stays NaN through NaN * q.
__device__ inline void block_scales(float amax, float inv_div, float& q_scale,
                                    float& dq_scale) {
  q_scale = amax > 0.f ? (FP8_MAX / amax) : 0.f;
  dq_scale = amax > 0.f ? (amax / FP8_MAX) * inv_div : 0.f;
  if (isinf(q_scale)) q_scale = dq_scale = 0.f;
}

}  // namespace torchft_amd
