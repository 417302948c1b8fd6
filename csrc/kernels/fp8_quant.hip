// Fused OCP-fp8(e4m3) block quantize / dequantize / reduce kernels for the
// quantized gradient collectives — CDNA4 (gfx950) native.
//
// Capability parity with the reference Triton trio
// (torchft/quantization.py:53-428) re-designed for MI355X:
//  * fixed 2048-element blocks (wave-64-friendly; uniform grid) instead of
//    per-row striping — one fp32 scale per block, payload stays 4B-aligned
//  * per-tensor block padding so a block never straddles tensors: the
//    block→tensor lookup is a wave-uniform scalar binary search
//  * bf16/fp16/fp32 inputs load 16 B/lane (vectorized); fp8 conversion uses
//    the native OCP e4m3 type (gfx950 v_cvt path) — NOT MI300X fnuz
//  * accumulation in the reduce kernel runs in fp32 in fixed rank order
//    0..W-1 so every rank computes bitwise-identical reductions
//
// Packed wire layout (what goes over RCCL alltoall/allgather, all-7-xGMI
// friendly): W equal slices, slice r = [fp32 dequant-scales of its blocks]
// ‖ [2048 fp8 bytes per block]. slice_bytes = B_pr*(4+2048).

#include <hip/hip_fp8.h>
#include <hip/hip_runtime.h>

#include "multi_tensor.h"

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

// ---- quantize --------------------------------------------------------------

// These two kernels move only 6 KB per workgroup, so their time is set by the
// chain of dependent scalar loads in front of the data access. They take the
// table as the plain pointers of its columns and test the range only: the
// shared block cursor (MtCursor, multi_tensor.h) costs them 3-4 % on an
// 8 B-parameter zoo, with or without its alignment term. Their bindings
// reject a tensor off a 16 B boundary instead.

// Grid: one workgroup per (padded) block. Blocks >= total_blocks write
// scale=0 + zero payload (padding slots).
template <typename T>
__global__ void quantize_fp8_kernel(
    const int64_t* __restrict__ tensor_ptrs,   // [n] device addresses
    const int64_t* __restrict__ block_prefix,  // [n+1]
    const int64_t* __restrict__ numels,        // [n]
    int n_tensors, int64_t total_blocks, int64_t blocks_per_rank,
    int64_t slice_bytes, uint8_t* __restrict__ pack) {
  const int64_t b = blockIdx.x;
  // destination inside the packed wire buffer
  const int64_t r = b / blocks_per_rank;
  const int64_t bl = b % blocks_per_rank;
  uint8_t* slice = pack + r * slice_bytes;
  float* scale_out = reinterpret_cast<float*>(slice) + bl;
  uint8_t* payload = slice + blocks_per_rank * 4 + bl * kMtBlock;

  float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool valid = b < total_blocks;
  int64_t offset_in_t = 0;
  const T* src = nullptr;
  int64_t numel = 0;
  if (valid) {
    const int t = find_tensor(block_prefix, n_tensors, b);
    offset_in_t = (b - block_prefix[t]) * kMtBlock + threadIdx.x * kMtEpt;
    src = reinterpret_cast<const T*>(tensor_ptrs[t]);
    numel = numels[t];
    if (offset_in_t + kMtEpt <= numel) {
      load8(src + offset_in_t, v);
    } else {
#pragma unroll
      for (int i = 0; i < kMtEpt; i++) {
        v[i] = (offset_in_t + i < numel) ? to_f32(src[offset_in_t + i]) : 0.0f;
      }
    }
  }

  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < kMtEpt; i++) amax = fmaxf(amax, fabsf(v[i]));
  amax = block_reduce_max(amax);

  float q_scale, dq_scale;
  block_scales(amax, 1.f, q_scale, dq_scale);

  uint8_t q[8];
#pragma unroll
  for (int i = 0; i < kMtEpt; i++) {
    fp8_t f8(v[i] * q_scale);
    q[i] = *reinterpret_cast<uint8_t*>(&f8);
  }
  *reinterpret_cast<uint2*>(payload + threadIdx.x * kMtEpt) =
      *reinterpret_cast<uint2*>(q);
  if (threadIdx.x == 0) *scale_out = dq_scale;
}

// ---- dequantize back into the tensors --------------------------------------

template <typename T>
__global__ void dequantize_fp8_kernel(
    const int64_t* __restrict__ tensor_ptrs,
    const int64_t* __restrict__ block_prefix,
    const int64_t* __restrict__ numels,
    int n_tensors, int64_t total_blocks, int64_t blocks_per_rank,
    int64_t slice_bytes, const uint8_t* __restrict__ pack) {
  const int64_t b = blockIdx.x;
  if (b >= total_blocks) return;  // padding slots map to no tensor
  const int64_t r = b / blocks_per_rank;
  const int64_t bl = b % blocks_per_rank;
  const uint8_t* slice = pack + r * slice_bytes;
  const float dq_scale = reinterpret_cast<const float*>(slice)[bl];
  const uint8_t* payload = slice + blocks_per_rank * 4 + bl * kMtBlock;

  const int t = find_tensor(block_prefix, n_tensors, b);
  const int64_t offset_in_t =
      (b - block_prefix[t]) * kMtBlock + threadIdx.x * kMtEpt;
  T* dst = reinterpret_cast<T*>(tensor_ptrs[t]);
  const int64_t numel = numels[t];

  uint8_t q[8];
  *reinterpret_cast<uint2*>(q) =
      *reinterpret_cast<const uint2*>(payload + threadIdx.x * kMtEpt);
  float v[8];
#pragma unroll
  for (int i = 0; i < kMtEpt; i++) {
    fp8_t f8 = *reinterpret_cast<fp8_t*>(&q[i]);
    v[i] = (float)f8 * dq_scale;
  }
  if (offset_in_t + kMtEpt <= numel) {
    store8(dst + offset_in_t, v);
  } else {
    for (int i = 0; i < kMtEpt; i++) {
      if (offset_in_t + i < numel) from_f32(&dst[offset_in_t + i], v[i]);
    }
  }
}

// ---- reduce W copies of this rank's slice ----------------------------------

// in: [world, slice_bytes] (every rank's quantized copy of OUR blocks),
// out: [slice_bytes] requantized sum (or avg). Accumulates fp32 in fixed
// rank order 0..W-1 → bitwise deterministic regardless of which rank runs it.
__global__ void reduce_fp8_slices_kernel(const uint8_t* __restrict__ in,
                                         uint8_t* __restrict__ out, int world,
                                         int64_t blocks_per_rank,
                                         int64_t slice_bytes, float inv_div) {
  const int64_t bl = blockIdx.x;  // local block index within the slice
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};

  for (int r = 0; r < world; r++) {
    const uint8_t* slice = in + (int64_t)r * slice_bytes;
    const float dq_scale = reinterpret_cast<const float*>(slice)[bl];
    const uint8_t* payload = slice + blocks_per_rank * 4 + bl * kMtBlock;
    uint8_t q[8];
    *reinterpret_cast<uint2*>(q) =
        *reinterpret_cast<const uint2*>(payload + threadIdx.x * kMtEpt);
#pragma unroll
    for (int i = 0; i < kMtEpt; i++) {
      fp8_t f8 = *reinterpret_cast<fp8_t*>(&q[i]);
      acc[i] += (float)f8 * dq_scale;
    }
  }

  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < kMtEpt; i++) amax = fmaxf(amax, fabsf(acc[i]));
  amax = block_reduce_max(amax);

  // inv_div folds AVG's 1/world into the stored dequant scale — the payload
  // bytes are identical for SUM and AVG.
  float q_scale, dq_scale;
  block_scales(amax, inv_div, q_scale, dq_scale);

  float* scale_out = reinterpret_cast<float*>(out) + bl;
  uint8_t* payload_out = out + blocks_per_rank * 4 + bl * kMtBlock;
  uint8_t q[8];
#pragma unroll
  for (int i = 0; i < kMtEpt; i++) {
    fp8_t f8(acc[i] * q_scale);
    q[i] = *reinterpret_cast<uint8_t*>(&f8);
  }
  *reinterpret_cast<uint2*>(payload_out + threadIdx.x * kMtEpt) =
      *reinterpret_cast<uint2*>(q);
  if (threadIdx.x == 0) *scale_out = dq_scale;
}

// ---- host-visible launchers (raw pointers; stream passed in) ---------------

void launch_quantize_dtype(int dtype_code, MultiTensorTable tb,
                           int64_t padded_blocks, int64_t blocks_per_rank,
                           int64_t slice_bytes, uint8_t* pack, hipStream_t stream) {
  if (padded_blocks <= 0) return;
  dispatch_dtype(dtype_code, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(quantize_fp8_kernel<T>, dim3((uint32_t)padded_blocks),
                       dim3(kMtThreads), 0, stream, tb.col(0), tb.prefix(), tb.numels(), tb.n,
                       tb.total_blocks, blocks_per_rank, slice_bytes, pack);
  });
}

void launch_dequantize_dtype(int dtype_code, MultiTensorTable tb,
                             int64_t padded_blocks, int64_t blocks_per_rank,
                             int64_t slice_bytes, const uint8_t* pack,
                             hipStream_t stream) {
  if (padded_blocks <= 0) return;
  dispatch_dtype(dtype_code, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(dequantize_fp8_kernel<T>, dim3((uint32_t)padded_blocks),
                       dim3(kMtThreads), 0, stream, tb.col(0), tb.prefix(), tb.numels(), tb.n,
                       tb.total_blocks, blocks_per_rank, slice_bytes, pack);
  });
}

void launch_reduce(const uint8_t* in, uint8_t* out, int world,
                   int64_t blocks_per_rank, int64_t slice_bytes, bool avg,
                   hipStream_t stream) {
  if (blocks_per_rank <= 0 || world <= 0) return;
  hipLaunchKernelGGL(reduce_fp8_slices_kernel, dim3((uint32_t)blocks_per_rank),
                     dim3(kMtThreads), 0, stream, in, out, world, blocks_per_rank,
                     slice_bytes, avg ? 1.0f / world : 1.0f);
}

}  // namespace torchft_amd
