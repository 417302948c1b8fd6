// MXFP4 block quantize / dequantize / reduce kernels for the quantized
// gradient collectives: the 4.25-bit wire pack, CDNA4 (gfx950) native.
//
// Format (docs/KERNELS.md, "mxfp4_quant.hip"). The pack keeps the block
// structure of the fp8 pack (fp8_quant.hip): 2048-element blocks, per-tensor
// block padding, W equal slices. Inside a block, 64 groups of 32 consecutive
// elements share one e8m0 scale byte (2^X, stored as X + 127) and every
// element is one e2m1 code (sign, {0, .5, 1, 1.5, 2, 3, 4, 6}), two to a
// byte, the even element in the low nibble. Slice r = [64 scale bytes per
// block] ‖ [1024 code bytes per block], block-major in both parts:
// slice_bytes = B_pr * 1088. The rules for X and for the codes are
// mxfp4_group.h's; every product with 2^X or 2^-X is exact, so the reduce
// gives every rank the same bits whatever the compiler contracts.
//
// Work split: ONE WAVE PER BLOCK, four blocks to a 256-lane workgroup.
// A lane holds 8 elements (one load8), so a group is 4 adjacent lanes and a
// wave covers 512 elements, 16 groups, per step; a block is 4 steps, written
// out unrolled so a lane has its four 16 B loads in flight at once. Nothing in
// this format needs the workgroup: the group maximum is two cross-lane steps
// (xor 1 and 2) inside the wave, so there is no LDS and no barrier, and the
// waves of a workgroup never wait for each other. The fp8 kernels, one
// workgroup per block, pay one chain of dependent scalar loads (the table
// search, the tensor's address and size) per wave for ONE 16 B load per lane;
// here the same chain stands in front of four. Several blocks per workgroup
// with a workgroup-wide loop was the alternative: it amortises the chain the
// same way but keeps four waves in lockstep for no gain, since no data is
// shared between them. The wave's block index goes through readfirstlane, so
// the table search stays on the scalar unit.
//
// Stores: a lane's 8 codes are one dword, 64 lanes store 256 contiguous bytes
// per step. The 64 scale bytes of a block are gathered across lanes (four
// shuffles per block) into 16 dwords, stored by lanes 0..15 as one 64 B run.
// All global writes are ordinary vector stores.

#include <hip/hip_runtime.h>

#include "multi_tensor.h"
#include "mxfp4_group.h"

namespace torchft_amd {

namespace {

constexpr int kWave = 64;
constexpr int kMxBlocksPerWg = kMtThreads / kWave;        // 4 waves, one block each
constexpr int kMxSteps = kMtBlock / (kWave * kMtEpt);     // 4 steps of 512 elements
constexpr int kMxStepCodeBytes = kWave * kMtEpt / 2;      // 256
constexpr int kMxStepGroups = kWave * kMtEpt / kMxGroup;  // 16
static_assert(kMxSteps == 4, "a lane's scale bytes of one block fill one dword");
static_assert(kMxGroup == 4 * kMtEpt, "a group is 4 adjacent lanes");

// the block this wave works on, wave-uniform (an SGPR)
__device__ inline int64_t wave_block() {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
  return (int64_t)blockIdx.x * kMxBlocksPerWg + wave;
}

// Where block b of a pack lives: scale bytes and code bytes
struct MxSlot {
  int64_t scales, codes;  // byte offsets into the pack
  __device__ MxSlot(int64_t b, int64_t blocks_per_rank) {
    const int64_t r = b / blocks_per_rank, bl = b % blocks_per_rank;
    const int64_t slice = r * blocks_per_rank * kMxBlockBytes;
    scales = slice + bl * kMxGroupsPerBlock;
    codes = slice + blocks_per_rank * kMxGroupsPerBlock + bl * kMxCodeBytesPerBlock;
  }
};

// Encode one block held as v[step][8] per lane: its 1024 code bytes to
// `codes`, its 64 scale bytes to `scales` (both 4 B-aligned).
__device__ inline void encode_block(const float (&v)[kMxSteps][kMtEpt],
                                    uint8_t* __restrict__ scales,
                                    uint8_t* __restrict__ codes) {
  const int lane = threadIdx.x % kWave;
  uint32_t my_scales = 0;  // byte j: the scale of this lane's group in step j
#pragma unroll
  for (int j = 0; j < kMxSteps; j++) {
    uint32_t amax = 0;
#pragma unroll
    for (int i = 0; i < kMtEpt; i++) amax = max(amax, mx_bits(v[j][i]) & 0x7FFFFFFFu);
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1, kWave));
    amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2, kWave));
    const uint32_t sb = mx_scale_byte(amax);
    my_scales |= sb << (8 * j);
    uint32_t word = 0;
    if (sb != kMxNanScale) {
      const float inv = mx_inv_scale(sb);
#pragma unroll
      for (int i = 0; i < kMtEpt; i++) word |= mx_code(v[j][i], inv) << (4 * i);
    }
    *reinterpret_cast<uint32_t*>(codes + j * kMxStepCodeBytes + lane * 4) = word;
  }
  // Scale byte g of the block belongs to step g / 16, lanes 4 * (g % 16) ...
  // + 3. Lane k < 16 assembles bytes 4k .. 4k + 3: step k / 4, taken from
  // lanes 16 * (k % 4) + 4 * i, i = 0 .. 3.
  const int k = lane % kMxStepGroups;
  uint32_t word = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t theirs = (uint32_t)__shfl((int)my_scales, 16 * (k % 4) + 4 * i, kWave);
    word |= ((theirs >> (8 * (k / 4))) & 0xFFu) << (8 * i);
  }
  if (lane < kMxStepGroups) *reinterpret_cast<uint32_t*>(scales + lane * 4) = word;
}

// This lane's 8 decoded values of step j of a block
__device__ inline void decode_step(const uint8_t* __restrict__ scales,
                                   const uint8_t* __restrict__ codes, int j,
                                   float (&v)[kMtEpt]) {
  const int lane = threadIdx.x % kWave;
  const float scale = mx_scale(scales[j * kMxStepGroups + lane / 4]);
  const uint32_t word =
      *reinterpret_cast<const uint32_t*>(codes + j * kMxStepCodeBytes + lane * 4);
#pragma unroll
  for (int i = 0; i < kMtEpt; i++) v[i] = mx_code_value(word >> (4 * i)) * scale;
}

}  // namespace

// ---- quantize --------------------------------------------------------------

// The table as the plain pointers of its columns, as in fp8_quant.hip (the
// binding refuses a tensor off a 16 B boundary). Blocks >= total_blocks are
// the padding slots of the last slice: zeros under the same rule.
template <typename T>
__global__ void __launch_bounds__(kMtThreads)
quantize_mxfp4_kernel(const int64_t* __restrict__ tensor_ptrs,
                      const int64_t* __restrict__ block_prefix,
                      const int64_t* __restrict__ numels, int n_tensors,
                      int64_t total_blocks, int64_t padded_blocks,
                      int64_t blocks_per_rank, uint8_t* __restrict__ pack) {
  const int64_t b = wave_block();
  if (b >= padded_blocks) return;
  const int lane = threadIdx.x % kWave;

  float v[kMxSteps][kMtEpt] = {};
  if (b < total_blocks) {
    const int t = find_tensor(block_prefix, n_tensors, b);
    const T* src = reinterpret_cast<const T*>(tensor_ptrs[t]);
    const int64_t numel = numels[t];
    const int64_t first = (b - block_prefix[t]) * kMtBlock + lane * kMtEpt;
    if ((b - block_prefix[t] + 1) * kMtBlock <= numel) {  // a whole block
#pragma unroll
      for (int j = 0; j < kMxSteps; j++) load8(src + first + j * kWave * kMtEpt, v[j]);
    } else {
#pragma unroll
      for (int j = 0; j < kMxSteps; j++) {
        const int64_t off = first + j * kWave * kMtEpt;
        if (off + kMtEpt <= numel) {
          load8(src + off, v[j]);
        } else {
#pragma unroll
          for (int i = 0; i < kMtEpt; i++)
            v[j][i] = off + i < numel ? to_f32(src[off + i]) : 0.0f;
        }
      }
    }
  }
  const MxSlot slot(b, blocks_per_rank);
  encode_block(v, pack + slot.scales, pack + slot.codes);
}

// ---- dequantize back into the tensors --------------------------------------

template <typename T>
__global__ void __launch_bounds__(kMtThreads)
dequantize_mxfp4_kernel(const int64_t* __restrict__ tensor_ptrs,
                        const int64_t* __restrict__ block_prefix,
                        const int64_t* __restrict__ numels, int n_tensors,
                        int64_t total_blocks, int64_t blocks_per_rank,
                        const uint8_t* __restrict__ pack) {
  const int64_t b = wave_block();
  if (b >= total_blocks) return;  // padding slots map to no tensor
  const int lane = threadIdx.x % kWave;
  const MxSlot slot(b, blocks_per_rank);

  const int t = find_tensor(block_prefix, n_tensors, b);
  T* dst = reinterpret_cast<T*>(tensor_ptrs[t]);
  const int64_t numel = numels[t];
  const int64_t first = (b - block_prefix[t]) * kMtBlock + lane * kMtEpt;
#pragma unroll
  for (int j = 0; j < kMxSteps; j++) {
    float v[kMtEpt];
    decode_step(pack + slot.scales, pack + slot.codes, j, v);
    const int64_t off = first + j * kWave * kMtEpt;
    if (off + kMtEpt <= numel) {
      store8(dst + off, v);
    } else {
      for (int i = 0; i < kMtEpt; i++) {
        if (off + i < numel) from_f32(&dst[off + i], v[i]);
      }
    }
  }
}

// ---- reduce W copies of this rank's slice ----------------------------------

// in: [world, slice_bytes], out: [slice_bytes]. fp32 accumulation from zero
// over ranks 0..W-1 in that order; AVG is one product with inv_div = fl(1/W)
// (a power-of-two scale cannot absorb it); then the quantizer's rule. A NaN
// scale byte from any rank makes the sum NaN and the group's byte 0xFF.
__global__ void __launch_bounds__(kMtThreads)
reduce_mxfp4_slices_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                           int world, int64_t blocks_per_rank, float inv_div) {
  const int64_t bl = wave_block();
  if (bl >= blocks_per_rank) return;
  const MxSlot slot(bl, blocks_per_rank);  // bl < blocks_per_rank: slice 0
  const int64_t slice_bytes = blocks_per_rank * kMxBlockBytes;

  float acc[kMxSteps][kMtEpt] = {};
  for (int r = 0; r < world; r++) {
    const uint8_t* slice = in + (int64_t)r * slice_bytes;
#pragma unroll
    for (int j = 0; j < kMxSteps; j++) {
      float v[kMtEpt];
      decode_step(slice + slot.scales, slice + slot.codes, j, v);
#pragma unroll
      for (int i = 0; i < kMtEpt; i++) acc[j][i] += v[i];
    }
  }
#pragma unroll
  for (int j = 0; j < kMxSteps; j++) {
#pragma unroll
    for (int i = 0; i < kMtEpt; i++) acc[j][i] *= inv_div;
  }
  encode_block(acc, out + slot.scales, out + slot.codes);
}

// ---- host-visible launchers (raw pointers; stream passed in) ---------------

static dim3 mx_grid(int64_t blocks) {
  return dim3((uint32_t)((blocks + kMxBlocksPerWg - 1) / kMxBlocksPerWg));
}

void launch_mxfp4_quantize(int dtype_code, MultiTensorTable tb, int64_t padded_blocks,
                           int64_t blocks_per_rank, uint8_t* pack, hipStream_t stream) {
  if (padded_blocks <= 0) return;
  dispatch_dtype(dtype_code, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(quantize_mxfp4_kernel<T>, mx_grid(padded_blocks), dim3(kMtThreads),
                       0, stream, tb.col(0), tb.prefix(), tb.numels(), tb.n,
                       tb.total_blocks, padded_blocks, blocks_per_rank, pack);
  });
}

void launch_mxfp4_dequantize(int dtype_code, MultiTensorTable tb, int64_t blocks_per_rank,
                             const uint8_t* pack, hipStream_t stream) {
  if (tb.total_blocks <= 0) return;
  dispatch_dtype(dtype_code, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(dequantize_mxfp4_kernel<T>, mx_grid(tb.total_blocks),
                       dim3(kMtThreads), 0, stream, tb.col(0), tb.prefix(), tb.numels(),
                       tb.n, tb.total_blocks, blocks_per_rank, pack);
  });
}

void launch_mxfp4_reduce(const uint8_t* in, uint8_t* out, int world,
                         int64_t blocks_per_rank, bool avg, hipStream_t stream) {
  if (blocks_per_rank <= 0 || world <= 0) return;
  hipLaunchKernelGGL(reduce_mxfp4_slices_kernel, mx_grid(blocks_per_rank),
                     dim3(kMtThreads), 0, stream, in, out, world, blocks_per_rank,
                     avg ? 1.0f / world : 1.0f);
}

}  // namespace torchft_amd
