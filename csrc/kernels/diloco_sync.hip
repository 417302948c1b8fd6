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
//
// With the fp8-quantized allreduce two more kernels put the wire pack of
// fp8_quant.hip in place of the pseudo-gradient tensors (further down):
// pseudograd_fp8_kernel and outer_sgd_fp8_kernel.

#include <hip/hip_runtime.h>

#include <type_traits>

#include "fp8_block.h"
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

// ---- the quantized sync: pseudo-gradient into the fp8 pack, step from it ----
//
// With should_quantize the pseudo-gradient only ever travels as the fp8 wire
// pack of fp8_quant.hip (W slices, slice r = [fp32 scales of its blocks] ‖
// [2048 codes per block]; per-tensor block padding). These two kernels sit at
// the two ends of that pack, so the bf16 pseudo-gradient is never stored:
//
//   pseudograd_fp8_kernel   pack = quantize(float(a) - float(b)), the
//                           quantizer's block math on the fp32 difference
//   outer_sgd_fp8_kernel    outer_sgd_kernel with d decoded from the reduced
//                           pack: d = code * (scale * inv_div)

// eight fp32 values times q_scale -> eight e4m3 codes, the quantizer's
// conversion (saturating, round to nearest even, NaN for non-finite)
__device__ inline uint2 encode8(const float (&v)[kMtEpt], float q_scale) {
  uint8_t q[kMtEpt];
#pragma unroll
  for (int i = 0; i < kMtEpt; i++) {
    fp8_t f8(v[i] * q_scale);
    q[i] = *reinterpret_cast<uint8_t*>(&f8);
  }
  return *reinterpret_cast<uint2*>(q);
}

// Where block `pb` of a pack lives: its scale and its 2048 codes. Byte is
// uint8_t for the kernel that writes the pack, const uint8_t for the reader.
template <typename Byte>
struct PackBlock {
  using Scale = std::conditional_t<std::is_const_v<Byte>, const float, float>;
  Scale* scale;
  Byte* codes;
  __device__ PackBlock(Byte* pack, int64_t pb, int64_t blocks_per_rank,
                       int64_t slice_bytes) {
    const int64_t r = pb / blocks_per_rank;
    const int64_t bl = pb % blocks_per_rank;
    Byte* slice = pack + r * slice_bytes;
    scale = reinterpret_cast<Scale*>(slice) + bl;
    codes = slice + blocks_per_rank * 4 + bl * kMtBlock;
  }
};

// Grid: one workgroup per (padded) pack block, as quantize_fp8_kernel, and its
// plain-column addressing (10 KB per workgroup: the dependent scalar loads in
// front of the data still set the time). Every tensor is 16 B-aligned (the
// binding checks), so only a tensor's last vector goes element by element.
// v = float(a) - float(b) is one fp32 rounding and never rounded to T; lanes
// past numel hold zeros; blocks >= total_blocks write scale 0 and zero codes.
template <typename T>
__global__ void __launch_bounds__(kMtThreads) pseudograd_fp8_kernel(
    const int64_t* __restrict__ a_ptrs,        // [n] minuends
    const int64_t* __restrict__ b_ptrs,        // [n] subtrahends
    const int64_t* __restrict__ block_prefix,  // [n+1]
    const int64_t* __restrict__ numels,        // [n]
    int n_tensors, int64_t total_blocks, int64_t blocks_per_rank,
    int64_t slice_bytes, uint8_t* __restrict__ pack) {
  const int64_t blk = blockIdx.x;
  const PackBlock<uint8_t> dst(pack, blk, blocks_per_rank, slice_bytes);

  float v[kMtEpt] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (blk < total_blocks) {
    const int t = find_tensor(block_prefix, n_tensors, blk);
    const int64_t off = (blk - block_prefix[t]) * kMtBlock + threadIdx.x * kMtEpt;
    const T* a = reinterpret_cast<const T*>(a_ptrs[t]);
    const T* b = reinterpret_cast<const T*>(b_ptrs[t]);
    const int64_t numel = numels[t];
    if (off + kMtEpt <= numel) {
      float bv[kMtEpt];
      load8(a + off, v);
      load8(b + off, bv);
#pragma unroll
      for (int i = 0; i < kMtEpt; i++) v[i] -= bv[i];
    } else {
#pragma unroll
      for (int i = 0; i < kMtEpt; i++)
        v[i] = (off + i < numel) ? to_f32(a[off + i]) - to_f32(b[off + i]) : 0.0f;
    }
  }

  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < kMtEpt; i++) amax = fmaxf(amax, fabsf(v[i]));
  amax = block_reduce_max(amax);

  float q_scale, dq_scale;
  block_scales(amax, 1.f, q_scale, dq_scale);

  *reinterpret_cast<uint2*>(dst.codes + threadIdx.x * kMtEpt) = encode8(v, q_scale);
  if (threadIdx.x == 0) *dst.scale = dq_scale;
}

// cols 0..2 = g, l, first pack block of the tensor (col 3 = m): one launch per
// (param group, pack). The group's tensors are a subset of the pack's, so
// logical block `blockIdx.x` of tensor t is pack block first_block[t] +
// (block - prefix[t]). The scale load is wave-uniform; scale * inv_div is
// folded once per block, and both products are single fp32 roundings that are
// kept out of any fma (d is the same value wherever outer_sgd_elem uses it).
// The codes are 8 B-aligned whatever the tensors are, so the lane always takes
// its eight codes in one load; g, l, m follow outer_sgd_kernel's two paths.
template <typename T, bool HAS_MOMENTUM>
__global__ void __launch_bounds__(kMtThreads)
outer_sgd_fp8_kernel(MultiTensorTable tb, const uint8_t* __restrict__ pack,
                     int64_t blocks_per_rank, int64_t slice_bytes, float inv_div,
                     float lr, float mu, int nesterov, float alpha) {
  const MtCursor c(tb, blockIdx.x, threadIdx.x);
  if (c.cnt == 0) return;
  const int64_t pg = c.addr(tb, 0), pl = c.addr(tb, 1);
  const int64_t pack_block = c.addr(tb, 2) + c.off / kMtBlock;
  int64_t pm = 0;
  if constexpr (HAS_MOMENTUM) pm = c.addr(tb, 3);
  T* g = c.at<T>(pg);
  T* l = c.at<T>(pl);
  T* m = nullptr;
  if constexpr (HAS_MOMENTUM) m = c.at<T>(pm);
  const bool nes = nesterov != 0;

  const PackBlock<const uint8_t> src(pack, pack_block, blocks_per_rank, slice_bytes);
  const float s = __fmul_rn(*src.scale, inv_div);
  const uint2 raw = *reinterpret_cast<const uint2*>(src.codes + threadIdx.x * kMtEpt);
  const uint8_t* q = reinterpret_cast<const uint8_t*>(&raw);
  float dv[kMtEpt];
#pragma unroll
  for (int i = 0; i < kMtEpt; i++) {
    const fp8_t f8 = *reinterpret_cast<const fp8_t*>(&q[i]);
    dv[i] = __fmul_rn((float)f8, s);
  }

  if (c.vec_ok(pg | pl | pm)) {
    float gv[kMtEpt], lv[kMtEpt], mv[kMtEpt] = {};
    load8(g, gv);
    load8(l, lv);
    if constexpr (HAS_MOMENTUM) load8(m, mv);
#pragma unroll
    for (int i = 0; i < kMtEpt; i++)
      outer_sgd_elem<T, HAS_MOMENTUM>(gv[i], dv[i], mv[i], lv[i], lr, mu, nes, alpha);
    if constexpr (HAS_MOMENTUM) store8(m, mv);
    store8(g, gv);
    store8(l, lv);
  } else {
#pragma unroll
    for (int i = 0; i < kMtEpt; i++) {
      if (i >= c.cnt) break;
      float gf = to_f32(g[i]), lf = to_f32(l[i]), mf = 0.f;
      if constexpr (HAS_MOMENTUM) mf = to_f32(m[i]);
      outer_sgd_elem<T, HAS_MOMENTUM>(gf, dv[i], mf, lf, lr, mu, nes, alpha);
      if constexpr (HAS_MOMENTUM) from_f32(m + i, mf);
      from_f32(g + i, gf);
      from_f32(l + i, lf);
    }
  }
}

void launch_pseudograd_fp8(int dtype_code, MultiTensorTable tb, int64_t padded_blocks,
                           int64_t blocks_per_rank, int64_t slice_bytes, uint8_t* pack,
                           hipStream_t stream) {
  if (padded_blocks <= 0) return;
  dispatch_dtype(dtype_code, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(pseudograd_fp8_kernel<T>, dim3((uint32_t)padded_blocks),
                       dim3(kMtThreads), 0, stream, tb.col(0), tb.col(1), tb.prefix(),
                       tb.numels(), tb.n, tb.total_blocks, blocks_per_rank, slice_bytes,
                       pack);
  });
}

void launch_outer_sgd_fp8(int dtype_code, bool has_momentum, MultiTensorTable tb,
                          const uint8_t* pack, int64_t blocks_per_rank,
                          int64_t slice_bytes, float inv_div, float lr, float mu,
                          bool nesterov, float alpha, hipStream_t stream) {
  if (tb.total_blocks <= 0) return;
  const dim3 grid((uint32_t)tb.total_blocks);
  const int nes = nesterov ? 1 : 0;
  dispatch_dtype(dtype_code, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (has_momentum)
      hipLaunchKernelGGL((outer_sgd_fp8_kernel<T, true>), grid, dim3(kMtThreads), 0,
                         stream, tb, pack, blocks_per_rank, slice_bytes, inv_div, lr, mu,
                         nes, alpha);
    else
      hipLaunchKernelGGL((outer_sgd_fp8_kernel<T, false>), grid, dim3(kMtThreads), 0,
                         stream, tb, pack, blocks_per_rank, slice_bytes, inv_div, lr, mu,
                         nes, alpha);
  });
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
