// Device side of the flash-attention tile image (fa_layout.h): fragment
// types, the register-staged tile-pair stream, the fragment reads and the
// tr_b16 read / counted-wait macros shared by flash_attn_fwd.hip and
// flash_attn_bwd.hip.
#pragma once

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fa_layout.h"

namespace torchft_amd {

using bf16 = __hip_bfloat16;
typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8_vec;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float f32x16;

// T14 async-STAGE split of one (tile A, tile B) pair: the global loads land
// in registers (issued a tile early, under the previous tile's MFMAs), the
// LDS writes follow later. Thread t carries Tile<ROWS>::kChunks uint4 per
// tensor, mapped by Tile<ROWS>::stage_*.
template <int ROWS>
struct TileRegs {
  uint4 a[Tile<ROWS>::kChunks], b[Tile<ROWS>::kChunks];
};

// ld = elements between consecutive sequence rows (layout-dependent)
template <int ROWS>
__device__ inline TileRegs<ROWS> load_tiles(const bf16* __restrict__ srcA,
                                            const bf16* __restrict__ srcB, int64_t ld) {
  using T = Tile<ROWS>;
  const int t = threadIdx.x;
  const int64_t off = (int64_t)T::stage_row(t) * ld + T::stage_chunk(t) * 8;
  TileRegs<ROWS> r;
#pragma unroll
  for (int c = 0; c < T::kChunks; c++) r.a[c] = reinterpret_cast<const uint4*>(srcA + off)[c];
#pragma unroll
  for (int c = 0; c < T::kChunks; c++) r.b[c] = reinterpret_cast<const uint4*>(srcB + off)[c];
  return r;
}

template <int ROWS>
__device__ inline void write_tiles(Tile<ROWS>* dstA, Tile<ROWS>* dstB,
                                   const TileRegs<ROWS>& r) {
  using T = Tile<ROWS>;
  const int t = threadIdx.x;
#pragma unroll
  for (int c = 0; c < T::kChunks; c++)
    *reinterpret_cast<uint4*>(dstA->sub + T::stage_addr(t, c)) = r.a[c];
#pragma unroll
  for (int c = 0; c < T::kChunks; c++)
    *reinterpret_cast<uint4*>(dstB->sub + T::stage_addr(t, c)) = r.b[c];
}

// contiguous 16-B fragment of a tile image (Tile::frag_addr)
template <int ROWS>
__device__ inline bf16x8_vec rm_frag(const unsigned char* tile, int tt, int row, int half) {
  return *reinterpret_cast<const bf16x8_vec*>(tile + Tile<ROWS>::frag_addr(tt, row, half));
}

__device__ inline bf16x8_vec pb_afrag(const unsigned char* pb, int h2, int half, int l31) {
  return *reinterpret_cast<const bf16x8_vec*>(pb + pb_afrag_addr(h2, half, l31));
}

// The DOC (document mask) kernel variants take their int32 arrays as a
// trailing parameter pack, so that the plain instantiations keep the parameter
// list, the kernarg layout and with them the code they had without the mask.
// doc_ptr<I>(pack...) is array I of the pack.
template <int I, class... R>
__device__ inline const int* doc_ptr(const int* first, R... rest) {
  if constexpr (I == 0) {
    return first;
  } else {
    return doc_ptr<I - 1>(rest...);
  }
}

// one hardware-transpose read: 4 bf16 = column (l&15), rows j=0..3 of the
// [4][16] block at (per-lane) byte address `addr` into the LDS image
#define TR_READ(dst, addr) \
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(dst) : "v"(addr))

// Counted wait: allow N newer LDS ops to stay in flight, and tie the
// registers the following MFMAs consume so they cannot be scheduled above
// the wait (explicit dataflow — "memory" alone would not order
// register-only MFMAs past an asm wait, §5.4 rule 18).
#define TR_WAIT4_KEEP(N, r0, r1, r2, r3)              \
  asm volatile("s_waitcnt lgkmcnt(" #N ")"            \
               : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3))
#define TR_WAIT2_KEEP(N, r0, r1) \
  asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(r0), "+v"(r1))

// the two tr_b16 reads of a lane (rows +0..3, +4..7) as one MFMA operand
__device__ inline bf16x8_vec tr_join(unsigned long long lo, unsigned long long hi) {
  union {
    struct {
      unsigned long long lo, hi;
    } u;
    bf16x8_vec v;
  } c;
  c.u.lo = lo;
  c.u.hi = hi;
  return c.v;
}

}  // namespace torchft_amd
