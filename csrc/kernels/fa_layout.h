// Address math of the flash-attention kernels (flash_attn_fwd.hip,
// flash_attn_bwd.hip): the sizes, the workgroup order, the subtiled LDS tile
// image, the thread -> chunk staging map, the tr_b16 read offsets, the pa/pb
// swizzle and the tile bounds of the document mask. Plain constexpr C++,
// callable from host and device; the device-only pieces built on it are in
// fa_tile.h. csrc/kernels/tests/fa_layout_test.cpp, fa_wg_order_test.cpp and
// fa_doc_bounds_test.cpp check every function here on the host.
#pragma once

#include "kernels.h"

namespace torchft_amd {

constexpr int kFaD = 128;        // head dim
constexpr int kFaWaves = 8;      // wave64s per workgroup
constexpr int kFaThreads = 512;
constexpr int kFaBlk = 32;       // rows of one wave's block (one MFMA tile)
static_assert(kFaThreads == kFaWaves * 64, "wave64");
// the attention launches put batch * heads in gridDim.y
constexpr int kFaMaxGridY = 65535;

// ---- workgroup order ----------------------------------------------------------
// The launches are (nx = blocks of 256 rows, ny = batch * heads). Under a
// causal mask the tiles a workgroup streams grow or shrink with its block x,
// and only one workgroup fits a CU, so the order in which blocks start
// decides how long the tail of a launch is. fa_wg_order maps the launch's
// block id to the (x, y) the kernel works on: with n = bx + nx * by, all ny
// (batch, head) pairs of the heaviest x come first and all pairs of the
// lightest x last. kFaHeavyLowX: x = 0 is the heaviest (dkdv, whose block x
// streams the query tiles at and after its keys); kFaHeavyHighX: x = nx - 1 is
// (dq and the forward, whose block x streams the keys at and before its rows).
// Without the causal flag the workgroups are equal and the map is the
// identity. It is a bijection of the grid either way
// (csrc/kernels/tests/fa_wg_order_test.cpp), every (x, y) does the work it
// always did, and results do not depend on the order blocks are dealt in:
// this is for speed only (docs/KERNELS.md, "Workgroup order").
// 32 bits hold n: q alone has nx * ny * 256 rows of 256 bytes, so n < 2^32
// wherever q fits in 2^48 bytes; the largest grid the bindings could admit
// (ny = kFaMaxGridY, S = 2^24) gives 65536 * 65535 < 2^32.
enum FaHeavy { kFaHeavyLowX, kFaHeavyHighX };
struct FaWg {
  int x, y;
};
TFT_HD constexpr FaWg fa_wg_order(unsigned bx, unsigned by, unsigned nx, unsigned ny,
                                  bool causal, FaHeavy heavy) {
  if (!causal) return {(int)bx, (int)by};
  const unsigned n = bx + nx * by;
  const unsigned rank = n / ny;
  return {(int)(heavy == kFaHeavyLowX ? rank : nx - 1 - rank), (int)(n % ny)};
}

// One ROWS x 128 bf16 tile in LDS = 8 subtiles of [ROWS rows][16 cols], each
// row-major and element-contiguous (tr_b16 needs its [4][16] blocks
// contiguous), so one image serves both fragment orientations: contiguous
// 16-B reads (k-dim = d) and hardware-transpose reads (k-dim = rows).
// Subtile stride = 65 * (ROWS / 2) bytes, i.e. ROWS * 32 + a ROWS/2-byte pad:
//   32 rows: 1040 = 1024 + 16. The 8 staging ds_write_b128 of a wave's lane
//     group land on 8 distinct bank quads (1024 would be 8-way conflicted).
//   64 rows: 2080 = 2048 + 32. 2080/4 = 520 = 8 (mod 32): the 8 staging
//     ds_write_b128 of a lane group hit 4 distinct bank quads (2-way);
//     = 8 (mod 64) keeps adjacent-subtile tr blocks mostly disjoint.
template <int ROWS>
struct Tile {
  static_assert(ROWS == 32 || ROWS == 64, "32- or 64-row tiles");
  static constexpr int kStride = 65 * (ROWS / 2);
  // 16-B chunks a thread stages per tensor; the 512 threads cover the tile
  static constexpr int kChunks = ROWS / 32;

  alignas(16) unsigned char sub[8 * kStride];

  // byte address of byte `byte_in_row` (0..31) of row `row` in subtile tt
  static TFT_HD constexpr int addr(int tt, int row, int byte_in_row) {
    return tt * kStride + row * 32 + byte_in_row;
  }

  // Staging map: thread t owns row t / (16/CH) and the 16-B chunks
  // (t % (16/CH)) * CH .. +CH of that row, CH = kChunks. Chunk c (8 d
  // columns) lives at subtile c/2, byte (c%2)*16 of its row.
  static TFT_HD constexpr int stage_row(int t) { return t / (16 / kChunks); }
  static TFT_HD constexpr int stage_chunk(int t) { return (t % (16 / kChunks)) * kChunks; }
  static TFT_HD constexpr int stage_addr(int t, int c) {
    return addr((stage_chunk(t) + c) >> 1, stage_row(t), ((stage_chunk(t) + c) & 1) * 16);
  }

  // Contiguous 16-B fragment (MFMA A/B operand with k-dim = d): k-slice tt
  // covers d = tt*16 + half*8 .. +8 of `row`.
  static TFT_HD constexpr int frag_addr(int tt, int row, int half) {
    return addr(tt, row, half * 16);
  }

  // tr_b16 reads (MFMA B operand with k-dim = rows). Per-lane invariant part:
  // subtile parity (l>>4)&1, k-half row offset (l>>5)*8 rows, chunk (l&15)*8 B.
  // A lane reads at tr_lane_off + tr_step_off(dt, h2) and that + 128 (rows
  // +4); joined, it holds [k = h2*16 + (l>>5)*8 + m][d = dt*32 + (l&31)],
  // m = 0..7, of a 32-row block. The second block of a 64-row tile is at
  // + 32*32.
  static TFT_HD constexpr unsigned tr_lane_off(int lane) {
    return ((lane >> 4) & 1) * kStride + ((lane >> 5) * 8) * 32 + (lane & 15) * 8;
  }
  static TFT_HD constexpr unsigned tr_step_off(int dt, int h2) {
    return dt * (2 * kStride) + h2 * 512;
  }
};

static_assert(Tile<32>::kStride == 1040 && Tile<64>::kStride == 2080, "subtile strides");
static_assert(sizeof(Tile<32>) == 8 * 1040 && sizeof(Tile<64>) == 8 * 2080, "no padding");

// element offset of sequence row s of head (b,h): bshd=1 means the storage is
// [B,S,H,D] (the model's projection layout, seen through a transpose view) —
// supporting it natively removes every layout copy the autograd path would
// otherwise pay.
TFT_HD constexpr int64_t row_off(int b, int h, int s, int H, int S, int bshd) {
  return bshd ? (((int64_t)b * S + s) * H + h) * kFaD
              : (((int64_t)b * H + h) * S + s) * kFaD;
}

// row of C/D register `reg` of a 32x32 MFMA in lane half `half` (col = l31)
TFT_HD constexpr int c_row(int reg, int half) {
  return (reg & 3) + 8 * (reg >> 2) + 4 * half;
}

// ---- document mask (causal within a document) -------------------------------
// Key j is visible to query i iff doc_start[i] <= j <= i, equally
// j <= i < doc_end[j]; both arrays are non-decreasing when DocMask built them.
// The kernels read them as they are: every bound below is clamped into the
// range the causal kernel uses, whatever int32 the arrays hold, so garbage
// costs correctness of the values and never an address
// (csrc/kernels/tests/fa_doc_bounds_test.cpp).
TFT_HD constexpr int fa_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Forward and dq: the first 64-key tile a workgroup streams. ds_first is
// doc_start of the workgroup's first query row (the smallest of its rows), nT
// the causal tile count (>= 1).
TFT_HD constexpr int doc_first_tile(int ds_first, int nT) {
  return fa_clamp(ds_first / 64, 0, nT - 1);
}
// Forward and dq, per wave: the 32-key block at kb0 ends before doc_start of
// the wave's first row, so none of its keys is visible to any of the 32 rows.
TFT_HD constexpr bool doc_block_skipped(int kb0, int ds_wave_first) {
  return kb0 + 31 < ds_wave_first;
}
// ... and the block needs the per-element test only if its first key lies
// below doc_start of the wave's last row.
TFT_HD constexpr bool doc_block_straddles(int kb0, int ds_wave_last) {
  return kb0 < ds_wave_last;
}
// the per-element test itself, on top of the causal one
TFT_HD constexpr bool doc_visible(int key, int ds_q) { return key >= ds_q; }

// dkdv: one past the last 32-query tile a workgroup streams. de_last is
// doc_end of the workgroup's last key (the largest of its keys); the causal
// range is [i_min, nQ) with i_min < nQ, and at least one tile stays.
TFT_HD constexpr int doc_last_qtile(int de_last, int i_min, int nQ) {
  return fa_clamp((fa_clamp(de_last, 0, nQ * kFaBlk) + kFaBlk - 1) / kFaBlk, i_min + 1, nQ);
}
// dkdv, per wave: query tile i starts at or past doc_end of the wave's last key
TFT_HD constexpr bool doc_qtile_skipped(int i, int de_wave_last) {
  return i * kFaBlk >= de_wave_last;
}
// ... and the tile needs the per-element test only if doc_start of its last
// query lies above the first key of the wave's block jb
TFT_HD constexpr bool doc_qtile_straddles(int ds_tile_last, int jb) {
  return ds_tile_last > jb * kFaBlk;
}

// pa/pb: a wave's 32 x 64 B transpose buffer (P or dS as bf16, [row][32 keys]),
// 16-B units XOR-swizzled by row.
TFT_HD constexpr int row_swz(int row, int byte_off) {
  return byte_off ^ ((((row >> 2) ^ (row >> 4)) & 3) << 4);
}
TFT_HD constexpr int pb_addr(int row, int byte_off) {
  return row * 64 + row_swz(row, byte_off);
}
// A-fragment read (row = l31, 8 consecutive elements at h2*16 + half*8)
TFT_HD constexpr int pb_afrag_addr(int h2, int half, int l31) {
  return pb_addr(l31, h2 * 32 + half * 16);
}
// pa/pb address of a lane's C element (row c_row(4*r4, half), col l31).
// The four rows c_row(4*r4 + r, half), r = 0..3, share one swizzle key, so
// they sit at +64*r: 4 address registers serve the 16 stores, not 16.
TFT_HD constexpr int pb_row4_addr(int r4, int half, int l31) {
  return pb_addr(8 * r4 + 4 * half, l31 * 2);
}

}  // namespace torchft_amd
