// Flash-attention BACKWARD for CDNA4 (gfx950) — bf16, D=128, causal + full,
// GQA-native (dK/dV accumulate over the query heads of each KV head in
// registers; no atomics anywhere).
//
// Motivation (profiles/SUMMARY.md): the stock aotriton backward is 31% of
// the Llama-8B step; this is a hand-written MFMA replacement. The forward
// stays on aten's flash kernel — we consume its logsumexp
// (P = exp(scale*S - LSE)) plus the usual FA2 delta D_i = rowsum(dO*O).
//
// Structure (FA2 split): kernel 1 computes dK/dV (grid over KV blocks),
// kernel 2 computes dQ (grid over Q blocks); both recompute S/P per tile.
// Each workgroup = 8 wave64s; each wave owns one 32-row block and holds its
// fp32 accumulators in the unified VGPR/AGPR file.
//
// Schedule (v3): the staged tiles live in ONE subtiled row-major LDS image
// (Tile<ROWS> of fa_layout.h: [8 d-subtiles][ROWS rows][16 cols], subtile
// stride 65 * ROWS/2 bytes) serving BOTH fragment orientations: contiguous
// ds_read_b128 for the S/dP chains and hardware-transpose
// ds_read_b64_tr_b16 for the dV/dK/dQ chains. This removes v2's separate
// transposed images and their 32-per-thread b16 scatter writes (the worst
// LDS citizen in the v2 profile). tr_b16 semantics verified by
// csrc/kernels/tr16_probe.hip on gfx950: with lane-linear 8-B addresses
// over a contiguous [4][16] bf16 block per 16-lane group, lane l receives
// column (l&15), elements j=0..3 = rows.
//
// Pipeline (v4): both tile streams are software-pipelined one tile deep
// (T14 async-STAGE split). A prologue stages tile 0; each iteration issues
// tile t+1's global loads into registers, computes tile t from img[t&1],
// then writes the registers to img[(t+1)&1] and takes ONE barrier. Only one
// workgroup fits a CU, so nothing else would cover the L2/HBM round trip.
// dkdv issues the prefetch between its two phases, which also lets the
// dV/dK phase double-buffer its tr_b16 reads. The arithmetic is untouched:
// results are bit-identical to the v3 loop.
//
// Document mask (DOC variants): causal within the documents of a packed row.
// dkdv ends its query-tile stream where the documents of its keys end, dq
// starts its key-tile stream where the documents of its rows start, and the
// per-element test runs only in tiles that straddle a boundary (bounds:
// fa_layout.h; docs/KERNELS.md).
//
// MFMA lane mappings (verified by mfma_probe.hip on gfx950):
//   A: row=lane&31, k=(lane>>5)*8+m   B: k=(lane>>5)*8+m, col=lane&31
//   C/D: col=lane&31, row=(reg&3)+8*(reg>>2)+4*(lane>>5)

#include <hip/hip_runtime.h>

#include <type_traits>

#include "fa_tile.h"

namespace torchft_amd {

// dkdv streams 32-row Q / dO tiles (geometry and staging: fa_layout.h)
struct ImageSet {
  Tile<32> a;  // Q
  Tile<32> b;  // dO
};

struct SmemFA {
  ImageSet img[2];                                  // double buffer
  alignas(16) unsigned char pa[kFaWaves][32 * 64];  // P transpose bufs
  alignas(16) unsigned char pb[kFaWaves][32 * 64];  // dS transpose bufs
  // per-wave V operand tile (8 slots) + the last two K k-slices (2 slots)
  // in A-fragment order (dkdv kernel only): [wave][slot][lane][8 bf16] =
  // one b128 per (slot, lane). The first six K k-slices live in VGPRs —
  // all eight would push the allocator over the 256-VGPR spill cliff.
  alignas(16) unsigned char v_ops[kFaWaves][10 * 64 * 16];
};

// ---- kernel 1: dK/dV ------------------------------------------------------
// DOC (both kernels): the document-mask variant (docs/KERNELS.md, "document
// mask"). Its arrays ride in the trailing pack (fa_tile.h, doc_ptr): dkdv
// takes doc_start and doc_end, dq doc_start alone.
template <bool DOC, class... DocP>
__global__ __launch_bounds__(kFaThreads, 1) void fa_bwd_dkdv_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const bf16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    bf16* __restrict__ dk, bf16* __restrict__ dv, int B, int Hq, int Hkv,
    int S, float scale, int causal, int bshd, DocP... docp) {
  static_assert(sizeof...(DocP) == (DOC ? 2 : 0), "DOC takes doc_start, doc_end");
  __shared__ SmemFA sm;
  const int G = Hq / Hkv;
  // causal: block 0 streams the most query tiles; all heads of it start first
  const FaWg wg =
      fa_wg_order(blockIdx.x, blockIdx.y, gridDim.x, gridDim.y, causal, kFaHeavyLowX);
  const int b = wg.y / Hkv;
  const int hkv = wg.y % Hkv;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int jb = wg.x * kFaWaves + wave;
  const bool active = jb * kFaBlk < S;
  const int nQ = S / kFaBlk;
  const int i_min = causal ? wg.x * kFaWaves : 0;
  // DOC: the query tiles end where the document of the workgroup's last key
  // ends; a wave stops computing at doc_end of its own last key (de_w)
  int i_hi = nQ, de_w = 0;
  const int* ds_base = nullptr;
  if constexpr (DOC) {
    ds_base = doc_ptr<0>(docp...) + (int64_t)b * S;
    const int* doc_end = doc_ptr<1>(docp...) + (int64_t)b * S;
    const int wg_last = min((wg.x + 1) * kFaWaves * kFaBlk, S) - 1;
    i_hi = doc_last_qtile(doc_end[wg_last], i_min, nQ);
    if (active) {
      de_w = __builtin_amdgcn_readfirstlane(doc_end[jb * kFaBlk + kFaBlk - 1]);
    }
  }
  const int nI = (DOC ? i_hi : nQ) - i_min;
  const int T = G * nI;  // flattened (g, i) iteration count

  // K fragments in VGPRs (the wave's fixed A-operand); V in wave-private
  // LDS in A-fragment order (both in VGPRs would blow the 256-VGPR file)
  unsigned char* vops = sm.v_ops[wave];
  bf16x8_vec kfrag[6];
  if (active) {
    const int64_t kv_off = row_off(b, hkv, jb * kFaBlk + l31, Hkv, S, bshd);
#pragma unroll
    for (int t = 0; t < 8; t++) {
      const bf16x8_vec kv =
          *reinterpret_cast<const bf16x8_vec*>(k + kv_off + t * 16 + half * 8);
      if (t < 6) {
        kfrag[t] = kv;
      } else {
        *reinterpret_cast<bf16x8_vec*>(vops + ((t + 2) * 64 + lane) * 16) = kv;
      }
      *reinterpret_cast<bf16x8_vec*>(vops + (t * 64 + lane) * 16) =
          *reinterpret_cast<const bf16x8_vec*>(v + kv_off + t * 16 + half * 8);
    }
  }

  f32x16 dk_acc[4] = {};
  f32x16 dv_acc[4] = {};

  const int64_t q_ld = bshd ? (int64_t)Hq * kFaD : kFaD;  // seq-row stride
  const float* lse_base = lse + ((int64_t)b * Hq + hkv * G) * S;
  const float* delta_base = delta + ((int64_t)b * Hq + hkv * G) * S;

  auto tile_src = [&](int t, const bf16* base) -> const bf16* {
    const int g = t / nI;
    const int i = i_min + t % nI;
    return base + row_off(b, hkv * G + g, i * kFaBlk, Hq, S, bshd);
  };

  const unsigned tr_off = Tile<32>::tr_lane_off(lane);

  // prologue: stage tile 0 and its row statistics
  TileRegs<32> nxt = load_tiles<32>(tile_src(0, q), tile_src(0, dout), q_ld);
  float lse_n = lse_base[i_min * kFaBlk + l31];
  float delta_n = delta_base[i_min * kFaBlk + l31];
  // DOC: doc_start of the lane's query, staged beside lse / delta
  int ds_n = 0;
  if constexpr (DOC) ds_n = ds_base[i_min * kFaBlk + l31];
  write_tiles(&sm.img[0].a, &sm.img[0].b, nxt);
  __syncthreads();

  for (int t = 0; t < T; t++) {
    const int cur = t & 1;
    const int i = i_min + t % nI;

    const float lse_q = lse_n;
    const float delta_q = delta_n;
    const int ds_q = ds_n;
    const bool more = t + 1 < T;  // wave-uniform
    const bool computes =
        active && !(causal && i < jb) && !(DOC && doc_qtile_skipped(i, de_w));

    // phase 1: S^T, dP^T, then P / dS into the wave's pa / pb
    if (computes) {
      const ImageSet* img = &sm.img[cur];

      // interleaved S^T / dP^T chains (independent accumulators)
      f32x16 s_acc = {};
      f32x16 dp_acc = {};
#pragma unroll
      for (int tt = 0; tt < 8; tt++) {
        const bf16x8_vec vf =
            *reinterpret_cast<const bf16x8_vec*>(vops + (tt * 64 + lane) * 16);
        const bf16x8_vec kf =
            tt < 6 ? kfrag[tt]
                   : *reinterpret_cast<const bf16x8_vec*>(
                         vops + ((tt + 2) * 64 + lane) * 16);
        s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            kf, rm_frag<32>(img->a.sub, tt, l31, half), s_acc, 0, 0, 0);
        dp_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            vf, rm_frag<32>(img->b.sub, tt, l31, half), dp_acc, 0, 0, 0);
      }

      unsigned char* pa = sm.pa[wave];
      unsigned char* pb = sm.pb[wave];
      // q row minus the lane's first key row: the causal test of C register
      // rg is one compare against the constant c_row(rg, 0)
      const int qk = (i - jb) * kFaBlk + l31 - 4 * half;
      // DOC: only a tile that straddles a boundary (wave-uniform test) has
      // keys below doc_start of its queries. Their scores become -inf there,
      // so the loop below, unchanged, gives them P = exp(-inf) = 0 and dS = 0.
      // dsk = doc_start of the lane's query minus the lane's first key row,
      // the causal test's form: key >= doc_start is c_row(rg, 0) >= dsk. The
      // clamp keeps the difference in range for any int32.
      if constexpr (DOC) {
        if (doc_qtile_straddles(__builtin_amdgcn_readlane(ds_q, 31), jb)) {
          const int dsk = fa_clamp(ds_q, 0, S) - jb * kFaBlk - 4 * half;
#pragma unroll
          for (int rg = 0; rg < 16; rg++) {
            if (c_row(rg, 0) < dsk) s_acc[rg] = -INFINITY;
          }
        }
      }
#pragma unroll
      for (int rg = 0; rg < 16; rg++) {
        const bool valid = !causal || (qk >= c_row(rg, 0));
        const float pv = valid ? __expf(scale * s_acc[rg] - lse_q) : 0.0f;
        const int wr = pb_row4_addr(rg >> 2, half, l31) + (rg & 3) * 64;
        *reinterpret_cast<bf16*>(pa + wr) = __float2bfloat16(pv);
        *reinterpret_cast<bf16*>(pb + wr) =
            __float2bfloat16(pv * (dp_acc[rg] - delta_q) * scale);
      }
    }

    // T14 split: tile t+1's global loads (and its lse/delta rows) issue
    // here, once the S/dP accumulators are dead (no VGPR cost at the
    // pressure peak), and land under the dV/dK MFMAs; the LDS write follows
    // the compute. Every wave takes part, computing or not. The last tile
    // forms no address.
    if (more) {
      const int64_t st = (int64_t)((t + 1) / nI) * S +
                         (i_min + (t + 1) % nI) * kFaBlk + l31;
      nxt = load_tiles<32>(tile_src(t + 1, q), tile_src(t + 1, dout), q_ld);
      lse_n = lse_base[st];
      delta_n = delta_base[st];
      if constexpr (DOC) ds_n = ds_base[(i_min + (t + 1) % nI) * kFaBlk + l31];
    }

    if (computes) {
      const ImageSet* img = &sm.img[cur];
      unsigned char* pa = sm.pa[wave];
      unsigned char* pb = sm.pb[wave];
      // phase 2: dV += P^T dO ; dK += dS^T Q. A-fragments (P, dS) come
      // from the wave-private pa / pb (same-wave DS ordering covers the RAW
      // with the stores of phase 1); B-fragments by hardware transpose,
      // software-pipelined one (dt,h2) iteration ahead: the next
      // iteration's 4 tr reads issue before this one's MFMAs, and the
      // counted lgkmcnt(4) leaves exactly those in flight (safe beside
      // compiler DS ops: DS completes in order, so "all but newest 4 done"
      // over-waits at worst). The second register set fits because phase 2
      // no longer shares its pressure peak with the S/dP accumulators.
      const unsigned a_base = (unsigned)(uintptr_t)img->a.sub + tr_off;
      const unsigned b_base = (unsigned)(uintptr_t)img->b.sub + tr_off;
      bf16x8_vec paf[2], pbf[2];
#pragma unroll
      for (int h2 = 0; h2 < 2; h2++) {
        paf[h2] = pb_afrag(pa, h2, half, l31);
        pbf[h2] = pb_afrag(pb, h2, half, l31);
      }
      unsigned long long fd0[2], fd1[2], fq0[2], fq1[2];
      TR_READ(fd0[0], b_base);
      TR_READ(fd1[0], b_base + 128);
      TR_READ(fq0[0], a_base);
      TR_READ(fq1[0], a_base + 128);
#pragma unroll
      for (int it = 0; it < 8; it++) {
        // dt fastest: consecutive MFMAs rotate over the four dv/dk
        // accumulators, so the 32-cycle dependent-accumulator latency of
        // the 32x32 MFMA never stalls the pipe (PMC: SQ_WAIT_INST_ANY)
        const int dt = it & 3;
        const int h2 = it >> 2;
        const int c = it & 1;
        const int n = c ^ 1;
        if (it < 7) {
          const unsigned nbase = Tile<32>::tr_step_off((it + 1) & 3, (it + 1) >> 2);
          TR_READ(fd0[n], b_base + nbase);
          TR_READ(fd1[n], b_base + nbase + 128);
          TR_READ(fq0[n], a_base + nbase);
          TR_READ(fq1[n], a_base + nbase + 128);
          TR_WAIT4_KEEP(4, fd0[c], fd1[c], fq0[c], fq1[c]);
        } else {
          TR_WAIT4_KEEP(0, fd0[c], fd1[c], fq0[c], fq1[c]);
        }
        dv_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            paf[h2], tr_join(fd0[c], fd1[c]), dv_acc[dt], 0, 0, 0);
        dk_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            pbf[h2], tr_join(fq0[c], fq1[c]), dk_acc[dt], 0, 0, 0);
      }
    }
    if (more) write_tiles(&sm.img[cur ^ 1].a, &sm.img[cur ^ 1].b, nxt);
    // One barrier per tile: img[cur^1] was last read in iteration t-1, and
    // every wave finished those reads before it passed that barrier.
    __syncthreads();
  }

  if (!active) return;
#pragma unroll
  for (int dt = 0; dt < 4; dt++) {
#pragma unroll
    for (int rg = 0; rg < 16; rg++) {
      const int key = c_row(rg, half);
      const int64_t row = row_off(b, hkv, jb * kFaBlk + key, Hkv, S, bshd);
      const int d = dt * 32 + l31;
      dk[row + d] = __float2bfloat16(dk_acc[dt][rg]);
      dv[row + d] = __float2bfloat16(dv_acc[dt][rg]);
    }
  }
}

// ---- dq-kernel 64-key tiles ------------------------------------------------
// Staging a 64-key K/V tile per barrier halves the per-MFMA staging/barrier
// overhead vs the 32-key tiles the dkdv kernel uses for its Q/dO stream.
struct SmemDq {
  Tile<64> k_img[2];
  Tile<64> v_img[2];
  alignas(16) unsigned char pb[kFaWaves][32 * 64];
};
// DOC: each wave keeps doc_start of its 32 query rows in LDS. The rows are C
// registers in dq, and sixteen more live VGPRs do not fit.
struct SmemDqDoc : SmemDq {
  alignas(16) int ds_row[kFaWaves][32];
};

// ---- kernel 2: dQ ---------------------------------------------------------
template <bool DOC, class... DocP>
__global__ __launch_bounds__(kFaThreads, 1) void fa_bwd_dq_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const bf16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    bf16* __restrict__ dq, int B, int Hq, int Hkv, int S, float scale,
    int causal, int bshd, DocP... docp) {
  static_assert(sizeof...(DocP) == (DOC ? 1 : 0), "DOC takes doc_start");
  __shared__ std::conditional_t<DOC, SmemDqDoc, SmemDq> sm;
  const int G = Hq / Hkv;
  // causal: the last q block streams the most key tiles; all heads of it
  // start first
  const FaWg wg =
      fa_wg_order(blockIdx.x, blockIdx.y, gridDim.x, gridDim.y, causal, kFaHeavyHighX);
  const int b = wg.y / Hq;
  const int hq = wg.y % Hq;
  const int hkv = hq / G;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int half = lane >> 5;
  const int l31 = lane & 31;
  const int bx = wg.x;
  const int ib = bx * kFaWaves + wave;
  const bool active = ib * kFaBlk < S;
  const int nK64 = (S + 63) / 64;
  const int kv_hi = causal ? (bx * kFaWaves + kFaWaves) * kFaBlk : S;
  const int T = causal ? (min(kv_hi, S) + 63) / 64 : nK64;

  bf16x8_vec qfrag[8], dofrag[8];
  float lse_row[16], delta_row[16];
  if (active) {
    const int64_t q_off = row_off(b, hq, ib * kFaBlk + l31, Hq, S, bshd);
#pragma unroll
    for (int t = 0; t < 8; t++) {
      qfrag[t] = *reinterpret_cast<const bf16x8_vec*>(q + q_off + t * 16 + half * 8);
      dofrag[t] = *reinterpret_cast<const bf16x8_vec*>(dout + q_off + t * 16 + half * 8);
    }
    const float* lse_head = lse + ((int64_t)b * Hq + hq) * S;
    const float* delta_head = delta + ((int64_t)b * Hq + hq) * S;
#pragma unroll
    for (int rg = 0; rg < 16; rg++) {
      const int row = ib * kFaBlk + c_row(rg, half);
      lse_row[rg] = lse_head[row];
      delta_row[rg] = delta_head[row];
    }
  }

  f32x16 dq_acc[4] = {};

  // DOC: as in the forward, the workgroup streams from the tile that holds
  // doc_start of its first row, a wave skips the blocks below doc_start of
  // its first row (ds_w0) and tests per element only below that of its last
  // row (ds_w1).
  int j0 = 0, ds_w0 = 0, ds_w1 = 0;
  if constexpr (DOC) {
    const int* doc_start = doc_ptr<0>(docp...) + (int64_t)b * S;
    j0 = doc_first_tile(doc_start[bx * kFaWaves * kFaBlk], T);
    int ds_lane = 0;
    if (active) ds_lane = doc_start[ib * kFaBlk + l31];
    if (half == 0) sm.ds_row[wave][l31] = ds_lane;
    ds_w0 = __builtin_amdgcn_readlane(ds_lane, 0);
    ds_w1 = __builtin_amdgcn_readlane(ds_lane, 31);
  }

  const int64_t kv_ld = bshd ? (int64_t)Hkv * kFaD : kFaD;
  const unsigned tr_off = Tile<64>::tr_lane_off(lane);

  auto tile_regs = [&](int j) -> TileRegs<64> {
    const int64_t off = row_off(b, hkv, j * 64, Hkv, S, bshd);
    return load_tiles<64>(k + off, v + off, kv_ld);
  };

  // prologue: stage key tile 0 (DOC: the first tile needed)
  TileRegs<64> pre = tile_regs(DOC ? j0 : 0);
  write_tiles(&sm.k_img[DOC ? j0 & 1 : 0], &sm.v_img[DOC ? j0 & 1 : 0], pre);
  __syncthreads();

  for (int j = DOC ? j0 : 0; j < T; j++) {
    const int cur = j & 1;
    // T14 split: key tile j+1's global loads land under tile j's MFMAs.
    // Wave-uniform guard: the last tile forms no address.
    const bool more = j + 1 < T;
    if (more) pre = tile_regs(j + 1);

    if (active && !(causal && j * 64 > ib * kFaBlk + kFaBlk - 1) &&
        !(DOC && doc_block_skipped(j * 64 + 32, ds_w0))) {
      const unsigned char* kimg = sm.k_img[cur].sub;
      const unsigned char* vimg = sm.v_img[cur].sub;
      const unsigned a_base = (unsigned)(uintptr_t)kimg + tr_off;
      unsigned char* pb = sm.pb[wave];

#pragma unroll
      for (int s = 0; s < 2; s++) {  // two 32-key halves per staged tile
        const int kb0 = j * 64 + s * 32;
        if (causal && kb0 > ib * kFaBlk + kFaBlk - 1) break;
        if (DOC && doc_block_skipped(kb0, ds_w0)) continue;

        f32x16 s_acc = {};
        f32x16 dp_acc = {};
#pragma unroll
        for (int tt = 0; tt < 8; tt++) {
          s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              qfrag[tt], rm_frag<64>(kimg, tt, s * 32 + l31, half), s_acc, 0, 0, 0);
          dp_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              dofrag[tt], rm_frag<64>(vimg, tt, s * 32 + l31, half), dp_acc, 0, 0, 0);
        }

        const int kg = kb0 + l31;
        // key minus the lane's first q row: the causal test of C register
        // rg is one compare against the constant c_row(rg, 0)
        const int kq = kg - ib * kFaBlk - 4 * half;
        // DOC: only a block that straddles a boundary (wave-uniform test) has
        // keys below doc_start of some row. Their scores become -inf there, so
        // the loop below, unchanged, gives them P = exp(-inf) = 0 and dS = 0.
        // The rows' doc_start come from the wave's LDS copy, four consecutive
        // rows per 16-B read.
        if constexpr (DOC) {
          if (doc_block_straddles(kb0, ds_w1)) {
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) {
              const int4 d4 =
                  *reinterpret_cast<const int4*>(&sm.ds_row[wave][c_row(4 * r4, half)]);
              if (!doc_visible(kg, d4.x)) s_acc[4 * r4] = -INFINITY;
              if (!doc_visible(kg, d4.y)) s_acc[4 * r4 + 1] = -INFINITY;
              if (!doc_visible(kg, d4.z)) s_acc[4 * r4 + 2] = -INFINITY;
              if (!doc_visible(kg, d4.w)) s_acc[4 * r4 + 3] = -INFINITY;
            }
          }
        }
#pragma unroll
        for (int rg = 0; rg < 16; rg++) {
          const bool valid = !causal || (c_row(rg, 0) >= kq);
          const float p = valid ? __expf(scale * s_acc[rg] - lse_row[rg]) : 0.0f;
          const float ds = p * (dp_acc[rg] - delta_row[rg]) * scale;
          *reinterpret_cast<bf16*>(pb + pb_row4_addr(rg >> 2, half, l31) +
                                   (rg & 3) * 64) = __float2bfloat16(ds);
        }

        bf16x8_vec pbf[2];
#pragma unroll
        for (int h2 = 0; h2 < 2; h2++) pbf[h2] = pb_afrag(pb, h2, half, l31);

        // dQ += dS K — K B-fragments by hardware transpose, pipelined one
        // iteration ahead; dt fastest rotates the four accumulators
        const unsigned s_base = a_base + (s * 32) * 32;
        unsigned long long fk0[2], fk1[2];
        TR_READ(fk0[0], s_base);
        TR_READ(fk1[0], s_base + 128);
#pragma unroll
        for (int it = 0; it < 8; it++) {
          const int dt = it & 3;
          const int h2 = it >> 2;
          const int cur2 = it & 1;
          const int nxt = cur2 ^ 1;
          if (it < 7) {
            const unsigned nbase = Tile<64>::tr_step_off((it + 1) & 3, (it + 1) >> 2);
            TR_READ(fk0[nxt], s_base + nbase);
            TR_READ(fk1[nxt], s_base + nbase + 128);
            TR_WAIT2_KEEP(2, fk0[cur2], fk1[cur2]);
          } else {
            TR_WAIT2_KEEP(0, fk0[cur2], fk1[cur2]);
          }
          dq_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              pbf[h2], tr_join(fk0[cur2], fk1[cur2]), dq_acc[dt], 0, 0, 0);
        }
      }
    }
    if (more) write_tiles(&sm.k_img[cur ^ 1], &sm.v_img[cur ^ 1], pre);
    // One barrier per tile: img[cur^1] was last read in iteration j-1, and
    // every wave finished those reads before it passed that barrier.
    __syncthreads();
  }

  if (!active) return;
#pragma unroll
  for (int dt = 0; dt < 4; dt++) {
#pragma unroll
    for (int rg = 0; rg < 16; rg++) {
      dq[row_off(b, hq, ib * kFaBlk + c_row(rg, half), Hq, S, bshd) + dt * 32 +
         l31] = __float2bfloat16(dq_acc[dt][rg]);
    }
  }
}


// delta = rowsum(dout * out) in fp32 — the FA2 backward's D_i term, one
// fused pass over the two bf16 tensors (the torch expression materialized
// fp32 copies of both). One wave per row, 16 B/lane loads.
__global__ void fa_delta_kernel(const bf16* __restrict__ dout,
                                const bf16* __restrict__ o,
                                float* __restrict__ delta, int64_t rows,
                                int Hq, int S, int bshd) {
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  // delta is dense [B,Hq,S]; with bshd storage the flat row order is
  // (b, s, h), so remap the output index
  int64_t didx = row;
  if (bshd) {
    const int h = (int)(row % Hq);
    const int64_t bs = row / Hq;
    const int s = (int)(bs % S);
    const int64_t bb = bs / S;
    didx = (bb * Hq + h) * S + s;
  }
  // 64 lanes x 2 contiguous bf16 cover the D=128 row
  const __hip_bfloat162 d2 =
      *reinterpret_cast<const __hip_bfloat162*>(dout + row * kFaD + lane * 2);
  const __hip_bfloat162 o2 =
      *reinterpret_cast<const __hip_bfloat162*>(o + row * kFaD + lane * 2);
  float2 df = __bfloat1622float2(d2);
  float2 of = __bfloat1622float2(o2);
  float v = df.x * of.x + df.y * of.y;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if (lane == 0) delta[didx] = v;
}

void launch_fa_delta(const void* dout, const void* o, float* delta,
                     int64_t rows, int Hq, int S, bool bshd,
                     hipStream_t stream) {
  const int waves_per_wg = 8;
  const int64_t nwg = (rows + waves_per_wg - 1) / waves_per_wg;
  hipLaunchKernelGGL(fa_delta_kernel, dim3((uint32_t)nwg), dim3(waves_per_wg * 64),
                     0, stream, (const bf16*)dout, (const bf16*)o, delta, rows,
                     Hq, S, bshd ? 1 : 0);
}

// ---- launchers ------------------------------------------------------------

void launch_fa_bwd(const void* q, const void* k, const void* v, const void* dout,
                   const float* lse, const float* delta, void* dq, void* dk,
                   void* dv, int B, int Hq, int Hkv, int S, float scale,
                   bool causal, bool bshd, const int* doc_start, const int* doc_end,
                   hipStream_t stream) {
  const int nblk = (S + kFaBlk * kFaWaves - 1) / (kFaBlk * kFaWaves);
  if (doc_start != nullptr && doc_end != nullptr) {
    hipLaunchKernelGGL((fa_bwd_dkdv_kernel<true, const int*, const int*>),
                       dim3(nblk, B * Hkv), dim3(kFaThreads), 0, stream, (const bf16*)q,
                       (const bf16*)k, (const bf16*)v, (const bf16*)dout, lse, delta,
                       (bf16*)dk, (bf16*)dv, B, Hq, Hkv, S, scale, 1, bshd ? 1 : 0,
                       doc_start, doc_end);
    hipLaunchKernelGGL((fa_bwd_dq_kernel<true, const int*>), dim3(nblk, B * Hq),
                       dim3(kFaThreads), 0, stream, (const bf16*)q, (const bf16*)k,
                       (const bf16*)v, (const bf16*)dout, lse, delta, (bf16*)dq, B, Hq,
                       Hkv, S, scale, 1, bshd ? 1 : 0, doc_start);
    return;
  }
  hipLaunchKernelGGL(fa_bwd_dkdv_kernel<false>, dim3(nblk, B * Hkv), dim3(kFaThreads), 0,
                     stream, (const bf16*)q, (const bf16*)k, (const bf16*)v,
                     (const bf16*)dout, lse, delta, (bf16*)dk, (bf16*)dv, B, Hq,
                     Hkv, S, scale, causal ? 1 : 0, bshd ? 1 : 0);
  hipLaunchKernelGGL(fa_bwd_dq_kernel<false>, dim3(nblk, B * Hq), dim3(kFaThreads), 0,
                     stream, (const bf16*)q, (const bf16*)k, (const bf16*)v,
                     (const bf16*)dout, lse, delta, (bf16*)dq, B, Hq, Hkv, S,
                     scale, causal ? 1 : 0, bshd ? 1 : 0);
}

}  // namespace torchft_amd
