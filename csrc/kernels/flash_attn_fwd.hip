// Flash-attention FORWARD for CDNA4 (gfx950) — bf16, D=128, causal+full,
// GQA-native. Produces O and the logsumexp the in-tree backward consumes
// (P = exp(scale*S - LSE)), replacing aten/aotriton's attn_fwd.
//
// Structure (guide §B "fused attention prefill", adapted):
//   grid (S/256, B*Hq); one 512-thread workgroup = 8 waves, wave w owns
//   q rows [Q0 + 32w, +32) of one query head. K/V stream through
//   double-buffered LDS tiles of KVBLK=64 keys, staged cooperatively and
//   SHARED by all 8 waves (same kv head under GQA).
//
//   Swapped QK^T: S_blk = mfma(A=K, B=Q^T) puts q in the MFMA column
//   (lane l31 = its q row), so the whole online softmax — running max m,
//   denominator l, P = exp(scale*s - m) — is lane-local per q: the lane
//   pair (l, l+32) holds the 2x16 key rows of one q and combines via
//   permlane32_swap. P converts to the PV A-fragment in-register with
//   v_cvt_pk_bf16_f32 + permlane32_swap (no LDS round trip, T12).
//
//   PV: B-fragments of V by ds_read_b64_tr_b16 hardware-transpose reads
//   from the row-major subtiled V image (the bwd kernel's recipe; probe:
//   tr16_probe.hip). O accumulates [16 q-rows][d=l31] per 32-d tile.
//
//   Online-softmax rescale: O's rows are q = c_row(reg) while m/l live at
//   lane q = l31, so a rescale needs an alpha broadcast through LDS. With
//   the defer-max threshold (T13, THR=8 in scaled-score units) the branch
//   is rare: the common path multiplies nothing. At a rescale EVERYTHING
//   still at the old max is scaled exactly once: the decision happens
//   before this block's P is exponentiated, and l folds alpha in the same
//   update (l = l*alpha + sum_p).
//
//   Document mask (DOC variant): causal within the documents of a packed
//   row. Key tiles outside the workgroup's / wave's documents are not
//   streamed or computed; the per-element test runs only in blocks that
//   straddle a boundary (bounds: fa_layout.h; docs/KERNELS.md).
//
// MFMA lane mappings (mfma_probe.hip):
//   A: row=lane&31, k=(lane>>5)*8+m   B: k=(lane>>5)*8+m, col=lane&31
//   C/D: col=lane&31, row=(reg&3)+8*(reg>>2)+4*(lane>>5)

#include <hip/hip_runtime.h>

#include "fa_tile.h"

namespace torchft_amd {

constexpr int kFwdKvBlk = 64;       // keys per staged K/V tile
constexpr float kFwdThr = 11.54f;   // defer-max threshold: 8 nats in log2 units
constexpr float kLog2e = 1.44269504089f;

// K/V tiles are Tile<64> (fa_layout.h), staged by the shared T14 stream of
// fa_tile.h: the loads issue an iteration EARLY (under the previous tile's
// MFMA phase, hiding the HBM latency); the writes land after the barrier
// that frees the buffer.
struct SmemFwd {
  Tile<64> k_img[2];
  Tile<64> v_img[2];
  alignas(16) float bcast[kFaWaves][32];  // alpha / 1/l broadcasts
};

// K A-fragment of 32-key block s of the staged tile: row = key s*32 + l31,
// k-dim = d slice tt. The row is formed here and not at the call site, where
// s*32 is shared with the causal test and the register assignment shifts
// (docs/KERNELS.md, attention tile geometry).
__device__ inline bf16x8_vec k_afrag(const unsigned char* img, int tt, int s, int half,
                                     int l31) {
  return rm_frag<64>(img, tt, s * 32 + l31, half);
}

// pack two f32 into one dword of 2 bf16 (no builtin on gfx950 — T12).
// The trailing s_nop provides the 2 wait states a later v_permlane32_swap
// needs after a VALU write of its operand — the compiler's hazard
// recognizer cannot see inside this asm (T21 hazard note).
__device__ inline unsigned cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2\n\ts_nop 1" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// exchange the 32-lane halves of two dwords (see T21):
// r0 = [a(0:31) | b(0:31)], r1 = [a(32:63) | b(32:63)]
__device__ inline void half_swap(unsigned& a, unsigned& b) {
  auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  a = r[0];
  b = r[1];
}

__device__ inline float half_combine_max(float v) {
  unsigned a = __float_as_uint(v), b = a;
  half_swap(a, b);
  return fmaxf(__uint_as_float(a), __uint_as_float(b));
}

__device__ inline float half_combine_sum(float v) {
  unsigned a = __float_as_uint(v), b = a;
  half_swap(a, b);
  return __uint_as_float(a) + __uint_as_float(b);
}

// DOC: the document-mask variant (docs/KERNELS.md, "document mask"). Its one
// extra argument, doc_start (int32 [B,S]), rides in the trailing pack so that
// the plain instantiation keeps its parameter list and its code.
template <bool DOC, class... DocP>
__global__ __launch_bounds__(kFaThreads, 1) void fa_fwd_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, bf16* __restrict__ out,
    float* __restrict__ lse, int B, int Hq, int Hkv, int S, float scale,
    int causal, int bshd, DocP... docp) {
  static_assert(sizeof...(DocP) == (DOC ? 1 : 0), "DOC takes doc_start");
  __shared__ SmemFwd sm;
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

  const int Q0 = wg.x * (kFaWaves * kFaBlk);
  const int my_q0 = Q0 + wave * kFaBlk;       // this wave's 32 q rows
  const int q_glob = my_q0 + l31;               // this lane's q row
  const bool active = my_q0 < S;

  // Q block in registers: lane holds Q[q_glob][tt*16 + half*8 .. +8]
  const int64_t lse_head = ((int64_t)b * Hq + hq) * S;  // lse is dense BHS
  bf16x8_vec qfrag[8];
  if (active) {
    const int64_t q_off = row_off(b, hq, q_glob, Hq, S, bshd);
#pragma unroll
    for (int tt = 0; tt < 8; tt++) {
      qfrag[tt] =
          *reinterpret_cast<const bf16x8_vec*>(q + q_off + tt * 16 + half * 8);
    }
  }

  const bf16* k_base = k + row_off(b, hkv, 0, Hkv, S, bshd);
  const bf16* v_base = v + row_off(b, hkv, 0, Hkv, S, bshd);
  const int64_t kv_ld = bshd ? (int64_t)Hkv * kFaD : kFaD;

  // number of KV tiles this WORKGROUP must stage
  const int kv_hi = causal ? min(S, Q0 + kFaWaves * kFaBlk) : S;
  const int nT = (kv_hi + kFwdKvBlk - 1) / kFwdKvBlk;

  // DOC: the workgroup streams from the tile that holds doc_start of its
  // first row; a wave skips the blocks below doc_start of its own first row
  // (ds_w0) and masks per element only below that of its last row (ds_w1).
  // The lane's q is its MFMA column, so the element test is lane-local.
  int j0 = 0, ds_q = 0, ds_w0 = 0, ds_w1 = 0;
  if constexpr (DOC) {
    const int* doc_start = doc_ptr<0>(docp...) + (int64_t)b * S;
    j0 = doc_first_tile(doc_start[Q0], nT);
    if (active) ds_q = doc_start[q_glob];
    ds_w0 = __builtin_amdgcn_readlane(ds_q, 0);
    ds_w1 = __builtin_amdgcn_readlane(ds_q, 31);
  }

  f32x16 o_acc[4] = {};
  // softmax runs in the log2 domain: m2 = max of (scale*log2e)*s, powers
  // of two via the native v_exp, one fma per element (exp2+fma fold)
  const float c2 = scale * kLog2e;
  float m_run = -1e30f;
  float l_run = 0.f;

  // the second-dispatched wave half loses VALU arbitration on every
  // segment; one static priority raise for it (T5 static form — the
  // condition must be provably wave-uniform or s_setprio goes under exec)
  if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= 256) {
    __builtin_amdgcn_s_setprio(1);
  }

  const unsigned tr_off = Tile<64>::tr_lane_off(lane);
  float* bc = sm.bcast[wave];

  TileRegs<64> staged =  // tile 0 (DOC: the first tile needed)
      DOC ? load_tiles<64>(k_base + (int64_t)j0 * kFwdKvBlk * kv_ld,
                           v_base + (int64_t)j0 * kFwdKvBlk * kv_ld, kv_ld)
          : load_tiles<64>(k_base, v_base, kv_ld);
  for (int j = DOC ? j0 : 0; j < nT; j++) {
    const int cur = j & 1;
    write_tiles(&sm.k_img[cur], &sm.v_img[cur], staged);
    __syncthreads();
    if (j + 1 < nT) {
      // issue the next tile's global loads now — they retire under this
      // tile's MFMA phase and are waited for by the write after the
      // next barrier (compiler-counted vmcnt)
      staged = load_tiles<64>(k_base + (int64_t)(j + 1) * kFwdKvBlk * kv_ld,
                       v_base + (int64_t)(j + 1) * kFwdKvBlk * kv_ld, kv_ld);
    }

    const int key0 = j * kFwdKvBlk;
    // this wave needs the tile only if some of its keys are visible
    if (active && (!causal || key0 <= my_q0 + kFaBlk - 1) &&
        !(DOC && doc_block_skipped(key0 + 32, ds_w0))) {
      const unsigned char* kimg = sm.k_img[cur].sub;
      const unsigned v_img_base = (unsigned)(uintptr_t)sm.v_img[cur].sub + tr_off;

#pragma unroll
      for (int s = 0; s < 2; s++) {  // two 32-key blocks per tile
        const int kb0 = key0 + s * 32;
        if (causal && kb0 > my_q0 + kFaBlk - 1) break;
        if (DOC && doc_block_skipped(kb0, ds_w0)) continue;

        f32x16 s_acc = {};
#pragma unroll
        for (int tt = 0; tt < 8; tt++) {
          s_acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              k_afrag(kimg, tt, s, half, l31), qfrag[tt], s_acc, 0, 0, 0);
        }

        // raw scores + causal mask; per-lane block max over its q.
        // One multiply converts the max to the log2 domain (c2 > 0
        // preserves order); each element pays a single fma inside exp2.
        const bool diag = causal && (kb0 + 31 > q_glob);
        float p[16];
        float bmax = -1e30f;
#pragma unroll
        for (int r = 0; r < 16; r++) {
          float sv = s_acc[r];
          if (diag && (kb0 + c_row(r, half) > q_glob)) sv = -1e30f;
          p[r] = sv;
          bmax = fmaxf(bmax, sv);
        }
        // DOC: the document test, only in the blocks that straddle a boundary
        // (wave-uniform branch: the other blocks run the causal code)
        bool dstr = false;
        if constexpr (DOC) dstr = doc_block_straddles(kb0, ds_w1);
        if (dstr) {
          bmax = -1e30f;
#pragma unroll
          for (int r = 0; r < 16; r++) {
            if (!doc_visible(kb0 + c_row(r, half), ds_q)) p[r] = -1e30f;
            bmax = fmaxf(bmax, p[r]);
          }
        }
        bmax = half_combine_max(bmax);  // both 16-key halves of this q
        // DOC: a row with no visible key in this block (its document starts
        // further down the wave's rows) must not move: without the guard a
        // row that has seen nothing yet would take m = -1e30 * c2 and give
        // its masked keys exp2(0) = 1. Its bmax stands in as m_run (no
        // rescale request, alpha = 1 if another row asks) and its P is 0.
        // Causality alone leaves every row of a streamed block its key kb0.
        const bool dead = dstr && bmax <= -1e30f;
        bmax = dead ? m_run : bmax * c2;

        // defer-max: rescale O only when the max moved past THR
        float m_use = m_run;
        if (!__all(bmax - m_run <= kFwdThr)) {
          const float m_new = fmaxf(m_run, bmax);
          const float alpha = exp2f(m_run - m_new);  // 0 on first tile
          // broadcast alpha to O's row layout and rescale
          if (half == 0) bc[l31] = alpha;
          __builtin_amdgcn_wave_barrier();
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
          for (int dt = 0; dt < 4; dt++) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
              o_acc[dt][r] *= bc[c_row(r, half)];
            }
          }
          l_run *= alpha;
          m_run = m_new;
          m_use = m_new;
        }

        // P = exp(s - m) (bounded by e^THR on the defer path), row sum,
        // and bf16 A-fragments for PV via cvt_pk + half swaps
        float psum = 0.f;
        unsigned pk[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
          const float e0 = exp2f(fmaf(p[2 * i], c2, -m_use));
          const float e1 = exp2f(fmaf(p[2 * i + 1], c2, -m_use));
          psum += e0 + e1;
          pk[i] = cvt_pk_bf16(e0, e1);
        }
        if (dstr && dead) {  // whatever exp2 made of the sentinels
          psum = 0.f;
#pragma unroll
          for (int i = 0; i < 8; i++) pk[i] = 0u;
        }
        l_run += half_combine_sum(psum);

        // assemble A-fragments: lane needs P[q][keys (l>>5)*8 + 0..7] per
        // 16-key step h2; own regs hold keys c_row(r,half) — pair halves
        // swap so [pk0,pk2',pk1,pk3'] become consecutive key pairs
        half_swap(pk[0], pk[2]);  // keys {0,1}|{8,9} <-> {4,5}|{12,13}
        half_swap(pk[1], pk[3]);  // keys {2,3}|{10,11} <-> {6,7}|{14,15}
        half_swap(pk[4], pk[6]);  // second 16-key step
        half_swap(pk[5], pk[7]);
        union {
          unsigned u[4];
          bf16x8_vec v;
        } pa0, pa1;
        pa0.u[0] = pk[0];
        pa0.u[1] = pk[1];
        pa0.u[2] = pk[2];
        pa0.u[3] = pk[3];
        pa1.u[0] = pk[4];
        pa1.u[1] = pk[5];
        pa1.u[2] = pk[6];
        pa1.u[3] = pk[7];

        // PV: V B-fragments by hardware transpose; k-dim = 16 keys per
        // h2. dt fastest so consecutive MFMAs rotate the four O
        // accumulators (dependent-latency hiding; see bwd kernels).
#pragma unroll
        for (int it = 0; it < 8; it++) {
          const int dt = it & 3;
          const int h2 = it >> 2;
          const unsigned base =
              v_img_base + Tile<64>::tr_step_off(dt, h2) + (s * 32) * 32;
          unsigned long long t0, t1;
          TR_READ(t0, base);
          TR_READ(t1, base + 128);
          TR_WAIT2_KEEP(0, t0, t1);
          o_acc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
              h2 ? pa1.v : pa0.v, tr_join(t0, t1), o_acc[dt], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  if (!active) return;

  // epilogue: O /= l (l lives at lane q=l31; O rows are c_row) and store.
  // bc is wave-private and the write/read are same-wave DS ops, ordered by
  // the LDS pipeline — no barrier (and a workgroup barrier would deadlock:
  // inactive waves returned above).
  if (half == 0) bc[l31] = 1.f / l_run;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int dt = 0; dt < 4; dt++) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int row = c_row(r, half);
      out[row_off(b, hq, my_q0 + row, Hq, S, bshd) + dt * 32 + l31] =
          __float2bfloat16(o_acc[dt][r] * bc[row]);
    }
  }
  if (half == 0) {
    // convert the log2-domain state back to the natural-log lse the
    // backward consumes: lse = ln2 * (m2 + log2(l))
    lse[lse_head + q_glob] = 0.6931471805599453f * (m_run + __log2f(l_run));
  }
}

void launch_fa_fwd(const void* q, const void* k, const void* v, void* out,
                   float* lse, int B, int Hq, int Hkv, int S, float scale,
                   bool causal, bool bshd, const int* doc_start, const int* doc_end,
                   hipStream_t stream) {
  const int rows_per_wg = kFaWaves * kFaBlk;
  const int nblk = (S + rows_per_wg - 1) / rows_per_wg;
  (void)doc_end;  // the forward is query-centric: doc_start says it all
  if (doc_start != nullptr) {
    hipLaunchKernelGGL((fa_fwd_kernel<true, const int*>), dim3(nblk, B * Hq),
                       dim3(kFaThreads), 0, stream, (const bf16*)q, (const bf16*)k,
                       (const bf16*)v, (bf16*)out, lse, B, Hq, Hkv, S, scale, 1,
                       bshd ? 1 : 0, doc_start);
    return;
  }
  hipLaunchKernelGGL(fa_fwd_kernel<false>, dim3(nblk, B * Hq), dim3(kFaThreads), 0,
                     stream, (const bf16*)q, (const bf16*)k, (const bf16*)v,
                     (bf16*)out, lse, B, Hq, Hkv, S, scale, causal ? 1 : 0,
                     bshd ? 1 : 0);
}

}  // namespace torchft_amd
