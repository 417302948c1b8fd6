// Stand-alone check of the rectangular-attention bounds (fa_layout.h), walked
// over the loops and the shifted wave tests of the three RECT kernels for
// Sq <= Sk in {256, ..., 2048}, causal and full: the kept elements are exactly
// the visible ones (key <= q + Sk - Sq), every staged tile and statistic lies
// inside its tensor, every key has a visible query, and the tile counts are
// ordered the way fa_wg_order deals the blocks. No torch, no HIP;
// tests/test_fa_rect_bounds.py builds it under ASan + UBSan and runs it.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../fa_layout.h"

namespace tft = torchft_amd;

static int failures = 0;
#define CHECK(cond) \
  do { \
    if (!(cond) && failures++ < 20) std::printf("line %d: CHECK(%s) failed\n", __LINE__, #cond); \
  } while (0)

constexpr int kBlk = tft::kFaBlk, kWaves = tft::kFaWaves, kWg = kBlk * kWaves;

// n[q * Sk + key]: how often a kernel kept (did not mask) the element
struct Kept {
  int Sq, Sk;
  std::vector<uint8_t> n;
  void add(int q, int key) {
    CHECK(q >= 0 && q < Sq && key >= 0 && key < Sk);
    n.at((size_t)q * Sk + key)++;
  }
};

// forward (a lane holds one q; keys counted from the diagonal's origin) and dq
// (rows in the C registers; the wave's rows moved onto the keys)
static void walk_q_centric(bool fwd, bool causal, Kept& kept) {
  const int Sq = kept.Sq, Sk = kept.Sk, off = Sk - Sq;
  for (int x = 0, before = 0; x < Sq / kWg; x++) {
    const int nT = (tft::rect_kv_end(x * kWg, off, Sk, causal) + 63) / 64;
    CHECK(nT >= 1 && nT >= before && nT * 64 <= Sk);  // inside k / v; heavy at x = nx - 1
    before = nT;
    for (int j = 0; j < nT; j++)
      for (int w = 0; w < kWaves; w++) {
        const int q0 = x * kWg + w * kBlk;
        const int key0 = fwd ? j * 64 - off : j * 64, row0 = fwd ? q0 : q0 + off;
        for (int s = 0; s < 2; s++) {
          const int kb0 = key0 + s * 32;
          if (causal && kb0 > row0 + kBlk - 1) break;
          for (int half = 0; half < 2; half++)
            for (int l31 = 0; l31 < 32; l31++)
              for (int rg = 0; rg < 16; rg++) {
                const int cr = tft::c_row(rg, half);
                if (fwd) {
                  const bool diag = causal && kb0 + 31 > q0 + l31;
                  if (!(diag && kb0 + cr > q0 + l31)) kept.add(q0 + l31, kb0 + cr + off);
                } else if (!causal || tft::c_row(rg, 0) >= kb0 + l31 - row0 - 4 * half) {
                  kept.add(q0 + cr, kb0 + l31);
                }
              }
        }
      }
  }
}

// dkdv: query tiles of 32 per 256-key workgroup, G query heads flattened
static void walk_dkdv(bool causal, int G, Kept& kept) {
  const int Sq = kept.Sq, Sk = kept.Sk, off = Sk - Sq, nQ = Sq / kBlk;
  for (int x = 0, before = nQ; x < Sk / kWg; x++) {
    const int i_min = tft::rect_first_qtile(x, off, causal), nI = nQ - i_min;
    CHECK(i_min >= 0 && nI >= 1 && nI <= before);  // heavy at x = 0
    before = nI;
    for (int t = 0; t < G * nI; t++) {
      const int g = t / nI, i = i_min + t % nI;
      // the staged q / dout tile and the lse / delta rows beside it
      CHECK(g < G && i * kBlk + kBlk <= Sq && (int64_t)g * Sq + i * kBlk + 31 < (int64_t)G * Sq);
      for (int w = 0; g == 0 && w < kWaves; w++) {  // the heads repeat the tiles
        const int jb = x * kWaves + w, jbq = jb - off / kBlk;
        if (causal && i < jbq) continue;
        for (int half = 0; half < 2; half++)
          for (int l31 = 0; l31 < 32; l31++)
            for (int rg = 0; rg < 16; rg++)
              if (!causal || (i - jbq) * kBlk + l31 - 4 * half >= tft::c_row(rg, 0))
                kept.add(i * kBlk + l31, jb * kBlk + tft::c_row(rg, half));
      }
    }
  }
}

int main() {
  // Sq = 512 against Sk = 768: the key blocks start at query tiles 0, 0, 8
  CHECK(tft::rect_first_qtile(0, 256, true) == 0 && tft::rect_first_qtile(1, 256, true) == 0 &&
        tft::rect_first_qtile(2, 256, true) == 8 && tft::rect_kv_end(0, 256, 768, true) == 512);
  for (int Sq = 256; Sq <= 2048; Sq += 256)
    for (int Sk = Sq; Sk <= 2048; Sk += 256)
      for (int causal = 0; causal < 2; causal++)
        for (int kernel = 0; kernel < 3; kernel++) {
          Kept kept{Sq, Sk, std::vector<uint8_t>((size_t)Sq * Sk, 0)};
          if (kernel < 2) walk_q_centric(kernel == 0, causal, kept);
          else walk_dkdv(causal, 3, kept);
          int wrong = 0;
          std::vector<int> seen(Sk, 0);  // dk / dv rows written from a query
          for (int q = 0; q < Sq; q++)
            for (int key = 0; key < Sk; key++) {
              const int visible = !causal || key <= q + Sk - Sq;
              wrong += kept.n[(size_t)q * Sk + key] != visible;
              seen[key] += kept.n[(size_t)q * Sk + key];
            }
          CHECK(wrong == 0);
          for (int key = 0; key < Sk; key++) CHECK(seen[key] >= 1);
        }
  std::printf(failures ? "%d check(s) failed\n" : "fa rect bounds ok\n", failures);
  return failures ? 1 : 0;
}
