// Stand-alone check of the document-mask bounds (fa_layout.h): the first key
// tile of the forward and dq, the last query tile of dkdv, the per-wave skip
// and straddle tests and the per-element tests, walked over the same loops the
// three kernels run. For layouts a DocMask would build, the elements the
// kernels keep are exactly the visible ones (doc_start[i] <= j <= i), so no
// visible pair is skipped and no hidden one is kept. For arbitrary int32
// contents, every tile index stays inside the causal kernel's range and no
// arithmetic overflows. No torch, no HIP; tests/test_doc_bounds.py builds it
// with the address and undefined-behaviour sanitizers and runs it.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../fa_layout.h"

namespace tft = torchft_amd;

namespace {

int failures = 0;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      if (failures < 20)                                             \
        std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      failures++;                                                    \
    }                                                                \
  } while (0)

constexpr int kBlk = tft::kFaBlk, kWaves = tft::kFaWaves, kWg = kBlk * kWaves;

struct Layout {
  int S;
  std::vector<int> ds, de;  // doc_start, doc_end
};

// kept[q * S + key]: how often a kernel kept (did not mask) the element
using Kept = std::vector<int>;

// the forward (kv64 = key tile of 64, a wave's lane holds one q) and dq (same
// bounds, rows in the C registers): both walk key tiles per 256-row workgroup
void walk_q_centric(const Layout& L, bool fwd, Kept* kept) {
  const int S = L.S;
  const int nblk = (S + kWg - 1) / kWg;
  for (int x = 0; x < nblk; x++) {
    const int Q0 = x * kWg;
    const int kv_hi = S < Q0 + kWg ? S : Q0 + kWg;
    const int nT = (kv_hi + 63) / 64;
    CHECK(Q0 < S && nT >= 1);
    const int j0 = tft::doc_first_tile(L.ds[Q0], nT);
    CHECK(j0 >= 0 && j0 <= nT - 1);
    for (int j = j0; j < nT; j++) {
      // the staged tile lies inside the tensor
      CHECK(j >= 0 && j * 64 + 64 <= S);
      for (int w = 0; w < kWaves; w++) {
        const int q0 = Q0 + w * kBlk;
        if (q0 >= S) continue;  // inactive wave
        const int ds_w0 = L.ds[q0], ds_w1 = L.ds[q0 + kBlk - 1];
        const int key0 = j * 64;
        if (key0 > q0 + kBlk - 1) continue;
        if (tft::doc_block_skipped(key0 + 32, ds_w0)) continue;
        for (int s = 0; s < 2; s++) {
          const int kb0 = key0 + s * 32;
          if (kb0 > q0 + kBlk - 1) break;
          if (tft::doc_block_skipped(kb0, ds_w0)) continue;
          const bool straddles = tft::doc_block_straddles(kb0, ds_w1);
          for (int half = 0; half < 2; half++)
            for (int l31 = 0; l31 < 32; l31++)
              for (int rg = 0; rg < 16; rg++) {
                // forward: lane = q, register = key; dq: the other way round
                const int q = q0 + (fwd ? l31 : tft::c_row(rg, half));
                const int key = kb0 + (fwd ? tft::c_row(rg, half) : l31);
                bool valid = key <= q;
                if (straddles && !tft::doc_visible(key, L.ds[q])) valid = false;
                if (valid && kept) (*kept)[(size_t)q * S + key]++;
              }
        }
      }
    }
  }
}

// dkdv: query tiles of 32 per 256-key workgroup, G query heads flattened
void walk_dkdv(const Layout& L, int G, Kept* kept) {
  const int S = L.S;
  const int nQ = S / kBlk;
  const int nblk = (S + kWg - 1) / kWg;
  for (int x = 0; x < nblk; x++) {
    const int i_min = x * kWaves;
    CHECK(i_min < nQ);
    const int wg_last = (S < (x + 1) * kWg ? S : (x + 1) * kWg) - 1;
    const int i_hi = tft::doc_last_qtile(L.de[wg_last], i_min, nQ);
    CHECK(i_hi > i_min && i_hi <= nQ);
    const int nI = i_hi - i_min;
    for (int t = 0; t < G * nI; t++) {
      const int g = t / nI, i = i_min + t % nI;
      CHECK(g >= 0 && g < G && i >= i_min && i * kBlk + kBlk <= S);
      if (g != 0) continue;  // the heads repeat the same tiles
      for (int w = 0; w < kWaves; w++) {
        const int jb = i_min + w;
        if (jb * kBlk >= S) continue;
        const int de_w = L.de[jb * kBlk + kBlk - 1];
        if (i < jb || tft::doc_qtile_skipped(i, de_w)) continue;
        const bool straddles = tft::doc_qtile_straddles(L.ds[i * kBlk + kBlk - 1], jb);
        for (int half = 0; half < 2; half++)
          for (int l31 = 0; l31 < 32; l31++) {
            const int q = i * kBlk + l31;
            const int qk = (i - jb) * kBlk + l31 - 4 * half;
            const int dsk = tft::fa_clamp(L.ds[q], 0, S) - jb * kBlk - 4 * half;
            for (int rg = 0; rg < 16; rg++) {
              const int key = jb * kBlk + tft::c_row(rg, half);
              const bool valid =
                  qk >= tft::c_row(rg, 0) && !(straddles && tft::c_row(rg, 0) < dsk);
              if (valid && kept) (*kept)[(size_t)q * S + key]++;
            }
          }
      }
    }
  }
}

Layout from_lengths(const std::vector<int>& lens) {
  Layout L;
  L.S = 0;
  for (int n : lens) L.S += n;
  int at = 0;
  for (int n : lens) {
    for (int p = 0; p < n; p++) {
      L.ds.push_back(at);
      L.de.push_back(at + n);
    }
    at += n;
  }
  return L;
}

void check_exact(const Layout& L) {
  const int S = L.S;
  for (int kernel = 0; kernel < 3; kernel++) {
    if (kernel == 0 && S % 256 != 0) continue;  // the forward needs S % 256 == 0
    Kept kept((size_t)S * S, 0);
    if (kernel < 2) {
      walk_q_centric(L, kernel == 0, &kept);
    } else {
      walk_dkdv(L, 3, &kept);
    }
    int wrong = 0;
    for (int q = 0; q < S; q++)
      for (int key = 0; key < S; key++) {
        const bool visible = L.ds[q] <= key && key <= q;
        // the mirror rule describes the same set
        if (visible != (key <= q && q < L.de[key])) wrong++;
        if (kept[(size_t)q * S + key] != (visible ? 1 : 0)) wrong++;
      }
    CHECK(wrong == 0);
  }
}

void check_monotone(std::mt19937& rng) {
  const std::vector<std::vector<int>> fixed = {
      {256}, {1, 31, 32, 33, 63, 96}, {5, 251}, {256, 256}, {300, 212},
      {64, 64, 64, 64, 64, 64, 64, 64}, {128}, {1, 127}, {127, 1}, {383, 1},
      {255, 1, 256}, {1, 1, 1, 1, 124, 256, 384}, {768}};
  for (const auto& lens : fixed) check_exact(from_lengths(lens));
  for (int trial = 0; trial < 60; trial++) {
    const int S = 128 * (1 + (int)(rng() % 8));
    std::vector<int> lens;
    int left = S;
    while (left > 0) {
      const int cap = (rng() % 3 == 0) ? 40 : 400;
      int n = 1 + (int)(rng() % cap);
      if (n > left) n = left;
      lens.push_back(n);
      left -= n;
    }
    check_exact(from_lengths(lens));
  }
}

void check_garbage(std::mt19937& rng) {
  const int extremes[] = {INT_MIN, INT_MIN + 1, -1, 0, 1, INT_MAX - 1, INT_MAX, 1 << 30,
                          -(1 << 30), 63, 64, 65, 255, 256, 257};
  const int n_ext = (int)(sizeof(extremes) / sizeof(extremes[0]));
  for (int trial = 0; trial < 60; trial++) {
    Layout L;
    L.S = 128 * (1 + (int)(rng() % 6));
    for (int p = 0; p < L.S; p++) {
      auto draw = [&]() -> int {
        switch (rng() % 3) {
          case 0: return extremes[rng() % n_ext];
          case 1: return (int)(rng() % (2 * L.S)) - L.S / 2;
          default: return (int)rng();
        }
      };
      L.ds.push_back(draw());
      L.de.push_back(draw());
    }
    // the CHECKs inside the walks hold the bounds to the causal ranges; the
    // kept elements are unspecified
    if (L.S % 256 == 0) walk_q_centric(L, true, nullptr);
    walk_q_centric(L, false, nullptr);
    walk_dkdv(L, 2, nullptr);
  }
}

void check_functions() {
  // clamped into the causal range for every input
  for (int nT : {1, 2, 4, 128}) {
    CHECK(tft::doc_first_tile(INT_MIN, nT) == 0);
    CHECK(tft::doc_first_tile(-1, nT) == 0);
    CHECK(tft::doc_first_tile(63, nT) == 0);
    CHECK(tft::doc_first_tile(64, nT) == (nT > 1 ? 1 : 0));
    CHECK(tft::doc_first_tile(INT_MAX, nT) == nT - 1);
  }
  CHECK(tft::doc_last_qtile(INT_MIN, 8, 16) == 9);
  CHECK(tft::doc_last_qtile(INT_MAX, 8, 16) == 16);
  CHECK(tft::doc_last_qtile(257, 8, 16) == 9);
  CHECK(tft::doc_last_qtile(288, 8, 16) == 9);
  CHECK(tft::doc_last_qtile(289, 8, 16) == 10);
  CHECK(tft::doc_last_qtile(512, 0, 16) == 16);
  CHECK(tft::doc_block_skipped(0, 32) && !tft::doc_block_skipped(0, 31));
  CHECK(!tft::doc_block_skipped(32, INT_MIN) && tft::doc_block_skipped(32, INT_MAX));
  CHECK(tft::doc_block_straddles(32, 33) && !tft::doc_block_straddles(32, 32));
  CHECK(tft::doc_qtile_skipped(2, 64) && !tft::doc_qtile_skipped(2, 65));
  CHECK(tft::doc_qtile_skipped(0, INT_MIN) && !tft::doc_qtile_skipped(0, INT_MAX));
}

}  // namespace

int main() {
  std::mt19937 rng(20261021);
  check_functions();
  check_monotone(rng);
  check_garbage(rng);
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("fa doc bounds ok\n");
  return 0;
}
