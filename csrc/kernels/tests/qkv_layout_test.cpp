// Stand-alone check of the address map of the fused QKV split + rotary kernels
// (qkv_layout.h): the items of a token cover its row of the projection and the
// q / k / v tensors exactly once, 16 B-aligned, the two halves of an item D/2
// apart inside one head, and rope_pos_row stays inside the tables for any
// int32. No torch, no HIP; tests/test_qkv_layout.py builds it with the address
// and undefined-behaviour sanitizers and runs it.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../qkv_layout.h"

namespace tft = torchft_amd;

namespace {

int failures = 0;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      failures++;                                                    \
    }                                                                \
  } while (0)

// marks [off, off + 8) of a tensor of n elements; out of range is a failure
// and marks nothing
void mark8(std::vector<int>& hits, int64_t off) {
  CHECK(off >= 0 && off % tft::kQkvHalf == 0 && off + tft::kQkvHalf <= (int64_t)hits.size());
  if (off < 0 || off + tft::kQkvHalf > (int64_t)hits.size()) return;
  for (int m = 0; m < tft::kQkvHalf; m++) hits[(size_t)off + m]++;
}

void check_shape(int Hq, int Hkv, int D) {
  const int tokens = 3;
  const int W = (Hq + 2 * Hkv) * D;
  const int ipt = tft::qkv_items_per_token(Hq, Hkv, D);
  CHECK(ipt * tft::kQkvItem == W);
  CHECK(tft::qkv_items_per_head(D) * tft::kQkvItem == D);

  std::vector<int> packed((size_t)tokens * W, 0);
  std::vector<int> split[3] = {std::vector<int>((size_t)tokens * Hq * D, 0),
                               std::vector<int>((size_t)tokens * Hkv * D, 0),
                               std::vector<int>((size_t)tokens * Hkv * D, 0)};
  for (int64_t token = 0; token < tokens; token++)
    for (int it = 0; it < ipt; it++) {
      const int slot = tft::qkv_item_slot(it, D);
      const int col = tft::qkv_item_col(it, D);
      const int cls = tft::qkv_slot_class(slot, Hq, Hkv);
      const int head = tft::qkv_slot_head(slot, Hq, Hkv);
      CHECK(slot >= 0 && slot < Hq + 2 * Hkv);
      CHECK(col >= 0 && col % tft::kQkvHalf == 0 && col + tft::kQkvHalf <= D / 2);
      CHECK(cls == tft::kQkvQ || cls == tft::kQkvK || cls == tft::kQkvV);
      // q heads, then k heads, then v heads
      CHECK(cls == (slot < Hq ? tft::kQkvQ : slot < Hq + Hkv ? tft::kQkvK : tft::kQkvV));
      const int heads = tft::qkv_class_heads(cls, Hq, Hkv);
      CHECK(heads == (cls == tft::kQkvQ ? Hq : Hkv));
      CHECK(head >= 0 && head < heads);
      CHECK(slot == (cls == tft::kQkvQ ? 0 : cls == tft::kQkvK ? Hq : Hq + Hkv) + head);

      // in: the item's two halves lie in the token's row, inside one head,
      // D/2 apart
      const int64_t p = tft::qkv_packed_off(token, it, Hq, Hkv, D);
      CHECK(p == token * W + (int64_t)slot * D + col);
      CHECK(p / W == token && (p + D / 2 + tft::kQkvHalf - 1) / W == token);
      CHECK((p % W) / D == slot && ((p + D / 2 + tft::kQkvHalf - 1) % W) / D == slot);
      mark8(packed, p);
      mark8(packed, p + D / 2);

      // out: the same two halves of head `head` of token `token` in the
      // item's own tensor
      const int64_t o = tft::qkv_split_off(token, it, Hq, Hkv, D);
      CHECK(o == (token * heads + head) * (int64_t)D + col);
      mark8(split[cls], o);
      mark8(split[cls], o + D / 2);
    }
  for (int n : packed) CHECK(n == 1);
  for (auto& t : split)
    for (int n : t) CHECK(n == 1);
}

void check_large() {
  // no 32-bit overflow: the last item of token 2^31 at the model's head counts
  const int Hq = 32, Hkv = 8, D = 128;
  const int64_t token = (int64_t)1 << 31;
  const int ipt = tft::qkv_items_per_token(Hq, Hkv, D);
  CHECK(tft::qkv_packed_off(token, ipt - 1, Hq, Hkv, D) ==
        token * 48 * 128 + 47 * 128 + 56);
  CHECK(tft::qkv_split_off(token, ipt - 1, Hq, Hkv, D) == (token * 8 + 7) * 128 + 56);
  CHECK(tft::qkv_split_off(token, 8 * Hq - 1, Hq, Hkv, D) == (token * 32 + 31) * 128 + 56);
}

void check_clamp() {
  const int rows[] = {1, 2, 3, 8192, INT_MAX};
  const int probes[] = {INT_MIN, INT_MIN + 1, -8193, -2, -1, 0,       1,
                        2,       3,           8191,  8192, 8193, INT_MAX - 1, INT_MAX};
  for (int n : rows) {
    for (int p : probes) {
      const int r = tft::rope_pos_row(p, n);
      CHECK(r >= 0 && r <= n - 1);
      if (p >= 0 && p < n) CHECK(r == p);  // in range: unchanged
      if (p < 0) CHECK(r == 0);
      if (p >= n) CHECK(r == n - 1);
    }
    // the whole int32 range at a prime stride (65,5xx probes per table size);
    // the ends and the neighbours of 0 and n are in `probes`
    for (int64_t p = INT_MIN; p <= INT_MAX; p += 65521) {
      const int r = tft::rope_pos_row((int)p, n);
      CHECK(r >= 0 && r <= n - 1);
    }
  }
}

}  // namespace

int main() {
  // Hq = Hkv, Hkv = 1, D = 16 (one item per head), D = 128 (the model's)
  check_shape(2, 1, 16);
  check_shape(4, 2, 128);
  check_shape(8, 2, 64);
  check_shape(3, 3, 128);
  check_shape(1, 1, 16);
  check_shape(5, 1, 48);
  check_shape(32, 8, 128);
  check_large();
  check_clamp();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("qkv layout ok\n");
  return 0;
}
