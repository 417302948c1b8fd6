// Address map of the fused QKV split + rotary kernels (qkv_rope.hip): where a
// lane's item lies in a token's row of the fused projection and where it goes
// in the separate q / k / v tensors, and the clamp of a rotary position into
// the tables. Plain constexpr C++, callable from host and device;
// csrc/kernels/tests/qkv_layout_test.cpp checks every function here on the
// host.
#pragma once

#include "kernels.h"

namespace torchft_amd {

// A token's row of the projection is W = (Hq + 2*Hkv) * D bf16: the Hq heads of
// q, then the Hkv heads of k, then the Hkv heads of v, D elements each. The
// row is cut into items of kQkvItem elements, one per lane. Item `it` belongs
// to head slot it / (D/16) and covers the columns i .. i+7 and
// D/2 + i .. D/2 + i+7 of that head, i = (it % (D/16)) * 8: the two 16 B
// halves of eight rotate-half pairs (x1 at i + m, x2 at D/2 + i + m).
// D % 16 == 0.
constexpr int kQkvItem = 16;
constexpr int kQkvHalf = kQkvItem / 2;  // elements of one 16 B access

enum QkvClass : int { kQkvQ = 0, kQkvK = 1, kQkvV = 2 };

TFT_HD constexpr int qkv_items_per_head(int D) { return D / kQkvItem; }
TFT_HD constexpr int qkv_items_per_token(int Hq, int Hkv, int D) {
  return (Hq + 2 * Hkv) * qkv_items_per_head(D);
}

// the head slot (0 .. Hq + 2*Hkv - 1) of item `it` and the first column of the
// item's lower half inside that head
TFT_HD constexpr int qkv_item_slot(int it, int D) { return it / qkv_items_per_head(D); }
TFT_HD constexpr int qkv_item_col(int it, int D) {
  return (it % qkv_items_per_head(D)) * kQkvHalf;
}

// which tensor a head slot belongs to, and its head index inside that tensor
TFT_HD constexpr int qkv_slot_class(int slot, int Hq, int Hkv) {
  return slot < Hq ? kQkvQ : (slot < Hq + Hkv ? kQkvK : kQkvV);
}
TFT_HD constexpr int qkv_slot_head(int slot, int Hq, int Hkv) {
  return slot < Hq ? slot : (slot < Hq + Hkv ? slot - Hq : slot - Hq - Hkv);
}
// heads of the tensor of class `cls`
TFT_HD constexpr int qkv_class_heads(int cls, int Hq, int Hkv) {
  return cls == kQkvQ ? Hq : Hkv;
}

// Element offset of the item's lower half in the fused [tokens, W] tensor; the
// upper half is D/2 further.
TFT_HD constexpr int64_t qkv_packed_off(int64_t token, int it, int Hq, int Hkv, int D) {
  return token * ((int64_t)(Hq + 2 * Hkv) * D) + (int64_t)qkv_item_slot(it, D) * D +
         qkv_item_col(it, D);
}
// ... and in its own [tokens, heads, D] tensor (q, k or v); the upper half is
// D/2 further there too.
TFT_HD constexpr int64_t qkv_split_off(int64_t token, int it, int Hq, int Hkv, int D) {
  const int slot = qkv_item_slot(it, D);
  const int heads = qkv_class_heads(qkv_slot_class(slot, Hq, Hkv), Hq, Hkv);
  return (token * heads + qkv_slot_head(slot, Hq, Hkv)) * (int64_t)D + qkv_item_col(it, D);
}

// The row of the cos / sin tables a position reads, clamped into
// [0, table_rows - 1] (table_rows >= 1). The kernels read `positions` as it
// is: an entry DocMask.positions() did not build costs correctness of the
// values and never an address outside the tables, the rule of the document
// arrays (fa_layout.h).
TFT_HD constexpr int rope_pos_row(int pos, int table_rows) {
  return pos < 0 ? 0 : (pos >= table_rows ? table_rows - 1 : pos);
}

}  // namespace torchft_amd
