// Stand-alone host check of philox.h: the published known-answer vectors of
// Philox4x32-10 and sr_bf16 over all 65536 draws of a handful of inputs. No
// torch, no HIP; tests/test_philox.py builds it under ASan + UBSan and runs it.
#include <cstdint>
#include <cstdio>

#include "../philox.h"

namespace tft = torchft_amd;

static int failures = 0;
#define CHECK(cond) \
  if (!(cond)) failures += std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond) > 0

// `bits` lies (low 16 bits) / 65536 of a bf16 step beyond `down`, the neighbour
// towards zero: exactly that many draws store `up`, all the others `down`
static void splits(uint32_t bits, uint16_t down, uint16_t up) {
  int n_up = 0, n_down = 0;
  for (uint32_t r = 0; r < 65536; r++) {
    n_up += tft::sr_bf16(bits, r) == up;
    n_down += tft::sr_bf16(bits, r) == down;
  }
  const int low = (int)(bits & 0xFFFFu);
  CHECK(tft::sr_finite(bits) && (bits >> 16) == down);
  CHECK(n_up == (low ? low : 65536) && n_down == (low ? 65536 - low : 65536));
}

int main() {
  const struct { tft::Philox4 c; uint32_t k0, k1; tft::Philox4 want; } kat[3] = {
      {{{0, 0, 0, 0}}, 0, 0, {{0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}}},
      {{{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}}, 0xffffffffu, 0xffffffffu,
       {{0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}}},
      {{{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}}, 0xa4093822u, 0x299f31d0u,
       {{0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}}}};
  for (const auto& k : kat)
    for (int i = 0; i < 4; i++) CHECK(tft::philox4x32_10(k.c, k.k0, k.k1).w[i] == k.want.w[i]);

  // element i of a lane's eight: bits 16 * (i & 1) ... + 16 of word i >> 1
  const tft::Philox4 r = {{0x11110000u, 0x33332222u, 0x55554444u, 0x77776666u}};
  for (int i = 0; i < 8; i++) CHECK(tft::philox_r16(r, i) == 0x1111u * (uint32_t)i);

  splits(0x3F800000u, 0x3F80, 0x3F80);  // 1.0, low bits 0: never changed
  splits(0xBF800000u, 0xBF80, 0xBF80);
  splits(0x3F804000u, 0x3F80, 0x3F81);  // a quarter step up: 16384 draws
  splits(0xBF804000u, 0xBF80, 0xBF81);  // the same away from zero
  splits(0x3FFFC000u, 0x3FFF, 0x4000);  // a carry into the exponent: 2.0
  splits(0x00000001u, 0x0000, 0x0001);  // an fp32 subnormal: one draw in 65536
  splits(0x80012345u, 0x8001, 0x8002);  // a bf16 subnormal
  splits(0x7F7FFFFFu, 0x7F7F, 0x7F80);  // the largest finite value: may become inf
  splits(0xFF7FFFFFu, 0xFF7F, 0xFF80);

  // inf and NaN are not sr_bf16's: the kernel stores them with from_f32. Added
  // bits carry a NaN of a large payload out of the NaNs: 0x7FFFFFFF + 1 is -0.
  CHECK(!tft::sr_finite(0x7F800000u) && !tft::sr_finite(0xFF800000u));
  CHECK(!tft::sr_finite(0x7F800001u) && !tft::sr_finite(0xFFFFFFFFu));
  CHECK(tft::sr_bf16(0x7FFFFFFFu, 1) == 0x8000);

  if (failures == 0) std::printf("philox ok\n");
  return failures == 0 ? 0 : 1;
}
