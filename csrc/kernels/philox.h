// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
// SC'11) and the stochastic rounding of an fp32 value to bf16 that
// fused_adamw.hip draws its bits for. Plain constexpr C++ for host and device,
// so a host program can check both (csrc/kernels/tests/philox_test.cpp).
#pragma once

#include <cstdint>

#include "kernels.h"

namespace torchft_amd {

struct Philox4 {
  uint32_t w[4];
};

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

// 128 random bits from a 128-bit counter and a 64-bit key: ten rounds of two
// 32 x 32 -> 64 multiplies, the key bumped between rounds.
TFT_HD constexpr Philox4 philox4x32_10(Philox4 c, uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c.w[0];
    const uint64_t p1 = (uint64_t)kPhiloxM1 * c.w[2];
    c = Philox4{{(uint32_t)(p1 >> 32) ^ c.w[1] ^ k0, (uint32_t)p1,
                 (uint32_t)(p0 >> 32) ^ c.w[3] ^ k1, (uint32_t)p0}};
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return c;
}

// The 16 bits of element i (0 .. 7) of a lane's eight: bits 16 * (i & 1) ...
// + 16 of output word i >> 1.
TFT_HD constexpr uint32_t philox_r16(const Philox4& r, int i) {
  return (r.w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
}

// inf and NaN: sr_bf16 is not for them
TFT_HD constexpr bool sr_finite(uint32_t bits) {
  return (bits & 0x7F800000u) != 0x7F800000u;
}

// bf16 bits of the finite fp32 value with the bits `bits`, rounded at random
// with the 16 uniform bits r16: the magnitude moves away from zero with
// probability (low 16 bits) / 2^16, the share of a bf16 step it lies above the
// neighbour towards zero, so the expectation is the value itself for either
// sign. Low bits of 0 never move; a carry into the exponent is the right
// neighbour; the largest finite values may become +-inf.
TFT_HD constexpr uint16_t sr_bf16(uint32_t bits, uint32_t r16) {
  return (uint16_t)((bits + (r16 & 0xFFFFu)) >> 16);
}

}  // namespace torchft_amd
