// Group math of the MXFP4 wire pack (mxfp4_quant.hip; docs/KERNELS.md,
// "mxfp4_quant.hip"): the e8m0 scale byte of a group of 32 elements, the e2m1
// code of an element under that scale, and the decoded value. Integer and
// fp32 arithmetic only, callable from host code, so a plain C++ program can
// hold it to the format's definition.
#pragma once

#include <cstdint>

#include "kernels.h"

namespace torchft_amd {

constexpr int kMxGroup = 32;                                // elements per scale byte
constexpr int kMxGroupsPerBlock = kMtBlock / kMxGroup;      // 64 scale bytes per block
constexpr int kMxCodeBytesPerBlock = kMtBlock / 2;          // two codes per byte
static_assert(kMxBlockBytes == kMxGroupsPerBlock + kMxCodeBytesPerBlock, "17 B per group");
constexpr uint32_t kMxNanScale = 0xFF;                      // the group decodes to NaN

TFT_HD inline uint32_t mx_bits(float v) { return __builtin_bit_cast(uint32_t, v); }
TFT_HD inline float mx_float(uint32_t b) { return __builtin_bit_cast(float, b); }

// The scale byte X + 127 of a group from the largest `bits & 0x7fffffff` of
// its elements. As unsigned integers these order like the magnitudes, with
// Inf and every NaN above all finite values, so one integer maximum serves
// both as fmaxf over |v| (which drops a NaN) and as the non-finite test.
// X = clamp(floor(log2 amax) - 2, -125, 125): the exponent field less 2, held
// at 2 from below (zero and subnormal amax have field 0); a finite field is at
// most 254, so the upper clamp never binds.
TFT_HD inline uint32_t mx_scale_byte(uint32_t amax_bits) {
  if (amax_bits >= 0x7F800000u) return kMxNanScale;
  const uint32_t e = amax_bits >> 23;
  return e > 4 ? e - 2 : 2;
}

// 2^-X and 2^X of a scale byte in [2, 252], both normal fp32 numbers
TFT_HD inline float mx_inv_scale(uint32_t byte) { return mx_float((254 - byte) << 23); }

// 2^X of any scale byte a pack may hold: 2^-127 for byte 0, NaN for 0xFF
TFT_HD inline float mx_scale(uint32_t byte) {
  return mx_float(byte == kMxNanScale ? 0x7FC00000u : byte ? byte << 23 : 0x00400000u);
}

// e2m1 code of v under inv_scale = 2^-X: |v| * 2^-X rounded to the grid
// {0, .5, 1, 1.5, 2, 3, 4, 6}, nearest, ties to the even code, above 6 to 6,
// the sign of v (of -0 too) in bit 3. v is finite.
//   below 1 the grid step is .5: adding 2^22, whose last place is .5, rounds
//   to nearest even and leaves the count of steps (0, 1, 2) in the low bits;
//   from 1 on the grid is fp32 cut to one mantissa bit: the usual add of just
//   under half, plus the kept bit for the tie, carries into the exponent by
//   itself, and (exponent, bit) less that of 1.0 is the code less 2.
TFT_HD inline uint32_t mx_code(float v, float inv_scale) {
  const uint32_t vb = mx_bits(v);
  float y = mx_float(vb & 0x7FFFFFFFu) * inv_scale;
  y = y < 6.f ? y : 6.f;
  const uint32_t yb = mx_bits(y);
  const uint32_t lo = mx_bits(y + 4194304.f) - 0x4A800000u;
  const uint32_t hi = ((yb + 0x1FFFFFu + ((yb >> 22) & 1u)) >> 22) - 252u;
  return ((vb >> 28) & 8u) | (y < 1.f ? lo : hi);
}

// lut[code & 7] with the sign of bit 3; times mx_scale() it is the decoded value
TFT_HD inline float mx_code_value(uint32_t code) {
  const uint32_t m = code & 7u;
  const uint32_t mag = m >= 2 ? (m + 252u) << 22 : m ? 0x3F000000u : 0u;
  return mx_float(mag | ((code & 8u) << 28));
}

}  // namespace torchft_amd
