// Stand-alone check of the attention launches' workgroup order (fa_wg_order
// in fa_layout.h): a bijection of the grid, heaviest block first under the
// causal flag, the identity without it, nothing overflowing at the largest
// grid the bindings admit. No torch, no HIP; tests/test_fa_wg_order.py builds
// it with the address and undefined-behaviour sanitizers and runs it.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../fa_layout.h"

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

// Tiles block x of a causal launch over nx blocks of 256 rows streams, as the
// kernels count them (S = 256 * nx):
//   dkdv  nQ - i_min = 8 * (nx - x) 32-row Q/dO tiles per query head of its
//         group (flash_attn_bwd.hip, nI)
//   dq    T = 4 * (x + 1) 64-key K/V tiles (flash_attn_bwd.hip, T)
//   fwd   nT = 4 * (x + 1) (flash_attn_fwd.hip, nT)
struct Kernel {
  const char* name;
  tft::FaHeavy heavy;
  int64_t (*tiles)(int x, int nx);
};
const Kernel kKernels[] = {
    {"dkdv", tft::kFaHeavyLowX, [](int x, int nx) { return (int64_t)8 * (nx - x); }},
    {"dq", tft::kFaHeavyHighX, [](int x, int) { return (int64_t)4 * (x + 1); }},
    {"fwd", tft::kFaHeavyHighX, [](int x, int) { return (int64_t)4 * (x + 1); }},
};

void check_grid(unsigned nx, unsigned ny) {
  for (const Kernel& kern : kKernels) {
    for (int causal = 0; causal < 2; causal++) {
      std::vector<unsigned char> seen((size_t)nx * ny, 0);
      int64_t prev_cost = INT64_MAX;
      int prev_x = -1;
      // n in launch order: blockIdx.x fastest
      for (unsigned by = 0; by < ny; by++) {
        for (unsigned bx = 0; bx < nx; bx++) {
          const tft::FaWg wg = tft::fa_wg_order(bx, by, nx, ny, causal != 0, kern.heavy);
          CHECK(wg.x >= 0 && (unsigned)wg.x < nx && wg.y >= 0 && (unsigned)wg.y < ny);
          if (wg.x < 0 || (unsigned)wg.x >= nx || wg.y < 0 || (unsigned)wg.y >= ny) return;
          unsigned char& s = seen[(size_t)wg.y * nx + wg.x];
          CHECK(s == 0);  // one-to-one, hence onto: the grid has nx * ny blocks
          s = 1;
          if (!causal) {
            CHECK((unsigned)wg.x == bx && (unsigned)wg.y == by);
            continue;
          }
          const int64_t cost = kern.tiles(wg.x, (int)nx);
          CHECK(cost <= prev_cost);                     // heaviest first
          if (cost == prev_cost) CHECK(wg.x == prev_x);  // equal cost: only y differs
          prev_cost = cost;
          prev_x = wg.x;
        }
      }
      if (failures) {
        std::printf("  at %s nx=%u ny=%u causal=%d\n", kern.name, nx, ny, causal);
        return;
      }
    }
  }
}

// the corners and the middle of the largest grid: ny = kFaMaxGridY and
// nx = 2^24 / 256. Its last block id is 65536 * 65535 - 1 < 2^32.
void check_largest() {
  const unsigned nx = (1u << 24) / (tft::kFaBlk * tft::kFaWaves);
  const unsigned ny = tft::kFaMaxGridY;
  static_assert((uint64_t)((1u << 24) / 256) * tft::kFaMaxGridY < (uint64_t)1 << 32,
                "n fits 32 bits");
  const unsigned bxs[] = {0, 1, nx / 2, nx - 2, nx - 1};
  const unsigned bys[] = {0, 1, ny / 2, ny - 2, ny - 1};
  for (const Kernel& kern : kKernels) {
    for (unsigned by : bys) {
      for (unsigned bx : bxs) {
        const tft::FaWg wg = tft::fa_wg_order(bx, by, nx, ny, true, kern.heavy);
        // the same map in 64 bits
        const uint64_t n = bx + (uint64_t)nx * by;
        const uint64_t rank = n / ny;
        const uint64_t x = kern.heavy == tft::kFaHeavyLowX ? rank : nx - 1 - rank;
        CHECK(wg.x >= 0 && (uint64_t)wg.x == x);
        CHECK(wg.y >= 0 && (uint64_t)wg.y == n % ny);
        const tft::FaWg id = tft::fa_wg_order(bx, by, nx, ny, false, kern.heavy);
        CHECK((unsigned)id.x == bx && (unsigned)id.y == by);
      }
    }
  }
  // first and last block: the heaviest and the lightest x
  CHECK(tft::fa_wg_order(0, 0, nx, ny, true, tft::kFaHeavyLowX).x == 0);
  CHECK(tft::fa_wg_order(0, 0, nx, ny, true, tft::kFaHeavyHighX).x == (int)nx - 1);
  CHECK(tft::fa_wg_order(nx - 1, ny - 1, nx, ny, true, tft::kFaHeavyLowX).x == (int)nx - 1);
  CHECK(tft::fa_wg_order(nx - 1, ny - 1, nx, ny, true, tft::kFaHeavyHighX).x == 0);
}

// usable in a constant expression, host and device alike
static_assert(tft::fa_wg_order(0, 0, 32, 32, true, tft::kFaHeavyLowX).x == 0, "");
static_assert(tft::fa_wg_order(0, 0, 32, 128, true, tft::kFaHeavyHighX).x == 31, "");
static_assert(tft::fa_wg_order(5, 7, 32, 128, false, tft::kFaHeavyHighX).y == 7, "");

}  // namespace

int main() {
  const unsigned nys[] = {1, 2, 3, 7, 8, 9, 32, 128, 65535};
  for (unsigned ny : nys) {
    for (unsigned nx = 1; nx <= 40; nx++) {
      // ny = 65535: a few nx keep the grid modest
      if (ny == 65535 && nx != 1 && nx != 2 && nx != 3 && nx != 40) continue;
      check_grid(nx, ny);
      if (failures) return 1;
    }
  }
  check_largest();
  if (failures) return 1;
  std::printf("fa wg order ok\n");
  return 0;
}
