// Stand-alone check of the flash-attention address math (fa_layout.h): the
// subtiled LDS tile image, the thread -> chunk staging map, the contiguous
// and the hardware-transpose fragment reads, and the pa/pb swizzle. No torch,
// no HIP; tests/test_fa_layout.py builds it with the address and
// undefined-behaviour sanitizers and runs it.
#include <cstdint>
#include <cstdio>
#include <cstring>
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

// the bf16 bit pattern the test gives tile element (row, d): distinct for
// every element of a 64 x 128 tile and never the poison 0xffff
uint16_t elem(int row, int d) { return (uint16_t)(row * tft::kFaD + d); }

uint16_t load16(const unsigned char* p) {
  uint16_t v;
  std::memcpy(&v, p, 2);
  return v;
}

// ds_read_b64_tr_b16 as tr16_probe.hip pinned it: a 16-lane group whose
// addresses are lane-linear 8 B over one contiguous 128-B [4][16] bf16 block
// gives lane l column (l & 15), rows j = 0..3. Checks that the 64 addresses
// have that form and stay inside rows of one subtile, then returns the lane's
// four elements.
template <int ROWS>
void tr_read(const tft::Tile<ROWS>& tile, const unsigned (&addrs)[64], uint16_t (&out)[64][4]) {
  using T = tft::Tile<ROWS>;
  for (int l = 0; l < 64; l++) {
    const unsigned base = addrs[l & ~15];
    CHECK(addrs[l] == base + (l & 15) * 8);
    CHECK(base + 128 <= sizeof(tile.sub));
    // the [4][16] block is four whole rows of one subtile, clear of the pad
    const unsigned in_sub = base % T::kStride;
    CHECK(in_sub % 32 == 0 && in_sub + 128 <= (unsigned)ROWS * 32);
    for (int j = 0; j < 4; j++) {
      const unsigned a = base + j * 32 + (l & 15) * 2;
      out[l][j] = a + 2 <= sizeof(tile.sub) ? load16(tile.sub + a) : 0xffff;
    }
  }
}

template <int ROWS>
void check_tile() {
  using T = tft::Tile<ROWS>;
  constexpr int CH = T::kChunks;
  static_assert(tft::kFaThreads * CH * 16 == ROWS * tft::kFaD * 2, "threads x chunks = tile");

  // source tile, row-major [ROWS][128], as it lies in global memory
  std::vector<uint16_t> src((size_t)ROWS * tft::kFaD);
  for (int r = 0; r < ROWS; r++)
    for (int d = 0; d < tft::kFaD; d++) src[(size_t)r * tft::kFaD + d] = elem(r, d);

  // staging: what load_tiles / write_tiles do for one tensor
  static T tile;
  std::memset(tile.sub, 0xff, sizeof(tile.sub));
  std::vector<int> chunk_writes(ROWS * 16, 0), byte_writes(sizeof(tile.sub), 0);
  for (int t = 0; t < tft::kFaThreads; t++) {
    const int row = T::stage_row(t), c0 = T::stage_chunk(t);
    CHECK(row == t / (16 / CH) && c0 == (t % (16 / CH)) * CH);
    CHECK(row >= 0 && row < ROWS && c0 >= 0 && c0 + CH <= 16);
    for (int c = 0; c < CH; c++) {
      const int a = T::stage_addr(t, c);
      CHECK(a >= 0 && a % 16 == 0 && a + 16 <= (int)sizeof(T));
      if (a < 0 || a + 16 > (int)sizeof(T)) continue;
      chunk_writes[row * 16 + c0 + c]++;
      for (int i = 0; i < 16; i++) byte_writes[a + i]++;
      std::memcpy(tile.sub + a, &src[(size_t)row * tft::kFaD + (c0 + c) * 8], 16);
    }
  }
  for (int w : chunk_writes) CHECK(w == 1);
  int written = 0;
  for (int w : byte_writes) {
    CHECK(w <= 1);
    written += w;
  }
  CHECK(written == ROWS * tft::kFaD * 2);
  // element (row, d) lands at subtile d/16, offset row*32 + (d%16)*2
  for (int r = 0; r < ROWS; r++)
    for (int d = 0; d < tft::kFaD; d++) {
      const int a = (d / 16) * T::kStride + r * 32 + (d % 16) * 2;
      CHECK(a == T::addr(d / 16, r, (d % 16) * 2));
      CHECK(load16(tile.sub + a) == elem(r, d));
    }

  // contiguous fragment: k-slice tt, half -> d = tt*16 + half*8 .. +8 of row
  for (int tt = 0; tt < 8; tt++)
    for (int r = 0; r < ROWS; r++)
      for (int half = 0; half < 2; half++) {
        const int a = T::frag_addr(tt, r, half);
        CHECK(a >= 0 && a % 16 == 0 && a + 16 <= (int)sizeof(T));
        for (int m = 0; m < 8; m++)
          CHECK(load16(tile.sub + a + 2 * m) == elem(r, tt * 16 + half * 8 + m));
      }

  // transpose reads: every step (dt, h2) of every 32-row block s; the read
  // at +0 and its partner at +128 joined give lane l the MFMA B operand
  // [k = h2*16 + (l>>5)*8 + m][d = dt*32 + (l&31)], m = 0..7, of block s
  for (int s = 0; s < ROWS / 32; s++)
    for (int dt = 0; dt < 4; dt++)
      for (int h2 = 0; h2 < 2; h2++) {
        CHECK(T::tr_step_off(dt, h2) == (unsigned)(dt * 2 * T::kStride + h2 * 512));
        for (int part = 0; part < 2; part++) {
          unsigned addrs[64];
          for (int l = 0; l < 64; l++)
            addrs[l] = T::tr_lane_off(l) + T::tr_step_off(dt, h2) + s * 32 * 32 + part * 128;
          uint16_t got[64][4];
          tr_read(tile, addrs, got);
          for (int l = 0; l < 64; l++)
            for (int j = 0; j < 4; j++) {
              const int k = h2 * 16 + (l >> 5) * 8 + part * 4 + j;
              CHECK(got[l][j] == elem(s * 32 + k, dt * 32 + (l & 31)));
            }
        }
      }
}

void check_pb() {
  // pb_addr: a bijection of the 32 x 64 B buffer that keeps the row and the
  // offset inside each 16-B unit
  std::vector<int> seen(32 * 64, 0);
  for (int row = 0; row < 32; row++)
    for (int off = 0; off < 64; off++) {
      const int a = tft::pb_addr(row, off);
      CHECK(a >= 0 && a < 32 * 64);
      if (a < 0 || a >= 32 * 64) continue;
      seen[a]++;
      CHECK(a / 64 == row && a % 16 == off % 16);
      CHECK(a == row * 64 + tft::row_swz(row, off));
    }
  for (int n : seen) CHECK(n == 1);

  // c_row covers the 32 rows once over (reg, half)
  std::vector<int> rows(32, 0);
  for (int reg = 0; reg < 16; reg++)
    for (int half = 0; half < 2; half++) rows[tft::c_row(reg, half)]++;
  for (int n : rows) CHECK(n == 1);

  // the four C rows of a register quad sit 64 B apart from one base address
  for (int r4 = 0; r4 < 4; r4++)
    for (int r = 0; r < 4; r++)
      for (int half = 0; half < 2; half++)
        for (int l31 = 0; l31 < 32; l31++)
          CHECK(tft::pb_row4_addr(r4, half, l31) + 64 * r ==
                tft::pb_addr(tft::c_row(4 * r4 + r, half), 2 * l31));

  // A-fragment read: one aligned 16-B unit holding columns
  // h2*16 + half*8 .. +8 of row l31
  for (int h2 = 0; h2 < 2; h2++)
    for (int half = 0; half < 2; half++)
      for (int l31 = 0; l31 < 32; l31++) {
        const int a = tft::pb_afrag_addr(h2, half, l31);
        CHECK(a >= 0 && a % 16 == 0 && a + 16 <= 32 * 64);
        for (int m = 0; m < 8; m++)
          CHECK(a + 2 * m == tft::pb_addr(l31, (h2 * 16 + half * 8 + m) * 2));
      }
}

void check_row_off() {
  // both layouts address the same logical [B,H,S,D] element space densely
  const int B = 2, H = 3, S = 5;
  for (int bshd = 0; bshd < 2; bshd++) {
    std::vector<int> hits(B * H * S, 0);
    for (int b = 0; b < B; b++)
      for (int h = 0; h < H; h++)
        for (int s = 0; s < S; s++) {
          const int64_t off = tft::row_off(b, h, s, H, S, bshd);
          CHECK(off % tft::kFaD == 0 && off >= 0 && off < (int64_t)B * H * S * tft::kFaD);
          hits[off / tft::kFaD]++;
          CHECK(off == (bshd ? ((int64_t)(b * S + s) * H + h) : ((int64_t)(b * H + h) * S + s)) *
                           tft::kFaD);
        }
    for (int n : hits) CHECK(n == 1);
  }
  // no 32-bit overflow at a large shape
  CHECK(tft::row_off(63, 31, 65535, 32, 65536, 1) ==
        (((int64_t)63 * 65536 + 65535) * 32 + 31) * 128);
}

}  // namespace

int main() {
  check_tile<32>();
  check_tile<64>();
  check_pb();
  check_row_off();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("fa layout ok\n");
  return 0;
}
