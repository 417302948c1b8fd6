// Stand-alone check of the multi-tensor table layout (multi_tensor_host.h)
// and of find_tensor (multi_tensor.h) compiled for the host. No torch, no
// HIP; tests/test_table_layout.py builds it with the address and
// undefined-behaviour sanitizers and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../multi_tensor.h"
#include "../multi_tensor_host.h"

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

constexpr int64_t kPoison = -0x5a5a5a5a5a5a5a5aLL;

int64_t ceil_blocks(int64_t numel) { return (numel + tft::kMtBlock - 1) / tft::kMtBlock; }

// fake address of column j of row i: distinct for every (table, i, j)
int64_t fake_addr(int table, int64_t i, int j) { return (table + 1) * 1000000 + i * 16 + j; }

std::vector<int64_t> fake_addrs(int table, int64_t n, int n_cols) {
  std::vector<int64_t> a;
  for (int64_t i = 0; i < n; i++)
    for (int j = 0; j < n_cols; j++) a.push_back(fake_addr(table, i, j));
  return a;
}

// the first tensor that owns `block`, by linear scan
int scan_tensor(const std::vector<int64_t>& numels, int64_t block) {
  int64_t first = 0;
  for (size_t t = 0; t < numels.size(); t++) {
    const int64_t nb = ceil_blocks(numels[t]);
    if (block < first + nb) return (int)t;
    first += nb;
  }
  return -1;
}

// one table alone in an exactly sized buffer between two poison words
void check_one(const std::vector<int64_t>& numels, int n_cols) {
  const int64_t n = (int64_t)numels.size();
  const int64_t words = tft::mt_table_words(n, n_cols);
  CHECK(words == (n_cols + 2) * n + 1);
  std::vector<int64_t> buf(words + 2, kPoison);
  const auto addrs = fake_addrs(0, n, n_cols);
  const int64_t blocks = tft::mt_write_table(buf.data() + 1, n, n_cols, addrs.data(),
                                            numels.data());
  CHECK(buf.front() == kPoison && buf.back() == kPoison);
  for (int64_t w = 1; w <= words; w++) CHECK(buf[w] != kPoison);

  int64_t want = 0;
  for (int64_t ne : numels) want += ceil_blocks(ne);
  CHECK(blocks == want);

  const tft::MultiTensorTable tb = tft::mt_view(buf.data(), 1, n, n_cols, blocks);
  CHECK(tb.n == n && tb.n_cols == n_cols && tb.total_blocks == want);
  CHECK(tb.prefix() + n + 1 == buf.data() + 1 + words);
  CHECK(tb.prefix()[0] == 0 && tb.prefix()[n] == want);
  for (int64_t i = 0; i < n; i++) {
    CHECK(tb.numels()[i] == numels[i]);
    CHECK(tb.prefix()[i + 1] - tb.prefix()[i] == ceil_blocks(numels[i]));
    for (int j = 0; j < n_cols; j++) CHECK(tb.col(j)[i] == fake_addr(0, i, j));
  }
  // every block finds the tensor a linear scan finds, inside its range
  for (int64_t b = 0; b < blocks; b++) {
    const int t = tft::find_tensor(tb.prefix(), tb.n, b);
    CHECK(t == scan_tensor(numels, b));
    CHECK(t >= 0 && t < n && numels[t] > 0);
    CHECK(tb.prefix()[t] <= b && b < tb.prefix()[t + 1]);
    CHECK((b - tb.prefix()[t]) * tft::kMtBlock < numels[t]);
  }
}

void check_packed() {
  const std::vector<int64_t> na = {2047, 0, 2048, 2049}, nb = {1, 5000};
  const int ka = 4, kb = 1;
  const int64_t wa = tft::mt_table_words((int64_t)na.size(), ka);
  const int64_t wb = tft::mt_table_words((int64_t)nb.size(), kb);
  std::vector<int64_t> buf(wa + wb + 1, kPoison);
  const auto aa = fake_addrs(0, (int64_t)na.size(), ka);
  const auto ab = fake_addrs(1, (int64_t)nb.size(), kb);
  const int64_t ba = tft::mt_write_table(buf.data(), (int64_t)na.size(), ka, aa.data(),
                                        na.data());
  const std::vector<int64_t> first(buf.begin(), buf.begin() + wa);
  const int64_t bb = tft::mt_write_table(buf.data() + wa, (int64_t)nb.size(), kb,
                                        ab.data(), nb.data());
  // the second table left the first alone and stayed inside its own words
  CHECK(std::vector<int64_t>(buf.begin(), buf.begin() + wa) == first);
  CHECK(buf.back() == kPoison);
  const auto ta = tft::mt_view(buf.data(), 0, (int64_t)na.size(), ka, ba);
  const auto tb = tft::mt_view(buf.data(), wa, (int64_t)nb.size(), kb, bb);
  CHECK(ta.prefix() + na.size() + 1 == tb.col(0));
  CHECK(ta.prefix()[0] == 0 && tb.prefix()[0] == 0);
  CHECK(ba == 1 + 0 + 1 + 2 && bb == 1 + 3);
  CHECK(tb.col(0)[1] == fake_addr(1, 1, 0) && tb.numels()[1] == 5000);
  CHECK(ta.col(3)[3] == fake_addr(0, 3, 3));
}

void check_block_limit() {
  // 2^31 blocks in all: refused. One block fewer: taken.
  const int64_t big = (int64_t(1) << 30) * tft::kMtBlock;
  for (int64_t last : {big, big - tft::kMtBlock}) {
    const std::vector<int64_t> numels = {big, last};
    std::vector<int64_t> buf(tft::mt_table_words(2, 1));
    const auto addrs = fake_addrs(0, 2, 1);
    const int64_t blocks = tft::mt_write_table(buf.data(), 2, 1, addrs.data(), numels.data());
    if (last == big)
      CHECK(blocks == -1);
    else
      CHECK(blocks == (int64_t(1) << 31) - 1);
  }
}

}  // namespace

int main() {
  const std::vector<std::vector<int64_t>> lists = {
      {1},
      {2047, 2048, 2049},
      {0, 0, 7, 2049},      // empties first
      {8, 0, 0, 5000, 0, 1},  // empties in the middle
      {3300, 2048, 0, 0},   // empties last
      {0, 0, 0},            // all empty
      {},
  };
  for (const auto& numels : lists)
    for (int n_cols : {1, 3, 5}) check_one(numels, n_cols);
  check_packed();
  check_block_limit();
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("table layout ok\n");
  return 0;
}
