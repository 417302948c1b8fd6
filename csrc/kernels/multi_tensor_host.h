// Host side of the multi-tensor table (kernels.h, MultiTensorTable): the one
// place that knows where a column starts. No torch, no HIP, so a plain C++
// program can test it (csrc/kernels/tests/table_layout_test.cpp).
#pragma once

#include <cstdint>

#include "kernels.h"

namespace torchft_amd {

// int64 words of a table with n rows and n_cols pointer columns
inline int64_t mt_table_words(int64_t n, int n_cols) {
  return (int64_t)(n_cols + 2) * n + 1;
}

// Writes one table at dst[0 .. mt_table_words(n, n_cols)):
//   [col 0 | ... | col n_cols-1 | numels | block_prefix (n+1)]
// `addrs` holds the tensor addresses row by row (addrs[i * n_cols + j] is
// column j of row i), `numels` one element count per row. The prefix starts
// at 0 whatever lies before dst, so several tables can share one buffer.
// Returns the number of logical blocks, or -1 (nothing usable written) when
// that reaches 2^31, more than one launch can index.
inline int64_t mt_write_table(int64_t* dst, int64_t n, int n_cols,
                              const int64_t* addrs, const int64_t* numels) {
  int64_t* out_numels = dst + (int64_t)n_cols * n;
  int64_t* prefix = out_numels + n;
  int64_t blocks = 0;
  for (int64_t i = 0; i < n; i++) {
    for (int j = 0; j < n_cols; j++) dst[(int64_t)j * n + i] = addrs[i * n_cols + j];
    out_numels[i] = numels[i];
    prefix[i] = blocks;
    // ceil without overflow for any numel >= 0
    blocks += numels[i] / kMtBlock + (numels[i] % kMtBlock != 0);
    if (blocks >= (int64_t(1) << 31)) return -1;
  }
  prefix[n] = blocks;
  return blocks;
}

// The view a launcher takes of a table written at word `offset` of a buffer
// whose device copy starts at `dev_words`.
inline MultiTensorTable mt_view(const int64_t* dev_words, int64_t offset, int64_t n,
                                int n_cols, int64_t total_blocks) {
  return MultiTensorTable{dev_words + offset, (int)n, n_cols, total_blocks};
}

}  // namespace torchft_amd
