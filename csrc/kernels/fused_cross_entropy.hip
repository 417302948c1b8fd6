// Fused cross-entropy forward + backward over bf16 logits — CDNA4 (gfx950).
//
// One 1024-thread workgroup per logits row. Pass 1 keeps an online
// (running max, sum of exp) pair per thread and combines it across the
// workgroup (wave64 shuffles, then LDS across the 16 waves, fixed order, no
// atomics: the result is bitwise reproducible). Pass 2 re-reads the row and
// overwrites it in place with the bf16 gradient, so the caller can feed the
// same buffer straight into the two backward GEMMs of the lm-head and nothing
// of size [rows, vocab] outlives its chunk.
//
//   lse      = logsumexp(x)
//   row_loss = lse - x[t] + z * lse^2
//   g[j]     = grad_scale * (softmax(x)[j] * (1 + 2 z lse) - [j == t])
//
// All math is fp32; the running max is subtracted before every exp, so
// |x| ~ 1e4 and -inf (masked vocabulary) entries are fine as long as a row
// has one finite logit. Rows with t == ignore_index give loss 0 and a zero
// gradient row. A target outside [0, V) that is not ignore_index gives a NaN
// loss and a NaN gradient row; no address is ever formed from it (the
// one-hot is a column compare and the x[t] read is guarded). A NaN or +inf
// logit gives a non-finite loss and no finite gradient element (NaN for +inf,
// where the definition has a +inf loss: inf - inf below); a target on a -inf
// logit gives a +inf loss and a finite gradient row.
//
// Any V >= 1 and any 2-byte-aligned row base: each row is split into a
// scalar head (up to the first 16-B boundary), whole 16-B bf16x8 vectors,
// and a scalar tail, so a vector access never crosses the end of its row.
// With V % 8 == 0 and a 16-B-aligned base the head and tail are empty.

#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "vec8.h"

namespace torchft_amd {

namespace {

using bf16 = __hip_bfloat16;

constexpr int kCeThreads = 1024;
constexpr int kCeWaves = kCeThreads / 64;

// (m, s) represents s * exp(m); the empty state is (-inf, 0). exp(-inf - m)
// is 0 for finite m; the only NaN trap is -inf - -inf, guarded here.
__device__ inline void ce_combine(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) {
    s = 0.f;
  } else {
    s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
  }
  m = mn;
}

// Row geometry shared by both passes: cols [0, head) scalar, then nvec
// 16-B vectors starting at col head, then cols [head + 8 nvec, V) scalar.
struct CeRowSplit {
  int head;
  int nvec;
  int nscalar;  // head + tail, <= 14
};

__device__ inline CeRowSplit ce_split(const bf16* xr, int V) {
  CeRowSplit r;
  const int mis = (int)(reinterpret_cast<uintptr_t>(xr) & 15);
  int head = ((16 - mis) & 15) >> 1;
  r.head = head < V ? head : V;
  r.nvec = (V - r.head) >> 3;
  r.nscalar = V - 8 * r.nvec;
  return r;
}

// column of the i-th scalar (head/tail) element
__device__ inline int ce_scalar_col(const CeRowSplit& sp, int i) {
  return i < sp.head ? i : i + 8 * sp.nvec;
}

__global__ void __launch_bounds__(kCeThreads)
cross_entropy_kernel(bf16* __restrict__ logits,
                     const int64_t* __restrict__ targets,
                     float* __restrict__ row_loss,
                     const float* __restrict__ grad_scale_p, int64_t rows,
                     int V, int64_t ignore_index, float z, int write_grad) {
  const int64_t row = blockIdx.x;
  if (row >= rows) return;
  const int tid = threadIdx.x;
  bf16* xr = logits + row * (int64_t)V;
  const CeRowSplit sp = ce_split(xr, V);
  bf16* xv = xr + sp.head;  // 16-B aligned

  const int64_t t = targets[row];

  if (t == ignore_index) {  // workgroup-uniform
    if (tid == 0) row_loss[row] = 0.f;
    if (write_grad) {
      const float zero[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int i = tid; i < sp.nvec; i += kCeThreads) store8(xv + 8 * i, zero);
      if (tid < sp.nscalar) xr[ce_scalar_col(sp, tid)] = __float2bfloat16(0.f);
    }
    return;
  }

  const bool t_ok = t >= 0 && t < (int64_t)V;
  const int tcol = t_ok ? (int)t : -1;
  // Read before the first barrier: pass 2 overwrites the row in place.
  float xt = 0.f;
  if (tid == 0) xt = t_ok ? __bfloat162float(xr[tcol]) : NAN;

  // ---- pass 1: online (max, sum exp) -------------------------------------
  float m = -INFINITY, s = 0.f;
  for (int i = tid; i < sp.nvec; i += kCeThreads) {
    float v[8];
    load8(xv + 8 * i, v);
    float vm = v[0];
#pragma unroll
    for (int k = 1; k < 8; k++) vm = fmaxf(vm, v[k]);
    const float mn = fmaxf(m, vm);
    if (mn != -INFINITY) {
      float acc = s * __expf(m - mn);
#pragma unroll
      for (int k = 0; k < 8; k++) acc += __expf(v[k] - mn);
      s = acc;
      m = mn;
    }
  }
  if (tid < sp.nscalar) {
    const float v = __bfloat162float(xr[ce_scalar_col(sp, tid)]);
    ce_combine(m, s, v, 1.f);
    // fmaxf drops a NaN, and a lane that has seen no finite logit (none has a
    // vector of its own when V is small) would stay at (-inf, 0), which every
    // later combine with another empty lane resets to s = 0: the row's loss
    // would come out finite. A finite m keeps the NaN in s through them all;
    // its value is of no account, every output of the row is NaN.
    if (v != v) {
      m = 0.f;
      s = v;
    }
  }

#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float m2 = __shfl_xor(m, off, 64);
    const float s2 = __shfl_xor(s, off, 64);
    ce_combine(m, s, m2, s2);
  }
  __shared__ float wm[kCeWaves];
  __shared__ float ws[kCeWaves];
  if ((tid & 63) == 0) {
    wm[tid >> 6] = m;
    ws[tid >> 6] = s;
  }
  __syncthreads();
  m = wm[0];
  s = ws[0];
#pragma unroll
  for (int w = 1; w < kCeWaves; w++) ce_combine(m, s, wm[w], ws[w]);

  const float log_s = logf(s);
  const float lse = m + log_s;
  if (tid == 0) {
    // (m - x[t]) first: both are bf16 values, so the large magnitudes
    // cancel before the O(log V) term is added
    row_loss[row] = (m - xt) + log_s + z * lse * lse;
  }
  if (!write_grad) return;

  // ---- pass 2: gradient in place ------------------------------------------
  const float gs = *grad_scale_p;
  // softmax = exp(x - m) / s, keeping the exponent argument an exact bf16
  // difference instead of x - lse
  const float coef = t_ok ? gs * (1.f + 2.f * z * lse) / s : NAN;
  for (int i = tid; i < sp.nvec; i += kCeThreads) {
    float v[8];
    load8(xv + 8 * i, v);
    const int col0 = sp.head + 8 * i;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const float g = coef * __expf(v[k] - m);
      v[k] = (col0 + k == tcol) ? g - gs : g;
    }
    store8(xv + 8 * i, v);
  }
  if (tid < sp.nscalar) {
    const int col = ce_scalar_col(sp, tid);
    float g = coef * __expf(__bfloat162float(xr[col]) - m);
    if (col == tcol) g -= gs;
    xr[col] = __float2bfloat16(g);
  }
}

}  // namespace

void launch_cross_entropy(void* logits, const int64_t* targets, float* row_loss,
                          const float* grad_scale, int64_t rows, int V,
                          int64_t ignore_index, float z_loss, bool write_grad,
                          hipStream_t stream) {
  if (rows == 0) return;
  hipLaunchKernelGGL(cross_entropy_kernel, dim3((uint32_t)rows), dim3(kCeThreads),
                     0, stream, (bf16*)logits, targets, row_loss, grad_scale, rows,
                     V, ignore_index, z_loss, write_grad ? 1 : 0);
}

}  // namespace torchft_amd
