// Multi-tensor fused AdamW step — CDNA4 (gfx950) native.
//
// One kernel launch updates every parameter tensor: bf16 params/grads,
// fp32 exp_avg/exp_avg_sq. The block→tensor mapping reuses the fp8-quant
// scheme (2048-element blocks, per-tensor padding, wave-uniform binary
// search) so the launch is a single uniform grid regardless of the
// parameter-shape zoo. HBM-bound: 4 reads + 3 writes per element, all
// 16 B/lane vectorized.
//
// Serves as the DiLoCo fused outer-optimizer step and the bench's inner
// optimizer (reference analogue: torchft delegates to torch.optim).

#include <hip/hip_runtime.h>

#include "multi_tensor.h"
#include "philox.h"

namespace torchft_amd {

using bf16 = __hip_bfloat16;

// bf16 bits of v rounded at random with r16 (philox.h); inf and NaN are stored
// as from_f32 stores them: added bits could carry a NaN out of the NaNs
__device__ inline uint32_t sr_bits(float v, uint32_t r16) {
  const uint32_t b = __float_as_uint(v);
  if (sr_finite(b)) return sr_bf16(b, r16);
  bf16 t;
  from_f32(&t, v);
  return __bfloat16_as_ushort(t);
}

// Table columns: 0 param, 1 grad (bf16), 2 exp_avg, 3 exp_avg_sq (fp32) and,
// in clip mode, 4 the device step counts. kClip = false is the plain step:
// bias corrections come from the host and stats/max_norm are unused (null).
// kClip = true is the clip mode: stats[0] holds the global sum of squared gradients (grad_norm.hip), the
// clip coefficient is folded into the gradient read, a non-finite norm
// leaves p/m/v untouched, and the bias corrections come from the per-tensor
// device step counts (bumped afterwards by adamw_bump_steps_kernel), so a
// skipped step costs no host sync and no bias-correction step.
//
// kRound (kernels.h, AdamwRounding; docs/KERNELS.md, "Rounding modes") is how
// p' reaches memory, the arithmetic of the step being one expression for all:
//   kRoundNearest     one round-to-nearest bf16 store. `key` is an empty pack,
//                     so these two instantiations have the argument list, and
//                     the ISA, they had before the template parameter.
//   kRoundStochastic  p' is rounded up or down at random, E[stored] = p'. The
//                     lane's 8 x 16 bits are one Philox4x32-10 call: counter
//                     {off / 8 low, high, step count being taken, stream id
//                     (the next column, a number)}, key = the seed (`key` is
//                     one SrKey). Nothing of the launch enters, so a tensor
//                     draws the same bits on the 16 B and the element path, in
//                     any table or block, and again when a skipped step is
//                     retried.
//   kRoundMaster      the next column is the fp32 master copy. It is the
//                     truth wherever bf16(master) has the bits of the stored
//                     p; elsewhere someone wrote p behind the optimizer's back
//                     and float(p) is. The step runs on that value, stores it
//                     as the new master and p = bf16(master).
template <bool kClip, int kRound, typename... Key>
__global__ void adamw_kernel(MultiTensorTable tb, float lr, float beta1, float beta2,
                             float eps, float weight_decay, float bc1, float bc2,
                             const float* __restrict__ stats, float max_norm, Key... key) {
  constexpr int kExtraCol = kClip ? 5 : 4;
  float coef = 1.f;
  if constexpr (kClip) {
    const float norm = sqrtf(stats[0]);
    if (!isfinite(norm)) return;  // skipped step: no store at all
    coef = fminf(1.f, max_norm / (norm + 1e-6f));  // torch's definition
  }
  const MtCursor c(tb, blockIdx.x, threadIdx.x);
  const int cnt = c.cnt;
  if (cnt == 0) return;
  int32_t taking = 0;  // the step count being taken, clip mode
  if constexpr (kClip) {
    taking = *reinterpret_cast<const int32_t*>(c.addr(tb, 4)) + 1;
    const float s = (float)taking;
    bc1 = 1.f - powf(beta1, s);
    bc2 = 1.f - powf(beta2, s);
  }

  const int64_t ap = c.addr(tb, 0), ag = c.addr(tb, 1);
  const int64_t am = c.addr(tb, 2), av = c.addr(tb, 3);
  bf16* p = c.at<bf16>(ap);
  const bf16* g = c.at<const bf16>(ag);
  float* m = c.at<float>(am);
  float* v = c.at<float>(av);

  int64_t aw = 0;
  if constexpr (kRound == kRoundMaster) aw = c.addr(tb, kExtraCol);
  float* w = c.at<float>(aw);

  const bool full = c.vec_ok(ap | ag | am | av | aw);

  float pv[kMtEpt], gv[kMtEpt], mv[kMtEpt], vv[kMtEpt];
  [[maybe_unused]] float wv[kMtEpt];
  if (full) {
    load8(p, pv);
    load8(g, gv);
    load8(m, mv);
    load8(v, vv);
    if constexpr (kRound == kRoundMaster) load8(w, wv);
  } else {
    for (int i = 0; i < cnt; i++) {
      pv[i] = to_f32(p[i]);
      gv[i] = to_f32(g[i]);
      mv[i] = m[i];
      vv[i] = v[i];
      if constexpr (kRound == kRoundMaster) wv[i] = w[i];
    }
  }

  if constexpr (kRound == kRoundMaster) {
    // per element, no flag and no sync; a NaN on either side compares unequal
    // or equal and is a NaN whichever is taken
#pragma unroll
    for (int i = 0; i < kMtEpt; i++) {
      if (!full && i >= cnt) break;
      if (__float_as_uint(d_round((bf16*)nullptr, wv[i])) == __float_as_uint(pv[i]))
        pv[i] = wv[i];
    }
  }

  if constexpr (kClip) {
    // Scale once, then hide the product from the optimizer: the update below
    // must see an opaque value, as the plain kernel sees its loaded gradient,
    // so that both instantiations get the same fma contraction and a
    // coefficient of exactly 1.0 reproduces the plain kernel's moments bit for
    // bit (tests/test_grad_clip_gpu.py holds them to that).
#pragma unroll
    for (int i = 0; i < kMtEpt; i++) {
      if (full || i < cnt) gv[i] *= coef;
      asm volatile("" : "+v"(gv[i]));
    }
  }

#pragma unroll
  for (int i = 0; i < kMtEpt; i++) {
    if (!full && i >= cnt) break;
    mv[i] = beta1 * mv[i] + (1.f - beta1) * gv[i];
    vv[i] = beta2 * vv[i] + (1.f - beta2) * gv[i] * gv[i];
    const float mhat = mv[i] / bc1;
    const float vhat = vv[i] / bc2;
    // decoupled weight decay
    pv[i] -= lr * (mhat / (sqrtf(vhat) + eps) + weight_decay * pv[i]);
  }

  if constexpr (kRound == kRoundStochastic) {
    const SrKey k{key...};
    const uint64_t vec = (uint64_t)c.off / kMtEpt;
    const Philox4 r = philox4x32_10(
        Philox4{{(uint32_t)vec, (uint32_t)(vec >> 32), kClip ? (uint32_t)taking : k.step,
                 (uint32_t)c.addr(tb, kExtraCol)}},
        k.seed_lo, k.seed_hi);
    if (full) {
      uint32_t raw[4];
#pragma unroll
      for (int i = 0; i < 4; i++)
        raw[i] = sr_bits(pv[2 * i], philox_r16(r, 2 * i)) |
                 sr_bits(pv[2 * i + 1], philox_r16(r, 2 * i + 1)) << 16;
      *reinterpret_cast<uint4*>(p) = make_uint4(raw[0], raw[1], raw[2], raw[3]);
      store8(m, mv);
      store8(v, vv);
    } else {
#pragma unroll
      for (int i = 0; i < kMtEpt; i++) {
        if (i >= cnt) break;
        p[i] = __ushort_as_bfloat16((unsigned short)sr_bits(pv[i], philox_r16(r, i)));
        m[i] = mv[i];
        v[i] = vv[i];
      }
    }
    return;
  }

  if (full) {
    store8(p, pv);
    store8(m, mv);
    store8(v, vv);
    if constexpr (kRound == kRoundMaster) store8(w, pv);
  } else {
    for (int i = 0; i < cnt; i++) {
      from_f32(p + i, pv[i]);
      m[i] = mv[i];
      v[i] = vv[i];
      if constexpr (kRound == kRoundMaster) w[i] = pv[i];
    }
  }
}

// adamw_kernel<kClip, kRound, Key...> with what the mode does not read
// (kernels.h, AdamwLaunch) filled in: bias corrections of 1, no stats
template <bool kClip, int kRound, typename... Key>
static void launch_as(const AdamwLaunch& a, hipStream_t stream, Key... key) {
  hipLaunchKernelGGL((adamw_kernel<kClip, kRound, Key...>), dim3((uint32_t)a.tb.total_blocks),
                     dim3(kMtThreads), 0, stream, a.tb, a.lr, a.beta1, a.beta2, a.eps,
                     a.weight_decay, kClip ? 1.f : a.bc1, kClip ? 1.f : a.bc2,
                     kClip ? a.stats : (const float*)nullptr, kClip ? a.max_norm : 0.f, key...);
}

void launch_adamw(const AdamwLaunch& a, hipStream_t stream) {
  if (a.tb.total_blocks <= 0) return;
  if (a.rounding == kRoundStochastic)
    a.clip ? launch_as<true, kRoundStochastic>(a, stream, a.key)
           : launch_as<false, kRoundStochastic>(a, stream, a.key);
  else if (a.rounding == kRoundMaster)
    a.clip ? launch_as<true, kRoundMaster>(a, stream) : launch_as<false, kRoundMaster>(a, stream);
  else
    a.clip ? launch_as<true, kRoundNearest>(a, stream) : launch_as<false, kRoundNearest>(a, stream);
}

// One thread per participating tensor, after every group's update on the same
// stream: a finite norm advances each device step count, a non-finite one
// advances the skipped counter instead. Thread 0 also publishes the norm.
__global__ void adamw_bump_steps_kernel(const int64_t* __restrict__ step_ptrs,
                                        int n_tensors,
                                        const float* __restrict__ stats,
                                        int32_t* __restrict__ skipped,
                                        float* __restrict__ norm_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const float norm = sqrtf(stats[0]);
  if (i == 0) norm_out[0] = norm;
  if (isfinite(norm)) {
    if (i < n_tensors) *reinterpret_cast<int32_t*>(step_ptrs[i]) += 1;
  } else if (i == 0) {
    skipped[0] += 1;
  }
}

void launch_adamw_bump_steps(const int64_t* step_ptrs, int n_tensors,
                             const float* stats, int32_t* skipped, float* norm_out,
                             hipStream_t stream) {
  if (n_tensors <= 0) return;
  hipLaunchKernelGGL(adamw_bump_steps_kernel, dim3((n_tensors + 255) / 256),
                     dim3(256), 0, stream, step_ptrs, n_tensors, stats, skipped,
                     norm_out);
}

}  // namespace torchft_amd
