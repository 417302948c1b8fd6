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

namespace torchft_amd {

using bf16 = __hip_bfloat16;

// Table columns: 0 param, 1 grad (bf16), 2 exp_avg, 3 exp_avg_sq (fp32) and,
// in clip mode, 4 the device step counts. kClip = false is the plain step:
// bias corrections come from the host and stats/max_norm are unused (null).
// kClip = true is the clip mode: stats[0] holds the global sum of squared gradients (grad_norm.hip), the
// clip coefficient is folded into the gradient read, a non-finite norm
// leaves p/m/v untouched, and the bias corrections come from the per-tensor
// device step counts (bumped afterwards by adamw_bump_steps_kernel), so a
// skipped step costs no host sync and no bias-correction step.
template <bool kClip>
__global__ void adamw_kernel(MultiTensorTable tb, float lr, float beta1, float beta2,
                             float eps, float weight_decay, float bc1, float bc2,
                             const float* __restrict__ stats, float max_norm) {
  float coef = 1.f;
  if constexpr (kClip) {
    const float norm = sqrtf(stats[0]);
    if (!isfinite(norm)) return;  // skipped step: no store at all
    coef = fminf(1.f, max_norm / (norm + 1e-6f));  // torch's definition
  }
  const MtCursor c(tb, blockIdx.x, threadIdx.x);
  const int cnt = c.cnt;
  if (cnt == 0) return;
  if constexpr (kClip) {
    const float s = (float)(*reinterpret_cast<const int32_t*>(c.addr(tb, 4)) + 1);
    bc1 = 1.f - powf(beta1, s);
    bc2 = 1.f - powf(beta2, s);
  }

  const int64_t ap = c.addr(tb, 0), ag = c.addr(tb, 1);
  const int64_t am = c.addr(tb, 2), av = c.addr(tb, 3);
  bf16* p = c.at<bf16>(ap);
  const bf16* g = c.at<const bf16>(ag);
  float* m = c.at<float>(am);
  float* v = c.at<float>(av);

  const bool full = c.vec_ok(ap | ag | am | av);

  float pv[kMtEpt], gv[kMtEpt], mv[kMtEpt], vv[kMtEpt];
  if (full) {
    load8(p, pv);
    load8(g, gv);
    load8(m, mv);
    load8(v, vv);
  } else {
    for (int i = 0; i < cnt; i++) {
      pv[i] = to_f32(p[i]);
      gv[i] = to_f32(g[i]);
      mv[i] = m[i];
      vv[i] = v[i];
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

  if (full) {
    store8(p, pv);
    store8(m, mv);
    store8(v, vv);
  } else {
    for (int i = 0; i < cnt; i++) {
      from_f32(p + i, pv[i]);
      m[i] = mv[i];
      v[i] = vv[i];
    }
  }
}

void launch_adamw(MultiTensorTable tb, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float bias_correction1,
                  float bias_correction2, hipStream_t stream) {
  if (tb.total_blocks <= 0) return;
  hipLaunchKernelGGL(adamw_kernel<false>, dim3((uint32_t)tb.total_blocks),
                     dim3(kMtThreads), 0, stream, tb, lr, beta1, beta2, eps,
                     weight_decay, bias_correction1, bias_correction2,
                     (const float*)nullptr, 0.f);
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

void launch_adamw_clip(MultiTensorTable tb, float lr, float beta1, float beta2,
                       float eps, float weight_decay, const float* stats,
                       float max_norm, hipStream_t stream) {
  if (tb.total_blocks <= 0) return;
  hipLaunchKernelGGL(adamw_kernel<true>, dim3((uint32_t)tb.total_blocks),
                     dim3(kMtThreads), 0, stream, tb, lr, beta1, beta2, eps,
                     weight_decay, 1.f, 1.f, stats, max_norm);
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
