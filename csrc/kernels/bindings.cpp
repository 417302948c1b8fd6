// torch-extension bindings for the CDNA4 kernels (fp8 quantized-collective
// trio, fused model ops, fused AdamW, DiLoCo outer sync). Tensor-level API consumed by
// torchft_amd.ops / torchft_amd.quantization.
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include <algorithm>
#include <cmath>

#include <vector>

#include "kernels.h"

namespace tft = torchft_amd;

namespace {

constexpr int64_t kQBlock = 2048;

struct PackGeom {
  int64_t total_blocks = 0;
  int64_t padded_blocks = 0;
  int64_t blocks_per_rank = 0;
  int64_t slice_bytes = 0;
};

PackGeom pack_geometry(const std::vector<at::Tensor>& tensors, int64_t world) {
  PackGeom g;
  for (auto& t : tensors) g.total_blocks += (t.numel() + kQBlock - 1) / kQBlock;
  g.padded_blocks = ((g.total_blocks + world - 1) / world) * world;
  g.blocks_per_rank = g.padded_blocks / world;
  g.slice_bytes = g.blocks_per_rank * (4 + kQBlock);
  return g;
}

// Builds the device-side metadata arrays (ptrs, block prefix, numels).
struct DeviceMeta {
  at::Tensor ptrs, prefix, numels;
};

DeviceMeta build_meta(const std::vector<at::Tensor>& tensors) {
  const int64_t n = (int64_t)tensors.size();
  auto opts = at::TensorOptions().dtype(at::kLong).pinned_memory(true);
  at::Tensor host = at::empty({3 * n + 1}, opts);
  int64_t* h = host.data_ptr<int64_t>();
  int64_t* ptrs = h;
  int64_t* numels = h + n;
  int64_t* prefix = h + 2 * n;  // n+1 entries
  int64_t acc = 0;
  for (int64_t i = 0; i < n; i++) {
    auto& t = tensors[i];
    TORCH_CHECK(t.is_contiguous(), "fp8 pack requires contiguous tensors");
    TORCH_CHECK(t.is_cuda(), "fp8 pack requires device tensors");
    ptrs[i] = (int64_t)t.data_ptr();
    numels[i] = t.numel();
    prefix[i] = acc;
    acc += (t.numel() + kQBlock - 1) / kQBlock;
  }
  prefix[n] = acc;
  at::Tensor dev = host.to(tensors[0].device(), /*non_blocking=*/true);
  DeviceMeta m;
  m.ptrs = dev.narrow(0, 0, n);
  m.numels = dev.narrow(0, n, n);
  m.prefix = dev.narrow(0, 2 * n, n + 1);
  return m;
}

}  // namespace

// ---- fp8 quantized-collective support --------------------------------------

int64_t fp8_pack_bytes(const std::vector<at::Tensor>& tensors, int64_t world) {
  auto g = pack_geometry(tensors, world);
  return g.slice_bytes * world;
}

int64_t fp8_slice_bytes(const std::vector<at::Tensor>& tensors, int64_t world) {
  return pack_geometry(tensors, world).slice_bytes;
}

void fp8_quantize(const std::vector<at::Tensor>& tensors, at::Tensor pack,
                  int64_t world) {
  TORCH_CHECK(!tensors.empty(), "need at least one tensor");
  auto g = pack_geometry(tensors, world);
  TORCH_CHECK(pack.numel() >= g.slice_bytes * world, "pack buffer too small");
  auto meta = build_meta(tensors);
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  auto st = tensors[0].scalar_type();
  for (auto& t : tensors) TORCH_CHECK(t.scalar_type() == st, "mixed dtypes");
  const int64_t* ptrs = meta.ptrs.data_ptr<int64_t>();
  const int64_t* prefix = meta.prefix.data_ptr<int64_t>();
  const int64_t* numels = meta.numels.data_ptr<int64_t>();
  uint8_t* p = pack.data_ptr<uint8_t>();
  int code = st == at::kBFloat16 ? 0 : st == at::kHalf ? 1 : st == at::kFloat ? 2 : -1;
  TORCH_CHECK(code >= 0, "unsupported dtype for fp8 quantize: ", st);
  tft::launch_quantize_dtype(code, ptrs, prefix, numels, (int)tensors.size(),
                             g.total_blocks, g.padded_blocks, g.blocks_per_rank,
                             g.slice_bytes, p, (tft_stream)stream);
}

void fp8_dequantize(const std::vector<at::Tensor>& tensors, at::Tensor pack,
                    int64_t world) {
  TORCH_CHECK(!tensors.empty(), "need at least one tensor");
  auto g = pack_geometry(tensors, world);
  auto meta = build_meta(tensors);
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  auto st = tensors[0].scalar_type();
  const int64_t* ptrs = meta.ptrs.data_ptr<int64_t>();
  const int64_t* prefix = meta.prefix.data_ptr<int64_t>();
  const int64_t* numels = meta.numels.data_ptr<int64_t>();
  const uint8_t* p = pack.data_ptr<uint8_t>();
  int code = st == at::kBFloat16 ? 0 : st == at::kHalf ? 1 : st == at::kFloat ? 2 : -1;
  TORCH_CHECK(code >= 0, "unsupported dtype for fp8 dequantize: ", st);
  tft::launch_dequantize_dtype(code, ptrs, prefix, numels, (int)tensors.size(),
                               g.total_blocks, g.padded_blocks, g.blocks_per_rank,
                               g.slice_bytes, p, (tft_stream)stream);
}

void fp8_reduce(at::Tensor recv, at::Tensor out, int64_t world, bool avg) {
  TORCH_CHECK(recv.is_cuda() && out.is_cuda());
  TORCH_CHECK(recv.numel() == out.numel() * world, "recv must hold world slices");
  const int64_t slice_bytes = out.numel();
  const int64_t blocks_per_rank = slice_bytes / (4 + kQBlock);
  TORCH_CHECK(blocks_per_rank * (4 + kQBlock) == slice_bytes, "bad slice size");
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  tft::launch_reduce(recv.data_ptr<uint8_t>(), out.data_ptr<uint8_t>(), (int)world,
                     blocks_per_rank, slice_bytes, avg, (tft_stream)stream);
}

// ---- fused model ops --------------------------------------------------------

std::vector<at::Tensor> rmsnorm_fwd(at::Tensor x, at::Tensor w, double eps) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.is_contiguous());
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kBFloat16 && w.is_contiguous());
  const int H = (int)x.size(-1);
  TORCH_CHECK(H % 8 == 0, "hidden dim must be a multiple of 8");
  const int64_t rows = x.numel() / H;
  auto y = at::empty_like(x);
  auto invrms = at::empty({rows}, x.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  tft::launch_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(),
                          invrms.data_ptr<float>(), rows, H, (float)eps,
                          (tft_stream)stream);
  return {y, invrms};
}

std::vector<at::Tensor> rmsnorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor w,
                                    at::Tensor invrms) {
  const int H = (int)x.size(-1);
  const int64_t rows = x.numel() / H;
  TORCH_CHECK(H * sizeof(float) <= 160 * 1024, "H too large for LDS dw buffer");
  auto dx = at::empty_like(x);
  auto dw = at::zeros({H}, x.options().dtype(at::kFloat));
  auto dyc = dy.contiguous();
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  tft::launch_rmsnorm_bwd(dyc.data_ptr(), x.data_ptr(), w.data_ptr(),
                          invrms.data_ptr<float>(), dx.data_ptr(),
                          dw.data_ptr<float>(), rows, H, (tft_stream)stream);
  return {dx, dw};
}

at::Tensor rope_apply(at::Tensor x, at::Tensor cos_tab, at::Tensor sin_tab,
                      bool backward) {
  // x: [B, S, Hh, D]
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 4);
  auto xc = x.contiguous();
  const int S = (int)x.size(1);
  const int Hh = (int)x.size(2);
  const int D = (int)x.size(3);
  TORCH_CHECK(D % 8 == 0, "head dim must be a multiple of 8");
  TORCH_CHECK(cos_tab.size(0) >= S && cos_tab.size(1) == D / 2, "cos table shape");
  auto out = at::empty_like(xc);
  const int64_t total_pairs = xc.numel() / 2;
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  tft::launch_rope(xc.data_ptr(), out.data_ptr(), cos_tab.data_ptr<float>(),
                   sin_tab.data_ptr<float>(), total_pairs, S, Hh, D, backward,
                   (tft_stream)stream);
  return out;
}

at::Tensor swiglu_fwd(at::Tensor a, at::Tensor b) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == at::kBFloat16);
  TORCH_CHECK(a.numel() % 8 == 0, "numel must be a multiple of 8");
  auto ac = a.contiguous();
  auto bc = b.contiguous();
  auto out = at::empty_like(ac);
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  tft::launch_swiglu_fwd(ac.data_ptr(), bc.data_ptr(), out.data_ptr(), ac.numel(),
                         (tft_stream)stream);
  return out;
}

at::Tensor swiglu_glu_fwd(at::Tensor gu) {
  TORCH_CHECK(gu.is_cuda() && gu.scalar_type() == at::kBFloat16);
  auto guc = gu.contiguous();
  const int64_t f = guc.size(-1) / 2;
  const int64_t rows = guc.numel() / (2 * f);
  TORCH_CHECK(f % 8 == 0, "glu width must be a multiple of 8");
  auto sizes = guc.sizes().vec();
  sizes.back() = f;
  auto out = at::empty(sizes, guc.options());
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  tft::launch_swiglu_glu_fwd(guc.data_ptr(), out.data_ptr(), rows, f,
                             (tft_stream)stream);
  return out;
}

at::Tensor swiglu_glu_bwd(at::Tensor dy, at::Tensor gu) {
  auto dyc = dy.contiguous();
  auto guc = gu.contiguous();
  const int64_t f = guc.size(-1) / 2;
  const int64_t rows = guc.numel() / (2 * f);
  auto dgu = at::empty_like(guc);
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  tft::launch_swiglu_glu_bwd(dyc.data_ptr(), guc.data_ptr(), dgu.data_ptr(),
                             rows, f, (tft_stream)stream);
  return dgu;
}

std::vector<at::Tensor> swiglu_bwd(at::Tensor dy, at::Tensor a, at::Tensor b) {
  auto dyc = dy.contiguous();
  auto ac = a.contiguous();
  auto bc = b.contiguous();
  auto da = at::empty_like(ac);
  auto db = at::empty_like(bc);
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  tft::launch_swiglu_bwd(dyc.data_ptr(), ac.data_ptr(), bc.data_ptr(),
                         da.data_ptr(), db.data_ptr(), ac.numel(),
                         (tft_stream)stream);
  return {da, db};
}

// ---- fused AdamW ------------------------------------------------------------

void adamw_step(const std::vector<at::Tensor>& params,
                const std::vector<at::Tensor>& grads,
                const std::vector<at::Tensor>& exp_avgs,
                const std::vector<at::Tensor>& exp_avg_sqs, double lr,
                double beta1, double beta2, double eps, double weight_decay,
                int64_t step) {
  const int64_t n = (int64_t)params.size();
  TORCH_CHECK(n > 0);
  auto opts = at::TensorOptions().dtype(at::kLong).pinned_memory(true);
  at::Tensor host = at::empty({6 * n + 1}, opts);
  int64_t* h = host.data_ptr<int64_t>();
  int64_t acc = 0;
  for (int64_t i = 0; i < n; i++) {
    TORCH_CHECK(params[i].is_contiguous() && grads[i].is_contiguous());
    TORCH_CHECK(params[i].scalar_type() == at::kBFloat16, "params must be bf16");
    TORCH_CHECK(exp_avgs[i].scalar_type() == at::kFloat, "states must be fp32");
    h[i] = (int64_t)params[i].data_ptr();
    h[n + i] = (int64_t)grads[i].data_ptr();
    h[2 * n + i] = (int64_t)exp_avgs[i].data_ptr();
    h[3 * n + i] = (int64_t)exp_avg_sqs[i].data_ptr();
    h[4 * n + i] = params[i].numel();
    h[5 * n + i] = acc;
    acc += (params[i].numel() + kQBlock - 1) / kQBlock;
  }
  h[6 * n] = acc;
  at::Tensor dev = host.to(params[0].device(), /*non_blocking=*/true);
  const int64_t* d = dev.data_ptr<int64_t>();
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  const float bc1 = 1.0f - std::pow((float)beta1, (float)step);
  const float bc2 = 1.0f - std::pow((float)beta2, (float)step);
  tft::launch_adamw(d, d + n, d + 2 * n, d + 3 * n, d + 4 * n, d + 5 * n, (int)n,
                    acc, (float)lr, (float)beta1, (float)beta2, (float)eps,
                    (float)weight_decay, bc1, bc2, (tft_stream)stream);
}

// ---- global gradient norm / clip ---------------------------------------------

namespace {

// One device table per call: for every dtype present, [ptrs | numels |
// block_prefix (n+1)] back to back, built in pinned memory and copied once.
struct GradGroup {
  int code = 0;  // dtype_code of kernels.h
  std::vector<const at::Tensor*> ts;
  int64_t off = 0;     // first int64 of this group's table
  int64_t blocks = 0;  // logical 2048-element blocks
};

struct GradTables {
  at::Tensor dev;
  std::vector<GradGroup> groups;
};

GradTables build_grad_tables(const std::vector<at::Tensor>& tensors) {
  TORCH_CHECK(!tensors.empty(), "need at least one tensor");
  GradTables tb;
  tb.groups.resize(3);
  for (int c = 0; c < 3; c++) tb.groups[c].code = c;
  for (auto& t : tensors) {
    TORCH_CHECK(t.is_cuda(), "grad norm requires device tensors");
    TORCH_CHECK(t.device() == tensors[0].device(), "tensors on different devices");
    TORCH_CHECK(t.is_contiguous(), "grad norm requires contiguous tensors");
    auto st = t.scalar_type();
    int code = st == at::kBFloat16 ? 0 : st == at::kHalf ? 1 : st == at::kFloat ? 2 : -1;
    TORCH_CHECK(code >= 0, "unsupported dtype for grad norm: ", st);
    if (t.numel() > 0) tb.groups[code].ts.push_back(&t);
  }
  int64_t words = 0;
  for (auto& g : tb.groups) {
    g.off = words;
    if (!g.ts.empty()) words += 3 * (int64_t)g.ts.size() + 1;
  }
  auto opts = at::TensorOptions().dtype(at::kLong).pinned_memory(true);
  at::Tensor host = at::empty({std::max<int64_t>(words, 1)}, opts);
  int64_t* h = host.data_ptr<int64_t>();
  for (auto& g : tb.groups) {
    const int64_t n = (int64_t)g.ts.size();
    int64_t* ptrs = h + g.off;
    int64_t* numels = ptrs + n;
    int64_t* prefix = numels + n;
    int64_t acc = 0;
    for (int64_t i = 0; i < n; i++) {
      ptrs[i] = (int64_t)g.ts[i]->data_ptr();
      numels[i] = g.ts[i]->numel();
      prefix[i] = acc;
      acc += (g.ts[i]->numel() + kQBlock - 1) / kQBlock;
    }
    if (n > 0) prefix[n] = acc;
    g.blocks = acc;
  }
  tb.dev = host.to(tensors[0].device(), /*non_blocking=*/true);
  return tb;
}

void check_max_blocks(int64_t max_blocks) {
  TORCH_CHECK(max_blocks >= 1 && max_blocks <= (int64_t(1) << 16),
              "max_blocks must be in [1, 65536], got ", max_blocks);
}

// partial sums per dtype group into one partials buffer, then one finalize
void run_sumsq(const GradTables& tb, int64_t max_blocks, at::Tensor& stats,
               tft_stream stream) {
  int64_t n_partials = 0;
  for (auto& g : tb.groups) n_partials += std::min(g.blocks, max_blocks);
  auto partials = at::empty({n_partials}, stats.options());
  const int64_t* d = tb.dev.data_ptr<int64_t>();
  int64_t at_partial = 0;
  for (auto& g : tb.groups) {
    const int64_t n = (int64_t)g.ts.size();
    const int64_t grid = std::min(g.blocks, max_blocks);
    if (grid == 0) continue;
    const int64_t* base = d + g.off;
    tft::launch_grad_sumsq_partial(g.code, base, base + n, base + 2 * n, (int)n,
                                   g.blocks, (int)grid,
                                   partials.data_ptr<float>() + at_partial, stream);
    at_partial += grid;
  }
  tft::launch_grad_sumsq_finalize(partials.data_ptr<float>(), (int)n_partials,
                                  stats.data_ptr<float>(), stream);
}

}  // namespace

// Sum of squares over every tensor, as a 1-element fp32 device tensor.
at::Tensor grad_sumsq(const std::vector<at::Tensor>& tensors, int64_t max_blocks) {
  check_max_blocks(max_blocks);
  auto tb = build_grad_tables(tensors);
  auto stats = at::empty({1}, tensors[0].options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  run_sumsq(tb, max_blocks, stats, (tft_stream)stream);
  return stats;
}

// Norm + in-place scale sharing one table; norm_reduce (or None) sees the
// 1-element sum of squares between the two. Returns the sum of squares.
at::Tensor clip_grad_norm(const std::vector<at::Tensor>& tensors, double max_norm,
                          int64_t max_blocks, py::object norm_reduce) {
  check_max_blocks(max_blocks);
  TORCH_CHECK(max_norm > 0.0, "max_norm must be > 0");
  auto tb = build_grad_tables(tensors);
  auto stats = at::empty({1}, tensors[0].options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  run_sumsq(tb, max_blocks, stats, (tft_stream)stream);
  if (!norm_reduce.is_none()) norm_reduce(stats);
  const int64_t* d = tb.dev.data_ptr<int64_t>();
  for (auto& g : tb.groups) {
    const int64_t n = (int64_t)g.ts.size();
    if (n == 0) continue;
    const int64_t* base = d + g.off;
    tft::launch_grad_scale(g.code, base, base + n, base + 2 * n, (int)n, g.blocks,
                           stats.data_ptr<float>(), (float)max_norm,
                           (tft_stream)stream);
  }
  return stats;
}

// FusedAdamW clip mode, one call per optimizer step. The tensor lists are flat
// over all param groups (group_sizes says how they split); the norm is global,
// then each group gets one update launch, then one launch bumps the device
// step counts (finite norm) or the skipped counter (non-finite).
void adamw_clip_step(const std::vector<at::Tensor>& params,
                     const std::vector<at::Tensor>& grads,
                     const std::vector<at::Tensor>& exp_avgs,
                     const std::vector<at::Tensor>& exp_avg_sqs,
                     const std::vector<at::Tensor>& steps,
                     const std::vector<int64_t>& group_sizes,
                     const std::vector<double>& lrs,
                     const std::vector<double>& beta1s,
                     const std::vector<double>& beta2s,
                     const std::vector<double>& epss,
                     const std::vector<double>& weight_decays, double max_norm,
                     int64_t max_blocks, at::Tensor stats, at::Tensor skipped,
                     at::Tensor norm_out, py::object norm_reduce) {
  const int64_t n = (int64_t)params.size();
  const int64_t ng = (int64_t)group_sizes.size();
  TORCH_CHECK(n > 0);
  TORCH_CHECK((int64_t)grads.size() == n && (int64_t)exp_avgs.size() == n &&
              (int64_t)exp_avg_sqs.size() == n && (int64_t)steps.size() == n);
  TORCH_CHECK((int64_t)lrs.size() == ng && (int64_t)beta1s.size() == ng &&
              (int64_t)beta2s.size() == ng && (int64_t)epss.size() == ng &&
              (int64_t)weight_decays.size() == ng);
  check_max_blocks(max_blocks);
  TORCH_CHECK(max_norm > 0.0, "max_grad_norm must be > 0");
  const auto dev = params[0].device();
  TORCH_CHECK(stats.device() == dev && stats.scalar_type() == at::kFloat &&
              stats.numel() >= 1 && stats.is_contiguous());
  TORCH_CHECK(norm_out.device() == dev && norm_out.scalar_type() == at::kFloat &&
              norm_out.numel() == 1);
  TORCH_CHECK(skipped.device() == dev && skipped.scalar_type() == at::kInt &&
              skipped.numel() == 1);

  // [param | grad | m | v | numel | step | prefix over all (n+1) |
  //  per-group prefixes (size_g + 1 each)]
  auto opts = at::TensorOptions().dtype(at::kLong).pinned_memory(true);
  at::Tensor host = at::empty({8 * n + 1 + ng}, opts);
  int64_t* h = host.data_ptr<int64_t>();
  int64_t* gprefix = h + 6 * n;
  int64_t* uprefix = h + 7 * n + 1;
  int64_t acc = 0;
  for (int64_t i = 0; i < n; i++) {
    TORCH_CHECK(params[i].is_cuda() && params[i].device() == dev &&
                grads[i].device() == dev && exp_avgs[i].device() == dev &&
                exp_avg_sqs[i].device() == dev && steps[i].device() == dev,
                "all tensors must be on the same device");
    TORCH_CHECK(params[i].is_contiguous() && grads[i].is_contiguous() &&
                exp_avgs[i].is_contiguous() && exp_avg_sqs[i].is_contiguous());
    TORCH_CHECK(params[i].scalar_type() == at::kBFloat16 &&
                grads[i].scalar_type() == at::kBFloat16,
                "params and grads must be bf16");
    TORCH_CHECK(exp_avgs[i].scalar_type() == at::kFloat &&
                exp_avg_sqs[i].scalar_type() == at::kFloat, "states must be fp32");
    const int64_t ne = params[i].numel();
    TORCH_CHECK(grads[i].numel() == ne && exp_avgs[i].numel() == ne &&
                exp_avg_sqs[i].numel() == ne, "size mismatch");
    TORCH_CHECK(steps[i].scalar_type() == at::kInt && steps[i].numel() == 1,
                "step must be a 1-element int32 device tensor");
    h[i] = (int64_t)params[i].data_ptr();
    h[n + i] = (int64_t)grads[i].data_ptr();
    h[2 * n + i] = (int64_t)exp_avgs[i].data_ptr();
    h[3 * n + i] = (int64_t)exp_avg_sqs[i].data_ptr();
    h[4 * n + i] = ne;
    h[5 * n + i] = (int64_t)steps[i].data_ptr();
    gprefix[i] = acc;
    acc += (ne + kQBlock - 1) / kQBlock;
  }
  gprefix[n] = acc;
  std::vector<int64_t> group_blocks(ng, 0);
  {
    int64_t first = 0, w = 0;
    for (int64_t g = 0; g < ng; g++) {
      TORCH_CHECK(group_sizes[g] >= 0 && first + group_sizes[g] <= n);
      for (int64_t i = 0; i <= group_sizes[g]; i++)
        uprefix[w + i] = gprefix[first + i] - gprefix[first];
      group_blocks[g] = gprefix[first + group_sizes[g]] - gprefix[first];
      w += group_sizes[g] + 1;
      first += group_sizes[g];
    }
    TORCH_CHECK(first == n, "group_sizes must cover every tensor");
  }
  at::Tensor table = host.to(dev, /*non_blocking=*/true);
  const int64_t* d = table.data_ptr<int64_t>();
  auto stream = (tft_stream)at::cuda::getCurrentCUDAStream().stream();

  const int64_t grid = std::min(acc, max_blocks);
  auto partials = at::empty({grid}, stats.options());
  tft::launch_grad_sumsq_partial(0, d + n, d + 4 * n, d + 6 * n, (int)n, acc,
                                 (int)grid, partials.data_ptr<float>(), stream);
  tft::launch_grad_sumsq_finalize(partials.data_ptr<float>(), (int)grid,
                                  stats.data_ptr<float>(), stream);
  if (!norm_reduce.is_none()) norm_reduce(stats.narrow(0, 0, 1));

  int64_t first = 0, w = 0;
  for (int64_t g = 0; g < ng; g++) {
    const int64_t cnt = group_sizes[g];
    if (cnt > 0)
      tft::launch_adamw_clip(d + first, d + n + first, d + 2 * n + first,
                             d + 3 * n + first, d + 4 * n + first,
                             d + 7 * n + 1 + w, d + 5 * n + first, (int)cnt,
                             group_blocks[g], (float)lrs[g], (float)beta1s[g],
                             (float)beta2s[g], (float)epss[g],
                             (float)weight_decays[g], stats.data_ptr<float>(),
                             (float)max_norm, stream);
    w += cnt + 1;
    first += cnt;
  }
  tft::launch_adamw_bump_steps(d + 5 * n, (int)n, stats.data_ptr<float>(),
                               skipped.data_ptr<int>(), norm_out.data_ptr<float>(),
                               stream);
}

// ---- fused DiLoCo outer sync ---------------------------------------------------

namespace {

// One pinned table for `lists.size()` parallel tensor lists of one dtype:
// [ptrs of list 0 | ... | ptrs of list k-1 | numels | block_prefix (n+1)],
// with zero-numel tensors left out. Copied to the device once.
struct SyncTable {
  at::Tensor dev;
  int64_t n = 0;       // tensors kept
  int64_t blocks = 0;  // logical 2048-element blocks
  int code = 0;        // dtype_code of kernels.h
};

SyncTable build_sync_table(const std::vector<const std::vector<at::Tensor>*>& lists,
                           const char* what) {
  const int64_t k = (int64_t)lists.size();
  const auto& first = *lists[0];
  const int64_t n_all = (int64_t)first.size();
  TORCH_CHECK(n_all > 0, what, ": need at least one tensor");
  const auto dev = first[0].device();
  const auto st = first[0].scalar_type();
  SyncTable tb;
  tb.code = st == at::kBFloat16 ? 0 : st == at::kHalf ? 1 : st == at::kFloat ? 2 : -1;
  TORCH_CHECK(tb.code >= 0, what, ": unsupported dtype ", st);
  std::vector<int64_t> keep;
  for (int64_t i = 0; i < n_all; i++) {
    for (int64_t j = 0; j < k; j++) {
      TORCH_CHECK((int64_t)lists[j]->size() == n_all, what, ": list lengths differ");
      const auto& t = (*lists[j])[i];
      TORCH_CHECK(t.is_cuda() && t.device() == dev, what,
                  ": all tensors must be on one device");
      TORCH_CHECK(t.scalar_type() == st, what, ": mixed dtypes (", st, " and ",
                  t.scalar_type(), ")");
      TORCH_CHECK(t.is_contiguous(), what, ": tensors must be contiguous");
      TORCH_CHECK(t.numel() == first[i].numel(), what, ": size mismatch at tensor ", i);
    }
    if (first[i].numel() > 0) keep.push_back(i);
  }
  tb.n = (int64_t)keep.size();
  if (tb.n == 0) return tb;
  const int64_t n = tb.n;
  auto opts = at::TensorOptions().dtype(at::kLong).pinned_memory(true);
  at::Tensor host = at::empty({(k + 2) * n + 1}, opts);
  int64_t* h = host.data_ptr<int64_t>();
  int64_t* numels = h + k * n;
  int64_t* prefix = h + (k + 1) * n;
  int64_t acc = 0;
  for (int64_t i = 0; i < n; i++) {
    for (int64_t j = 0; j < k; j++) h[j * n + i] = (int64_t)(*lists[j])[keep[i]].data_ptr();
    numels[i] = first[keep[i]].numel();
    prefix[i] = acc;
    acc += (numels[i] + kQBlock - 1) / kQBlock;
  }
  prefix[n] = acc;
  TORCH_CHECK(acc < (int64_t(1) << 31), what, ": too many elements for one launch");
  tb.blocks = acc;
  tb.dev = host.to(dev, /*non_blocking=*/true);
  return tb;
}

}  // namespace

// outs[i] = minuends[i] - subtrahends[i], one launch for the whole list
void diloco_pseudograd(const std::vector<at::Tensor>& outs,
                       const std::vector<at::Tensor>& minuends,
                       const std::vector<at::Tensor>& subtrahends) {
  auto tb = build_sync_table({&outs, &minuends, &subtrahends}, "pseudograd_");
  if (tb.n == 0) return;
  const int64_t n = tb.n;
  const int64_t* d = tb.dev.data_ptr<int64_t>();
  auto stream = (tft_stream)at::cuda::getCurrentCUDAStream().stream();
  tft::launch_pseudograd(tb.code, d, d + n, d + 2 * n, d + 3 * n, d + 4 * n, (int)n,
                         tb.blocks, stream);
}

// Outer SGD step + re-snapshot + lerp for one param group; momentum_bufs is
// empty when momentum == 0.
void diloco_outer_step(const std::vector<at::Tensor>& snapshots,
                       const std::vector<at::Tensor>& params,
                       const std::vector<at::Tensor>& pseudograds,
                       const std::vector<at::Tensor>& momentum_bufs, double lr,
                       double momentum, bool nesterov, double alpha) {
  const bool has_m = momentum != 0.0;
  TORCH_CHECK(has_m == !momentum_bufs.empty(),
              "diloco_outer_step_: momentum buffers are needed exactly when "
              "momentum != 0");
  TORCH_CHECK(alpha >= 0.0 && alpha <= 1.0, "alpha must be in [0, 1], got ", alpha);
  std::vector<const std::vector<at::Tensor>*> lists = {&snapshots, &params, &pseudograds};
  if (has_m) lists.push_back(&momentum_bufs);
  auto tb = build_sync_table(lists, "diloco_outer_step_");
  if (tb.n == 0) return;
  const int64_t n = tb.n;
  const int64_t k = (int64_t)lists.size();
  const int64_t* d = tb.dev.data_ptr<int64_t>();
  auto stream = (tft_stream)at::cuda::getCurrentCUDAStream().stream();
  tft::launch_outer_sgd(tb.code, has_m, d, d + n, d + 2 * n,
                        has_m ? d + 3 * n : nullptr, d + k * n, d + (k + 1) * n, (int)n,
                        tb.blocks, (float)lr, (float)momentum, nesterov, (float)alpha,
                        stream);
}

// ---- flash attention backward (appended) -----------------------------------

// true when a logical [B,H,S,D] tensor is a transpose view of contiguous
// [B,S,H,D] storage (the model's projection layout)
static bool is_bshd(const at::Tensor& t) {
  return t.dim() == 4 && t.stride(3) == 1 && t.stride(1) == t.size(3) &&
         t.stride(2) == t.size(1) * t.size(3) &&
         t.stride(0) == t.size(1) * t.size(2) * t.size(3);
}

// contiguous in logical [B,H,S,D] order
static bool is_bhsd(const at::Tensor& t) { return t.is_contiguous(); }

at::Tensor fa_delta(at::Tensor dout, at::Tensor out) {
  TORCH_CHECK(dout.is_cuda() && dout.scalar_type() == at::kBFloat16);
  TORCH_CHECK(dout.size(-1) == 128);
  const bool bshd = is_bshd(dout) && is_bshd(out);
  auto dc = bshd ? dout : dout.contiguous();
  auto oc = bshd ? out : out.contiguous();
  const int64_t rows = dc.numel() / 128;
  // delta is always dense [B, Hq, S]
  auto delta = at::empty({dout.size(0), dout.size(1), dout.size(2)},
                         dout.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  tft::launch_fa_delta(dc.data_ptr(), oc.data_ptr(), delta.data_ptr<float>(),
                       rows, (int)dout.size(1), (int)dout.size(2), bshd,
                       (tft_stream)stream);
  return delta;
}

std::vector<at::Tensor> fa_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                               double scale, bool causal) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16 && q.dim() == 4);
  TORCH_CHECK(q.size(3) == 128, "fa_fwd supports head_dim=128 only");
  TORCH_CHECK(q.size(2) % 256 == 0, "fa_fwd requires seq % 256 == 0");
  const int64_t B = q.size(0), Hq = q.size(1), S = q.size(2);
  const int64_t Hkv = k.size(1);
  TORCH_CHECK(Hq % Hkv == 0, "Hq must be a multiple of Hkv");
  const bool bshd = is_bshd(q) && is_bshd(k) && is_bshd(v);
  auto qc = bshd ? q : q.contiguous();
  auto kc = bshd ? k : k.contiguous();
  auto vc = bshd ? v : v.contiguous();
  // out matches the input layout: with bshd storage the logical [B,Hq,S,D]
  // result is a transpose view of a [B,S,Hq,D] buffer (so a later
  // .transpose(1,2).reshape() in the model is free)
  auto out = bshd
                 ? at::empty({B, S, Hq, (int64_t)128}, q.options()).transpose(1, 2)
                 : at::empty_like(qc);
  auto lse = at::empty({B, Hq, S}, q.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  tft::launch_fa_fwd(qc.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                     out.data_ptr(), lse.data_ptr<float>(), (int)B, (int)Hq,
                     (int)Hkv, (int)S, (float)scale, causal, bshd,
                     (tft_stream)stream);
  return {out, lse};
}

std::vector<at::Tensor> fa_bwd(at::Tensor q, at::Tensor k, at::Tensor v,
                               at::Tensor dout, at::Tensor lse, at::Tensor delta,
                               double scale, bool causal) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16 && q.dim() == 4);
  TORCH_CHECK(q.size(3) == 128, "fa_bwd supports head_dim=128 only");
  TORCH_CHECK(q.size(2) % 128 == 0, "fa_bwd requires seq % 128 == 0");
  const int64_t B = q.size(0), Hq = q.size(1), S = q.size(2);
  const int64_t Hkv = k.size(1);
  TORCH_CHECK(Hq % Hkv == 0, "Hq must be a multiple of Hkv");
  const bool bshd = is_bshd(q) && is_bshd(k) && is_bshd(v) && is_bshd(dout);
  auto qc = bshd ? q : q.contiguous();
  auto kc = bshd ? k : k.contiguous();
  auto vc = bshd ? v : v.contiguous();
  auto doc = bshd ? dout : dout.contiguous();
  auto lsec = lse.contiguous().to(at::kFloat);
  auto deltac = delta.contiguous().to(at::kFloat);
  TORCH_CHECK(lsec.numel() == B * Hq * S, "lse shape mismatch");
  // gradients come back in the inputs' layout (bshd: transpose views of
  // [B,S,H,D] buffers) so the autograd graph above never copies
  auto mk = [&](const at::Tensor& like) {
    if (!bshd) return at::empty_like(like.contiguous());
    return at::empty({like.size(0), like.size(2), like.size(1), like.size(3)},
                     like.options())
        .transpose(1, 2);
  };
  auto dq = mk(q);
  auto dk = mk(k);
  auto dv = mk(v);
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  tft::launch_fa_bwd(qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), doc.data_ptr(),
                     lsec.data_ptr<float>(), deltac.data_ptr<float>(),
                     dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), (int)B,
                     (int)Hq, (int)Hkv, (int)S, (float)scale, causal, bshd,
                     (tft_stream)stream);
  return {dq, dk, dv};
}

// ---- fused cross-entropy ------------------------------------------------------

// Per-row loss (fp32 [R]); with write_grad the bf16 logits are overwritten
// in place by grad_scale * d(row_loss)/d(logits).
at::Tensor cross_entropy_fwd_bwd(at::Tensor logits, at::Tensor targets,
                                 int64_t ignore_index, double z_loss,
                                 at::Tensor grad_scale, bool write_grad) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kBFloat16 &&
                  logits.dim() == 2,
              "logits must be a bf16 [R, V] device tensor");
  TORCH_CHECK(logits.is_contiguous(), "logits must be contiguous (row stride == V)");
  const int64_t R = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1 && V < (int64_t(1) << 31), "vocab size out of range: ", V);
  TORCH_CHECK(R < (int64_t(1) << 31), "too many rows for one launch: ", R);
  TORCH_CHECK(targets.is_cuda() && targets.scalar_type() == at::kLong &&
                  targets.dim() == 1 && targets.size(0) == R &&
                  targets.is_contiguous(),
              "targets must be a contiguous int64 [R] device tensor");
  TORCH_CHECK(grad_scale.is_cuda() && grad_scale.scalar_type() == at::kFloat &&
                  grad_scale.numel() == 1,
              "grad_scale must be a 1-element fp32 device tensor");
  TORCH_CHECK(targets.device() == logits.device() &&
                  grad_scale.device() == logits.device(),
              "all tensors must be on the same device");
  TORCH_CHECK(z_loss >= 0.0, "z_loss must be >= 0");
  auto row_loss = at::empty({R}, logits.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  tft::launch_cross_entropy(logits.data_ptr(), targets.data_ptr<int64_t>(),
                            row_loss.data_ptr<float>(),
                            grad_scale.data_ptr<float>(), R, (int)V, ignore_index,
                            (float)z_loss, write_grad, (tft_stream)stream);
  return row_loss;
}

at::Tensor mfma_probe(at::Tensor A, at::Tensor B) {
  TORCH_CHECK(A.is_cuda() && A.scalar_type() == at::kBFloat16);
  TORCH_CHECK(A.sizes() == at::IntArrayRef({32, 16}) &&
              B.sizes() == at::IntArrayRef({16, 32}));
  auto D = at::zeros({32, 32}, A.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream().stream();
  tft::launch_mfma_probe(A.contiguous().data_ptr(), B.contiguous().data_ptr(),
                         D.data_ptr<float>(), (tft_stream)stream);
  return D;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "torchft_amd CDNA4 (gfx950) HIP kernels";
  m.def("fp8_pack_bytes", &fp8_pack_bytes);
  m.def("fp8_slice_bytes", &fp8_slice_bytes);
  m.def("fp8_quantize", &fp8_quantize);
  m.def("fp8_dequantize", &fp8_dequantize);
  m.def("fp8_reduce", &fp8_reduce);
  m.def("rmsnorm_fwd", &rmsnorm_fwd);
  m.def("rmsnorm_bwd", &rmsnorm_bwd);
  m.def("rope_apply", &rope_apply);
  m.def("swiglu_fwd", &swiglu_fwd);
  m.def("swiglu_glu_fwd", &swiglu_glu_fwd);
  m.def("swiglu_glu_bwd", &swiglu_glu_bwd);
  m.def("swiglu_bwd", &swiglu_bwd);
  m.def("adamw_step", &adamw_step);
  m.def("adamw_clip_step", &adamw_clip_step,
        "FusedAdamW step with fused global-norm clip and non-finite skip");
  m.def("grad_sumsq", &grad_sumsq,
        "global sum of squares of a tensor list: 1-element fp32 device tensor");
  m.def("clip_grad_norm", &clip_grad_norm,
        "in-place global-norm clip; returns the pre-clip sum of squares");
  m.def("diloco_pseudograd", &diloco_pseudograd,
        "multi-tensor outs[i] = minuends[i] - subtrahends[i]");
  m.def("diloco_outer_step", &diloco_outer_step,
        "fused DiLoCo outer SGD step, re-snapshot and local-progress lerp");
  m.def("fa_fwd", &fa_fwd);
  m.def("fa_delta", &fa_delta);
  m.def("fa_bwd", &fa_bwd,
        "flash-attention backward (bf16, D=128): returns (dq, dk, dv)");
  m.def("cross_entropy_fwd_bwd", &cross_entropy_fwd_bwd,
        "fused cross-entropy: returns row_loss, writes the gradient in place");
  m.def("mfma_probe", &mfma_probe, "mfma_f32_32x32x16_bf16 layout probe");
}

