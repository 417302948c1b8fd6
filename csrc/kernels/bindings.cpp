// torch-extension bindings for the CDNA4 kernels (fp8 quantized-collective
// trio, fused model ops, fused AdamW, DiLoCo outer sync, flash attention).
// Tensor-level API consumed by torchft_amd.ops / torchft_amd.quantization.
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include <c10/util/accumulate.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "fa_layout.h"
#include "kernels.h"
#include "multi_tensor_host.h"
#include "qkv_layout.h"

namespace tft = torchft_amd;

namespace {

using TensorList = std::vector<at::Tensor>;

struct PackGeom {
  int64_t total_blocks = 0;
  int64_t padded_blocks = 0;
  int64_t blocks_per_rank = 0;
  int64_t slice_bytes = 0;
};

PackGeom pack_geometry(const TensorList& tensors, int64_t world, const char* what) {
  TORCH_CHECK(world >= 1, what, ": world must be >= 1, got ", world);
  PackGeom g;
  for (auto& t : tensors) g.total_blocks += (t.numel() + tft::kMtBlock - 1) / tft::kMtBlock;
  g.padded_blocks = ((g.total_blocks + world - 1) / world) * world;
  g.blocks_per_rank = g.padded_blocks / world;
  g.slice_bytes = g.blocks_per_rank * (4 + tft::kMtBlock);
  return g;
}

// dtype_code of kernels.h, -1 for a dtype the multi-tensor kernels do not take
int dtype_code(at::ScalarType st) {
  return st == at::kBFloat16 ? tft::kBF16
         : st == at::kHalf   ? tft::kF16
         : st == at::kFloat  ? tft::kF32
                             : -1;
}

// One pointer column of a table to be: a tensor list and the dtype every
// entry must have. `one_element` columns (device step counts) hold 1-element
// tensors instead of tensors of the row's size.
struct Column {
  const TensorList* list;
  at::ScalarType dtype;
  bool one_element = false;
};

// Every multi-tensor table of one binding call (kernels.h, MultiTensorTable):
// add() validates and stages, upload() lays them out back to back in ONE
// pinned buffer and copies it to the device once, table() hands a launcher
// its view. The same rules hold for every user: all tensors on the device of
// the first, the column's dtype, contiguous, the columns of a row equal in
// size, the lists equal in length. Zero-numel rows are left out, so they
// cost no block and an all-empty table launches nothing. Users whose kernels
// have no element path for a tensor off a 16 B boundary (the fp8 pack) ask
// for `need_16b_alignment`, and such a tensor is refused here.
class TableSet {
 public:
  TableSet(const at::Tensor& first, const char* what, bool need_16b_alignment = false)
      : dev_(first.device()), what_(what), need_16b_alignment_(need_16b_alignment) {
    TORCH_CHECK(first.is_cuda(), what_, ": requires device tensors");
  }

  // rows [first, first + count) of the parallel lists as one table
  int add(const std::vector<Column>& cols, int64_t first, int64_t count) {
    Staged st;
    st.n_cols = (int)cols.size();
    const int64_t len = (int64_t)cols[0].list->size();
    TORCH_CHECK(first >= 0 && count >= 0 && first + count <= len, what_,
                ": rows out of range");
    for (auto& c : cols)
      TORCH_CHECK((int64_t)c.list->size() == len, what_, ": list lengths differ");
    for (int64_t i = first; i < first + count; i++) {
      const int64_t ne = (*cols[0].list)[i].numel();
      for (auto& c : cols) {
        const at::Tensor& t = (*c.list)[i];
        TORCH_CHECK(t.is_cuda() && t.device() == dev_, what_,
                    ": all tensors must be on one device");
        TORCH_CHECK(t.scalar_type() == c.dtype, what_, ": mixed dtypes (expected ",
                    c.dtype, ", got ", t.scalar_type(), " at tensor ", i, ")");
        TORCH_CHECK(t.is_contiguous(), what_, ": tensors must be contiguous");
        TORCH_CHECK(t.numel() == (c.one_element ? 1 : ne), what_,
                    ": size mismatch at tensor ", i);
      }
      if (ne == 0) continue;
      for (auto& c : cols) {
        const int64_t addr = (int64_t)(*c.list)[i].data_ptr();
        TORCH_CHECK(!need_16b_alignment_ || (addr & 15) == 0, what_, ": tensor ", i,
                    " does not start on a 16-byte boundary");
        st.addrs.push_back(addr);
      }
      st.numels.push_back(ne);
    }
    st.offset = words_;
    words_ += tft::mt_table_words((int64_t)st.numels.size(), st.n_cols);
    staged_.push_back(std::move(st));
    return (int)staged_.size() - 1;
  }
  int add(const std::vector<Column>& cols) {
    return add(cols, 0, (int64_t)cols[0].list->size());
  }

  void upload() {
    auto opts = at::TensorOptions().dtype(at::kLong).pinned_memory(true);
    at::Tensor host = at::empty({words_}, opts);
    int64_t* h = host.data_ptr<int64_t>();
    for (auto& st : staged_) {
      st.blocks = tft::mt_write_table(h + st.offset, (int64_t)st.numels.size(), st.n_cols,
                                      st.addrs.data(), st.numels.data());
      TORCH_CHECK(st.blocks >= 0, what_, ": too many elements for one launch");
    }
    dev_words_ = host.to(dev_, /*non_blocking=*/true);
  }

  // after upload()
  tft::MultiTensorTable table(int handle) const {
    const Staged& st = staged_[handle];
    return tft::mt_view(dev_words_.data_ptr<int64_t>(), st.offset,
                        (int64_t)st.numels.size(), st.n_cols, st.blocks);
  }

 private:
  struct Staged {
    int n_cols = 0;
    std::vector<int64_t> addrs;  // row by row
    std::vector<int64_t> numels;
    int64_t offset = 0;  // first int64 word of this table
    int64_t blocks = 0;
  };
  at::Device dev_;
  const char* what_;
  bool need_16b_alignment_;
  std::vector<Staged> staged_;
  int64_t words_ = 0;
  at::Tensor dev_words_;
};

// The wire buffer of a quantize / dequantize call: contiguous uint8 on the
// tensors' device, large enough for every slice. A host `pack` would hand the
// kernel a host pointer, a short one lets it run past the end.
void check_pack(const at::Tensor& pack, const TensorList& tensors, const PackGeom& g,
                int64_t world, const char* what) {
  TORCH_CHECK(pack.scalar_type() == at::kByte, what, ": pack must be uint8, got ",
              pack.scalar_type());
  TORCH_CHECK(pack.is_cuda() && pack.device() == tensors[0].device(), what,
              ": pack must be on the tensors' device (", tensors[0].device(), "), got ",
              pack.device());
  TORCH_CHECK(pack.is_contiguous(), what, ": pack must be contiguous");
  TORCH_CHECK(pack.numel() >= g.slice_bytes * world, what, ": pack holds ", pack.numel(),
              " bytes, needs ", g.slice_bytes * world);
}

// dtype_code of a call whose tensors all share the dtype of the first; the
// table's checks hold the others to it
int first_dtype_code(const TensorList& tensors, const char* what) {
  TORCH_CHECK(!tensors.empty(), what, ": need at least one tensor");
  const int code = dtype_code(tensors[0].scalar_type());
  TORCH_CHECK(code >= 0, what, ": unsupported dtype ", tensors[0].scalar_type());
  return code;
}

tft_stream current_stream() {
  return (tft_stream)at::cuda::getCurrentCUDAStream().stream();
}

}  // namespace

// ---- fp8 quantized-collective support --------------------------------------
// table: col 0 = the tensors, all of the first one's dtype and 16 B-aligned

int64_t fp8_pack_bytes(const std::vector<at::Tensor>& tensors, int64_t world) {
  auto g = pack_geometry(tensors, world, "fp8_pack_bytes");
  return g.slice_bytes * world;
}

int64_t fp8_slice_bytes(const std::vector<at::Tensor>& tensors, int64_t world) {
  return pack_geometry(tensors, world, "fp8_slice_bytes").slice_bytes;
}

void fp8_quantize(const std::vector<at::Tensor>& tensors, at::Tensor pack,
                  int64_t world) {
  const int code = first_dtype_code(tensors, "fp8_quantize");
  TORCH_CHECK(tensors[0].is_cuda(), "fp8_quantize: requires device tensors");
  auto g = pack_geometry(tensors, world, "fp8_quantize");
  check_pack(pack, tensors, g, world, "fp8_quantize");
  TableSet tables(tensors[0], "fp8_quantize", /*need_16b_alignment=*/true);
  const int h = tables.add({{&tensors, tensors[0].scalar_type()}});
  tables.upload();
  tft::launch_quantize_dtype(code, tables.table(h), g.padded_blocks, g.blocks_per_rank,
                             g.slice_bytes, pack.data_ptr<uint8_t>(), current_stream());
}

void fp8_dequantize(const std::vector<at::Tensor>& tensors, at::Tensor pack,
                    int64_t world) {
  const int code = first_dtype_code(tensors, "fp8_dequantize");
  TORCH_CHECK(tensors[0].is_cuda(), "fp8_dequantize: requires device tensors");
  auto g = pack_geometry(tensors, world, "fp8_dequantize");
  check_pack(pack, tensors, g, world, "fp8_dequantize");
  TableSet tables(tensors[0], "fp8_dequantize", /*need_16b_alignment=*/true);
  const int h = tables.add({{&tensors, tensors[0].scalar_type()}});
  tables.upload();
  tft::launch_dequantize_dtype(code, tables.table(h), g.padded_blocks,
                               g.blocks_per_rank, g.slice_bytes,
                               pack.data_ptr<uint8_t>(), current_stream());
}

void fp8_reduce(at::Tensor recv, at::Tensor out, int64_t world, bool avg) {
  TORCH_CHECK(recv.is_cuda() && recv.scalar_type() == at::kByte && recv.is_contiguous(),
              "fp8_reduce: recv must be a contiguous uint8 device tensor");
  TORCH_CHECK(out.device() == recv.device() && out.scalar_type() == at::kByte &&
                  out.is_contiguous(),
              "fp8_reduce: out must be a contiguous uint8 tensor on recv's device");
  TORCH_CHECK(world >= 1, "fp8_reduce: world must be >= 1, got ", world);
  TORCH_CHECK(recv.numel() == out.numel() * world,
              "fp8_reduce: recv must hold world slices of out's size");
  const int64_t slice_bytes = out.numel();
  const int64_t blocks_per_rank = slice_bytes / (4 + tft::kMtBlock);
  TORCH_CHECK(blocks_per_rank * (4 + tft::kMtBlock) == slice_bytes,
              "fp8_reduce: out is not a whole number of blocks");
  if (blocks_per_rank == 0) return;  // nothing but empty tensors: no launch
  tft::launch_reduce(recv.data_ptr<uint8_t>(), out.data_ptr<uint8_t>(), (int)world,
                     blocks_per_rank, slice_bytes, avg, current_stream());
}

// ---- fused model ops --------------------------------------------------------

namespace {

// The inputs of one RMSNorm / RoPE / SwiGLU / QKV-split call and the one rule they are
// held to: every tensor is on the device of the first and has the dtype its
// role asks for (bf16 activations, weights and gradients; fp32 invrms and
// rotary tables). in() hands back what the kernel reads: made contiguous, and
// copied to a fresh allocation if its first element is off a 16 B boundary
// (the kernels use 16 B accesses), so nothing is refused for its layout.
// Every refusal names the binding and the argument and comes before a launch;
// the launchers start nothing for zero rows or elements.
struct OpArgs {
  const char* what;
  at::Tensor first;  // x, a or gu, as the kernel reads it

  OpArgs(const char* what_, const char* name, const at::Tensor& t) : what(what_) {
    TORCH_CHECK(t.is_cuda(), what, ": ", name, " must be a device tensor");
    TORCH_CHECK(t.dim() >= 1, what, ": ", name, " must have at least one dimension");
    dev_ = t.device();
    first = in(name, t, at::kBFloat16);
  }

  at::Tensor in(const char* name, const at::Tensor& t, at::ScalarType dtype) const {
    TORCH_CHECK(t.device() == dev_, what, ": ", name, " must be on the device of the ",
                "first tensor (", dev_, "), got ", t.device());
    TORCH_CHECK(t.scalar_type() == dtype, what, ": ", name, " must be ", dtype, ", got ",
                t.scalar_type());
    at::Tensor c = t.contiguous();
    if ((reinterpret_cast<uintptr_t>(c.data_ptr()) & 15) != 0) c = c.clone();
    return c;
  }
  // a bf16 tensor of exactly these sizes
  at::Tensor shaped(const char* name, const at::Tensor& t, at::IntArrayRef sizes) const {
    TORCH_CHECK(t.sizes() == sizes, what, ": ", name, " must have the shape ", sizes,
                ", got ", t.sizes());
    return in(name, t, at::kBFloat16);
  }
  // a tensor of exactly `numel` elements, any shape
  at::Tensor flat(const char* name, const at::Tensor& t, at::ScalarType dtype,
                  int64_t numel) const {
    TORCH_CHECK(t.numel() == numel, what, ": ", name, " must have ", numel,
                " elements, got ", t.sizes());
    return in(name, t, dtype);
  }
  // a size the kernels index with int and read 8 (or 4 pairs) at a time
  int dim8(const char* name, int64_t v) const {
    TORCH_CHECK(v % 8 == 0 && v < (int64_t(1) << 30), what, ": ", name,
                " must be a multiple of 8 below 2^30, got ", v);
    return (int)v;
  }
  void grid_ok(const char* name, int64_t grid) const {
    TORCH_CHECK(grid < (int64_t(1) << 31), what, ": ", name,
                " is too large for one launch (", grid, " workgroups)");
  }
  // elements per index of the last dimension
  int64_t rows() const {
    return c10::multiply_integers(first.sizes().slice(0, first.dim() - 1));
  }

 private:
  at::Device dev_ = at::kCPU;
};

}  // namespace

std::vector<at::Tensor> rmsnorm_fwd(at::Tensor x, at::Tensor w, double eps) {
  OpArgs a("rmsnorm_fwd", "x", x);
  const int H = a.dim8("the last dimension of x (H)", a.first.size(-1));
  const int64_t rows = a.rows();
  a.grid_ok("x", rows);
  auto wc = a.flat("w", w, at::kBFloat16, H);
  auto y = at::empty_like(a.first);
  auto invrms = at::empty({rows}, a.first.options().dtype(at::kFloat));
  tft::launch_rmsnorm_fwd(a.first.data_ptr(), wc.data_ptr(), y.data_ptr(),
                          invrms.data_ptr<float>(), rows, H, (float)eps,
                          current_stream());
  return {y, invrms};
}

std::vector<at::Tensor> rmsnorm_bwd(at::Tensor dy, at::Tensor x, at::Tensor w,
                                    at::Tensor invrms) {
  OpArgs a("rmsnorm_bwd", "x", x);
  const int H = a.dim8("the last dimension of x (H)", a.first.size(-1));
  TORCH_CHECK(H * (int64_t)sizeof(float) + tft::kRmsnormBwdStaticLdsBytes <=
                  tft::kRmsnormBwdMaxLdsBytes,
              "rmsnorm_bwd: the last dimension of x (H) is too large for the LDS dw ",
              "buffer, got ", H);
  const int64_t rows = a.rows();
  auto dyc = a.shaped("dy", dy, x.sizes());
  auto wc = a.flat("w", w, at::kBFloat16, H);
  auto invc = a.flat("invrms", invrms, at::kFloat, rows);
  auto dx = at::empty_like(a.first);
  auto dw = at::zeros({H}, a.first.options().dtype(at::kFloat));
  const int status = tft::launch_rmsnorm_bwd(
      dyc.data_ptr(), a.first.data_ptr(), wc.data_ptr(), invc.data_ptr<float>(),
      dx.data_ptr(), dw.data_ptr<float>(), rows, H, current_stream());
  TORCH_CHECK(status == 0, "rmsnorm_bwd: the launch failed with HIP error ", status);
  return {dx, dw};
}

at::Tensor rope_apply(at::Tensor x, at::Tensor cos_tab, at::Tensor sin_tab,
                      bool backward) {
  // x: [B, S, Hh, D]
  OpArgs a("rope_apply", "x", x);
  TORCH_CHECK(x.dim() == 4, "rope_apply: x must be 4-D [B, S, Hh, D], got ", x.sizes());
  const int D = a.dim8("the last dimension of x (D)", x.size(3));
  const int64_t S = x.size(1), Hh = x.size(2);
  TORCH_CHECK(S < (int64_t(1) << 31) && Hh < (int64_t(1) << 31),
              "rope_apply: x has too many positions or heads, got ", x.sizes());
  TORCH_CHECK(cos_tab.dim() == 2 && cos_tab.size(0) >= S && cos_tab.size(1) == D / 2,
              "rope_apply: cos_tab must be [at least ", S, ", ", D / 2, "], got ",
              cos_tab.sizes());
  TORCH_CHECK(sin_tab.sizes() == cos_tab.sizes(), "rope_apply: sin_tab must have the ",
              "shape of cos_tab ", cos_tab.sizes(), ", got ", sin_tab.sizes());
  auto cosc = a.in("cos_tab", cos_tab, at::kFloat);
  auto sinc = a.in("sin_tab", sin_tab, at::kFloat);
  const int64_t total_pairs = a.first.numel() / 2;
  a.grid_ok("x", tft::elementwise_grid(total_pairs, 4));
  auto out = at::empty_like(a.first);
  tft::launch_rope(a.first.data_ptr(), out.data_ptr(), cosc.data_ptr<float>(),
                   sinc.data_ptr<float>(), total_pairs, (int)S, (int)Hh, D, backward,
                   current_stream());
  return out;
}

namespace {

// a of the plain SwiGLU, its element count checked
const at::Tensor& swiglu_a(const OpArgs& args) {
  const int64_t n = args.first.numel();
  TORCH_CHECK(n % 8 == 0, args.what, ": a must have a multiple of 8 elements, got ", n);
  args.grid_ok("a", tft::elementwise_grid(n, 8));
  return args.first;
}

// f of a packed gu = [..., 2f], checked
int64_t glu_width(const OpArgs& a) {
  const int64_t last = a.first.size(-1);
  TORCH_CHECK(last % 2 == 0, a.what, ": the last dimension of gu must be even, got ", last);
  TORCH_CHECK((last / 2) % 8 == 0, a.what, ": half the last dimension of gu (f) must be ",
              "a multiple of 8, got ", last / 2);
  a.grid_ok("gu", tft::elementwise_grid(a.first.numel() / 2, 8));
  return last / 2;
}

}  // namespace

at::Tensor swiglu_fwd(at::Tensor a, at::Tensor b) {
  OpArgs args("swiglu_fwd", "a", a);
  const at::Tensor& ac = swiglu_a(args);
  auto bc = args.shaped("b", b, a.sizes());
  auto out = at::empty_like(ac);
  tft::launch_swiglu_fwd(ac.data_ptr(), bc.data_ptr(), out.data_ptr(), ac.numel(),
                         current_stream());
  return out;
}

std::vector<at::Tensor> swiglu_bwd(at::Tensor dy, at::Tensor a, at::Tensor b) {
  OpArgs args("swiglu_bwd", "a", a);
  const at::Tensor& ac = swiglu_a(args);
  auto dyc = args.shaped("dy", dy, a.sizes());
  auto bc = args.shaped("b", b, a.sizes());
  auto da = at::empty_like(ac);
  auto db = at::empty_like(bc);
  tft::launch_swiglu_bwd(dyc.data_ptr(), ac.data_ptr(), bc.data_ptr(), da.data_ptr(),
                         db.data_ptr(), ac.numel(), current_stream());
  return {da, db};
}

at::Tensor swiglu_glu_fwd(at::Tensor gu) {
  OpArgs a("swiglu_glu_fwd", "gu", gu);
  const int64_t f = glu_width(a);
  auto sizes = a.first.sizes().vec();
  sizes.back() = f;
  auto out = at::empty(sizes, a.first.options());
  tft::launch_swiglu_glu_fwd(a.first.data_ptr(), out.data_ptr(), a.rows(), f,
                             current_stream());
  return out;
}

at::Tensor swiglu_glu_bwd(at::Tensor dy, at::Tensor gu) {
  OpArgs a("swiglu_glu_bwd", "gu", gu);
  const int64_t f = glu_width(a);
  auto sizes = a.first.sizes().vec();
  sizes.back() = f;
  auto dyc = a.shaped("dy", dy, sizes);
  auto dgu = at::empty_like(a.first);
  tft::launch_swiglu_glu_bwd(dyc.data_ptr(), a.first.data_ptr(), dgu.data_ptr(), a.rows(), f,
                             current_stream());
  return dgu;
}

// ---- fused QKV split + rotary ---------------------------------------------------

namespace {

// What qkv_rope_fwd and qkv_rope_bwd share once the activations are known: the
// head dimension, the rotary tables (rope_apply's rule, with one row enough
// when `positions` picks the rows), the optional per-token positions, and the
// grid.
struct QkvRopeArgs {
  int D = 0;
  int table_rows = 0;
  at::Tensor cos, sin, positions;

  // name: the activation the sizes come from (qkv or dq); Hq, Hkv below 2^30
  QkvRopeArgs(const OpArgs& a, const char* name, int64_t B, int64_t S, int64_t Hq,
              int64_t Hkv, int64_t D_, const at::Tensor& cos_tab,
              const at::Tensor& sin_tab, const c10::optional<at::Tensor>& pos) {
    TORCH_CHECK(D_ >= 16 && D_ % 16 == 0 && D_ < (int64_t(1) << 30), a.what,
                ": the head dimension of ", name, " (D) must be a multiple of 16 below ",
                "2^30, got ", D_);
    D = (int)D_;
    TORCH_CHECK(S < (int64_t(1) << 31) && (Hq + 2 * Hkv) * D_ < (int64_t(1) << 31), a.what,
                ": ", name, " has too many positions or too wide a row, got S = ", S,
                ", W = ", (Hq + 2 * Hkv) * D_);
    const int64_t min_rows = pos.has_value() ? 1 : S;
    TORCH_CHECK(cos_tab.dim() == 2 && cos_tab.size(0) >= min_rows &&
                    cos_tab.size(1) == D / 2,
                a.what, ": cos_tab must be [at least ", min_rows, ", ", D / 2, "], got ",
                cos_tab.sizes());
    TORCH_CHECK(sin_tab.sizes() == cos_tab.sizes(), a.what, ": sin_tab must have the ",
                "shape of cos_tab ", cos_tab.sizes(), ", got ", sin_tab.sizes());
    cos = a.in("cos_tab", cos_tab, at::kFloat);
    sin = a.in("sin_tab", sin_tab, at::kFloat);
    // the kernels clamp a position into [0, table_rows - 1] as an int; with
    // no rows (and so no tokens) nothing is launched
    table_rows = (int)std::min<int64_t>(cos_tab.size(0), INT32_MAX);
    if (pos.has_value()) {
      TORCH_CHECK(pos->is_cuda(), a.what, ": positions must be a device tensor");
      positions = a.flat("positions", *pos, at::kInt, B * S);
    }
    const int64_t items = B * S * tft::qkv_items_per_token((int)Hq, (int)Hkv, D);
    a.grid_ok(name, tft::elementwise_grid(items, 1));
  }

  const int* positions_ptr() const {
    return positions.defined() ? positions.data_ptr<int>() : nullptr;
  }
};

}  // namespace

// qkv [B, S, (n_heads + 2 * n_kv_heads) * D] -> q [B, S, n_heads, D] and
// k, v [B, S, n_kv_heads, D], q and k rotated; positions: int32, B * S
// elements, the table row of every token (row s without it).
std::vector<at::Tensor> qkv_rope_fwd(at::Tensor qkv, at::Tensor cos_tab, at::Tensor sin_tab,
                                     int64_t n_heads, int64_t n_kv_heads,
                                     c10::optional<at::Tensor> positions) {
  OpArgs a("qkv_rope_fwd", "qkv", qkv);
  TORCH_CHECK(qkv.dim() == 3, "qkv_rope_fwd: qkv must be 3-D [B, S, W], got ", qkv.sizes());
  TORCH_CHECK(n_heads >= 1, "qkv_rope_fwd: n_heads must be >= 1, got ", n_heads);
  TORCH_CHECK(n_kv_heads >= 1, "qkv_rope_fwd: n_kv_heads must be >= 1, got ", n_kv_heads);
  const int64_t B = qkv.size(0), S = qkv.size(1), W = qkv.size(2);
  TORCH_CHECK(n_heads < (int64_t(1) << 30) && n_kv_heads < (int64_t(1) << 30) &&
                  W % (n_heads + 2 * n_kv_heads) == 0,
              "qkv_rope_fwd: the last dimension of qkv (W = ", W, ") must be divisible by ",
              "n_heads + 2 * n_kv_heads = ", n_heads, " + 2 * ", n_kv_heads);
  QkvRopeArgs r(a, "qkv", B, S, n_heads, n_kv_heads, W / (n_heads + 2 * n_kv_heads),
                cos_tab, sin_tab, positions);
  auto q = at::empty({B, S, n_heads, r.D}, a.first.options());
  auto k = at::empty({B, S, n_kv_heads, r.D}, a.first.options());
  auto v = at::empty({B, S, n_kv_heads, r.D}, a.first.options());
  tft::launch_qkv_rope_fwd(a.first.data_ptr(), q.data_ptr(), k.data_ptr(), v.data_ptr(),
                           r.cos.data_ptr<float>(), r.sin.data_ptr<float>(),
                           r.positions_ptr(), r.table_rows, B * S, (int)S, (int)n_heads,
                           (int)n_kv_heads, r.D, current_stream());
  return {q, k, v};
}

// The transpose: dq [B, S, Hq, D], dk and dv [B, S, Hkv, D] ->
// dqkv [B, S, (Hq + 2 * Hkv) * D], every element written.
at::Tensor qkv_rope_bwd(at::Tensor dq, at::Tensor dk, at::Tensor dv, at::Tensor cos_tab,
                        at::Tensor sin_tab, c10::optional<at::Tensor> positions) {
  OpArgs a("qkv_rope_bwd", "dq", dq);
  TORCH_CHECK(dq.dim() == 4, "qkv_rope_bwd: dq must be 4-D [B, S, Hq, D], got ", dq.sizes());
  const int64_t B = dq.size(0), S = dq.size(1), Hq = dq.size(2), D = dq.size(3);
  TORCH_CHECK(Hq >= 1, "qkv_rope_bwd: dq must have at least one head, got ", dq.sizes());
  TORCH_CHECK(dk.dim() == 4 && dk.size(0) == B && dk.size(1) == S && dk.size(2) >= 1 &&
                  dk.size(3) == D,
              "qkv_rope_bwd: dk must be [B, S, Hkv, D] with dq's B, S and D, got ",
              dk.sizes(), " against ", dq.sizes());
  const int64_t Hkv = dk.size(2);
  TORCH_CHECK(Hq < (int64_t(1) << 30) && Hkv < (int64_t(1) << 30),
              "qkv_rope_bwd: dq or dk has too many heads");
  QkvRopeArgs r(a, "dq", B, S, Hq, Hkv, D, cos_tab, sin_tab, positions);
  auto dkc = a.in("dk", dk, at::kBFloat16);
  auto dvc = a.shaped("dv", dv, dk.sizes());
  auto dqkv = at::empty({B, S, (Hq + 2 * Hkv) * D}, a.first.options());
  tft::launch_qkv_rope_bwd(a.first.data_ptr(), dkc.data_ptr(), dvc.data_ptr(),
                           dqkv.data_ptr(), r.cos.data_ptr<float>(),
                           r.sin.data_ptr<float>(), r.positions_ptr(), r.table_rows, B * S,
                           (int)S, (int)Hq, (int)Hkv, r.D, current_stream());
  return dqkv;
}

// ---- fused AdamW ------------------------------------------------------------

void adamw_step(const std::vector<at::Tensor>& params,
                const std::vector<at::Tensor>& grads,
                const std::vector<at::Tensor>& exp_avgs,
                const std::vector<at::Tensor>& exp_avg_sqs, double lr,
                double beta1, double beta2, double eps, double weight_decay,
                int64_t step) {
  TORCH_CHECK(!params.empty(), "adamw_step: need at least one tensor");
  TableSet tables(params[0], "adamw_step");
  const int h = tables.add({{&params, at::kBFloat16},
                            {&grads, at::kBFloat16},
                            {&exp_avgs, at::kFloat},
                            {&exp_avg_sqs, at::kFloat}});
  tables.upload();
  const float bc1 = 1.0f - std::pow((float)beta1, (float)step);
  const float bc2 = 1.0f - std::pow((float)beta2, (float)step);
  tft::launch_adamw(tables.table(h), (float)lr, (float)beta1, (float)beta2, (float)eps,
                    (float)weight_decay, bc1, bc2, current_stream());
}

// ---- global gradient norm / clip ---------------------------------------------

namespace {

// One table per dtype present, all in one TableSet
struct GradTables {
  TensorList by_dtype[3];  // indexed by dtype_code
  int handle[3] = {-1, -1, -1};
};

void add_grad_tables(TableSet& tables, const TensorList& tensors, GradTables& gt) {
  for (auto& t : tensors) {
    const int code = dtype_code(t.scalar_type());
    TORCH_CHECK(code >= 0, "unsupported dtype for grad norm: ", t.scalar_type());
    gt.by_dtype[code].push_back(t);
  }
  const at::ScalarType dtypes[3] = {at::kBFloat16, at::kHalf, at::kFloat};
  for (int c = 0; c < 3; c++)
    if (!gt.by_dtype[c].empty()) gt.handle[c] = tables.add({{&gt.by_dtype[c], dtypes[c]}});
}

void check_max_blocks(int64_t max_blocks) {
  TORCH_CHECK(max_blocks >= 1 && max_blocks <= (int64_t(1) << 16),
              "max_blocks must be in [1, 65536], got ", max_blocks);
}

// partial sums of every table (dtype code, view) into one partials buffer,
// then one finalize
void run_sumsq(const std::vector<std::pair<int, tft::MultiTensorTable>>& tbs,
               int64_t max_blocks, at::Tensor& stats, tft_stream stream) {
  int64_t n_partials = 0;
  for (auto& ct : tbs) n_partials += std::min(ct.second.total_blocks, max_blocks);
  auto partials = at::empty({n_partials}, stats.options());
  int64_t at_partial = 0;
  for (auto& ct : tbs) {
    const int64_t grid = std::min(ct.second.total_blocks, max_blocks);
    tft::launch_grad_sumsq_partial(ct.first, ct.second, (int)grid,
                                   partials.data_ptr<float>() + at_partial, stream);
    at_partial += grid;
  }
  tft::launch_grad_sumsq_finalize(partials.data_ptr<float>(), (int)n_partials,
                                  stats.data_ptr<float>(), stream);
}

std::vector<std::pair<int, tft::MultiTensorTable>> grad_views(const TableSet& tables,
                                                              const GradTables& gt) {
  std::vector<std::pair<int, tft::MultiTensorTable>> out;
  for (int c = 0; c < 3; c++)
    if (gt.handle[c] >= 0) out.emplace_back(c, tables.table(gt.handle[c]));
  return out;
}

}  // namespace

// Sum of squares over every tensor, as a 1-element fp32 device tensor.
at::Tensor grad_sumsq(const std::vector<at::Tensor>& tensors, int64_t max_blocks) {
  check_max_blocks(max_blocks);
  TORCH_CHECK(!tensors.empty(), "need at least one tensor");
  TableSet tables(tensors[0], "grad norm");
  GradTables gt;
  add_grad_tables(tables, tensors, gt);
  tables.upload();
  auto stats = at::empty({1}, tensors[0].options().dtype(at::kFloat));
  run_sumsq(grad_views(tables, gt), max_blocks, stats, current_stream());
  return stats;
}

// Norm + in-place scale sharing one table; norm_reduce (or None) sees the
// 1-element sum of squares between the two. Returns the sum of squares.
at::Tensor clip_grad_norm(const std::vector<at::Tensor>& tensors, double max_norm,
                          int64_t max_blocks, py::object norm_reduce) {
  check_max_blocks(max_blocks);
  TORCH_CHECK(max_norm > 0.0, "max_norm must be > 0");
  TORCH_CHECK(!tensors.empty(), "need at least one tensor");
  TableSet tables(tensors[0], "grad norm");
  GradTables gt;
  add_grad_tables(tables, tensors, gt);
  tables.upload();
  auto stats = at::empty({1}, tensors[0].options().dtype(at::kFloat));
  auto stream = current_stream();
  const auto views = grad_views(tables, gt);
  run_sumsq(views, max_blocks, stats, stream);
  if (!norm_reduce.is_none()) norm_reduce(stats);
  for (auto& ct : views)
    tft::launch_grad_scale(ct.first, ct.second, stats.data_ptr<float>(), (float)max_norm,
                           stream);
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
  TORCH_CHECK(n > 0, "adamw_clip_step: need at least one tensor");
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

  // one norm table over every gradient, one update table per param group
  // (its prefix starts at 0 again), and every step count for the bump launch,
  // those of zero-numel parameters included
  TableSet tables(params[0], "adamw_clip_step");
  const int h_norm = tables.add({{&grads, at::kBFloat16}});
  std::vector<int> h_update(ng);
  int64_t first = 0;
  for (int64_t g = 0; g < ng; g++) {
    TORCH_CHECK(group_sizes[g] >= 0 && first + group_sizes[g] <= n);
    h_update[g] = tables.add({{&params, at::kBFloat16},
                              {&grads, at::kBFloat16},
                              {&exp_avgs, at::kFloat},
                              {&exp_avg_sqs, at::kFloat},
                              {&steps, at::kInt, /*one_element=*/true}},
                             first, group_sizes[g]);
    first += group_sizes[g];
  }
  TORCH_CHECK(first == n, "group_sizes must cover every tensor");
  const int h_steps = tables.add({{&steps, at::kInt, /*one_element=*/true}});
  tables.upload();
  auto stream = current_stream();

  run_sumsq({{tft::kBF16, tables.table(h_norm)}}, max_blocks, stats, stream);
  if (!norm_reduce.is_none()) norm_reduce(stats.narrow(0, 0, 1));

  for (int64_t g = 0; g < ng; g++)
    tft::launch_adamw_clip(tables.table(h_update[g]), (float)lrs[g], (float)beta1s[g],
                           (float)beta2s[g], (float)epss[g], (float)weight_decays[g],
                           stats.data_ptr<float>(), (float)max_norm, stream);
  const auto st = tables.table(h_steps);
  tft::launch_adamw_bump_steps(st.col(0), st.n, stats.data_ptr<float>(),
                               skipped.data_ptr<int>(), norm_out.data_ptr<float>(),
                               stream);
}

// ---- fused DiLoCo outer sync ---------------------------------------------------

// outs[i] = minuends[i] - subtrahends[i], one launch for the whole list
void diloco_pseudograd(const std::vector<at::Tensor>& outs,
                       const std::vector<at::Tensor>& minuends,
                       const std::vector<at::Tensor>& subtrahends) {
  const int code = first_dtype_code(outs, "pseudograd_");
  const auto st = outs[0].scalar_type();
  TableSet tables(outs[0], "pseudograd_");
  const int h = tables.add({{&outs, st}, {&minuends, st}, {&subtrahends, st}});
  tables.upload();
  tft::launch_pseudograd(code, tables.table(h), current_stream());
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
  const int code = first_dtype_code(snapshots, "diloco_outer_step_");
  const auto st = snapshots[0].scalar_type();
  std::vector<Column> cols = {{&snapshots, st}, {&params, st}, {&pseudograds, st}};
  if (has_m) cols.push_back({&momentum_bufs, st});
  TableSet tables(snapshots[0], "diloco_outer_step_");
  const int h = tables.add(cols);
  tables.upload();
  tft::launch_outer_sgd(code, has_m, tables.table(h), (float)lr, (float)momentum,
                        nesterov, (float)alpha, current_stream());
}

// ---- flash attention ----------------------------------------------------------

namespace {

// true when a logical [B,H,S,D] tensor is a transpose view of contiguous
// [B,S,H,D] storage (the model's projection layout)
bool is_bshd(const at::Tensor& t) {
  return t.dim() == 4 && t.stride(3) == 1 && t.stride(1) == t.size(3) &&
         t.stride(2) == t.size(1) * t.size(3) &&
         t.stride(0) == t.size(1) * t.size(2) * t.size(3);
}

// The tensors of one attention call and the one rule they are held to. Every
// logical [B,H,S,128] tensor is bf16 on the device of the first ("q"; dout for
// fa_delta) with its batch and sequence length; its heads equal q's, or divide
// them for k / v. Layout: if every tensor is a [B,S,H,D]-backed transpose view
// the kernels take them as they are (bshd), otherwise each is made contiguous;
// outputs are allocated in the layout the inputs resolved to.
struct FaArgs {
  const char* what;
  std::vector<at::Tensor> ts;  // q first
  bool bshd = true;

  FaArgs(const char* what_, const char* name, const at::Tensor& q, int seq_multiple)
      : what(what_) {
    TORCH_CHECK(q.is_cuda(), what, ": ", name, " must be a device tensor");
    check_kind(name, q);
    TORCH_CHECK(q.size(2) % seq_multiple == 0, what, " requires seq % ", seq_multiple,
                " == 0");
    push(q);
  }

  // dout / out: q's shape
  void add(const char* name, const at::Tensor& t) {
    check_kind(name, t);
    TORCH_CHECK(t.sizes() == q().sizes(), what, ": ", name, " must have the shape of ",
                "the first tensor, got ", t.sizes(), " against ", q().sizes());
    push(t);
  }

  // k and v: one shape, q's batch and sequence, heads dividing q's
  void add_kv(const at::Tensor& k, const at::Tensor& v) {
    check_kind("k", k);
    check_kind("v", v);
    TORCH_CHECK(k.size(0) == q().size(0) && k.size(2) == q().size(2), what,
                ": k must have q's batch and sequence length, got ", k.sizes(), " against ",
                q().sizes());
    TORCH_CHECK(k.size(1) > 0 && q().size(1) % k.size(1) == 0,
                "Hq must be a multiple of Hkv (k has ", k.size(1), " heads)");
    TORCH_CHECK(v.sizes() == k.sizes(), what, ": v must have k's shape, got ", v.sizes(),
                " against ", k.sizes());
    push(k);
    push(v);
  }

  // lse / delta: B*Hq*S row statistics on q's device, as dense fp32
  at::Tensor stat(const char* name, const at::Tensor& t) const {
    TORCH_CHECK(t.device() == q().device(), what, ": ", name, " must be on q's device");
    TORCH_CHECK(t.numel() == q().size(0) * q().size(1) * q().size(2), what, ": ", name,
                " shape mismatch (", t.numel(), " elements, need B*Hq*S)");
    return t.contiguous().to(at::kFloat);
  }

  // doc_start / doc_end, the document mask: both or neither, only with
  // causal, each int32 on q's device with B*S elements, made contiguous
  void add_doc(const c10::optional<at::Tensor>& ds, const c10::optional<at::Tensor>& de,
               bool causal) {
    TORCH_CHECK(ds.has_value() == de.has_value(), what, ": ",
                ds.has_value() ? "doc_end" : "doc_start", " is missing (doc_start and ",
                "doc_end are given together or not at all)");
    if (!ds.has_value()) return;
    TORCH_CHECK(causal, what, ": doc_start / doc_end need causal=True");
    doc_start = doc("doc_start", *ds);
    doc_end = doc("doc_end", *de);
  }
  // null without a mask
  const int* doc_start_ptr() const {
    return doc_start.defined() ? doc_start.data_ptr<int>() : nullptr;
  }
  const int* doc_end_ptr() const {
    return doc_end.defined() ? doc_end.data_ptr<int>() : nullptr;
  }

  const at::Tensor& q() const { return ts[0]; }
  // nothing to compute: a zero batch or sequence. The launchers take no zero
  // grid, so the bindings return their (empty) outputs unlaunched.
  bool empty() const { return q().numel() == 0; }
  // B * Hq is gridDim.y of the forward and dq launches; dkdv's B * Hkv is no
  // larger, since k's heads divide q's
  void check_grid() const {
    const int64_t rows = q().size(0) * q().size(1);
    TORCH_CHECK(rows <= tft::kFaMaxGridY, what, ": q has batch * heads = ", rows,
                ", above the ", tft::kFaMaxGridY, " one launch covers");
  }
  // tensor i as the kernels read it
  at::Tensor in(size_t i) const { return bshd ? ts[i] : ts[i].contiguous(); }
  // an uninitialized tensor of ts[i]'s logical shape in the resolved layout:
  // with bshd a transpose view of a [B,S,H,D] buffer, so a later
  // .transpose(1, 2).reshape() in the model is free and gradients reach the
  // projections without a copy
  at::Tensor out_like(size_t i) const {
    const at::Tensor& t = ts[i];
    if (!bshd) return at::empty(t.sizes(), t.options());
    return at::empty({t.size(0), t.size(2), t.size(1), t.size(3)}, t.options())
        .transpose(1, 2);
  }

 private:
  at::Tensor doc_start, doc_end;

  at::Tensor doc(const char* name, const at::Tensor& t) const {
    TORCH_CHECK(t.scalar_type() == at::kInt, what, ": ", name,
                " must be an int32 tensor, got ", t.scalar_type());
    TORCH_CHECK(t.device() == q().device(), what, ": ", name, " must be on q's device");
    TORCH_CHECK(t.numel() == q().size(0) * q().size(2), what, ": ", name,
                " shape mismatch (", t.numel(), " elements, need B*S)");
    return t.contiguous();
  }
  void check_kind(const char* name, const at::Tensor& t) const {
    TORCH_CHECK(t.scalar_type() == at::kBFloat16 && t.dim() == 4, what, ": ", name,
                " must be a 4-D bf16 tensor, got ", t.dim(), "-D ", t.scalar_type());
    TORCH_CHECK(ts.empty() || t.device() == q().device(), what, ": ", name,
                " must be on the device of the first tensor");
    TORCH_CHECK(t.size(3) == tft::kFaD, what, " supports head_dim=128 only (", name,
                " has ", t.size(3), ")");
  }
  void push(const at::Tensor& t) {
    bshd = bshd && is_bshd(t);
    ts.push_back(t);
  }
};

}  // namespace

at::Tensor fa_delta(at::Tensor dout, at::Tensor out) {
  FaArgs a("fa_delta", "dout", dout, /*seq_multiple=*/1);
  a.add("out", out);
  // delta is always dense [B, Hq, S]
  auto delta = at::empty({dout.size(0), dout.size(1), dout.size(2)},
                         dout.options().dtype(at::kFloat));
  if (a.empty()) return delta;
  auto dc = a.in(0), oc = a.in(1);
  tft::launch_fa_delta(dc.data_ptr(), oc.data_ptr(), delta.data_ptr<float>(),
                       dc.numel() / tft::kFaD, (int)dout.size(1), (int)dout.size(2),
                       a.bshd, current_stream());
  return delta;
}

std::vector<at::Tensor> fa_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                               double scale, bool causal,
                               c10::optional<at::Tensor> doc_start,
                               c10::optional<at::Tensor> doc_end) {
  FaArgs a("fa_fwd", "q", q, /*seq_multiple=*/256);
  a.add_kv(k, v);
  a.add_doc(doc_start, doc_end, causal);
  a.check_grid();
  auto out = a.out_like(0);
  auto lse = at::empty({q.size(0), q.size(1), q.size(2)}, q.options().dtype(at::kFloat));
  if (a.empty()) return {out, lse};
  auto qc = a.in(0), kc = a.in(1), vc = a.in(2);
  tft::launch_fa_fwd(qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(),
                     lse.data_ptr<float>(), (int)q.size(0), (int)q.size(1), (int)k.size(1),
                     (int)q.size(2), (float)scale, causal, a.bshd, a.doc_start_ptr(),
                     a.doc_end_ptr(), current_stream());
  return {out, lse};
}

std::vector<at::Tensor> fa_bwd(at::Tensor q, at::Tensor k, at::Tensor v,
                               at::Tensor dout, at::Tensor lse, at::Tensor delta,
                               double scale, bool causal,
                               c10::optional<at::Tensor> doc_start,
                               c10::optional<at::Tensor> doc_end) {
  FaArgs a("fa_bwd", "q", q, /*seq_multiple=*/128);
  a.add_kv(k, v);
  a.add("dout", dout);
  a.add_doc(doc_start, doc_end, causal);
  a.check_grid();
  auto lsec = a.stat("lse", lse), deltac = a.stat("delta", delta);
  auto dq = a.out_like(0), dk = a.out_like(1), dv = a.out_like(2);
  if (a.empty()) return {dq, dk, dv};
  auto qc = a.in(0), kc = a.in(1), vc = a.in(2), doc = a.in(3);
  tft::launch_fa_bwd(qc.data_ptr(), kc.data_ptr(), vc.data_ptr(), doc.data_ptr(),
                     lsec.data_ptr<float>(), deltac.data_ptr<float>(), dq.data_ptr(),
                     dk.data_ptr(), dv.data_ptr(), (int)q.size(0), (int)q.size(1),
                     (int)k.size(1), (int)q.size(2), (float)scale, causal, a.bshd,
                     a.doc_start_ptr(), a.doc_end_ptr(), current_stream());
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
  tft::launch_cross_entropy(logits.data_ptr(), targets.data_ptr<int64_t>(),
                            row_loss.data_ptr<float>(),
                            grad_scale.data_ptr<float>(), R, (int)V, ignore_index,
                            (float)z_loss, write_grad, current_stream());
  return row_loss;
}

at::Tensor mfma_probe(at::Tensor A, at::Tensor B) {
  TORCH_CHECK(A.is_cuda() && A.scalar_type() == at::kBFloat16);
  TORCH_CHECK(A.sizes() == at::IntArrayRef({32, 16}) &&
              B.sizes() == at::IntArrayRef({16, 32}));
  auto D = at::zeros({32, 32}, A.options().dtype(at::kFloat));
  tft::launch_mfma_probe(A.contiguous().data_ptr(), B.contiguous().data_ptr(),
                         D.data_ptr<float>(), current_stream());
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
  m.def("qkv_rope_fwd", &qkv_rope_fwd, py::arg("qkv"), py::arg("cos_tab"),
        py::arg("sin_tab"), py::arg("n_heads"), py::arg("n_kv_heads"),
        py::arg("positions") = py::none(),
        "fused QKV split + rotary: returns [q, k, v], contiguous [B, S, H, D]");
  m.def("qkv_rope_bwd", &qkv_rope_bwd, py::arg("dq"), py::arg("dk"), py::arg("dv"),
        py::arg("cos_tab"), py::arg("sin_tab"), py::arg("positions") = py::none(),
        "transpose of qkv_rope_fwd: returns dqkv [B, S, (Hq + 2 * Hkv) * D]");
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
  m.def("fa_fwd", &fa_fwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"),
        py::arg("causal"), py::arg("doc_start") = py::none(),
        py::arg("doc_end") = py::none(),
        "flash-attention forward (bf16, D=128): returns (out, lse)");
  m.def("fa_delta", &fa_delta);
  m.def("fa_bwd", &fa_bwd, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("dout"),
        py::arg("lse"), py::arg("delta"), py::arg("scale"), py::arg("causal"),
        py::arg("doc_start") = py::none(), py::arg("doc_end") = py::none(),
        "flash-attention backward (bf16, D=128): returns (dq, dk, dv)");
  m.def("cross_entropy_fwd_bwd", &cross_entropy_fwd_bwd,
        "fused cross-entropy: returns row_loss, writes the gradient in place");
  m.def("mfma_probe", &mfma_probe, "mfma_f32_32x32x16_bf16 layout probe");
}

