// dgraph_amd — dispatcher registration of DropEdge fused into the CSR aggregation
// (csrc/kernels/spmm_drop.hip; ops/kernels.py: spmm_drop, kept_degree) and of the host
// evaluation of its keep decision (edge_keep_host, the counterpart of attn_keep_mask_host).
// Every dtype, device, shape, stride and range contract the kernels rely on is checked here;
// column ids are the caller's contract, as for spmm (x, col_scale and col_ids must cover
// every column id of the pattern).
//
// No rows or no entries return at once, before any launch: without entries spmm_drop still
// owes out = beta * out on the rows of the pattern, and kept_degree (not accumulating) zeros,
// which torch does.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include "check.h"
#include "kernels/kernels.h"
#include "kernels/philox.h"

namespace dgraph {
namespace {

using OptT = c10::optional<at::Tensor>;

bool has(const OptT& t) { return t.has_value() && t->defined(); }

// a contiguous 1-D tensor of `dtype` with at least n elements on ref's device, or null
const void* vec_of(const OptT& t, const at::Tensor& ref, at::ScalarType dtype, int64_t n,
                   const char* op, const char* name) {
  if (!has(t)) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->device() == ref.device() && t->scalar_type() == dtype &&
                  t->dim() == 1 && t->is_contiguous() && t->numel() >= n,
              op, ": ", name, " must be contiguous ", dtype, " [>= ", n, "] on ", ref.device(),
              ", got ", t->scalar_type(), " ", t->sizes());
  return t->numel() > 0 ? t->data_ptr() : nullptr;
}

// the pattern, the ids and the seed, shared by both ops; out_rows: rows of the output array
SpmmDropArgs pattern_args(const char* op, const at::Tensor& rowptr, const at::Tensor& col,
                          const at::Tensor& ref, int64_t out_rows, int64_t num_cols,
                          const OptT& row_map, const OptT& row_ids, const OptT& col_ids,
                          int64_t row_base, int64_t col_base, const at::Tensor& seed, double p,
                          bool undirected, bool transposed) {
  TORCH_CHECK(rowptr.is_cuda() && rowptr.device() == ref.device() &&
                  rowptr.scalar_type() == at::kLong && rowptr.is_contiguous() &&
                  rowptr.dim() == 1 && rowptr.numel() >= 1,
              op, ": rowptr must be contiguous int64 on ", ref.device());
  TORCH_CHECK(col.is_cuda() && col.device() == ref.device() && col.is_contiguous() &&
                  col.dim() == 1 &&
                  (col.scalar_type() == at::kInt || col.scalar_type() == at::kLong),
              op, ": col must be contiguous int32/int64 on ", ref.device());
  TORCH_CHECK(seed.is_cuda() && seed.device() == ref.device() &&
                  seed.scalar_type() == at::kLong && seed.numel() == 1,
              op, ": seed must be ONE int64 on ", ref.device(), " (the kernel reads it)");
  TORCH_CHECK(p >= 0.0 && p < 1.0, op, ": p must lie in [0, 1), got ", p);
  TORCH_CHECK(row_base >= 0 && col_base >= 0, op, ": id bases must be non-negative");
  SpmmDropArgs a;
  a.nrows = rowptr.numel() - 1;
  TORCH_CHECK(a.nrows <= 0x7fffffff, op, ": ", a.nrows, " rows do not fit int32");
  a.rowptr = rowptr.data_ptr<int64_t>();
  a.col = col.numel() > 0 ? col.data_ptr() : nullptr;
  a.it = col.scalar_type() == at::kInt ? IType::I32 : IType::I64;
  if (has(row_map)) {
    a.row_map = static_cast<const int64_t*>(
        vec_of(row_map, ref, at::kLong, a.nrows, op, "row_map"));
    TORCH_CHECK(row_map->numel() == a.nrows, op, ": row_map must have the CSR's ", a.nrows,
                " rows");
  } else {
    TORCH_CHECK(out_rows >= a.nrows, op, ": the output has ", out_rows, " rows, the CSR ",
                a.nrows);
  }
  a.row_ids = static_cast<const int64_t*>(vec_of(row_ids, ref, at::kLong, out_rows, op,
                                                 "row_ids"));
  a.col_ids = static_cast<const int64_t*>(vec_of(col_ids, ref, at::kLong, num_cols, op,
                                                 "col_ids"));
  a.row_base = row_base;
  a.col_base = col_base;
  a.seed = seed.data_ptr<int64_t>();
  a.thr = edge_keep_threshold(p);
  a.undirected = undirected;
  a.transposed = transposed;
  return a;
}

void spmm_drop_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& x,
                  at::Tensor& out, const at::Tensor& seed, double p, bool undirected,
                  bool transposed, const OptT& col_scale, const OptT& row_scale, double beta,
                  const OptT& row_map, const OptT& row_ids, const OptT& col_ids,
                  int64_t row_base, int64_t col_base) {
  const char* op = "spmm_drop_f32";
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.scalar_type() == at::kFloat, op,
              ": x must be a 2-D float32 GPU tensor (bf16 rows are not supported)");
  const c10::DeviceGuard guard(x.device());
  const int64_t F = x.size(1);
  TORCH_CHECK(F >= 1 && F <= 0x7fffffff, op, ": F must be at least 1, got ", F);
  TORCH_CHECK(out.is_cuda() && out.device() == x.device() && out.scalar_type() == at::kFloat &&
                  out.dim() == 2 && out.size(1) == F,
              op, ": out must be float32 [rows, ", F, "] on ", x.device(), ", got ",
              out.scalar_type(), " ", out.sizes());
  for (const at::Tensor* t : {&x, static_cast<const at::Tensor*>(&out)}) {
    TORCH_CHECK(t->stride(1) == 1 || F == 1, op, ": rows need unit column stride, got strides ",
                t->strides());
    TORCH_CHECK(t->size(0) <= 1 || t->stride(0) >= F, op, ": a row stride ", t->stride(0),
                " is below the width ", F);
  }
  const SpmmDropArgs a =
      pattern_args(op, rowptr, col, x, out.size(0), x.size(0), row_map, row_ids, col_ids,
                   row_base, col_base, seed, p, undirected, transposed);
  const float* cs = static_cast<const float*>(
      vec_of(col_scale, x, at::kFloat, x.size(0), op, "col_scale"));
  const float* rs = static_cast<const float*>(
      vec_of(row_scale, x, at::kFloat, out.size(0), op, "row_scale"));
  if (a.nrows <= 0) return;
  if (col.numel() == 0) {  // out = beta * out on the rows of the pattern, no launch
    if (has(row_map)) {
      if (beta == 0.0) out.index_fill_(0, *row_map, 0.0);
      else if (beta != 1.0) out.index_copy_(0, *row_map, out.index_select(0, *row_map) * beta);
    } else {
      at::Tensor rows = out.narrow(0, 0, a.nrows);
      if (beta == 0.0) rows.zero_();
      else if (beta != 1.0) rows.mul_(beta);
    }
    return;
  }
  TORCH_CHECK(x.size(0) > 0, op, ": entries but no rows of x");
  DG_HIP_CHECK(spmm_drop_f32(a, cs, rs, x.data_ptr<float>(), x.size(0) > 1 ? x.stride(0) : F,
                             out.data_ptr<float>(), out.size(0) > 1 ? out.stride(0) : F,
                             static_cast<int>(F), static_cast<float>(beta),
                             c10::hip::getCurrentHIPStream(x.device().index()).stream()));
}

void kept_degree_op(const at::Tensor& rowptr, const at::Tensor& col, at::Tensor& kept,
                    const at::Tensor& seed, double p, bool undirected, bool transposed,
                    bool accumulate, const OptT& row_map, const OptT& row_ids,
                    const OptT& col_ids, int64_t num_cols, int64_t row_base, int64_t col_base) {
  const char* op = "kept_degree";
  TORCH_CHECK(kept.is_cuda() && kept.scalar_type() == at::kInt && kept.dim() == 1 &&
                  kept.is_contiguous(),
              op, ": kept must be a contiguous int32 GPU vector");
  const c10::DeviceGuard guard(kept.device());
  TORCH_CHECK(num_cols >= 0, op, ": num_cols must be non-negative");
  const SpmmDropArgs a =
      pattern_args(op, rowptr, col, kept, kept.numel(), num_cols, row_map, row_ids, col_ids,
                   row_base, col_base, seed, p, undirected, transposed);
  if (a.nrows <= 0) return;
  if (col.numel() == 0) {  // no launch
    if (!accumulate) {
      if (has(row_map)) kept.index_fill_(0, *row_map, 0);
      else kept.narrow(0, 0, a.nrows).zero_();
    }
    return;
  }
  DG_HIP_CHECK(kept_degree(a, kept.data_ptr<int32_t>(), accumulate,
                           c10::hip::getCurrentHIPStream(kept.device().index()).stream()));
}

// keep[i] of the edges a[i] <- b[i] (dst, src): the device function on the host
at::Tensor edge_keep_host(int64_t seed, const at::Tensor& a, const at::Tensor& b, double p,
                          bool undirected) {
  TORCH_CHECK(!a.is_cuda() && !b.is_cuda() && a.scalar_type() == at::kLong &&
                  b.scalar_type() == at::kLong && a.dim() == 1 && b.dim() == 1 &&
                  a.numel() == b.numel(),
              "edge_keep_host: a and b must be CPU int64 vectors of one length");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "edge_keep_host: p must lie in [0, 1), got ", p);
  const uint32_t thr = edge_keep_threshold(p);
  const at::Tensor ac = a.contiguous(), bc = b.contiguous();
  const int64_t* pa = ac.data_ptr<int64_t>();
  const int64_t* pb = bc.data_ptr<int64_t>();
  at::Tensor keep = at::empty({a.numel()}, at::TensorOptions().dtype(at::kBool));
  bool* out = keep.data_ptr<bool>();
  for (int64_t i = 0; i < a.numel(); ++i) {
    TORCH_CHECK(pa[i] >= 0 && pb[i] >= 0, "edge_keep_host: ids must be non-negative");
    out[i] = edge_keep(static_cast<uint64_t>(seed), pa[i], pb[i], thr, undirected);
  }
  return keep;
}

}  // namespace
}  // namespace dgraph

TORCH_LIBRARY_FRAGMENT(dgraph_amd, m) {
  m.def("spmm_drop_f32(Tensor rowptr, Tensor col, Tensor x, Tensor(a!) out, Tensor seed, "
        "float p, bool undirected, bool transposed, Tensor? col_scale, Tensor? row_scale, "
        "float beta, Tensor? row_map, Tensor? row_ids, Tensor? col_ids, int row_base, "
        "int col_base) -> ()");
  m.def("kept_degree(Tensor rowptr, Tensor col, Tensor(a!) kept, Tensor seed, float p, "
        "bool undirected, bool transposed, bool accumulate, Tensor? row_map, Tensor? row_ids, "
        "Tensor? col_ids, int num_cols, int row_base, int col_base) -> ()");
  m.def("edge_keep_host(int seed, Tensor a, Tensor b, float p, bool undirected=False) -> Tensor",
        &dgraph::edge_keep_host);
}

TORCH_LIBRARY_IMPL(dgraph_amd, CUDA, m) {
  m.impl("spmm_drop_f32", &dgraph::spmm_drop_op);
  m.impl("kept_degree", &dgraph::kept_degree_op);
}
