// dgraph_amd — dispatcher registration of the softmax aggregation kernels with edge features
// (csrc/kernels/spmm_softmax_edge.hip; ops/kernels.py: segment_softmax_edge /
// segment_softmax_edge_bwd). Every shape, dtype, device, stride and alignment contract the
// kernels rely on is checked here, by the rules of bindings_softmax.cpp: VEC = 4 (16-B
// accesses) when F is a multiple of 4, else 1; every row array, the edge rows e and de
// included, then needs a row stride that is a multiple of VEC and a base aligned to VEC
// elements, and one that is not raises here instead of running four times as many loads.
// Column ids are the caller's contract.
//
// Zero rows and zero F return at once, and so does a second pass or a backward without
// entries (nothing to merge; no de row to write, the dt partial rows are zeroed). A first
// pass with rows and no entries is legal (x and e may then have no rows): the launched
// kernel reads neither and writes the empty-row results (0, -inf).
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include "check.h"
#include "kernels/kernels.h"

namespace dgraph {
namespace {

using OptT = c10::optional<at::Tensor>;

hipStream_t cur_stream(const at::Tensor& t) {
  return c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

const at::Tensor* opt_t(const OptT& t) { return (t.has_value() && t->defined()) ? &*t : nullptr; }

// [rows >= min_rows (exactly min_rows when exact), F] fp32 on ref's device, unit column
// stride, rows not overlapping
void rows_of(const at::Tensor& t, const at::Tensor& ref, int64_t min_rows, int64_t F,
             const char* name, bool exact = false) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), "segment_softmax_edge: ", name,
              " must be on ", ref.device());
  TORCH_CHECK(t.scalar_type() == at::kFloat, "segment_softmax_edge: ", name,
              " must be float32, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.size(1) == F &&
                  (exact ? t.size(0) == min_rows : t.size(0) >= min_rows),
              "segment_softmax_edge: ", name, " must be [", exact ? "" : ">= ", min_rows, ", ",
              F, "], got ", t.sizes());
  if (t.size(0) == 0 || F == 0) return;
  TORCH_CHECK(t.stride(1) == 1 || F == 1, "segment_softmax_edge: ", name,
              " must have unit column stride, got strides ", t.strides());
  TORCH_CHECK(t.size(0) == 1 || t.stride(0) >= F, "segment_softmax_edge: ", name,
              " has a row stride ", t.stride(0), " below its width ", F);
  if (F % 4 == 0)
    TORCH_CHECK((t.size(0) == 1 || t.stride(0) % 4 == 0) &&
                    reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                "segment_softmax_edge: ", name, " (width ", F, ", a multiple of 4) needs a row "
                "stride divisible by 4 and a 16-B aligned base, got strides ", t.strides());
}

// the temperature: contiguous fp32 [F]
void temperature(const at::Tensor& t, const at::Tensor& ref, int64_t F) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device() && t.scalar_type() == at::kFloat &&
                  t.dim() == 1 && t.numel() == F && t.is_contiguous(),
              "segment_softmax_edge: t must be contiguous float32 [", F, "] on ", ref.device(),
              ", got ", t.scalar_type(), " ", t.sizes());
  TORCH_CHECK(F % 4 != 0 || reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "segment_softmax_edge: t (width ", F, ", a multiple of 4) needs a 16-B aligned "
              "base");
}

IType pattern(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& ref) {
  TORCH_CHECK(rowptr.is_cuda() && rowptr.device() == ref.device() &&
                  rowptr.scalar_type() == at::kLong && rowptr.is_contiguous() &&
                  rowptr.dim() == 1 && rowptr.numel() >= 1,
              "segment_softmax_edge: rowptr must be contiguous int64 on ", ref.device());
  TORCH_CHECK(col.is_cuda() && col.device() == ref.device() && col.is_contiguous() &&
                  col.dim() == 1 &&
                  (col.scalar_type() == at::kInt || col.scalar_type() == at::kLong),
              "segment_softmax_edge: col must be contiguous int32/int64 on ", ref.device());
  return col.scalar_type() == at::kInt ? IType::I32 : IType::I64;
}

// a row stride the kernel may multiply a slot number by (one row: its width)
int64_t ld(const at::Tensor& t, int64_t F) { return t.size(0) > 1 ? t.stride(0) : F; }

void segment_softmax_edge_fwd_op(const at::Tensor& rowptr, const at::Tensor& col,
                                 const at::Tensor& x, const at::Tensor& e, const at::Tensor& t,
                                 at::Tensor& out, at::Tensor& lse, bool relu, double eps,
                                 bool second, const OptT& row_map) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2, "segment_softmax_edge: x must be a 2-D GPU tensor");
  const c10::DeviceGuard guard(x.device());
  const int64_t F = x.size(1);
  rows_of(x, x, 0, F, "x");
  temperature(t, x, F);
  const IType it = pattern(rowptr, col, x);
  rows_of(e, x, col.numel(), F, "e", /*exact=*/true);
  const int64_t nrows = rowptr.numel() - 1;
  // output rows: the CSR rows, or wherever row_map sends them
  const int64_t* rmap = nullptr;
  int64_t min_rows = nrows;
  if (const at::Tensor* rm = opt_t(row_map)) {
    TORCH_CHECK(rm->is_cuda() && rm->device() == x.device() && rm->scalar_type() == at::kLong &&
                    rm->is_contiguous() && rm->numel() == nrows,
                "segment_softmax_edge: row_map must be contiguous int64 [nrows] on ",
                x.device());
    rmap = rm->data_ptr<int64_t>();
    min_rows = 0;  // the map's values are the caller's contract
  }
  rows_of(out, x, min_rows, F, "out");
  rows_of(lse, x, min_rows, F, "lse");
  if (nrows <= 0 || F == 0) return;
  if (second && col.numel() == 0) return;  // nothing to merge: the incumbent stands
  TORCH_CHECK(col.numel() == 0 || x.size(0) > 0,
              "segment_softmax_edge: entries but no source rows");
  DG_HIP_CHECK(segment_softmax_edge_fwd(
      it, rowptr.data_ptr<int64_t>(), col.data_ptr(), x.data_ptr<float>(), ld(x, F),
      e.data_ptr<float>(), ld(e, F), t.data_ptr<float>(), out.data_ptr<float>(), ld(out, F),
      lse.data_ptr<float>(), ld(lse, F), nrows, static_cast<int>(F), relu,
      static_cast<float>(eps), second, rmap, cur_stream(x)));
}

void segment_softmax_edge_bwd_op(const at::Tensor& rowptr, const at::Tensor& col,
                                 const at::Tensor& x, const at::Tensor& e, const at::Tensor& t,
                                 const at::Tensor& g, const at::Tensor& out_fwd,
                                 const at::Tensor& lse, at::Tensor& de, bool relu, double eps,
                                 const OptT& dt_part) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2, "segment_softmax_edge: x must be a 2-D GPU tensor");
  const c10::DeviceGuard guard(x.device());
  const int64_t F = x.size(1);
  const IType it = pattern(rowptr, col, x);
  const int64_t nrows = rowptr.numel() - 1;
  const int64_t nnz = col.numel();
  rows_of(x, x, 0, F, "x");
  rows_of(e, x, nnz, F, "e", /*exact=*/true);
  rows_of(de, x, nnz, F, "de");
  temperature(t, x, F);
  rows_of(g, x, nrows, F, "g");
  rows_of(out_fwd, x, nrows, F, "out_fwd");
  rows_of(lse, x, nrows, F, "lse");
  float* part = nullptr;
  const at::Tensor* dp = opt_t(dt_part);
  if (dp != nullptr) {
    const int64_t P = segment_softmax_edge_dt_parts(nrows);
    TORCH_CHECK(dp->is_cuda() && dp->device() == x.device() &&
                    dp->scalar_type() == at::kFloat && dp->dim() == 2 && dp->size(0) == P &&
                    dp->size(1) == F && dp->is_contiguous(),
                "segment_softmax_edge: dt_part must be contiguous float32 [", P, ", ", F,
                "] on ", x.device(), ", got ", dp->sizes());
    TORCH_CHECK(F % 4 != 0 || dp->numel() == 0 ||
                    reinterpret_cast<uintptr_t>(dp->data_ptr()) % 16 == 0,
                "segment_softmax_edge: dt_part needs a 16-B aligned base");
    if (dp->numel() > 0) part = dp->data_ptr<float>();
  }
  if (nrows <= 0 || F == 0) return;
  if (nnz == 0) {  // no slot: no de row; dt is zero
    if (dp != nullptr) {
      at::Tensor z = *dp;
      z.zero_();
    }
    return;
  }
  TORCH_CHECK(x.size(0) > 0, "segment_softmax_edge: entries but no source rows");
  DG_HIP_CHECK(segment_softmax_edge_bwd(
      it, rowptr.data_ptr<int64_t>(), col.data_ptr(), x.data_ptr<float>(), ld(x, F),
      e.data_ptr<float>(), ld(e, F), t.data_ptr<float>(), g.data_ptr<float>(), ld(g, F),
      out_fwd.data_ptr<float>(), ld(out_fwd, F), lse.data_ptr<float>(), ld(lse, F),
      de.data_ptr<float>(), ld(de, F), part, nrows, static_cast<int>(F), relu,
      static_cast<float>(eps), cur_stream(x)));
}

int64_t segment_softmax_edge_dt_parts_op(int64_t nrows) {
  return segment_softmax_edge_dt_parts(nrows);
}

}  // namespace
}  // namespace dgraph

TORCH_LIBRARY_FRAGMENT(dgraph_amd, m) {
  m.def("segment_softmax_edge_fwd(Tensor rowptr, Tensor col, Tensor x, Tensor e, Tensor t, "
        "Tensor(a!) out, Tensor(b!) lse, bool relu, float eps, bool second, Tensor? row_map) "
        "-> ()");
  m.def("segment_softmax_edge_bwd(Tensor rowptr, Tensor col, Tensor x, Tensor e, Tensor t, "
        "Tensor g, Tensor out_fwd, Tensor lse, Tensor(a!) de, bool relu, float eps, "
        "Tensor(b!)? dt_part) -> ()");
  m.def("segment_softmax_edge_dt_parts(int nrows) -> int",
        &dgraph::segment_softmax_edge_dt_parts_op);
}

TORCH_LIBRARY_IMPL(dgraph_amd, CUDA, m) {
  m.impl("segment_softmax_edge_fwd", &dgraph::segment_softmax_edge_fwd_op);
  m.impl("segment_softmax_edge_bwd", &dgraph::segment_softmax_edge_bwd_op);
}
