// dgraph_amd — dispatcher registration of the fused softmax aggregation kernels
// (csrc/kernels/spmm_softmax.hip; ops/kernels.py: segment_softmax / segment_softmax_bwd).
// Every shape, dtype, device, stride and alignment contract the kernels rely on is checked
// here. The vector width follows from the row width: VEC = 4 (16-B accesses) when F is a
// multiple of 4, else 1; every array then needs a row stride that is a multiple of VEC and a
// base aligned to VEC elements, and one that is not raises here instead of running four times
// as many loads. Column ids are the caller's contract, as for segment_extreme.
//
// Zero rows and zero F return at once, and so does a second pass or a backward without
// entries (nothing to merge; dx is zeroed). A first pass with rows and no entries is legal
// (x may then have no rows): the launched kernel reads neither col nor x and writes the
// empty-row results (0, -inf).
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

// [rows >= min_rows, F] fp32 on ref's device, unit column stride, rows not overlapping
void rows_of(const at::Tensor& t, const at::Tensor& ref, int64_t min_rows, int64_t F,
             const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), "segment_softmax: ", name,
              " must be on ", ref.device());
  TORCH_CHECK(t.scalar_type() == at::kFloat, "segment_softmax: ", name,
              " must be float32, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.size(1) == F && t.size(0) >= min_rows, "segment_softmax: ", name,
              " must be [>= ", min_rows, ", ", F, "], got ", t.sizes());
  if (t.size(0) == 0 || F == 0) return;
  TORCH_CHECK(t.stride(1) == 1 || F == 1, "segment_softmax: ", name,
              " must have unit column stride, got strides ", t.strides());
  TORCH_CHECK(t.size(0) == 1 || t.stride(0) >= F, "segment_softmax: ", name,
              " has a row stride ", t.stride(0), " below its width ", F);
  if (F % 4 == 0)
    TORCH_CHECK((t.size(0) == 1 || t.stride(0) % 4 == 0) &&
                    reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                "segment_softmax: ", name, " (width ", F, ", a multiple of 4) needs a row "
                "stride divisible by 4 and a 16-B aligned base, got strides ", t.strides());
}

// the temperature: contiguous fp32 [F]
void temperature(const at::Tensor& t, const at::Tensor& ref, int64_t F) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device() && t.scalar_type() == at::kFloat &&
                  t.dim() == 1 && t.numel() == F && t.is_contiguous(),
              "segment_softmax: t must be contiguous float32 [", F, "] on ", ref.device(),
              ", got ", t.scalar_type(), " ", t.sizes());
  TORCH_CHECK(F % 4 != 0 || reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              "segment_softmax: t (width ", F, ", a multiple of 4) needs a 16-B aligned base");
}

IType pattern(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& ref,
              const char* what) {
  TORCH_CHECK(rowptr.is_cuda() && rowptr.device() == ref.device() &&
                  rowptr.scalar_type() == at::kLong && rowptr.is_contiguous() &&
                  rowptr.dim() == 1 && rowptr.numel() >= 1,
              "segment_softmax: ", what, "rowptr must be contiguous int64 on ", ref.device());
  TORCH_CHECK(col.is_cuda() && col.device() == ref.device() && col.is_contiguous() &&
                  col.dim() == 1 &&
                  (col.scalar_type() == at::kInt || col.scalar_type() == at::kLong),
              "segment_softmax: ", what, "col must be contiguous int32/int64 on ",
              ref.device());
  return col.scalar_type() == at::kInt ? IType::I32 : IType::I64;
}

void segment_softmax_fwd_op(const at::Tensor& rowptr, const at::Tensor& col,
                            const at::Tensor& x, const at::Tensor& t, at::Tensor& out,
                            at::Tensor& lse, bool second, const OptT& row_map) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2, "segment_softmax: x must be a 2-D GPU tensor");
  const c10::DeviceGuard guard(x.device());
  const int64_t F = x.size(1);
  rows_of(x, x, 0, F, "x");
  temperature(t, x, F);
  const IType it = pattern(rowptr, col, x, "");
  const int64_t nrows = rowptr.numel() - 1;
  // output rows: the CSR rows, or wherever row_map sends them
  const int64_t* rmap = nullptr;
  int64_t min_rows = nrows;
  if (const at::Tensor* rm = opt_t(row_map)) {
    TORCH_CHECK(rm->is_cuda() && rm->device() == x.device() && rm->scalar_type() == at::kLong &&
                    rm->is_contiguous() && rm->numel() == nrows,
                "segment_softmax: row_map must be contiguous int64 [nrows] on ", x.device());
    rmap = rm->data_ptr<int64_t>();
    min_rows = 0;  // the map's values are the caller's contract, as for segment_extreme
  }
  rows_of(out, x, min_rows, F, "out");
  rows_of(lse, x, min_rows, F, "lse");
  if (nrows <= 0 || F == 0) return;
  if (second && col.numel() == 0) return;  // nothing to merge: the incumbent stands
  TORCH_CHECK(col.numel() == 0 || x.size(0) > 0, "segment_softmax: entries but no source rows");
  DG_HIP_CHECK(segment_softmax_fwd(it, rowptr.data_ptr<int64_t>(), col.data_ptr(),
                                   x.data_ptr<float>(), x.stride(0), t.data_ptr<float>(),
                                   out.data_ptr<float>(), out.stride(0), lse.data_ptr<float>(),
                                   lse.stride(0), nrows, static_cast<int>(F), second, rmap,
                                   cur_stream(x)));
}

void segment_softmax_bwd_op(const at::Tensor& t_rowptr, const at::Tensor& t_col,
                            const at::Tensor& x, const at::Tensor& t, const at::Tensor& g,
                            const at::Tensor& out_fwd, const at::Tensor& lse, at::Tensor& dx,
                            const OptT& dt_part) {
  TORCH_CHECK(dx.is_cuda() && dx.dim() == 2, "segment_softmax: dx must be a 2-D GPU tensor");
  const c10::DeviceGuard guard(dx.device());
  const int64_t F = dx.size(1);
  const IType it = pattern(t_rowptr, t_col, dx, "transposed ");
  const int64_t nrows = t_rowptr.numel() - 1;
  rows_of(dx, dx, nrows, F, "dx");
  rows_of(x, dx, nrows, F, "x");
  temperature(t, dx, F);
  // destination rows: the arrays the transposed column ids index have the same row count
  TORCH_CHECK(g.dim() == 2, "segment_softmax: g must be 2-D");
  const int64_t nd = g.size(0);
  rows_of(g, dx, 0, F, "g");
  rows_of(out_fwd, dx, nd, F, "out_fwd");
  rows_of(lse, dx, nd, F, "lse");
  float* part = nullptr;
  const at::Tensor* dp = opt_t(dt_part);
  if (dp != nullptr) {
    const int64_t P = segment_softmax_dt_parts(nrows);
    TORCH_CHECK(dp->is_cuda() && dp->device() == dx.device() &&
                    dp->scalar_type() == at::kFloat && dp->dim() == 2 && dp->size(0) == P &&
                    dp->size(1) == F && dp->is_contiguous(),
                "segment_softmax: dt_part must be contiguous float32 [", P, ", ", F, "] on ",
                dx.device(), ", got ", dp->sizes());
    TORCH_CHECK(F % 4 != 0 || dp->numel() == 0 ||
                    reinterpret_cast<uintptr_t>(dp->data_ptr()) % 16 == 0,
                "segment_softmax: dt_part needs a 16-B aligned base");
    if (dp->numel() > 0) part = dp->data_ptr<float>();
  }
  if (nrows <= 0 || F == 0) return;
  if (t_col.numel() == 0) {  // no entry contributes (there may be no destination rows)
    dx.narrow(0, 0, nrows).zero_();
    if (dp != nullptr) {
      at::Tensor z = *dp;
      z.zero_();
    }
    return;
  }
  TORCH_CHECK(nd > 0, "segment_softmax: entries but no destination rows");
  DG_HIP_CHECK(segment_softmax_bwd(it, t_rowptr.data_ptr<int64_t>(), t_col.data_ptr(),
                                   x.data_ptr<float>(), x.stride(0), t.data_ptr<float>(),
                                   g.data_ptr<float>(), g.stride(0), out_fwd.data_ptr<float>(),
                                   out_fwd.stride(0), lse.data_ptr<float>(), lse.stride(0),
                                   dx.data_ptr<float>(), dx.stride(0), part, nrows,
                                   static_cast<int>(F), cur_stream(dx)));
}

int64_t segment_softmax_dt_parts_op(int64_t nrows) { return segment_softmax_dt_parts(nrows); }

}  // namespace
}  // namespace dgraph

TORCH_LIBRARY_FRAGMENT(dgraph_amd, m) {
  m.def("segment_softmax_fwd(Tensor rowptr, Tensor col, Tensor x, Tensor t, Tensor(a!) out, "
        "Tensor(b!) lse, bool second, Tensor? row_map) -> ()");
  m.def("segment_softmax_bwd(Tensor t_rowptr, Tensor t_col, Tensor x, Tensor t, Tensor g, "
        "Tensor out_fwd, Tensor lse, Tensor(a!) dx, Tensor(b!)? dt_part) -> ()");
  m.def("segment_softmax_dt_parts(int nrows) -> int", &dgraph::segment_softmax_dt_parts_op);
}

TORCH_LIBRARY_IMPL(dgraph_amd, CUDA, m) {
  m.impl("segment_softmax_fwd", &dgraph::segment_softmax_fwd_op);
  m.impl("segment_softmax_bwd", &dgraph::segment_softmax_bwd_op);
}
