// dgraph_amd — dispatcher registration of the fused gated aggregation kernels
// (csrc/kernels/spmm_gated.hip; ops/kernels.py: segment_gated / segment_gated_bwd_src).
// Every shape, dtype, device, stride and alignment contract the kernels rely on is checked
// here. The vector width follows from the row width: VEC = 4 (16-B accesses) when F is a
// multiple of 4, else 1; every array then needs a row stride that is a multiple of VEC and a
// base aligned to VEC elements, and one that is not raises here instead of running four times
// as many loads. Column ids are the caller's contract, as for segment_softmax.
//
// Zero rows and zero F return at once, and so does an accumulate pass without entries (the
// earlier result stands); a backward without entries zeroes dq / dv. A first pass with rows
// and no entries is legal (q / v may then have no rows): the launched kernel reads neither
// col nor q / v and writes zeros.
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
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), "segment_gated: ", name,
              " must be on ", ref.device());
  TORCH_CHECK(t.scalar_type() == at::kFloat, "segment_gated: ", name,
              " must be float32, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.size(1) == F && t.size(0) >= min_rows, "segment_gated: ", name,
              " must be [>= ", min_rows, ", ", F, "], got ", t.sizes());
  if (t.size(0) == 0 || F == 0) return;
  TORCH_CHECK(t.stride(1) == 1 || F == 1, "segment_gated: ", name,
              " must have unit column stride, got strides ", t.strides());
  TORCH_CHECK(t.size(0) == 1 || t.stride(0) >= F, "segment_gated: ", name,
              " has a row stride ", t.stride(0), " below its width ", F);
  if (F % 4 == 0)
    TORCH_CHECK((t.size(0) == 1 || t.stride(0) % 4 == 0) &&
                    reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                "segment_gated: ", name, " (width ", F, ", a multiple of 4) needs a row "
                "stride divisible by 4 and a 16-B aligned base, got strides ", t.strides());
}

IType pattern(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& ref,
              const char* what) {
  TORCH_CHECK(rowptr.is_cuda() && rowptr.device() == ref.device() &&
                  rowptr.scalar_type() == at::kLong && rowptr.is_contiguous() &&
                  rowptr.dim() == 1 && rowptr.numel() >= 1,
              "segment_gated: ", what, "rowptr must be contiguous int64 on ", ref.device());
  TORCH_CHECK(col.is_cuda() && col.device() == ref.device() && col.is_contiguous() &&
                  col.dim() == 1 &&
                  (col.scalar_type() == at::kInt || col.scalar_type() == at::kLong),
              "segment_gated: ", what, "col must be contiguous int32/int64 on ", ref.device());
  return col.scalar_type() == at::kInt ? IType::I32 : IType::I64;
}

void segment_gated_fwd_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& k,
                          const at::Tensor& q, const at::Tensor& v, at::Tensor& out,
                          const OptT& ds, bool accumulate) {
  TORCH_CHECK(k.is_cuda() && k.dim() == 2, "segment_gated: k must be a 2-D GPU tensor");
  const c10::DeviceGuard guard(k.device());
  const int64_t F = k.size(1);
  const IType it = pattern(rowptr, col, k, "");
  const int64_t nrows = rowptr.numel() - 1;
  rows_of(k, k, nrows, F, "k");
  // source rows: q and v are indexed by the same column ids
  TORCH_CHECK(q.dim() == 2 && v.dim() == 2 && q.size(0) == v.size(0),
              "segment_gated: q and v must be 2-D with the same row count");
  rows_of(q, k, 0, F, "q");
  rows_of(v, k, 0, F, "v");
  rows_of(out, k, nrows, F, "out");
  const at::Tensor* d = opt_t(ds);
  if (d != nullptr) rows_of(*d, k, nrows, F, "ds");
  if (nrows <= 0 || F == 0) return;
  if (accumulate && col.numel() == 0) return;  // nothing to add: the earlier result stands
  TORCH_CHECK(col.numel() == 0 || q.size(0) > 0, "segment_gated: entries but no source rows");
  DG_HIP_CHECK(segment_gated_fwd(
      it, rowptr.data_ptr<int64_t>(), col.data_ptr(), k.data_ptr<float>(), k.stride(0),
      q.data_ptr<float>(), q.stride(0), v.data_ptr<float>(), v.stride(0),
      out.data_ptr<float>(), out.stride(0), d != nullptr ? d->data_ptr<float>() : nullptr,
      d != nullptr ? d->stride(0) : 0, nrows, static_cast<int>(F), accumulate, cur_stream(k)));
}

void segment_gated_bwd_src_op(const at::Tensor& t_rowptr, const at::Tensor& t_col,
                              const at::Tensor& k, const at::Tensor& q, const at::Tensor& v,
                              const at::Tensor& g, at::Tensor& dq, at::Tensor& dv) {
  TORCH_CHECK(dq.is_cuda() && dq.dim() == 2, "segment_gated: dq must be a 2-D GPU tensor");
  const c10::DeviceGuard guard(dq.device());
  const int64_t F = dq.size(1);
  const IType it = pattern(t_rowptr, t_col, dq, "transposed ");
  const int64_t nrows = t_rowptr.numel() - 1;
  rows_of(dq, dq, nrows, F, "dq");
  rows_of(dv, dq, nrows, F, "dv");
  rows_of(q, dq, nrows, F, "q");
  rows_of(v, dq, nrows, F, "v");
  // destination rows: the arrays the transposed column ids index have the same row count
  TORCH_CHECK(g.dim() == 2, "segment_gated: g must be 2-D");
  const int64_t nd = g.size(0);
  rows_of(g, dq, 0, F, "g");
  rows_of(k, dq, nd, F, "k");
  if (nrows <= 0 || F == 0) return;
  if (t_col.numel() == 0) {  // no entry contributes (there may be no destination rows)
    dq.narrow(0, 0, nrows).zero_();
    dv.narrow(0, 0, nrows).zero_();
    return;
  }
  TORCH_CHECK(nd > 0, "segment_gated: entries but no destination rows");
  DG_HIP_CHECK(segment_gated_bwd_src(
      it, t_rowptr.data_ptr<int64_t>(), t_col.data_ptr(), k.data_ptr<float>(), k.stride(0),
      q.data_ptr<float>(), q.stride(0), v.data_ptr<float>(), v.stride(0), g.data_ptr<float>(),
      g.stride(0), dq.data_ptr<float>(), dq.stride(0), dv.data_ptr<float>(), dv.stride(0),
      nrows, static_cast<int>(F), cur_stream(dq)));
}

}  // namespace
}  // namespace dgraph

TORCH_LIBRARY_FRAGMENT(dgraph_amd, m) {
  m.def("segment_gated_fwd(Tensor rowptr, Tensor col, Tensor k, Tensor q, Tensor v, "
        "Tensor(a!) out, Tensor(b!)? ds, bool accumulate) -> ()");
  m.def("segment_gated_bwd_src(Tensor t_rowptr, Tensor t_col, Tensor k, Tensor q, Tensor v, "
        "Tensor g, Tensor(a!) dq, Tensor(b!) dv) -> ()");
}

TORCH_LIBRARY_IMPL(dgraph_amd, CUDA, m) {
  m.impl("segment_gated_fwd", &dgraph::segment_gated_fwd_op);
  m.impl("segment_gated_bwd_src", &dgraph::segment_gated_bwd_src_op);
}
