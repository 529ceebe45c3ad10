// dgraph_amd — dispatcher registration of the gated aggregation kernels with bf16 storage
// (csrc/kernels/spmm_gated_bf16.hip; ops/kernels.py: segment_gated / segment_gated_bwd_src on
// bf16 rows). Every contract the kernels rely on is checked here, before any launch: k, q, v
// and g bfloat16, the outputs bfloat16 or float32 (out and ds alike, dq and dv alike), one
// device, unit column stride, F a multiple of 8, every row stride a multiple of 8 elements
// (of 4 for an fp32 output) and every base 16-B aligned, the row counts, and accumulate only
// into fp32 outputs: an accumulated bf16 sum would be rounded twice. Column ids are the
// caller's contract, as for the fp32 ops.
//
// Zero rows and zero F return at once, and so does an accumulate pass without entries (the
// earlier result stands). A first pass or a backward whose pattern has no entries writes its
// zeros with plain fills: a launched kernel gathers row 0 of the source (destination) arrays
// for the slots past a row's end, and only a pattern with entries guarantees that row.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include "attn_check.h"
#include "check.h"
#include "kernels/kernels.h"

namespace dgraph {
namespace {

constexpr const char* kOp = "segment_gated_bf16";  // the prefix of every message

// an output: [>= min_rows, F] of `dt` (bfloat16 or float32) on ref's device, 16-B rows
DType out_rows(const at::Tensor& t, const at::Tensor& ref, at::ScalarType dt, int64_t min_rows,
               int64_t F, const char* name) {
  TORCH_CHECK(dt == at::kBFloat16 || dt == at::kFloat, kOp, ": ", name,
              " must be bfloat16 or float32, got ", dt);
  if (dt == at::kBFloat16) {
    rows_bf16(kOp, t, ref, min_rows, F, name);
    return DType::BF16;
  }
  rows_f32(kOp, t, ref, min_rows, F, name);
  return DType::F32;
}

int64_t width(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 2, kOp, ": ", name, " must be a 2-D GPU tensor");
  TORCH_CHECK(t.size(1) % 8 == 0, kOp, ": the width must be a multiple of 8 (eight bf16 "
              "channels per lane), got ", t.size(1));
  return t.size(1);
}

void segment_gated_bf16_fwd_op(const at::Tensor& rowptr, const at::Tensor& col,
                               const at::Tensor& k, const at::Tensor& q, const at::Tensor& v,
                               at::Tensor& out, const c10::optional<at::Tensor>& ds,
                               bool accumulate) {
  const int64_t F = width(k, "k");
  const c10::DeviceGuard guard(k.device());
  const IType it = pattern(kOp, rowptr, col, k, true);
  const int64_t nrows = rowptr.numel() - 1;
  if (nrows <= 0 || F == 0) return;
  rows_bf16(kOp, k, k, nrows, F, "k");
  // source rows: q and v are indexed by the same column ids
  TORCH_CHECK(q.dim() == 2 && v.dim() == 2 && q.size(0) == v.size(0), kOp,
              ": q and v must be 2-D with the same row count");
  rows_bf16(kOp, q, k, 0, F, "q");
  rows_bf16(kOp, v, k, 0, F, "v");
  const DType odt = out_rows(out, k, out.scalar_type(), nrows, F, "out");
  const at::Tensor* d = opt_t(ds);
  if (d != nullptr) out_rows(*d, k, out.scalar_type(), nrows, F, "ds");
  TORCH_CHECK(!accumulate || odt == DType::F32, kOp, ": accumulate needs float32 out / ds (a "
              "bfloat16 sum would be rounded twice), got ", out.scalar_type());
  if (col.numel() == 0) {
    if (accumulate) return;  // nothing to add: the earlier result stands
    out.narrow(0, 0, nrows).zero_();
    if (d != nullptr) d->narrow(0, 0, nrows).zero_();
    return;
  }
  TORCH_CHECK(q.size(0) > 0, kOp, ": entries but no source rows");
  DG_HIP_CHECK(segment_gated_bf16_fwd(
      it, odt, rowptr.data_ptr<int64_t>(), col.data_ptr(), bf16_ptr(k), k.stride(0),
      bf16_ptr(q), q.stride(0), bf16_ptr(v), v.stride(0), out.data_ptr(), out.stride(0),
      d != nullptr ? d->data_ptr() : nullptr, d != nullptr ? d->stride(0) : 0, nrows,
      static_cast<int>(F), accumulate, cur_stream(k)));
}

void segment_gated_bf16_bwd_src_op(const at::Tensor& t_rowptr, const at::Tensor& t_col,
                                   const at::Tensor& k, const at::Tensor& q,
                                   const at::Tensor& v, const at::Tensor& g, at::Tensor& dq,
                                   at::Tensor& dv) {
  const int64_t F = width(q, "q");
  const c10::DeviceGuard guard(q.device());
  const IType it = pattern(kOp, t_rowptr, t_col, q, true);
  const int64_t nrows = t_rowptr.numel() - 1;
  if (nrows <= 0 || F == 0) return;
  rows_bf16(kOp, q, q, nrows, F, "q");
  rows_bf16(kOp, v, q, nrows, F, "v");
  const DType odt = out_rows(dq, q, dq.scalar_type(), nrows, F, "dq");
  out_rows(dv, q, dq.scalar_type(), nrows, F, "dv");
  // destination rows: the arrays the transposed column ids index have the same row count
  TORCH_CHECK(g.dim() == 2, kOp, ": g must be 2-D");
  const int64_t nd = g.size(0);
  rows_bf16(kOp, g, q, 0, F, "g");
  rows_bf16(kOp, k, q, nd, F, "k");
  if (t_col.numel() == 0) {  // no entry contributes (there may be no destination rows)
    dq.narrow(0, 0, nrows).zero_();
    dv.narrow(0, 0, nrows).zero_();
    return;
  }
  TORCH_CHECK(nd > 0, kOp, ": entries but no destination rows");
  DG_HIP_CHECK(segment_gated_bf16_bwd_src(
      it, odt, t_rowptr.data_ptr<int64_t>(), t_col.data_ptr(), bf16_ptr(k), k.stride(0),
      bf16_ptr(q), q.stride(0), bf16_ptr(v), v.stride(0), bf16_ptr(g), g.stride(0),
      dq.data_ptr(), dq.stride(0), dv.data_ptr(), dv.stride(0), nrows, static_cast<int>(F),
      cur_stream(q)));
}

}  // namespace
}  // namespace dgraph

TORCH_LIBRARY_FRAGMENT(dgraph_amd, m) {
  m.def("segment_gated_bf16_fwd(Tensor rowptr, Tensor col, Tensor k, Tensor q, Tensor v, "
        "Tensor(a!) out, Tensor(b!)? ds, bool accumulate) -> ()");
  m.def("segment_gated_bf16_bwd_src(Tensor t_rowptr, Tensor t_col, Tensor k, Tensor q, "
        "Tensor v, Tensor g, Tensor(a!) dq, Tensor(b!) dv) -> ()");
}

TORCH_LIBRARY_IMPL(dgraph_amd, CUDA, m) {
  m.impl("segment_gated_bf16_fwd", &dgraph::segment_gated_bf16_fwd_op);
  m.impl("segment_gated_bf16_bwd_src", &dgraph::segment_gated_bf16_bwd_src_op);
}
