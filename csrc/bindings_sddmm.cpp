// dgraph_amd — dispatcher registration of the per-edge dot products (SDDMM,
// csrc/kernels/sddmm.hip; ops/kernels.py: edge_dot). Every shape, dtype, device, stride and
// alignment contract the kernel relies on is checked here. A shape that takes the vector path
// (sddmm_vec_shape_ok: four elements per lane and access) needs a and b with bases aligned
// to four elements and row strides divisible by 4, and one that is not raises here instead of
// running four times as many loads; every other shape needs unit column stride only. Column
// ids are the caller's contract, as for spmm.
//
// No entries, no rows or F == 0 return at once, before any launch (the scores of F == 0 are
// zeros: the caller's fill).
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include "check.h"
#include "kernels/kernels.h"

namespace dgraph {
namespace {

using OptT = c10::optional<at::Tensor>;

// [rows >= min_rows, F] fp32 / bf16 on ref's device, unit column stride, rows not overlapping
void rows_of(const at::Tensor& t, const at::Tensor& ref, int64_t min_rows, int64_t F, bool vec,
             const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), "edge_dot: ", name, " must be on ",
              ref.device());
  TORCH_CHECK(t.scalar_type() == ref.scalar_type(), "edge_dot: ", name, " must be ",
              ref.scalar_type(), " like a, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.size(1) == F && t.size(0) >= min_rows, "edge_dot: ", name,
              " must be [>= ", min_rows, ", ", F, "], got ", t.sizes());
  if (t.size(0) == 0 || F == 0) return;
  TORCH_CHECK(t.stride(1) == 1 || F == 1, "edge_dot: ", name,
              " must have unit column stride, got strides ", t.strides());
  TORCH_CHECK(t.size(0) == 1 || t.stride(0) >= F, "edge_dot: ", name, " has a row stride ",
              t.stride(0), " below its width ", F);
  if (vec)
    TORCH_CHECK((t.size(0) == 1 || t.stride(0) % 4 == 0) &&
                    reinterpret_cast<uintptr_t>(t.data_ptr()) % (4 * t.element_size()) == 0,
                "edge_dot: ", name, " (head width a multiple of 4) needs a row stride divisible "
                "by 4 and a base aligned to 4 elements, got strides ", t.strides());
}

void edge_dot_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& a,
                 const at::Tensor& b, at::Tensor& out, int64_t heads, double scale,
                 const OptT& row_scale) {
  TORCH_CHECK(a.is_cuda() && a.dim() == 2, "edge_dot: a must be a 2-D GPU tensor");
  TORCH_CHECK(a.scalar_type() == at::kFloat || a.scalar_type() == at::kBFloat16,
              "edge_dot: a must be float32 or bfloat16, got ", a.scalar_type());
  const c10::DeviceGuard guard(a.device());
  const int64_t F = a.size(1);
  TORCH_CHECK(heads > 0 && F % heads == 0 && F <= 0x7fffffff, "edge_dot: heads ", heads,
              " must divide the width ", F);
  TORCH_CHECK(rowptr.is_cuda() && rowptr.device() == a.device() &&
                  rowptr.scalar_type() == at::kLong && rowptr.is_contiguous() &&
                  rowptr.dim() == 1 && rowptr.numel() >= 1,
              "edge_dot: rowptr must be contiguous int64 on ", a.device());
  TORCH_CHECK(col.is_cuda() && col.device() == a.device() && col.is_contiguous() &&
                  col.dim() == 1 &&
                  (col.scalar_type() == at::kInt || col.scalar_type() == at::kLong),
              "edge_dot: col must be contiguous int32/int64 on ", a.device());
  const IType it = col.scalar_type() == at::kInt ? IType::I32 : IType::I64;
  const DType dt = a.scalar_type() == at::kFloat ? DType::F32 : DType::BF16;
  const int64_t nrows = rowptr.numel() - 1, nnz = col.numel();
  TORCH_CHECK(nrows <= 0x7fffffff, "edge_dot: ", nrows, " rows do not fit int32");
  const bool vec = sddmm_vec_shape_ok(static_cast<int>(F), static_cast<int>(heads));
  TORCH_CHECK(a.size(0) == nrows, "edge_dot: a must have the CSR's ", nrows, " rows, got ",
              a.sizes());
  rows_of(a, a, nrows, F, vec, "a");
  TORCH_CHECK(b.dim() == 2, "edge_dot: b must be 2-D");
  rows_of(b, a, 0, F, vec, "b");
  TORCH_CHECK(out.is_cuda() && out.device() == a.device() && out.scalar_type() == at::kFloat &&
                  out.dim() == 2 && out.size(0) == nnz && out.size(1) == heads &&
                  out.is_contiguous(),
              "edge_dot: out must be contiguous float32 [", nnz, ", ", heads, "] on ",
              a.device(), ", got ", out.scalar_type(), " ", out.sizes());
  const float* rs = nullptr;
  if (row_scale.has_value() && row_scale->defined()) {
    TORCH_CHECK(row_scale->is_cuda() && row_scale->device() == a.device() &&
                    row_scale->scalar_type() == at::kFloat && row_scale->dim() == 1 &&
                    row_scale->numel() == nrows && row_scale->is_contiguous(),
                "edge_dot: row_scale must be contiguous float32 [", nrows, "] on ", a.device());
    if (nrows > 0) rs = row_scale->data_ptr<float>();
  }
  if (nnz == 0 || nrows <= 0 || F == 0) return;
  TORCH_CHECK(b.size(0) > 0, "edge_dot: entries but no rows of b");
  DG_HIP_CHECK(sddmm_csr(dt, it, rowptr.data_ptr<int64_t>(), col.data_ptr(), nrows, nnz,
                         a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0),
                         static_cast<int>(F), static_cast<int>(heads),
                         static_cast<float>(scale), rs, out.data_ptr<float>(),
                         c10::hip::getCurrentHIPStream(a.device().index()).stream()));
}

bool edge_dot_vec_path_op(int64_t F, int64_t heads) {
  return sddmm_vec_shape_ok(static_cast<int>(F), static_cast<int>(heads));
}
int64_t edge_dot_grid_cap_op() { return sddmm_grid_cap(); }
int64_t edge_dot_chunk_slots_op(int64_t F, int64_t heads) {
  return sddmm_chunk_slots(static_cast<int>(F), static_cast<int>(heads));
}

}  // namespace
}  // namespace dgraph

TORCH_LIBRARY_FRAGMENT(dgraph_amd, m) {
  m.def("edge_dot(Tensor rowptr, Tensor col, Tensor a, Tensor b, Tensor(a!) out, int heads, "
        "float scale, Tensor? row_scale) -> ()");
  m.def("edge_dot_vec_path(int F, int heads) -> bool", &dgraph::edge_dot_vec_path_op);
  m.def("edge_dot_grid_cap() -> int", &dgraph::edge_dot_grid_cap_op);
  m.def("edge_dot_chunk_slots(int F, int heads) -> int", &dgraph::edge_dot_chunk_slots_op);
}

TORCH_LIBRARY_IMPL(dgraph_amd, CUDA, m) { m.impl("edge_dot", &dgraph::edge_dot_op); }
