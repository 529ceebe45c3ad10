// dgraph_amd — argument checkers shared by the bindings of the fused fp32 attention kernels
// (bindings_gat.cpp, bindings_gatv2.cpp, bindings_dot_attn.cpp). `op` is the op family's
// name, the prefix of every message ("gatv2", "dot_attn_edge", ...).
#pragma once

#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include "kernels/kernels.h"

namespace dgraph {

inline hipStream_t cur_stream(const at::Tensor& t) {
  return c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

inline const at::Tensor* opt_t(const c10::optional<at::Tensor>& t) {
  return (t.has_value() && t->defined()) ? &*t : nullptr;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// a feature array: [>= min_rows, C] float32, unit column stride, 16-B aligned rows
inline void rows_f32(const char* op, const at::Tensor& t, const at::Tensor& ref,
                     int64_t min_rows, int64_t cols, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), op, ": ", name, " must be on ",
              ref.device());
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.dim() == 2 && t.size(1) == cols &&
                  t.size(0) >= min_rows,
              op, ": ", name, " must be float32 [>= ", min_rows, ", ", cols, "], got ",
              t.sizes());
  if (t.size(0) == 0) return;
  TORCH_CHECK(t.stride(1) == 1 && t.stride(0) % 4 == 0 && t.stride(0) >= cols &&
                  al16(t.data_ptr()),
              op, ": ", name, " must have unit column stride, a row stride divisible by 4 "
              "and 16-B alignment, got strides ", t.strides());
}

// per-head arrays: [>= min_rows, heads] with unit column stride and the shared row stride
inline void per_head(const char* op, const at::Tensor& t, const at::Tensor& ref,
                     int64_t min_rows, int64_t heads, int64_t lds, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device() && t.scalar_type() == at::kFloat &&
                  t.dim() == 2 && t.size(1) == heads && t.size(0) >= min_rows,
              op, ": ", name, " must be float32 [>= ", min_rows, ", ", heads, "] on ",
              ref.device(), ", got ", t.sizes());
  if (t.size(0) == 0) return;
  TORCH_CHECK((heads == 1 || t.stride(1) == 1) && t.stride(0) == lds && lds >= heads,
              op, ": ", name, " must have unit column stride and row stride ", lds,
              ", got strides ", t.strides());
}

// a CSR pattern on ref's device; col_1d: col must also be 1-D (the ops whose per-entry
// operands are indexed by col's positions)
inline IType pattern(const char* op, const at::Tensor& rowptr, const at::Tensor& col,
                     const at::Tensor& ref, bool col_1d = false) {
  TORCH_CHECK(rowptr.is_cuda() && rowptr.device() == ref.device() &&
                  rowptr.scalar_type() == at::kLong && rowptr.is_contiguous() &&
                  rowptr.dim() == 1 && rowptr.numel() >= 1,
              op, ": rowptr must be contiguous int64 on ", ref.device());
  TORCH_CHECK(col.is_cuda() && col.device() == ref.device() && col.is_contiguous() &&
                  (!col_1d || col.dim() == 1) &&
                  (col.scalar_type() == at::kInt || col.scalar_type() == at::kLong),
              op, ": col must be contiguous int32/int64 on ", ref.device());
  return col.scalar_type() == at::kInt ? IType::I32 : IType::I64;
}

}  // namespace dgraph
