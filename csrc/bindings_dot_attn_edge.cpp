// dgraph_amd — dispatcher registration of the fused fp32 dot-product attention kernels with
// edge features (csrc/kernels/dot_attn_edge_f32.hip; ops/dot_attn.py). Every shape, dtype,
// stride and alignment contract the kernels rely on is checked here, before any launch;
// column ids and transposed slots are built once per pattern by the Python caller
// (ops/gat.py: GatPattern).
//
// Empty sides are legal and never reach a kernel, as in bindings_dot_attn.cpp. In addition a
// pattern with no entries (col.numel() == 0, so ee / dee / w have no rows) never launches:
// the empty-row results (zeros) are written with plain fills.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include "check.h"
#include "kernels/kernels.h"

namespace dgraph {
namespace {

hipStream_t cur_stream(const at::Tensor& t) {
  return c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

const at::Tensor* opt_t(const c10::optional<at::Tensor>& t) {
  return (t.has_value() && t->defined()) ? &*t : nullptr;
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// a feature array: [>= min_rows, C] float32, unit column stride, 16-B aligned rows
void rows_f32(const at::Tensor& t, const at::Tensor& ref, int64_t min_rows, int64_t cols,
              const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), "dot_attn_edge: ", name,
              " must be on ", ref.device());
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.dim() == 2 && t.size(1) == cols &&
                  t.size(0) >= min_rows,
              "dot_attn_edge: ", name, " must be float32 [>= ", min_rows, ", ", cols,
              "], got ", t.sizes());
  if (t.size(0) == 0) return;
  TORCH_CHECK(t.stride(1) == 1 && t.stride(0) % 4 == 0 && t.stride(0) >= cols &&
                  al16(t.data_ptr()),
              "dot_attn_edge: ", name, " must have unit column stride, a row stride divisible "
              "by 4 and 16-B alignment, got strides ", t.strides());
}

// a per-edge feature array (ee, dee): exactly one row per entry of the pattern
void edge_rows_f32(const at::Tensor& t, const at::Tensor& ref, int64_t nnz, int64_t cols,
                   const char* name) {
  rows_f32(t, ref, nnz, cols, name);
  TORCH_CHECK(t.size(0) == nnz, "dot_attn_edge: ", name, " must have one row per entry (",
              nnz, "), got ", t.sizes());
}

// per-head arrays: [>= min_rows, heads] with unit column stride and the shared row stride
void per_head(const at::Tensor& t, const at::Tensor& ref, int64_t min_rows, int64_t heads,
              int64_t lds, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device() && t.scalar_type() == at::kFloat &&
                  t.dim() == 2 && t.size(1) == heads && t.size(0) >= min_rows,
              "dot_attn_edge: ", name, " must be float32 [>= ", min_rows, ", ", heads, "] on ",
              ref.device(), ", got ", t.sizes());
  if (t.size(0) == 0) return;
  TORCH_CHECK((heads == 1 || t.stride(1) == 1) && t.stride(0) == lds && lds >= heads,
              "dot_attn_edge: ", name, " must have unit column stride and row stride ", lds,
              ", got strides ", t.strides());
}

// the per-slot weights: [nnz, 2 heads] float32 with unit column stride
void weights(const at::Tensor& w, const at::Tensor& ref, int64_t nnz, int64_t heads) {
  TORCH_CHECK(w.is_cuda() && w.device() == ref.device() && w.scalar_type() == at::kFloat &&
                  w.dim() == 2 && w.size(1) == 2 * heads && w.size(0) == nnz,
              "dot_attn_edge: w must be float32 [", nnz, ", ", 2 * heads, "] on ",
              ref.device(), ", got ", w.sizes());
  if (nnz == 0) return;
  TORCH_CHECK(w.stride(1) == 1 && w.stride(0) >= 2 * heads,
              "dot_attn_edge: w must have unit column stride, got strides ", w.strides());
}

IType pattern(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& ref) {
  TORCH_CHECK(rowptr.is_cuda() && rowptr.device() == ref.device() &&
                  rowptr.scalar_type() == at::kLong && rowptr.is_contiguous() &&
                  rowptr.dim() == 1 && rowptr.numel() >= 1,
              "dot_attn_edge: rowptr must be contiguous int64 on ", ref.device());
  TORCH_CHECK(col.is_cuda() && col.device() == ref.device() && col.is_contiguous() &&
                  col.dim() == 1 &&
                  (col.scalar_type() == at::kInt || col.scalar_type() == at::kLong),
              "dot_attn_edge: col must be contiguous int32/int64 on ", ref.device());
  return col.scalar_type() == at::kInt ? IType::I32 : IType::I64;
}

int width(const at::Tensor& q, int64_t heads) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 2, "dot_attn_edge: q must be a 2-D device tensor");
  const int C = static_cast<int>(q.size(1));
  TORCH_CHECK(heads > 0 && heads <= 8 && dot_attn_f32_shape_ok(C, static_cast<int>(heads)),
              "dot_attn_edge: unsupported width ", C, " / heads ", heads,
              " (C in 64/128/256, heads in 1/2/4/8, >= 2 lanes of 4 channels per head)");
  return C;
}

// the two gathered sources of fwd / bwd_dst, as the kernels take them
struct Sources {
  const float *k, *v, *k2 = nullptr, *v2 = nullptr;
  int64_t ldk, ldv, ldk2 = 0, ldv2 = 0, nsplit = 0, rows = 0;
};

Sources sources(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                const c10::optional<at::Tensor>& k2, const c10::optional<at::Tensor>& v2,
                int64_t nsplit, int C) {
  rows_f32(k, q, 0, C, "k");
  rows_f32(v, q, k.size(0), C, "v");
  const at::Tensor* p2 = opt_t(k2);
  const at::Tensor* w2 = opt_t(v2);
  TORCH_CHECK((p2 == nullptr) == (w2 == nullptr), "dot_attn_edge: k2 and v2 come together");
  TORCH_CHECK(nsplit >= 0 && nsplit < (int64_t(1) << 32), "dot_attn_edge: bad nsplit");
  Sources s;
  s.k = k.data_ptr<float>();
  s.v = v.data_ptr<float>();
  s.ldk = k.stride(0);
  s.ldv = v.stride(0);
  s.rows = k.size(0);
  if (p2) {
    rows_f32(*p2, q, 0, C, "k2");
    rows_f32(*w2, q, p2->size(0), C, "v2");
    TORCH_CHECK(k.size(0) >= nsplit, "dot_attn_edge: k has fewer rows than nsplit");
    if (p2->size(0) > 0) {
      s.k2 = p2->data_ptr<float>();
      s.v2 = w2->data_ptr<float>();
      s.ldk2 = p2->stride(0);
      s.ldv2 = w2->stride(0);
      s.nsplit = nsplit;
      s.rows += p2->size(0);
    }
  }
  return s;
}

// q/out rows = CSR rows; k, v (+ k2, v2 past nsplit) = the gathered rows; ee rows = slots
void dot_attn_edge_fwd_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& q,
                          const at::Tensor& k, const at::Tensor& v,
                          const c10::optional<at::Tensor>& k2,
                          const c10::optional<at::Tensor>& v2, int64_t nsplit,
                          const at::Tensor& ee, at::Tensor& out, double beta,
                          at::Tensor& stat_m, at::Tensor& stat_l, int64_t heads,
                          double scale) {
  const c10::DeviceGuard guard(q.device());
  const int C = width(q, heads);
  const IType it = pattern(rowptr, col, q);
  const int64_t R = rowptr.numel() - 1;
  const int64_t nnz = col.numel();
  const int64_t lds = stat_m.dim() == 2 ? stat_m.stride(0) : 0;
  rows_f32(q, q, R, C, "q");
  const Sources s = sources(q, k, v, k2, v2, nsplit, C);
  edge_rows_f32(ee, q, nnz, C, "ee");
  rows_f32(out, q, R, C, "out");
  per_head(stat_m, q, R, heads, lds, "stat_m");
  per_head(stat_l, q, R, heads, lds, "stat_l");
  if (R == 0) return;
  TORCH_CHECK(s.rows > 0 || nnz == 0, "dot_attn_edge: entries but no source rows");
  if (nnz == 0) {  // every row is empty
    at::Tensor o = out.narrow(0, 0, R);
    if (beta == 0.0) o.zero_(); else o.mul_(beta);
    stat_l.narrow(0, 0, R).zero_();
    return;
  }
  DG_HIP_CHECK(dot_attn_edge_fwd_f32(
      it, rowptr.data_ptr<int64_t>(), col.data_ptr(), R, C, static_cast<int>(heads), lds,
      static_cast<float>(scale), q.data_ptr<float>(), q.stride(0), s.k, s.ldk, s.v, s.ldv,
      s.k2, s.ldk2, s.v2, s.ldv2, s.nsplit, ee.data_ptr<float>(), ee.stride(0),
      out.data_ptr<float>(), out.stride(0), static_cast<float>(beta),
      stat_m.data_ptr<float>(), stat_l.data_ptr<float>(), cur_stream(q)));
}

void dot_attn_edge_bwd_dst_op(const at::Tensor& rowptr, const at::Tensor& col,
                              const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                              const c10::optional<at::Tensor>& k2,
                              const c10::optional<at::Tensor>& v2, int64_t nsplit,
                              const at::Tensor& ee, const at::Tensor& stat_m,
                              const at::Tensor& stat_l, const at::Tensor& g,
                              const at::Tensor& c, at::Tensor& dq, at::Tensor& dee,
                              at::Tensor& w, int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  const int C = width(q, heads);
  const IType it = pattern(rowptr, col, q);
  const int64_t R = rowptr.numel() - 1;
  const int64_t nnz = col.numel();
  const int64_t lds = stat_m.dim() == 2 ? stat_m.stride(0) : 0;
  rows_f32(q, q, R, C, "q");
  const Sources s = sources(q, k, v, k2, v2, nsplit, C);
  edge_rows_f32(ee, q, nnz, C, "ee");
  per_head(stat_m, q, R, heads, lds, "stat_m");
  per_head(stat_l, q, R, heads, lds, "stat_l");
  per_head(c, q, R, heads, lds, "c");
  rows_f32(g, q, R, C, "g");
  rows_f32(dq, q, R, C, "dq");
  edge_rows_f32(dee, q, nnz, C, "dee");
  weights(w, q, nnz, heads);
  if (R == 0) return;
  TORCH_CHECK(s.rows > 0 || nnz == 0, "dot_attn_edge: entries but no source rows");
  if (nnz == 0) {
    dq.narrow(0, 0, R).zero_();
    return;
  }
  DG_HIP_CHECK(dot_attn_edge_bwd_dst_f32(
      it, rowptr.data_ptr<int64_t>(), col.data_ptr(), R, C, static_cast<int>(heads), lds,
      static_cast<float>(scale), q.data_ptr<float>(), q.stride(0), s.k, s.ldk, s.v, s.ldv,
      s.k2, s.ldk2, s.v2, s.ldv2, s.nsplit, ee.data_ptr<float>(), ee.stride(0),
      stat_m.data_ptr<float>(), stat_l.data_ptr<float>(), g.data_ptr<float>(), g.stride(0),
      c.data_ptr<float>(), dq.data_ptr<float>(), dq.stride(0), dee.data_ptr<float>(),
      dee.stride(0), w.data_ptr<float>(), w.stride(0), cur_stream(q)));
}

// rows = source rows (the transposed pattern; dk, dv); col = destination rows; t_slot = the
// forward slot (row of w) of each transposed entry
void dot_attn_edge_bwd_src_op(const at::Tensor& rowptr, const at::Tensor& col,
                              const at::Tensor& t_slot, const at::Tensor& q,
                              const at::Tensor& g, const at::Tensor& w, at::Tensor& dk,
                              at::Tensor& dv, int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  const int C = width(q, heads);
  const IType it = pattern(rowptr, col, q);
  const int64_t R = rowptr.numel() - 1;
  const int64_t nd = q.size(0);
  const int64_t nnz = col.numel();
  TORCH_CHECK(t_slot.is_cuda() && t_slot.device() == q.device() && t_slot.is_contiguous() &&
                  t_slot.dim() == 1 && t_slot.scalar_type() == col.scalar_type() &&
                  t_slot.numel() == nnz,
              "dot_attn_edge: t_slot must be contiguous, of col's dtype and length (", nnz,
              ") on ", q.device());
  rows_f32(q, q, 0, C, "q");
  rows_f32(g, q, nd, C, "g");
  weights(w, q, nnz, heads);
  rows_f32(dk, q, R, C, "dk");
  rows_f32(dv, q, R, C, "dv");
  if (R == 0) return;
  TORCH_CHECK(nd > 0 || nnz == 0, "dot_attn_edge: entries but no destination rows");
  if (nnz == 0) {  // no entries: every source row's gradient is 0
    dk.narrow(0, 0, R).zero_();
    dv.narrow(0, 0, R).zero_();
    return;
  }
  DG_HIP_CHECK(dot_attn_edge_bwd_src_f32(
      it, rowptr.data_ptr<int64_t>(), col.data_ptr(), t_slot.data_ptr(), R, C,
      static_cast<int>(heads), static_cast<float>(scale), q.data_ptr<float>(), q.stride(0),
      g.data_ptr<float>(), g.stride(0), w.data_ptr<float>(), w.stride(0),
      dk.data_ptr<float>(), dk.stride(0), dv.data_ptr<float>(), dv.stride(0), cur_stream(q)));
}

}  // namespace
}  // namespace dgraph

TORCH_LIBRARY_FRAGMENT(dgraph_amd, m) {
  m.def("dot_attn_edge_fwd_f32(Tensor rowptr, Tensor col, Tensor q, Tensor k, Tensor v, "
        "Tensor? k2, Tensor? v2, int nsplit, Tensor ee, Tensor(a!) out, float beta, "
        "Tensor(b!) stat_m, Tensor(c!) stat_l, int heads, float scale) -> ()");
  m.def("dot_attn_edge_bwd_dst_f32(Tensor rowptr, Tensor col, Tensor q, Tensor k, Tensor v, "
        "Tensor? k2, Tensor? v2, int nsplit, Tensor ee, Tensor stat_m, Tensor stat_l, "
        "Tensor g, Tensor c, Tensor(a!) dq, Tensor(b!) dee, Tensor(c!) w, int heads, "
        "float scale) -> ()");
  m.def("dot_attn_edge_bwd_src_f32(Tensor rowptr, Tensor col, Tensor t_slot, Tensor q, "
        "Tensor g, Tensor w, Tensor(a!) dk, Tensor(b!) dv, int heads, float scale) -> ()");
}

TORCH_LIBRARY_IMPL(dgraph_amd, CUDA, m) {
  m.impl("dot_attn_edge_fwd_f32", &dgraph::dot_attn_edge_fwd_op);
  m.impl("dot_attn_edge_bwd_dst_f32", &dgraph::dot_attn_edge_bwd_dst_op);
  m.impl("dot_attn_edge_bwd_src_f32", &dgraph::dot_attn_edge_bwd_src_op);
}
