// dgraph_amd — dispatcher registration of the fused fp32 dot-product attention kernels
// (csrc/kernels/dot_attn_f32.hip; ops/dot_attn.py). Every shape, dtype, stride and alignment
// contract the kernels rely on is checked here; column ids are checked against the operand
// rows once per pattern by the Python caller (ops/gat.py: GatPattern).
//
// Empty sides are legal and never reach a kernel: a relation with no destination rows
// returns; one whose gathered side has no rows at all (the pattern then has no entries)
// writes the empty-row result (zeros) with plain fills. A second source with 0 rows is
// treated as absent, and with 0 first-source rows (nsplit = 0) every column, the padding
// slots' column 0 included, reads the second source — so row 0 of whatever a launched
// kernel gathers from always exists. The carry forward differs on the empty sides: its
// carried state is the result, so it writes nothing there.
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
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), "dot_attn: ", name, " must be on ",
              ref.device());
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.dim() == 2 && t.size(1) == cols &&
                  t.size(0) >= min_rows,
              "dot_attn: ", name, " must be float32 [>= ", min_rows, ", ", cols, "], got ",
              t.sizes());
  if (t.size(0) == 0) return;
  TORCH_CHECK(t.stride(1) == 1 && t.stride(0) % 4 == 0 && t.stride(0) >= cols &&
                  al16(t.data_ptr()),
              "dot_attn: ", name, " must have unit column stride, a row stride divisible by 4 "
              "and 16-B alignment, got strides ", t.strides());
}

// per-head arrays: [>= min_rows, heads] with unit column stride and the shared row stride
void per_head(const at::Tensor& t, const at::Tensor& ref, int64_t min_rows, int64_t heads,
              int64_t lds, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device() && t.scalar_type() == at::kFloat &&
                  t.dim() == 2 && t.size(1) == heads && t.size(0) >= min_rows,
              "dot_attn: ", name, " must be float32 [>= ", min_rows, ", ", heads, "] on ",
              ref.device(), ", got ", t.sizes());
  if (t.size(0) == 0) return;
  TORCH_CHECK((heads == 1 || t.stride(1) == 1) && t.stride(0) == lds && lds >= heads,
              "dot_attn: ", name, " must have unit column stride and row stride ", lds,
              ", got strides ", t.strides());
}

IType pattern(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& ref) {
  TORCH_CHECK(rowptr.is_cuda() && rowptr.device() == ref.device() &&
                  rowptr.scalar_type() == at::kLong && rowptr.is_contiguous() &&
                  rowptr.dim() == 1 && rowptr.numel() >= 1,
              "dot_attn: rowptr must be contiguous int64 on ", ref.device());
  TORCH_CHECK(col.is_cuda() && col.device() == ref.device() && col.is_contiguous() &&
                  (col.scalar_type() == at::kInt || col.scalar_type() == at::kLong),
              "dot_attn: col must be contiguous int32/int64 on ", ref.device());
  return col.scalar_type() == at::kInt ? IType::I32 : IType::I64;
}

int width(const at::Tensor& q, int64_t heads) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 2, "dot_attn: q must be a 2-D device tensor");
  const int C = static_cast<int>(q.size(1));
  TORCH_CHECK(heads > 0 && heads <= 8 && dot_attn_f32_shape_ok(C, static_cast<int>(heads)),
              "dot_attn: unsupported width ", C, " / heads ", heads,
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
  TORCH_CHECK((p2 == nullptr) == (w2 == nullptr), "dot_attn: k2 and v2 come together");
  TORCH_CHECK(nsplit >= 0 && nsplit < (int64_t(1) << 32), "dot_attn: bad nsplit");
  Sources s;
  s.k = k.data_ptr<float>();
  s.v = v.data_ptr<float>();
  s.ldk = k.stride(0);
  s.ldv = v.stride(0);
  s.rows = k.size(0);
  if (p2) {
    rows_f32(*p2, q, 0, C, "k2");
    rows_f32(*w2, q, p2->size(0), C, "v2");
    TORCH_CHECK(k.size(0) >= nsplit, "dot_attn: k has fewer rows than nsplit");
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

// q/out rows = CSR rows; k, v (+ k2, v2 past nsplit) = the gathered rows
void dot_attn_fwd_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& q,
                     const at::Tensor& k, const at::Tensor& v,
                     const c10::optional<at::Tensor>& k2, const c10::optional<at::Tensor>& v2,
                     int64_t nsplit, at::Tensor& out, double beta, at::Tensor& stat_m,
                     at::Tensor& stat_l, int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  const int C = width(q, heads);
  const IType it = pattern(rowptr, col, q);
  const int64_t R = rowptr.numel() - 1;
  const int64_t lds = stat_m.dim() == 2 ? stat_m.stride(0) : 0;
  rows_f32(q, q, R, C, "q");
  const Sources s = sources(q, k, v, k2, v2, nsplit, C);
  rows_f32(out, q, R, C, "out");
  per_head(stat_m, q, R, heads, lds, "stat_m");
  per_head(stat_l, q, R, heads, lds, "stat_l");
  if (R == 0) return;
  if (s.rows == 0) {  // nothing to gather from: every row is empty
    TORCH_CHECK(col.numel() == 0, "dot_attn: entries but no source rows");
    at::Tensor o = out.narrow(0, 0, R);
    if (beta == 0.0) o.zero_(); else o.mul_(beta);
    stat_l.narrow(0, 0, R).zero_();
    return;
  }
  DG_HIP_CHECK(dot_attn_fwd_f32(it, rowptr.data_ptr<int64_t>(), col.data_ptr(), R, C,
                                static_cast<int>(heads), lds, static_cast<float>(scale),
                                q.data_ptr<float>(), q.stride(0), s.k, s.ldk, s.v, s.ldv, s.k2,
                                s.ldk2, s.v2, s.ldv2, s.nsplit, out.data_ptr<float>(),
                                out.stride(0), static_cast<float>(beta),
                                stat_m.data_ptr<float>(), stat_l.data_ptr<float>(),
                                cur_stream(q)));
}

// the forward from a carried (out, stat_m, stat_l). The carried state is the result of an
// empty side: no destination rows or no source rows at all write nothing (the plain forward
// zeroes out and stat_l there).
void dot_attn_fwd_carry_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& q,
                           const at::Tensor& k, const at::Tensor& v,
                           const c10::optional<at::Tensor>& k2,
                           const c10::optional<at::Tensor>& v2, int64_t nsplit,
                           at::Tensor& out, at::Tensor& stat_m, at::Tensor& stat_l,
                           int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  const int C = width(q, heads);
  const IType it = pattern(rowptr, col, q);
  const int64_t R = rowptr.numel() - 1;
  const int64_t lds = stat_m.dim() == 2 ? stat_m.stride(0) : 0;
  rows_f32(q, q, R, C, "q");
  const Sources s = sources(q, k, v, k2, v2, nsplit, C);
  rows_f32(out, q, R, C, "out");
  per_head(stat_m, q, R, heads, lds, "stat_m");
  per_head(stat_l, q, R, heads, lds, "stat_l");
  if (R == 0) return;
  if (s.rows == 0) {
    TORCH_CHECK(col.numel() == 0, "dot_attn: entries but no source rows");
    return;
  }
  DG_HIP_CHECK(dot_attn_fwd_carry_f32(it, rowptr.data_ptr<int64_t>(), col.data_ptr(), R, C,
                                      static_cast<int>(heads), lds, static_cast<float>(scale),
                                      q.data_ptr<float>(), q.stride(0), s.k, s.ldk, s.v, s.ldv,
                                      s.k2, s.ldk2, s.v2, s.ldv2, s.nsplit,
                                      out.data_ptr<float>(), out.stride(0),
                                      stat_m.data_ptr<float>(), stat_l.data_ptr<float>(),
                                      cur_stream(q)));
}

void dot_attn_bwd_dst_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& q,
                         const at::Tensor& k, const at::Tensor& v,
                         const c10::optional<at::Tensor>& k2,
                         const c10::optional<at::Tensor>& v2, int64_t nsplit,
                         const at::Tensor& stat_m, const at::Tensor& stat_l,
                         const at::Tensor& g, const at::Tensor& c, at::Tensor& dq,
                         int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  const int C = width(q, heads);
  const IType it = pattern(rowptr, col, q);
  const int64_t R = rowptr.numel() - 1;
  const int64_t lds = stat_m.dim() == 2 ? stat_m.stride(0) : 0;
  rows_f32(q, q, R, C, "q");
  const Sources s = sources(q, k, v, k2, v2, nsplit, C);
  per_head(stat_m, q, R, heads, lds, "stat_m");
  per_head(stat_l, q, R, heads, lds, "stat_l");
  per_head(c, q, R, heads, lds, "c");
  rows_f32(g, q, R, C, "g");
  rows_f32(dq, q, R, C, "dq");
  if (R == 0) return;
  if (s.rows == 0) {
    TORCH_CHECK(col.numel() == 0, "dot_attn: entries but no source rows");
    dq.narrow(0, 0, R).zero_();
    return;
  }
  DG_HIP_CHECK(dot_attn_bwd_dst_f32(it, rowptr.data_ptr<int64_t>(), col.data_ptr(), R, C,
                                    static_cast<int>(heads), lds, static_cast<float>(scale),
                                    q.data_ptr<float>(), q.stride(0), s.k, s.ldk, s.v, s.ldv,
                                    s.k2, s.ldk2, s.v2, s.ldv2, s.nsplit,
                                    stat_m.data_ptr<float>(), stat_l.data_ptr<float>(),
                                    g.data_ptr<float>(), g.stride(0), c.data_ptr<float>(),
                                    dq.data_ptr<float>(), dq.stride(0), cur_stream(q)));
}

// rows = source rows (the transposed pattern; k, v, dk, dv); col = destination rows
void dot_attn_bwd_src_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& q,
                         const at::Tensor& g, const at::Tensor& k, const at::Tensor& v,
                         const at::Tensor& stat_m, const at::Tensor& stat_l,
                         const at::Tensor& c, at::Tensor& dk, at::Tensor& dv, int64_t heads,
                         double scale) {
  const c10::DeviceGuard guard(q.device());
  const int C = width(q, heads);
  const IType it = pattern(rowptr, col, q);
  const int64_t R = rowptr.numel() - 1;
  const int64_t nd = q.size(0);
  const int64_t lds = stat_m.dim() == 2 ? stat_m.stride(0) : 0;
  rows_f32(q, q, 0, C, "q");
  rows_f32(g, q, nd, C, "g");
  per_head(stat_m, q, nd, heads, lds, "stat_m");
  per_head(stat_l, q, nd, heads, lds, "stat_l");
  per_head(c, q, nd, heads, lds, "c");
  rows_f32(k, q, R, C, "k");
  rows_f32(v, q, R, C, "v");
  rows_f32(dk, q, R, C, "dk");
  rows_f32(dv, q, R, C, "dv");
  if (R == 0) return;
  if (nd == 0) {  // no destination rows: no entries, every source row's gradient is 0
    TORCH_CHECK(col.numel() == 0, "dot_attn: entries but no destination rows");
    dk.narrow(0, 0, R).zero_();
    dv.narrow(0, 0, R).zero_();
    return;
  }
  DG_HIP_CHECK(dot_attn_bwd_src_f32(it, rowptr.data_ptr<int64_t>(), col.data_ptr(), R, C,
                                    static_cast<int>(heads), lds, static_cast<float>(scale),
                                    q.data_ptr<float>(), q.stride(0), g.data_ptr<float>(),
                                    g.stride(0), k.data_ptr<float>(), k.stride(0),
                                    v.data_ptr<float>(), v.stride(0), stat_m.data_ptr<float>(),
                                    stat_l.data_ptr<float>(), c.data_ptr<float>(),
                                    dk.data_ptr<float>(), dk.stride(0), dv.data_ptr<float>(),
                                    dv.stride(0), cur_stream(q)));
}

}  // namespace
}  // namespace dgraph

TORCH_LIBRARY_FRAGMENT(dgraph_amd, m) {
  m.def("dot_attn_fwd_f32(Tensor rowptr, Tensor col, Tensor q, Tensor k, Tensor v, "
        "Tensor? k2, Tensor? v2, int nsplit, Tensor(a!) out, float beta, Tensor(b!) stat_m, "
        "Tensor(c!) stat_l, int heads, float scale) -> ()");
  m.def("dot_attn_fwd_carry_f32(Tensor rowptr, Tensor col, Tensor q, Tensor k, Tensor v, "
        "Tensor? k2, Tensor? v2, int nsplit, Tensor(a!) out, Tensor(b!) stat_m, "
        "Tensor(c!) stat_l, int heads, float scale) -> ()");
  m.def("dot_attn_bwd_dst_f32(Tensor rowptr, Tensor col, Tensor q, Tensor k, Tensor v, "
        "Tensor? k2, Tensor? v2, int nsplit, Tensor stat_m, Tensor stat_l, Tensor g, "
        "Tensor c, Tensor(a!) dq, int heads, float scale) -> ()");
  m.def("dot_attn_bwd_src_f32(Tensor rowptr, Tensor col, Tensor q, Tensor g, Tensor k, "
        "Tensor v, Tensor stat_m, Tensor stat_l, Tensor c, Tensor(a!) dk, Tensor(b!) dv, "
        "int heads, float scale) -> ()");
}

TORCH_LIBRARY_IMPL(dgraph_amd, CUDA, m) {
  m.impl("dot_attn_fwd_f32", &dgraph::dot_attn_fwd_op);
  m.impl("dot_attn_fwd_carry_f32", &dgraph::dot_attn_fwd_carry_op);
  m.impl("dot_attn_bwd_dst_f32", &dgraph::dot_attn_bwd_dst_op);
  m.impl("dot_attn_bwd_src_f32", &dgraph::dot_attn_bwd_src_op);
}
