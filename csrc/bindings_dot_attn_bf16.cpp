// dgraph_amd — dispatcher registration of the dot-product attention kernels with bf16 storage
// (csrc/kernels/dot_attn_bf16.hip; ops/dot_attn.py). Every dtype, shape, stride, 16-B
// alignment and the device the kernels rely on is checked here, before any launch; column
// ids are checked against the operand rows once per pattern by the Python caller
// (ops/gat.py: GatPattern).
//
// Empty sides are legal and never reach a kernel. An array of a side only has to hold that
// side's rows, so 0 rows pass every check of a side with no rows: a rank with no destination
// rows returns; one whose part of the pattern has no entries (no source rows at all, or rows
// that nothing points at) writes the empty-row result (zeros) with plain fills. A second
// source with 0 rows is treated as absent, and with 0 first-source rows (nsplit = 0) every
// column, the padding slots' column 0 included, reads the second source — so row 0 of
// whatever a launched kernel gathers from always exists.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include "attn_check.h"
#include "check.h"
#include "kernels/kernels.h"

namespace dgraph {
namespace {

constexpr const char* kOp = "dot_attn_bf16";  // the prefix of every message

uint16_t* bf16_out(at::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

// contiguous [>= min_rows, heads] float32
void heads_f32(const at::Tensor& t, const at::Tensor& ref, int64_t min_rows, int64_t heads,
               const char* name) {
  per_head(kOp, t, ref, min_rows, heads, heads, name);
}

// the pattern (int32 columns only: GatPattern builds nothing else), the width and the scalars
// every kernel takes; `ref` is the op's first feature operand
DotAttnBf16Args common(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& ref,
                       int64_t heads, double scale) {
  TORCH_CHECK(ref.is_cuda() && ref.dim() == 2, "dot_attn_bf16: q must be a 2-D device tensor");
  const int C = static_cast<int>(ref.size(1));
  TORCH_CHECK(heads > 0 && dot_attn_bf16_shape_ok(C, static_cast<int>(heads)),
              "dot_attn_bf16: unsupported width ", C, " / heads ", heads,
              " (C in 64/128/256, heads in 1/2/4/8)");
  pattern(kOp, rowptr, col, ref, /*col_1d=*/true);
  TORCH_CHECK(col.scalar_type() == at::kInt,
              "dot_attn_bf16: col must be int32 (GatPattern's index type), got ",
              col.scalar_type());
  DotAttnBf16Args a{};
  a.rowptr = rowptr.data_ptr<int64_t>();
  a.col = col.data_ptr<int32_t>();
  a.nrows = rowptr.numel() - 1;
  a.C = C;
  a.scale = static_cast<float>(scale);
  return a;
}

// fwd / bwd_dst: q rows = CSR rows; k, v (+ k2, v2 past nsplit) = the gathered rows. Returns
// the number of source rows the kernel could gather from.
int64_t dst_side(DotAttnBf16Args& a, const at::Tensor& q, const at::Tensor& k,
                 const at::Tensor& v, const c10::optional<at::Tensor>& k2,
                 const c10::optional<at::Tensor>& v2, int64_t nsplit) {
  const int C = a.C;
  rows_bf16(kOp, q, q, a.nrows, C, "q");
  rows_bf16(kOp, k, q, 0, C, "k");
  rows_bf16(kOp, v, q, k.size(0), C, "v");
  const at::Tensor* p2 = opt_t(k2);
  const at::Tensor* w2 = opt_t(v2);
  TORCH_CHECK((p2 == nullptr) == (w2 == nullptr), "dot_attn_bf16: k2 and v2 come together");
  TORCH_CHECK(nsplit >= 0 && nsplit < (int64_t(1) << 31), "dot_attn_bf16: bad nsplit");
  a.q = bf16_ptr(q);
  a.ldq = q.stride(0);
  a.k = bf16_ptr(k);
  a.ldk = k.stride(0);
  a.v = bf16_ptr(v);
  a.ldv = v.stride(0);
  int64_t rows = k.size(0);
  if (p2) {
    rows_bf16(kOp, *p2, q, 0, C, "k2");
    rows_bf16(kOp, *w2, q, p2->size(0), C, "v2");
    TORCH_CHECK(k.size(0) >= nsplit, "dot_attn_bf16: k has fewer rows than nsplit");
    if (p2->size(0) > 0) {
      a.k2 = bf16_ptr(*p2);
      a.ldk2 = p2->stride(0);
      a.v2 = bf16_ptr(*w2);
      a.ldv2 = w2->stride(0);
      a.nsplit = nsplit;
      rows += p2->size(0);
    }
  }
  return rows;
}

void dot_attn_fwd_bf16_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& q,
                          const at::Tensor& k, const at::Tensor& v,
                          const c10::optional<at::Tensor>& k2,
                          const c10::optional<at::Tensor>& v2, int64_t nsplit, at::Tensor& out,
                          at::Tensor& stat_m, at::Tensor& stat_l, int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  DotAttnBf16Args a = common(rowptr, col, q, heads, scale);
  const int64_t R = a.nrows;
  const int64_t src = dst_side(a, q, k, v, k2, v2, nsplit);
  rows_bf16(kOp, out, q, R, a.C, "out");
  heads_f32(stat_m, q, R, heads, "stat_m");
  heads_f32(stat_l, q, R, heads, "stat_l");
  if (R == 0) return;
  TORCH_CHECK(src > 0 || col.numel() == 0, "dot_attn_bf16: entries but no source rows");
  if (col.numel() == 0) {  // every row is empty
    out.narrow(0, 0, R).zero_();
    stat_l.narrow(0, 0, R).zero_();
    return;
  }
  a.out = bf16_out(out);
  a.ldo = out.stride(0);
  a.stat_m = stat_m.data_ptr<float>();
  a.stat_l = stat_l.data_ptr<float>();
  DG_HIP_CHECK(dot_attn_fwd_bf16(a, static_cast<int>(heads), cur_stream(q)));
}

// writes c (what the source side reads) and dq
void dot_attn_bwd_dst_bf16_op(const at::Tensor& rowptr, const at::Tensor& col,
                              const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                              const c10::optional<at::Tensor>& k2,
                              const c10::optional<at::Tensor>& v2, int64_t nsplit,
                              const at::Tensor& stat_m, const at::Tensor& stat_l,
                              const at::Tensor& g, at::Tensor& c, at::Tensor& dq,
                              int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  DotAttnBf16Args a = common(rowptr, col, q, heads, scale);
  const int64_t R = a.nrows;
  const int64_t src = dst_side(a, q, k, v, k2, v2, nsplit);
  heads_f32(stat_m, q, R, heads, "stat_m");
  heads_f32(stat_l, q, R, heads, "stat_l");
  rows_bf16(kOp, g, q, R, a.C, "g");
  heads_f32(c, q, R, heads, "c");
  rows_bf16(kOp, dq, q, R, a.C, "dq");
  if (R == 0) return;
  TORCH_CHECK(src > 0 || col.numel() == 0, "dot_attn_bf16: entries but no source rows");
  if (col.numel() == 0) {
    c.narrow(0, 0, R).zero_();
    dq.narrow(0, 0, R).zero_();
    return;
  }
  a.stat_m = const_cast<float*>(stat_m.data_ptr<float>());
  a.stat_l = const_cast<float*>(stat_l.data_ptr<float>());
  a.g = bf16_ptr(g);
  a.ldg = g.stride(0);
  a.c = c.data_ptr<float>();
  a.dq = bf16_out(dq);
  a.lddq = dq.stride(0);
  DG_HIP_CHECK(dot_attn_bwd_dst_bf16(a, static_cast<int>(heads), cur_stream(q)));
}

// rows = source rows (the transposed pattern, or a slice of its row pointer; k, v, dk, dv);
// col = destination rows (q, g and the per-head arrays)
void dot_attn_bwd_src_bf16_op(const at::Tensor& rowptr, const at::Tensor& col,
                              const at::Tensor& q, const at::Tensor& g, const at::Tensor& k,
                              const at::Tensor& v, const at::Tensor& stat_m,
                              const at::Tensor& stat_l, const at::Tensor& c, at::Tensor& dk,
                              at::Tensor& dv, int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  DotAttnBf16Args a = common(rowptr, col, q, heads, scale);
  const int64_t R = a.nrows, nd = q.size(0);
  rows_bf16(kOp, q, q, 0, a.C, "q");
  rows_bf16(kOp, g, q, nd, a.C, "g");
  heads_f32(stat_m, q, nd, heads, "stat_m");
  heads_f32(stat_l, q, nd, heads, "stat_l");
  heads_f32(c, q, nd, heads, "c");
  rows_bf16(kOp, k, q, R, a.C, "k");
  rows_bf16(kOp, v, q, R, a.C, "v");
  rows_bf16(kOp, dk, q, R, a.C, "dk");
  rows_bf16(kOp, dv, q, R, a.C, "dv");
  if (R == 0) return;
  TORCH_CHECK(nd > 0 || col.numel() == 0, "dot_attn_bf16: entries but no destination rows");
  if (col.numel() == 0) {  // no entries: every source row's gradient is 0
    dk.narrow(0, 0, R).zero_();
    dv.narrow(0, 0, R).zero_();
    return;
  }
  a.q = bf16_ptr(q);
  a.ldq = q.stride(0);
  a.g = bf16_ptr(g);
  a.ldg = g.stride(0);
  a.k = bf16_ptr(k);
  a.ldk = k.stride(0);
  a.v = bf16_ptr(v);
  a.ldv = v.stride(0);
  a.stat_m = const_cast<float*>(stat_m.data_ptr<float>());
  a.stat_l = const_cast<float*>(stat_l.data_ptr<float>());
  a.c = const_cast<float*>(c.data_ptr<float>());
  a.dk = bf16_out(dk);
  a.lddk = dk.stride(0);
  a.dv = bf16_out(dv);
  a.lddv = dv.stride(0);
  DG_HIP_CHECK(dot_attn_bwd_src_bf16(a, static_cast<int>(heads), cur_stream(q)));
}

}  // namespace
}  // namespace dgraph

TORCH_LIBRARY_FRAGMENT(dgraph_amd, m) {
  m.def("dot_attn_fwd_bf16(Tensor rowptr, Tensor col, Tensor q, Tensor k, Tensor v, "
        "Tensor? k2, Tensor? v2, int nsplit, Tensor(a!) out, Tensor(b!) stat_m, "
        "Tensor(c!) stat_l, int heads, float scale) -> ()");
  m.def("dot_attn_bwd_dst_bf16(Tensor rowptr, Tensor col, Tensor q, Tensor k, Tensor v, "
        "Tensor? k2, Tensor? v2, int nsplit, Tensor stat_m, Tensor stat_l, Tensor g, "
        "Tensor(a!) c, Tensor(b!) dq, int heads, float scale) -> ()");
  m.def("dot_attn_bwd_src_bf16(Tensor rowptr, Tensor col, Tensor q, Tensor g, Tensor k, "
        "Tensor v, Tensor stat_m, Tensor stat_l, Tensor c, Tensor(a!) dk, Tensor(b!) dv, "
        "int heads, float scale) -> ()");
}

TORCH_LIBRARY_IMPL(dgraph_amd, CUDA, m) {
  m.impl("dot_attn_fwd_bf16", &dgraph::dot_attn_fwd_bf16_op);
  m.impl("dot_attn_bwd_dst_bf16", &dgraph::dot_attn_bwd_dst_bf16_op);
  m.impl("dot_attn_bwd_src_bf16", &dgraph::dot_attn_bwd_src_bf16_op);
}
