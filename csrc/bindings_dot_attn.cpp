// dgraph_amd — dispatcher registration of the fused fp32 dot-product attention kernels
// (csrc/kernels/dot_attn_f32.h; ops/dot_attn.py): plain and carry-in, with edge features,
// with attention dropout, and the host side of the keep-mask generator
// (csrc/kernels/philox.h). Every shape, dtype, stride and alignment contract the kernels
// rely on is checked here, before any launch; column ids and transposed slots are checked /
// built once per pattern by the Python caller (ops/gat.py: GatPattern).
//
// Empty sides are legal and never reach a kernel: a relation with no destination rows
// returns; one whose gathered side has no rows at all (the pattern then has no entries)
// writes the empty-row result (zeros) with plain fills. A second source with 0 rows is
// treated as absent, and with 0 first-source rows (nsplit = 0) every column, the padding
// slots' column 0 included, reads the second source — so row 0 of whatever a launched
// kernel gathers from always exists. The carry forward differs on the empty sides: its
// carried state is the result, so it writes nothing there. With edge features a pattern
// with no entries (col.numel() == 0, so ee / dee / w have no rows) never launches either.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include "attn_check.h"
#include "check.h"
#include "kernels/kernels.h"
#include "kernels/philox.h"

namespace dgraph {
namespace {

// the op families' names: the prefix of their error messages
constexpr const char* kPlain = "dot_attn";
constexpr const char* kEdge = "dot_attn_edge";
constexpr const char* kDrop = "dot_attn_drop";

// the family of a variant's ops (the carry forward belongs to the plain ones)
const char* family(DotVariant v) {
  return v == DotVariant::Edge ? kEdge : v == DotVariant::Drop ? kDrop : kPlain;
}

// Edge and Drop index per-entry operands (ee, w, the mask) by col's positions: col is 1-D
bool col_1d(DotVariant v) { return v == DotVariant::Edge || v == DotVariant::Drop; }

int width(const char* op, const at::Tensor& q, int64_t heads) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 2, op, ": q must be a 2-D device tensor");
  const int C = static_cast<int>(q.size(1));
  TORCH_CHECK(heads > 0 && heads <= 8 && dot_attn_f32_shape_ok(C, static_cast<int>(heads)),
              op, ": unsupported width ", C, " / heads ", heads,
              " (C in 64/128/256, heads in 1/2/4/8, >= 2 lanes of 4 channels per head)");
  return C;
}

// a per-edge feature array (ee, dee): exactly one row per entry of the pattern
void edge_rows_f32(const at::Tensor& t, const at::Tensor& ref, int64_t nnz, int64_t cols,
                   const char* name) {
  rows_f32(kEdge, t, ref, nnz, cols, name);
  TORCH_CHECK(t.size(0) == nnz, "dot_attn_edge: ", name, " must have one row per entry (",
              nnz, "), got ", t.sizes());
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

// the mask's parameters as the kernels take them
struct Drop {
  const int64_t* seed;
  uint32_t thr;
  float inv_keep;
};

Drop dropout(const at::Tensor& seed, double p, const at::Tensor& ref) {
  TORCH_CHECK(seed.is_cuda() && seed.device() == ref.device() &&
                  seed.scalar_type() == at::kLong && seed.numel() == 1,
              "dot_attn_drop: seed must be a 1-element int64 tensor on ", ref.device());
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dot_attn_drop: p must lie in [0, 1), got ", p);
  return Drop{seed.data_ptr<int64_t>(), attn_keep_threshold(p),
              1.f / (1.f - static_cast<float>(p))};
}

void set_drop(DotAttnArgs& a, const Drop& d) {
  a.seed = d.seed;
  a.thr = d.thr;
  a.inv_keep = d.inv_keep;
}

// the two gathered sources of fwd / bwd_dst, as the kernels take them
struct Sources {
  const float *k, *v, *k2 = nullptr, *v2 = nullptr;
  int64_t ldk, ldv, ldk2 = 0, ldv2 = 0, nsplit = 0, rows = 0;
};

Sources sources(const char* op, const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                const c10::optional<at::Tensor>& k2, const c10::optional<at::Tensor>& v2,
                int64_t nsplit, int C) {
  rows_f32(op, k, q, 0, C, "k");
  rows_f32(op, v, q, k.size(0), C, "v");
  const at::Tensor* p2 = opt_t(k2);
  const at::Tensor* w2 = opt_t(v2);
  TORCH_CHECK((p2 == nullptr) == (w2 == nullptr), op, ": k2 and v2 come together");
  TORCH_CHECK(nsplit >= 0 && nsplit < (int64_t(1) << 32), op, ": bad nsplit");
  Sources s;
  s.k = k.data_ptr<float>();
  s.v = v.data_ptr<float>();
  s.ldk = k.stride(0);
  s.ldv = v.stride(0);
  s.rows = k.size(0);
  if (p2) {
    rows_f32(op, *p2, q, 0, C, "k2");
    rows_f32(op, *w2, q, p2->size(0), C, "v2");
    TORCH_CHECK(k.size(0) >= nsplit, op, ": k has fewer rows than nsplit");
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

// What an op has once its pattern and its first operands are checked: the kernels'
// arguments filled that far, the index type, the kernel's rows R, the pattern's entries and
// the rows of the other side (gathered source rows; bwd_src: destination rows).
struct Call {
  DotAttnArgs a{};
  DotVariant variant;
  IType it;
  int64_t R, nnz, other;
};

// fwd / bwd_dst: q rows = CSR rows; k, v (+ k2, v2 past nsplit) = the gathered rows
Call dst_side(DotVariant variant, const at::Tensor& rowptr, const at::Tensor& col,
              const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
              const c10::optional<at::Tensor>& k2, const c10::optional<at::Tensor>& v2,
              int64_t nsplit, const at::Tensor& stat_m, int64_t heads, double scale) {
  const char* op = family(variant);
  Call c;
  c.variant = variant;
  DotAttnArgs& a = c.a;
  a.C = width(op, q, heads);
  c.it = pattern(op, rowptr, col, q, col_1d(variant));
  c.R = rowptr.numel() - 1;
  c.nnz = col.numel();
  a.lds = stat_m.dim() == 2 ? stat_m.stride(0) : 0;
  rows_f32(op, q, q, c.R, a.C, "q");
  const Sources s = sources(op, q, k, v, k2, v2, nsplit, a.C);
  c.other = s.rows;
  a.rowptr = rowptr.data_ptr<int64_t>();
  a.col = col.data_ptr();
  a.nrows = c.R;
  a.scale = static_cast<float>(scale);
  a.q = q.data_ptr<float>();
  a.ldq = q.stride(0);
  a.k = s.k;
  a.ldk = s.ldk;
  a.v = s.v;
  a.ldv = s.ldv;
  a.k2 = s.k2;
  a.ldk2 = s.ldk2;
  a.v2 = s.v2;
  a.ldv2 = s.ldv2;
  a.nsplit = s.nsplit;
  return c;
}

// bwd_src: rows = source rows (the transposed pattern; dk, dv); col = destination rows (q,
// g); t_slot = the forward slot of each transposed entry, or nullptr where none is taken;
// stat_m = the destinations' statistics, whose row stride is lds, or nullptr likewise
Call src_side(DotVariant variant, const at::Tensor& rowptr, const at::Tensor& col,
              const at::Tensor* t_slot, const at::Tensor& q, const at::Tensor& g,
              const at::Tensor* stat_m, int64_t heads, double scale) {
  const char* op = family(variant);
  Call c;
  c.variant = variant;
  DotAttnArgs& a = c.a;
  a.C = width(op, q, heads);
  c.it = pattern(op, rowptr, col, q, col_1d(variant));
  a.lds = stat_m && stat_m->dim() == 2 ? stat_m->stride(0) : 0;
  c.R = rowptr.numel() - 1;
  c.other = q.size(0);
  c.nnz = col.numel();
  if (t_slot) {
    TORCH_CHECK(t_slot->is_cuda() && t_slot->device() == q.device() &&
                    t_slot->is_contiguous() && t_slot->dim() == 1 &&
                    t_slot->scalar_type() == col.scalar_type() && t_slot->numel() == c.nnz,
                op, ": t_slot must be contiguous, of col's dtype and length (", c.nnz, ") on ",
                q.device());
  }
  rows_f32(op, q, q, 0, a.C, "q");
  rows_f32(op, g, q, c.other, a.C, "g");
  a.rowptr = rowptr.data_ptr<int64_t>();
  a.col = col.data_ptr();
  a.t_slot = t_slot ? t_slot->data_ptr() : nullptr;
  a.nrows = c.R;
  a.scale = static_cast<float>(scale);
  a.q = q.data_ptr<float>();
  a.ldq = q.stride(0);
  a.g = g.data_ptr<float>();
  a.ldg = g.stride(0);
  return c;
}

void set_out(DotAttnArgs& a, at::Tensor& out, at::Tensor& stat_m, at::Tensor& stat_l) {
  a.out = out.data_ptr<float>();
  a.ldo = out.stride(0);
  a.stat_m = stat_m.data_ptr<float>();
  a.stat_l = stat_l.data_ptr<float>();
}

// the statistics, c, g and dq of bwd_dst
void set_dst_grads(DotAttnArgs& a, const at::Tensor& stat_m, const at::Tensor& stat_l,
                   const at::Tensor& g, const at::Tensor& c, at::Tensor& dq) {
  a.stat_m = stat_m.data_ptr<float>();
  a.stat_l = stat_l.data_ptr<float>();
  a.g = g.data_ptr<float>();
  a.ldg = g.stride(0);
  a.c = c.data_ptr<float>();
  a.dq = dq.data_ptr<float>();
  a.lddq = dq.stride(0);
}

void set_src_grads(DotAttnArgs& a, at::Tensor& dk, at::Tensor& dv) {
  a.dk = dk.data_ptr<float>();
  a.lddk = dk.stride(0);
  a.dv = dv.data_ptr<float>();
  a.lddv = dv.stride(0);
}

// the resident k, v and the destinations' statistics of the recomputing bwd_src kernels
void set_src_recompute(DotAttnArgs& a, const at::Tensor& k, const at::Tensor& v,
                       const at::Tensor& stat_m, const at::Tensor& stat_l,
                       const at::Tensor& c) {
  a.k = k.data_ptr<float>();
  a.ldk = k.stride(0);
  a.v = v.data_ptr<float>();
  a.ldv = v.stride(0);
  a.stat_m = stat_m.data_ptr<float>();
  a.stat_l = stat_l.data_ptr<float>();
  a.c = c.data_ptr<float>();
}

void launch(DotKind kind, const Call& c, int64_t heads, const at::Tensor& q) {
  DG_HIP_CHECK(
      dot_attn_launch(kind, c.variant, c.it, static_cast<int>(heads), c.a, cur_stream(q)));
}

// ------------------------------------------------------------------------ plain and carry
void dot_attn_fwd_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& q,
                     const at::Tensor& k, const at::Tensor& v,
                     const c10::optional<at::Tensor>& k2, const c10::optional<at::Tensor>& v2,
                     int64_t nsplit, at::Tensor& out, double beta, at::Tensor& stat_m,
                     at::Tensor& stat_l, int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  Call c = dst_side(DotVariant::Plain, rowptr, col, q, k, v, k2, v2, nsplit, stat_m, heads,
                    scale);
  const int64_t R = c.R;
  rows_f32(kPlain, out, q, R, c.a.C, "out");
  per_head(kPlain, stat_m, q, R, heads, c.a.lds, "stat_m");
  per_head(kPlain, stat_l, q, R, heads, c.a.lds, "stat_l");
  if (R == 0) return;
  if (c.other == 0) {  // nothing to gather from: every row is empty
    TORCH_CHECK(col.numel() == 0, "dot_attn: entries but no source rows");
    at::Tensor o = out.narrow(0, 0, R);
    if (beta == 0.0) o.zero_(); else o.mul_(beta);
    stat_l.narrow(0, 0, R).zero_();
    return;
  }
  set_out(c.a, out, stat_m, stat_l);
  c.a.beta = static_cast<float>(beta);
  launch(DotKind::Fwd, c, heads, q);
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
  Call c = dst_side(DotVariant::Carry, rowptr, col, q, k, v, k2, v2, nsplit, stat_m, heads,
                    scale);
  const int64_t R = c.R;
  rows_f32(kPlain, out, q, R, c.a.C, "out");
  per_head(kPlain, stat_m, q, R, heads, c.a.lds, "stat_m");
  per_head(kPlain, stat_l, q, R, heads, c.a.lds, "stat_l");
  if (R == 0) return;
  if (c.other == 0) {
    TORCH_CHECK(col.numel() == 0, "dot_attn: entries but no source rows");
    return;
  }
  set_out(c.a, out, stat_m, stat_l);
  launch(DotKind::Fwd, c, heads, q);
}

void dot_attn_bwd_dst_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& q,
                         const at::Tensor& k, const at::Tensor& v,
                         const c10::optional<at::Tensor>& k2,
                         const c10::optional<at::Tensor>& v2, int64_t nsplit,
                         const at::Tensor& stat_m, const at::Tensor& stat_l,
                         const at::Tensor& g, const at::Tensor& c, at::Tensor& dq,
                         int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  Call d = dst_side(DotVariant::Plain, rowptr, col, q, k, v, k2, v2, nsplit, stat_m, heads,
                    scale);
  const int64_t R = d.R;
  per_head(kPlain, stat_m, q, R, heads, d.a.lds, "stat_m");
  per_head(kPlain, stat_l, q, R, heads, d.a.lds, "stat_l");
  per_head(kPlain, c, q, R, heads, d.a.lds, "c");
  rows_f32(kPlain, g, q, R, d.a.C, "g");
  rows_f32(kPlain, dq, q, R, d.a.C, "dq");
  if (R == 0) return;
  if (d.other == 0) {
    TORCH_CHECK(col.numel() == 0, "dot_attn: entries but no source rows");
    dq.narrow(0, 0, R).zero_();
    return;
  }
  set_dst_grads(d.a, stat_m, stat_l, g, c, dq);
  launch(DotKind::BwdDst, d, heads, q);
}

// rows = source rows (the transposed pattern; k, v, dk, dv); col = destination rows
void dot_attn_bwd_src_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& q,
                         const at::Tensor& g, const at::Tensor& k, const at::Tensor& v,
                         const at::Tensor& stat_m, const at::Tensor& stat_l,
                         const at::Tensor& c, at::Tensor& dk, at::Tensor& dv, int64_t heads,
                         double scale) {
  const c10::DeviceGuard guard(q.device());
  Call s = src_side(DotVariant::Plain, rowptr, col, nullptr, q, g, &stat_m, heads, scale);
  const int64_t R = s.R, nd = s.other;
  const int64_t lds = s.a.lds;
  per_head(kPlain, stat_m, q, nd, heads, lds, "stat_m");
  per_head(kPlain, stat_l, q, nd, heads, lds, "stat_l");
  per_head(kPlain, c, q, nd, heads, lds, "c");
  rows_f32(kPlain, k, q, R, s.a.C, "k");
  rows_f32(kPlain, v, q, R, s.a.C, "v");
  rows_f32(kPlain, dk, q, R, s.a.C, "dk");
  rows_f32(kPlain, dv, q, R, s.a.C, "dv");
  if (R == 0) return;
  if (nd == 0) {  // no destination rows: no entries, every source row's gradient is 0
    TORCH_CHECK(col.numel() == 0, "dot_attn: entries but no destination rows");
    dk.narrow(0, 0, R).zero_();
    dv.narrow(0, 0, R).zero_();
    return;
  }
  set_src_recompute(s.a, k, v, stat_m, stat_l, c);
  set_src_grads(s.a, dk, dv);
  launch(DotKind::BwdSrc, s, heads, q);
}

// -------------------------------------------------------------------------- edge features
// ee rows = slots
void dot_attn_edge_fwd_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& q,
                          const at::Tensor& k, const at::Tensor& v,
                          const c10::optional<at::Tensor>& k2,
                          const c10::optional<at::Tensor>& v2, int64_t nsplit,
                          const at::Tensor& ee, at::Tensor& out, double beta,
                          at::Tensor& stat_m, at::Tensor& stat_l, int64_t heads,
                          double scale) {
  const c10::DeviceGuard guard(q.device());
  Call c = dst_side(DotVariant::Edge, rowptr, col, q, k, v, k2, v2, nsplit, stat_m, heads,
                    scale);
  const int64_t R = c.R, nnz = c.nnz;
  edge_rows_f32(ee, q, nnz, c.a.C, "ee");
  rows_f32(kEdge, out, q, R, c.a.C, "out");
  per_head(kEdge, stat_m, q, R, heads, c.a.lds, "stat_m");
  per_head(kEdge, stat_l, q, R, heads, c.a.lds, "stat_l");
  if (R == 0) return;
  TORCH_CHECK(c.other > 0 || nnz == 0, "dot_attn_edge: entries but no source rows");
  if (nnz == 0) {  // every row is empty
    at::Tensor o = out.narrow(0, 0, R);
    if (beta == 0.0) o.zero_(); else o.mul_(beta);
    stat_l.narrow(0, 0, R).zero_();
    return;
  }
  c.a.ee = ee.data_ptr<float>();
  c.a.ldee = ee.stride(0);
  set_out(c.a, out, stat_m, stat_l);
  c.a.beta = static_cast<float>(beta);
  launch(DotKind::Fwd, c, heads, q);
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
  Call d = dst_side(DotVariant::Edge, rowptr, col, q, k, v, k2, v2, nsplit, stat_m, heads,
                    scale);
  const int64_t R = d.R, nnz = d.nnz;
  edge_rows_f32(ee, q, nnz, d.a.C, "ee");
  per_head(kEdge, stat_m, q, R, heads, d.a.lds, "stat_m");
  per_head(kEdge, stat_l, q, R, heads, d.a.lds, "stat_l");
  per_head(kEdge, c, q, R, heads, d.a.lds, "c");
  rows_f32(kEdge, g, q, R, d.a.C, "g");
  rows_f32(kEdge, dq, q, R, d.a.C, "dq");
  edge_rows_f32(dee, q, nnz, d.a.C, "dee");
  weights(w, q, nnz, heads);
  if (R == 0) return;
  TORCH_CHECK(d.other > 0 || nnz == 0, "dot_attn_edge: entries but no source rows");
  if (nnz == 0) {
    dq.narrow(0, 0, R).zero_();
    return;
  }
  d.a.ee = ee.data_ptr<float>();
  d.a.ldee = ee.stride(0);
  set_dst_grads(d.a, stat_m, stat_l, g, c, dq);
  d.a.dee = dee.data_ptr<float>();
  d.a.lddee = dee.stride(0);
  d.a.w = w.data_ptr<float>();
  d.a.ldw = w.stride(0);
  launch(DotKind::BwdDst, d, heads, q);
}

// t_slot = the forward slot (row of w) of each transposed entry
void dot_attn_edge_bwd_src_op(const at::Tensor& rowptr, const at::Tensor& col,
                              const at::Tensor& t_slot, const at::Tensor& q,
                              const at::Tensor& g, const at::Tensor& w, at::Tensor& dk,
                              at::Tensor& dv, int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  Call s = src_side(DotVariant::Edge, rowptr, col, &t_slot, q, g, nullptr, heads, scale);
  const int64_t R = s.R, nd = s.other, nnz = s.nnz;
  weights(w, q, nnz, heads);
  rows_f32(kEdge, dk, q, R, s.a.C, "dk");
  rows_f32(kEdge, dv, q, R, s.a.C, "dv");
  if (R == 0) return;
  TORCH_CHECK(nd > 0 || nnz == 0, "dot_attn_edge: entries but no destination rows");
  if (nnz == 0) {  // no entries: every source row's gradient is 0
    dk.narrow(0, 0, R).zero_();
    dv.narrow(0, 0, R).zero_();
    return;
  }
  s.a.w = w.data_ptr<float>();
  s.a.ldw = w.stride(0);
  set_src_grads(s.a, dk, dv);
  launch(DotKind::BwdSrc, s, heads, q);
}

// ---------------------------------------------------------------------- attention dropout
void dot_attn_drop_fwd_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& q,
                          const at::Tensor& k, const at::Tensor& v,
                          const c10::optional<at::Tensor>& k2,
                          const c10::optional<at::Tensor>& v2, int64_t nsplit, at::Tensor& out,
                          at::Tensor& stat_m, at::Tensor& stat_l, const at::Tensor& seed,
                          double p, int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  Call c = dst_side(DotVariant::Drop, rowptr, col, q, k, v, k2, v2, nsplit, stat_m, heads,
                    scale);
  const int64_t R = c.R;
  rows_f32(kDrop, out, q, R, c.a.C, "out");
  per_head(kDrop, stat_m, q, R, heads, c.a.lds, "stat_m");
  per_head(kDrop, stat_l, q, R, heads, c.a.lds, "stat_l");
  const Drop d = dropout(seed, p, q);
  if (R == 0) return;
  if (c.other == 0) {  // nothing to gather from: every row is empty
    TORCH_CHECK(col.numel() == 0, "dot_attn_drop: entries but no source rows");
    out.narrow(0, 0, R).zero_();
    stat_l.narrow(0, 0, R).zero_();
    return;
  }
  set_out(c.a, out, stat_m, stat_l);
  set_drop(c.a, d);
  launch(DotKind::Fwd, c, heads, q);
}

void dot_attn_drop_bwd_dst_op(const at::Tensor& rowptr, const at::Tensor& col,
                              const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                              const c10::optional<at::Tensor>& k2,
                              const c10::optional<at::Tensor>& v2, int64_t nsplit,
                              const at::Tensor& stat_m, const at::Tensor& stat_l,
                              const at::Tensor& g, const at::Tensor& c, at::Tensor& dq,
                              const at::Tensor& seed, double p, int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  Call d = dst_side(DotVariant::Drop, rowptr, col, q, k, v, k2, v2, nsplit, stat_m, heads,
                    scale);
  const int64_t R = d.R;
  per_head(kDrop, stat_m, q, R, heads, d.a.lds, "stat_m");
  per_head(kDrop, stat_l, q, R, heads, d.a.lds, "stat_l");
  per_head(kDrop, c, q, R, heads, d.a.lds, "c");
  rows_f32(kDrop, g, q, R, d.a.C, "g");
  rows_f32(kDrop, dq, q, R, d.a.C, "dq");
  const Drop dr = dropout(seed, p, q);
  if (R == 0) return;
  if (d.other == 0) {
    TORCH_CHECK(col.numel() == 0, "dot_attn_drop: entries but no source rows");
    dq.narrow(0, 0, R).zero_();
    return;
  }
  set_dst_grads(d.a, stat_m, stat_l, g, c, dq);
  set_drop(d.a, dr);
  launch(DotKind::BwdDst, d, heads, q);
}

// t_slot = the forward slot of each transposed entry (what the mask is keyed on)
void dot_attn_drop_bwd_src_op(const at::Tensor& rowptr, const at::Tensor& col,
                              const at::Tensor& t_slot, const at::Tensor& q,
                              const at::Tensor& g, const at::Tensor& k, const at::Tensor& v,
                              const at::Tensor& stat_m, const at::Tensor& stat_l,
                              const at::Tensor& c, at::Tensor& dk, at::Tensor& dv,
                              const at::Tensor& seed, double p, int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  Call s = src_side(DotVariant::Drop, rowptr, col, &t_slot, q, g, &stat_m, heads, scale);
  const int64_t R = s.R, nd = s.other;
  const int64_t lds = s.a.lds;
  per_head(kDrop, stat_m, q, nd, heads, lds, "stat_m");
  per_head(kDrop, stat_l, q, nd, heads, lds, "stat_l");
  per_head(kDrop, c, q, nd, heads, lds, "c");
  rows_f32(kDrop, k, q, R, s.a.C, "k");
  rows_f32(kDrop, v, q, R, s.a.C, "v");
  rows_f32(kDrop, dk, q, R, s.a.C, "dk");
  rows_f32(kDrop, dv, q, R, s.a.C, "dv");
  const Drop d = dropout(seed, p, q);
  if (R == 0) return;
  if (nd == 0) {  // no destination rows: no entries, every source row's gradient is 0
    TORCH_CHECK(s.nnz == 0, "dot_attn_drop: entries but no destination rows");
    dk.narrow(0, 0, R).zero_();
    dv.narrow(0, 0, R).zero_();
    return;
  }
  set_src_recompute(s.a, k, v, stat_m, stat_l, c);
  set_src_grads(s.a, dk, dv);
  set_drop(s.a, d);
  launch(DotKind::BwdSrc, s, heads, q);
}

// The host side of philox.h: keep[s, h] for the slots first_slot .. first_slot + num_slots
// (bool [num_slots, heads] on the CPU), so the C++ generator can be compared with the torch
// one (ops/philox.py) without a GPU.
at::Tensor attn_keep_mask_host(int64_t seed, int64_t num_slots, int64_t heads, double p,
                               int64_t first_slot) {
  TORCH_CHECK(num_slots >= 0 && heads >= 1 && heads <= 32 && first_slot >= 0,
              "attn_keep_mask_host: num_slots >= 0, 1 <= heads <= 32, first_slot >= 0");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "attn_keep_mask_host: p must lie in [0, 1), got ", p);
  const uint32_t thr = attn_keep_threshold(p);
  at::Tensor keep = at::empty({num_slots, heads}, at::TensorOptions().dtype(at::kBool));
  bool* out = keep.data_ptr<bool>();
  for (int64_t s = 0; s < num_slots; ++s) {
    const uint32_t bits = attn_keep_bits(static_cast<uint64_t>(seed), first_slot + s, thr,
                                         static_cast<int>(heads));
    for (int64_t h = 0; h < heads; ++h) out[s * heads + h] = (bits >> h) & 1u;
  }
  return keep;
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
  m.def("dot_attn_edge_fwd_f32(Tensor rowptr, Tensor col, Tensor q, Tensor k, Tensor v, "
        "Tensor? k2, Tensor? v2, int nsplit, Tensor ee, Tensor(a!) out, float beta, "
        "Tensor(b!) stat_m, Tensor(c!) stat_l, int heads, float scale) -> ()");
  m.def("dot_attn_edge_bwd_dst_f32(Tensor rowptr, Tensor col, Tensor q, Tensor k, Tensor v, "
        "Tensor? k2, Tensor? v2, int nsplit, Tensor ee, Tensor stat_m, Tensor stat_l, "
        "Tensor g, Tensor c, Tensor(a!) dq, Tensor(b!) dee, Tensor(c!) w, int heads, "
        "float scale) -> ()");
  m.def("dot_attn_edge_bwd_src_f32(Tensor rowptr, Tensor col, Tensor t_slot, Tensor q, "
        "Tensor g, Tensor w, Tensor(a!) dk, Tensor(b!) dv, int heads, float scale) -> ()");
  m.def("dot_attn_drop_fwd_f32(Tensor rowptr, Tensor col, Tensor q, Tensor k, Tensor v, "
        "Tensor? k2, Tensor? v2, int nsplit, Tensor(a!) out, Tensor(b!) stat_m, "
        "Tensor(c!) stat_l, Tensor seed, float p, int heads, float scale) -> ()");
  m.def("dot_attn_drop_bwd_dst_f32(Tensor rowptr, Tensor col, Tensor q, Tensor k, Tensor v, "
        "Tensor? k2, Tensor? v2, int nsplit, Tensor stat_m, Tensor stat_l, Tensor g, "
        "Tensor c, Tensor(a!) dq, Tensor seed, float p, int heads, float scale) -> ()");
  m.def("dot_attn_drop_bwd_src_f32(Tensor rowptr, Tensor col, Tensor t_slot, Tensor q, "
        "Tensor g, Tensor k, Tensor v, Tensor stat_m, Tensor stat_l, Tensor c, "
        "Tensor(a!) dk, Tensor(b!) dv, Tensor seed, float p, int heads, float scale) -> ()");
  m.def("attn_keep_mask_host(int seed, int num_slots, int heads, float p, "
        "int first_slot=0) -> Tensor",
        &dgraph::attn_keep_mask_host);
}

TORCH_LIBRARY_IMPL(dgraph_amd, CUDA, m) {
  m.impl("dot_attn_fwd_f32", &dgraph::dot_attn_fwd_op);
  m.impl("dot_attn_fwd_carry_f32", &dgraph::dot_attn_fwd_carry_op);
  m.impl("dot_attn_bwd_dst_f32", &dgraph::dot_attn_bwd_dst_op);
  m.impl("dot_attn_bwd_src_f32", &dgraph::dot_attn_bwd_src_op);
  m.impl("dot_attn_edge_fwd_f32", &dgraph::dot_attn_edge_fwd_op);
  m.impl("dot_attn_edge_bwd_dst_f32", &dgraph::dot_attn_edge_bwd_dst_op);
  m.impl("dot_attn_edge_bwd_src_f32", &dgraph::dot_attn_edge_bwd_src_op);
  m.impl("dot_attn_drop_fwd_f32", &dgraph::dot_attn_drop_fwd_op);
  m.impl("dot_attn_drop_bwd_dst_f32", &dgraph::dot_attn_drop_bwd_dst_op);
  m.impl("dot_attn_drop_bwd_src_f32", &dgraph::dot_attn_drop_bwd_src_op);
}
