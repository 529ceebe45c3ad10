// dgraph_amd — dispatcher registration of the fused fp32 dot-product attention kernels with
// attention dropout (csrc/kernels/dot_attn_drop_f32.hip; ops/dot_attn.py) and of the host
// side of the keep-mask generator (csrc/kernels/philox.h). Every shape, dtype, stride and
// alignment contract the kernels rely on is checked here, before any launch; column ids and
// transposed slots are built once per pattern by the Python caller (ops/gat.py: GatPattern).
//
// Empty sides are legal and never reach a kernel, as in bindings_dot_attn.cpp: a relation
// with no destination rows returns; one whose gathered side has no rows at all writes the
// empty-row result (zeros) with plain fills.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include "check.h"
#include "kernels/kernels.h"
#include "kernels/philox.h"

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
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), "dot_attn_drop: ", name,
              " must be on ", ref.device());
  TORCH_CHECK(t.scalar_type() == at::kFloat && t.dim() == 2 && t.size(1) == cols &&
                  t.size(0) >= min_rows,
              "dot_attn_drop: ", name, " must be float32 [>= ", min_rows, ", ", cols,
              "], got ", t.sizes());
  if (t.size(0) == 0) return;
  TORCH_CHECK(t.stride(1) == 1 && t.stride(0) % 4 == 0 && t.stride(0) >= cols &&
                  al16(t.data_ptr()),
              "dot_attn_drop: ", name, " must have unit column stride, a row stride divisible "
              "by 4 and 16-B alignment, got strides ", t.strides());
}

// per-head arrays: [>= min_rows, heads] with unit column stride and the shared row stride
void per_head(const at::Tensor& t, const at::Tensor& ref, int64_t min_rows, int64_t heads,
              int64_t lds, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device() && t.scalar_type() == at::kFloat &&
                  t.dim() == 2 && t.size(1) == heads && t.size(0) >= min_rows,
              "dot_attn_drop: ", name, " must be float32 [>= ", min_rows, ", ", heads, "] on ",
              ref.device(), ", got ", t.sizes());
  if (t.size(0) == 0) return;
  TORCH_CHECK((heads == 1 || t.stride(1) == 1) && t.stride(0) == lds && lds >= heads,
              "dot_attn_drop: ", name, " must have unit column stride and row stride ", lds,
              ", got strides ", t.strides());
}

IType pattern(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& ref) {
  TORCH_CHECK(rowptr.is_cuda() && rowptr.device() == ref.device() &&
                  rowptr.scalar_type() == at::kLong && rowptr.is_contiguous() &&
                  rowptr.dim() == 1 && rowptr.numel() >= 1,
              "dot_attn_drop: rowptr must be contiguous int64 on ", ref.device());
  TORCH_CHECK(col.is_cuda() && col.device() == ref.device() && col.is_contiguous() &&
                  col.dim() == 1 &&
                  (col.scalar_type() == at::kInt || col.scalar_type() == at::kLong),
              "dot_attn_drop: col must be contiguous int32/int64 on ", ref.device());
  return col.scalar_type() == at::kInt ? IType::I32 : IType::I64;
}

int width(const at::Tensor& q, int64_t heads) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 2, "dot_attn_drop: q must be a 2-D device tensor");
  const int C = static_cast<int>(q.size(1));
  TORCH_CHECK(heads > 0 && heads <= 8 && dot_attn_f32_shape_ok(C, static_cast<int>(heads)),
              "dot_attn_drop: unsupported width ", C, " / heads ", heads,
              " (C in 64/128/256, heads in 1/2/4/8, >= 2 lanes of 4 channels per head)");
  return C;
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
  TORCH_CHECK((p2 == nullptr) == (w2 == nullptr), "dot_attn_drop: k2 and v2 come together");
  TORCH_CHECK(nsplit >= 0 && nsplit < (int64_t(1) << 32), "dot_attn_drop: bad nsplit");
  Sources s;
  s.k = k.data_ptr<float>();
  s.v = v.data_ptr<float>();
  s.ldk = k.stride(0);
  s.ldv = v.stride(0);
  s.rows = k.size(0);
  if (p2) {
    rows_f32(*p2, q, 0, C, "k2");
    rows_f32(*w2, q, p2->size(0), C, "v2");
    TORCH_CHECK(k.size(0) >= nsplit, "dot_attn_drop: k has fewer rows than nsplit");
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
void dot_attn_drop_fwd_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& q,
                          const at::Tensor& k, const at::Tensor& v,
                          const c10::optional<at::Tensor>& k2,
                          const c10::optional<at::Tensor>& v2, int64_t nsplit, at::Tensor& out,
                          at::Tensor& stat_m, at::Tensor& stat_l, const at::Tensor& seed,
                          double p, int64_t heads, double scale) {
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
  const Drop d = dropout(seed, p, q);
  if (R == 0) return;
  if (s.rows == 0) {  // nothing to gather from: every row is empty
    TORCH_CHECK(col.numel() == 0, "dot_attn_drop: entries but no source rows");
    out.narrow(0, 0, R).zero_();
    stat_l.narrow(0, 0, R).zero_();
    return;
  }
  DG_HIP_CHECK(dot_attn_drop_fwd_f32(
      it, rowptr.data_ptr<int64_t>(), col.data_ptr(), R, C, static_cast<int>(heads), lds,
      static_cast<float>(scale), q.data_ptr<float>(), q.stride(0), s.k, s.ldk, s.v, s.ldv,
      s.k2, s.ldk2, s.v2, s.ldv2, s.nsplit, out.data_ptr<float>(), out.stride(0),
      stat_m.data_ptr<float>(), stat_l.data_ptr<float>(), d.seed, d.thr, d.inv_keep,
      cur_stream(q)));
}

void dot_attn_drop_bwd_dst_op(const at::Tensor& rowptr, const at::Tensor& col,
                              const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                              const c10::optional<at::Tensor>& k2,
                              const c10::optional<at::Tensor>& v2, int64_t nsplit,
                              const at::Tensor& stat_m, const at::Tensor& stat_l,
                              const at::Tensor& g, const at::Tensor& c, at::Tensor& dq,
                              const at::Tensor& seed, double p, int64_t heads, double scale) {
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
  const Drop d = dropout(seed, p, q);
  if (R == 0) return;
  if (s.rows == 0) {
    TORCH_CHECK(col.numel() == 0, "dot_attn_drop: entries but no source rows");
    dq.narrow(0, 0, R).zero_();
    return;
  }
  DG_HIP_CHECK(dot_attn_drop_bwd_dst_f32(
      it, rowptr.data_ptr<int64_t>(), col.data_ptr(), R, C, static_cast<int>(heads), lds,
      static_cast<float>(scale), q.data_ptr<float>(), q.stride(0), s.k, s.ldk, s.v, s.ldv,
      s.k2, s.ldk2, s.v2, s.ldv2, s.nsplit, stat_m.data_ptr<float>(),
      stat_l.data_ptr<float>(), g.data_ptr<float>(), g.stride(0), c.data_ptr<float>(),
      dq.data_ptr<float>(), dq.stride(0), d.seed, d.thr, d.inv_keep, cur_stream(q)));
}

// rows = source rows (the transposed pattern; k, v, dk, dv); col = destination rows; t_slot =
// the forward slot of each transposed entry (what the mask is keyed on)
void dot_attn_drop_bwd_src_op(const at::Tensor& rowptr, const at::Tensor& col,
                              const at::Tensor& t_slot, const at::Tensor& q,
                              const at::Tensor& g, const at::Tensor& k, const at::Tensor& v,
                              const at::Tensor& stat_m, const at::Tensor& stat_l,
                              const at::Tensor& c, at::Tensor& dk, at::Tensor& dv,
                              const at::Tensor& seed, double p, int64_t heads, double scale) {
  const c10::DeviceGuard guard(q.device());
  const int C = width(q, heads);
  const IType it = pattern(rowptr, col, q);
  const int64_t R = rowptr.numel() - 1;
  const int64_t nd = q.size(0);
  const int64_t nnz = col.numel();
  const int64_t lds = stat_m.dim() == 2 ? stat_m.stride(0) : 0;
  TORCH_CHECK(t_slot.is_cuda() && t_slot.device() == q.device() && t_slot.is_contiguous() &&
                  t_slot.dim() == 1 && t_slot.scalar_type() == col.scalar_type() &&
                  t_slot.numel() == nnz,
              "dot_attn_drop: t_slot must be contiguous, of col's dtype and length (", nnz,
              ") on ", q.device());
  rows_f32(q, q, 0, C, "q");
  rows_f32(g, q, nd, C, "g");
  per_head(stat_m, q, nd, heads, lds, "stat_m");
  per_head(stat_l, q, nd, heads, lds, "stat_l");
  per_head(c, q, nd, heads, lds, "c");
  rows_f32(k, q, R, C, "k");
  rows_f32(v, q, R, C, "v");
  rows_f32(dk, q, R, C, "dk");
  rows_f32(dv, q, R, C, "dv");
  const Drop d = dropout(seed, p, q);
  if (R == 0) return;
  if (nd == 0) {  // no destination rows: no entries, every source row's gradient is 0
    TORCH_CHECK(nnz == 0, "dot_attn_drop: entries but no destination rows");
    dk.narrow(0, 0, R).zero_();
    dv.narrow(0, 0, R).zero_();
    return;
  }
  DG_HIP_CHECK(dot_attn_drop_bwd_src_f32(
      it, rowptr.data_ptr<int64_t>(), col.data_ptr(), t_slot.data_ptr(), R, C,
      static_cast<int>(heads), lds, static_cast<float>(scale), q.data_ptr<float>(),
      q.stride(0), g.data_ptr<float>(), g.stride(0), k.data_ptr<float>(), k.stride(0),
      v.data_ptr<float>(), v.stride(0), stat_m.data_ptr<float>(), stat_l.data_ptr<float>(),
      c.data_ptr<float>(), dk.data_ptr<float>(), dk.stride(0), dv.data_ptr<float>(),
      dv.stride(0), d.seed, d.thr, d.inv_keep, cur_stream(q)));
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
  m.impl("dot_attn_drop_fwd_f32", &dgraph::dot_attn_drop_fwd_op);
  m.impl("dot_attn_drop_bwd_dst_f32", &dgraph::dot_attn_drop_bwd_dst_op);
  m.impl("dot_attn_drop_bwd_src_f32", &dgraph::dot_attn_drop_bwd_src_op);
}
