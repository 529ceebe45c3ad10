// dgraph_amd — dispatcher registration of the GATv2 attention kernels with bf16 storage
// (csrc/kernels/gatv2_bf16.hip; ops/gatv2.py). Every dtype, shape, stride, 16-B alignment and
// the device the kernels rely on is checked here, before any launch; column ids are checked
// against the operand rows once per pattern by the Python caller (ops/gat.py: GatPattern).
//
// Empty sides are legal and never reach a kernel. An array of a side only has to hold that
// side's rows, so 0 rows pass every check of a side with no rows: a rank with no destination
// rows returns; one whose part of the pattern has no entries (no source rows at all, or rows
// that nothing points at) writes the empty-row result (zeros; da_part zero-filled) with plain
// fills. A second source with 0 rows is treated as absent, and with 0 first-source rows
// (nsplit = 0) every column, the padding slots' column 0 included, reads the second source —
// so row 0 of whatever a launched kernel gathers from always exists.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include "attn_check.h"
#include "check.h"
#include "kernels/kernels.h"

namespace dgraph {
namespace {

constexpr const char* kOp = "gatv2_bf16";  // the prefix of every message

uint16_t* bf16_out(at::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

// the pattern (int32 columns only: GatPattern builds nothing else), the width, the attention
// vector and the scalars every kernel takes; `xd` is the op's first feature operand
GatV2Bf16Args common(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& xd,
                     const at::Tensor& att, const at::Tensor& stat_m, int64_t heads,
                     double slope) {
  TORCH_CHECK(xd.is_cuda() && xd.dim() == 2, "gatv2_bf16: xd must be a 2-D device tensor");
  const int C = static_cast<int>(xd.size(1));
  TORCH_CHECK(heads > 0 && gatv2_bf16_shape_ok(C, static_cast<int>(heads)),
              "gatv2_bf16: unsupported width ", C, " / heads ", heads,
              " (C in 64/128/256, heads in 1/2/4/8)");
  pattern(kOp, rowptr, col, xd);
  TORCH_CHECK(col.scalar_type() == at::kInt,
              "gatv2_bf16: col must be int32 (GatPattern's index type), got ",
              col.scalar_type());
  TORCH_CHECK(att.is_cuda() && att.device() == xd.device() &&
                  att.scalar_type() == at::kFloat && att.dim() == 1 && att.size(0) == C &&
                  att.stride(0) == 1 && al16(att.data_ptr()),
              "gatv2_bf16: att must be a contiguous, 16-B aligned float32 [", C, "] on ",
              xd.device(), ", got ", att.scalar_type(), " ", att.sizes());
  GatV2Bf16Args a{};
  a.rowptr = rowptr.data_ptr<int64_t>();
  a.col = col.data_ptr<int32_t>();
  a.nrows = rowptr.numel() - 1;
  a.C = C;
  a.slope = static_cast<float>(slope);
  a.att = att.data_ptr<float>();
  // the per-head arrays share stat_m's row stride (heads for an array without rows)
  a.lds = stat_m.dim() == 2 && stat_m.size(0) > 0 ? stat_m.stride(0) : heads;
  return a;
}

// fwd / bwd_dst: xd rows = CSR rows; xs (+ xs2 past nsplit) = the gathered rows. Returns the
// number of source rows the kernel could gather from.
int64_t dst_side(GatV2Bf16Args& a, const at::Tensor& xd, const at::Tensor& xs,
                 const c10::optional<at::Tensor>& xs2, int64_t nsplit) {
  const int C = a.C;
  rows_bf16(kOp, xd, xd, a.nrows, C, "xd");
  rows_bf16(kOp, xs, xd, 0, C, "xs");
  const at::Tensor* p2 = opt_t(xs2);
  TORCH_CHECK(nsplit >= 0 && nsplit < (int64_t(1) << 31), "gatv2_bf16: bad nsplit");
  a.xd = bf16_ptr(xd);
  a.ldxd = xd.stride(0);
  int64_t rows = xs.size(0);
  if (rows > 0) {
    a.xs = bf16_ptr(xs);
    a.ldxs = xs.stride(0);
  }
  if (p2) {
    rows_bf16(kOp, *p2, xd, 0, C, "xs2");
    TORCH_CHECK(xs.size(0) >= nsplit, "gatv2_bf16: xs has fewer rows than nsplit");
    if (p2->size(0) > 0) {
      a.xs2 = bf16_ptr(*p2);
      a.ldxs2 = p2->stride(0);
      a.nsplit = nsplit;
      rows += p2->size(0);
    }
  }
  return rows;
}

void gatv2_fwd_bf16_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& xd,
                       const at::Tensor& xs, const c10::optional<at::Tensor>& xs2,
                       int64_t nsplit, const at::Tensor& att, at::Tensor& out,
                       at::Tensor& stat_m, at::Tensor& stat_l, int64_t heads, double slope) {
  const c10::DeviceGuard guard(xd.device());
  GatV2Bf16Args a = common(rowptr, col, xd, att, stat_m, heads, slope);
  const int64_t R = a.nrows;
  const int64_t src = dst_side(a, xd, xs, xs2, nsplit);
  rows_bf16(kOp, out, xd, R, a.C, "out");
  per_head(kOp, stat_m, xd, R, heads, a.lds, "stat_m");
  per_head(kOp, stat_l, xd, R, heads, a.lds, "stat_l");
  if (R == 0) return;
  TORCH_CHECK(src > 0 || col.numel() == 0, "gatv2_bf16: entries but no source rows");
  if (col.numel() == 0) {  // every row is empty
    out.narrow(0, 0, R).zero_();
    stat_l.narrow(0, 0, R).zero_();
    return;
  }
  a.out = bf16_out(out);
  a.ldo = out.stride(0);
  a.stat_m = stat_m.data_ptr<float>();
  a.stat_l = stat_l.data_ptr<float>();
  DG_HIP_CHECK(gatv2_fwd_bf16(a, static_cast<int>(heads), cur_stream(xd)));
}

// writes c (what the source side reads), dxd and every row of da_part
// (contiguous [gatv2_bf16_da_parts(R, C), C])
void gatv2_bwd_dst_bf16_op(const at::Tensor& rowptr, const at::Tensor& col,
                           const at::Tensor& xd, const at::Tensor& xs,
                           const c10::optional<at::Tensor>& xs2, int64_t nsplit,
                           const at::Tensor& att, const at::Tensor& stat_m,
                           const at::Tensor& stat_l, const at::Tensor& g, at::Tensor& c,
                           at::Tensor& dxd, at::Tensor& da_part, int64_t heads, double slope) {
  const c10::DeviceGuard guard(xd.device());
  GatV2Bf16Args a = common(rowptr, col, xd, att, stat_m, heads, slope);
  const int64_t R = a.nrows;
  const int64_t src = dst_side(a, xd, xs, xs2, nsplit);
  per_head(kOp, stat_m, xd, R, heads, a.lds, "stat_m");
  per_head(kOp, stat_l, xd, R, heads, a.lds, "stat_l");
  per_head(kOp, c, xd, R, heads, a.lds, "c");
  rows_bf16(kOp, g, xd, R, a.C, "g");
  rows_bf16(kOp, dxd, xd, R, a.C, "dxd");
  const int64_t P = gatv2_bf16_da_parts(R, a.C);
  TORCH_CHECK(da_part.is_cuda() && da_part.device() == xd.device() &&
                  da_part.scalar_type() == at::kFloat && da_part.dim() == 2 &&
                  da_part.size(0) == P && da_part.size(1) == a.C &&
                  (P == 0 || (da_part.is_contiguous() && al16(da_part.data_ptr()))),
              "gatv2_bf16: da_part must be contiguous, 16-B aligned float32 [", P, ", ", a.C,
              "] on ", xd.device(), ", got ", da_part.sizes());
  if (R == 0) return;
  TORCH_CHECK(src > 0 || col.numel() == 0, "gatv2_bf16: entries but no source rows");
  if (col.numel() == 0) {
    c.narrow(0, 0, R).zero_();
    dxd.narrow(0, 0, R).zero_();
    da_part.zero_();
    return;
  }
  a.stat_m = const_cast<float*>(stat_m.data_ptr<float>());
  a.stat_l = const_cast<float*>(stat_l.data_ptr<float>());
  a.g = bf16_ptr(g);
  a.ldg = g.stride(0);
  a.c = c.data_ptr<float>();
  a.dxd = bf16_out(dxd);
  a.lddxd = dxd.stride(0);
  a.da_part = da_part.data_ptr<float>();
  DG_HIP_CHECK(gatv2_bwd_dst_bf16(a, static_cast<int>(heads), cur_stream(xd)));
}

// rows = source rows (the transposed pattern, or a slice of its row pointer; xs, dxs);
// col = destination rows (xd, g and the per-head arrays)
void gatv2_bwd_src_bf16_op(const at::Tensor& rowptr, const at::Tensor& col,
                           const at::Tensor& xd, const at::Tensor& g, const at::Tensor& xs,
                           const at::Tensor& att, const at::Tensor& stat_m,
                           const at::Tensor& stat_l, const at::Tensor& c, at::Tensor& dxs,
                           int64_t heads, double slope) {
  const c10::DeviceGuard guard(xd.device());
  GatV2Bf16Args a = common(rowptr, col, xd, att, stat_m, heads, slope);
  const int64_t R = a.nrows, nd = xd.size(0);
  rows_bf16(kOp, xd, xd, 0, a.C, "xd");
  rows_bf16(kOp, g, xd, nd, a.C, "g");
  per_head(kOp, stat_m, xd, nd, heads, a.lds, "stat_m");
  per_head(kOp, stat_l, xd, nd, heads, a.lds, "stat_l");
  per_head(kOp, c, xd, nd, heads, a.lds, "c");
  rows_bf16(kOp, xs, xd, R, a.C, "xs");
  rows_bf16(kOp, dxs, xd, R, a.C, "dxs");
  if (R == 0) return;
  TORCH_CHECK(nd > 0 || col.numel() == 0, "gatv2_bf16: entries but no destination rows");
  if (col.numel() == 0) {  // no entries: every source row's gradient is 0
    dxs.narrow(0, 0, R).zero_();
    return;
  }
  a.xd = bf16_ptr(xd);
  a.ldxd = xd.stride(0);
  a.g = bf16_ptr(g);
  a.ldg = g.stride(0);
  a.xs = bf16_ptr(xs);
  a.ldxs = xs.stride(0);
  a.stat_m = const_cast<float*>(stat_m.data_ptr<float>());
  a.stat_l = const_cast<float*>(stat_l.data_ptr<float>());
  a.c = const_cast<float*>(c.data_ptr<float>());
  a.dxs = bf16_out(dxs);
  a.lddxs = dxs.stride(0);
  DG_HIP_CHECK(gatv2_bwd_src_bf16(a, static_cast<int>(heads), cur_stream(xd)));
}

// rows of da_part for a relation of R destination rows at width C (no device work)
int64_t gatv2_bf16_da_parts_op(int64_t R, int64_t C) {
  TORCH_CHECK(R >= 0 && (C == 64 || C == 128 || C == 256), "gatv2_bf16: bad (R, C) = (", R,
              ", ", C, ")");
  return gatv2_bf16_da_parts(R, static_cast<int>(C));
}

}  // namespace
}  // namespace dgraph

TORCH_LIBRARY_FRAGMENT(dgraph_amd, m) {
  m.def("gatv2_fwd_bf16(Tensor rowptr, Tensor col, Tensor xd, Tensor xs, Tensor? xs2, "
        "int nsplit, Tensor att, Tensor(a!) out, Tensor(b!) stat_m, Tensor(c!) stat_l, "
        "int heads, float slope) -> ()");
  m.def("gatv2_bwd_dst_bf16(Tensor rowptr, Tensor col, Tensor xd, Tensor xs, Tensor? xs2, "
        "int nsplit, Tensor att, Tensor stat_m, Tensor stat_l, Tensor g, Tensor(a!) c, "
        "Tensor(b!) dxd, Tensor(c!) da_part, int heads, float slope) -> ()");
  m.def("gatv2_bwd_src_bf16(Tensor rowptr, Tensor col, Tensor xd, Tensor g, Tensor xs, "
        "Tensor att, Tensor stat_m, Tensor stat_l, Tensor c, Tensor(a!) dxs, int heads, "
        "float slope) -> ()");
  m.def("gatv2_bf16_da_parts(int R, int C) -> int", &dgraph::gatv2_bf16_da_parts_op);
}

TORCH_LIBRARY_IMPL(dgraph_amd, CUDA, m) {
  m.impl("gatv2_fwd_bf16", &dgraph::gatv2_fwd_bf16_op);
  m.impl("gatv2_bwd_dst_bf16", &dgraph::gatv2_bwd_dst_bf16_op);
  m.impl("gatv2_bwd_src_bf16", &dgraph::gatv2_bwd_src_bf16_op);
}
