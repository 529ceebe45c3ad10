// dgraph_amd — dispatcher registration of the fused fp32 GATv2 attention kernels
// (csrc/kernels/gatv2_f32.hip; ops/gatv2.py). Every shape, dtype, stride and alignment
// contract the kernels rely on is checked here; column ids are checked against the operand
// rows once per pattern by the Python caller (ops/gat.py: GatPattern).
//
// Empty sides are legal and never reach a kernel: a relation with no destination rows
// returns; one whose gathered side has no rows at all (the pattern then has no entries)
// writes the empty-row result (zeros; da_part zero-filled) with plain fills. A second source
// with 0 rows is treated as absent, and with 0 first-source rows (nsplit = 0) every column,
// the padding slots' column 0 included, reads the second source — so row 0 of whatever a
// launched kernel gathers from always exists.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include "attn_check.h"
#include "check.h"
#include "kernels/kernels.h"

namespace dgraph {
namespace {

constexpr const char* kOp = "gatv2";  // the prefix of every message

int width(const at::Tensor& xd, int64_t heads) {
  TORCH_CHECK(xd.is_cuda() && xd.dim() == 2, "gatv2: xd must be a 2-D device tensor");
  const int C = static_cast<int>(xd.size(1));
  TORCH_CHECK(heads > 0 && heads <= 8 && gatv2_f32_shape_ok(C, static_cast<int>(heads)),
              "gatv2: unsupported width ", C, " / heads ", heads,
              " (C in 64/128/256, heads in 1/2/4/8, >= 2 lanes of 4 channels per head)");
  return C;
}

// the attention vector: contiguous float32 [C], 16-B aligned
const float* att_vec(const at::Tensor& att, const at::Tensor& ref, int C) {
  TORCH_CHECK(att.is_cuda() && att.device() == ref.device() &&
                  att.scalar_type() == at::kFloat && att.dim() == 1 && att.size(0) == C &&
                  att.stride(0) == 1 && al16(att.data_ptr()),
              "gatv2: att must be a contiguous, 16-B aligned float32 [", C, "] on ",
              ref.device(), ", got ", att.sizes());
  return att.data_ptr<float>();
}

// the two gathered sources of fwd / bwd_dst, as the kernels take them
struct Sources {
  const float *xs, *xs2 = nullptr;
  int64_t ldxs, ldxs2 = 0, nsplit = 0, rows = 0;
};

Sources sources(const at::Tensor& xd, const at::Tensor& xs,
                const c10::optional<at::Tensor>& xs2, int64_t nsplit, int C) {
  rows_f32(kOp, xs, xd, 0, C, "xs");
  const at::Tensor* p2 = opt_t(xs2);
  TORCH_CHECK(nsplit >= 0 && nsplit < (int64_t(1) << 32), "gatv2: bad nsplit");
  Sources s;
  s.xs = xs.data_ptr<float>();
  s.ldxs = xs.stride(0);
  s.rows = xs.size(0);
  if (p2) {
    rows_f32(kOp, *p2, xd, 0, C, "xs2");
    TORCH_CHECK(xs.size(0) >= nsplit, "gatv2: xs has fewer rows than nsplit");
    if (p2->size(0) > 0) {
      s.xs2 = p2->data_ptr<float>();
      s.ldxs2 = p2->stride(0);
      s.nsplit = nsplit;
      s.rows += p2->size(0);
    }
  }
  return s;
}

// xd/out rows = CSR rows; xs (+ xs2 past nsplit) = the gathered rows
void gatv2_fwd_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& xd,
                  const at::Tensor& xs, const c10::optional<at::Tensor>& xs2, int64_t nsplit,
                  const at::Tensor& att, at::Tensor& out, double beta, at::Tensor& stat_m,
                  at::Tensor& stat_l, int64_t heads, double slope) {
  const c10::DeviceGuard guard(xd.device());
  const int C = width(xd, heads);
  const IType it = pattern(kOp, rowptr, col, xd);
  const int64_t R = rowptr.numel() - 1;
  const int64_t lds = stat_m.dim() == 2 ? stat_m.stride(0) : 0;
  rows_f32(kOp, xd, xd, R, C, "xd");
  const Sources s = sources(xd, xs, xs2, nsplit, C);
  const float* ap = att_vec(att, xd, C);
  rows_f32(kOp, out, xd, R, C, "out");
  per_head(kOp, stat_m, xd, R, heads, lds, "stat_m");
  per_head(kOp, stat_l, xd, R, heads, lds, "stat_l");
  if (R == 0) return;
  if (s.rows == 0) {  // nothing to gather from: every row is empty
    TORCH_CHECK(col.numel() == 0, "gatv2: entries but no source rows");
    at::Tensor o = out.narrow(0, 0, R);
    if (beta == 0.0) o.zero_(); else o.mul_(beta);
    stat_l.narrow(0, 0, R).zero_();
    return;
  }
  DG_HIP_CHECK(gatv2_fwd_f32(it, rowptr.data_ptr<int64_t>(), col.data_ptr(), R, C,
                             static_cast<int>(heads), lds, static_cast<float>(slope), ap,
                             xd.data_ptr<float>(), xd.stride(0), s.xs, s.ldxs, s.xs2, s.ldxs2,
                             s.nsplit, out.data_ptr<float>(), out.stride(0),
                             static_cast<float>(beta), stat_m.data_ptr<float>(),
                             stat_l.data_ptr<float>(), cur_stream(xd)));
}

// da_part: contiguous [gatv2_da_parts(R, C), C]; every row is written
void gatv2_bwd_dst_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& xd,
                      const at::Tensor& xs, const c10::optional<at::Tensor>& xs2,
                      int64_t nsplit, const at::Tensor& att, const at::Tensor& stat_m,
                      const at::Tensor& stat_l, const at::Tensor& g, const at::Tensor& c,
                      at::Tensor& dxd, at::Tensor& da_part, int64_t heads, double slope) {
  const c10::DeviceGuard guard(xd.device());
  const int C = width(xd, heads);
  const IType it = pattern(kOp, rowptr, col, xd);
  const int64_t R = rowptr.numel() - 1;
  const int64_t lds = stat_m.dim() == 2 ? stat_m.stride(0) : 0;
  rows_f32(kOp, xd, xd, R, C, "xd");
  const Sources s = sources(xd, xs, xs2, nsplit, C);
  const float* ap = att_vec(att, xd, C);
  per_head(kOp, stat_m, xd, R, heads, lds, "stat_m");
  per_head(kOp, stat_l, xd, R, heads, lds, "stat_l");
  per_head(kOp, c, xd, R, heads, lds, "c");
  rows_f32(kOp, g, xd, R, C, "g");
  rows_f32(kOp, dxd, xd, R, C, "dxd");
  const int64_t P = gatv2_da_parts(R, C);
  TORCH_CHECK(da_part.is_cuda() && da_part.device() == xd.device() &&
                  da_part.scalar_type() == at::kFloat && da_part.dim() == 2 &&
                  da_part.size(0) == P && da_part.size(1) == C &&
                  (P == 0 || (da_part.is_contiguous() && al16(da_part.data_ptr()))),
              "gatv2: da_part must be contiguous, 16-B aligned float32 [", P, ", ", C, "] on ",
              xd.device(), ", got ", da_part.sizes());
  if (R == 0) return;
  if (s.rows == 0) {
    TORCH_CHECK(col.numel() == 0, "gatv2: entries but no source rows");
    dxd.narrow(0, 0, R).zero_();
    da_part.zero_();
    return;
  }
  DG_HIP_CHECK(gatv2_bwd_dst_f32(it, rowptr.data_ptr<int64_t>(), col.data_ptr(), R, C,
                                 static_cast<int>(heads), lds, static_cast<float>(slope), ap,
                                 xd.data_ptr<float>(), xd.stride(0), s.xs, s.ldxs, s.xs2,
                                 s.ldxs2, s.nsplit, stat_m.data_ptr<float>(),
                                 stat_l.data_ptr<float>(), g.data_ptr<float>(), g.stride(0),
                                 c.data_ptr<float>(), dxd.data_ptr<float>(), dxd.stride(0),
                                 da_part.data_ptr<float>(), cur_stream(xd)));
}

// rows = source rows (the transposed pattern; xs, dxs); col = destination rows
void gatv2_bwd_src_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& xd,
                      const at::Tensor& g, const at::Tensor& xs, const at::Tensor& att,
                      const at::Tensor& stat_m, const at::Tensor& stat_l, const at::Tensor& c,
                      at::Tensor& dxs, int64_t heads, double slope) {
  const c10::DeviceGuard guard(xd.device());
  const int C = width(xd, heads);
  const IType it = pattern(kOp, rowptr, col, xd);
  const int64_t R = rowptr.numel() - 1;
  const int64_t nd = xd.size(0);
  const int64_t lds = stat_m.dim() == 2 ? stat_m.stride(0) : 0;
  rows_f32(kOp, xd, xd, 0, C, "xd");
  rows_f32(kOp, g, xd, nd, C, "g");
  const float* ap = att_vec(att, xd, C);
  per_head(kOp, stat_m, xd, nd, heads, lds, "stat_m");
  per_head(kOp, stat_l, xd, nd, heads, lds, "stat_l");
  per_head(kOp, c, xd, nd, heads, lds, "c");
  rows_f32(kOp, xs, xd, R, C, "xs");
  rows_f32(kOp, dxs, xd, R, C, "dxs");
  if (R == 0) return;
  if (nd == 0) {  // no destination rows: no entries, every source row's gradient is 0
    TORCH_CHECK(col.numel() == 0, "gatv2: entries but no destination rows");
    dxs.narrow(0, 0, R).zero_();
    return;
  }
  DG_HIP_CHECK(gatv2_bwd_src_f32(it, rowptr.data_ptr<int64_t>(), col.data_ptr(), R, C,
                                 static_cast<int>(heads), lds, static_cast<float>(slope), ap,
                                 xd.data_ptr<float>(), xd.stride(0), g.data_ptr<float>(),
                                 g.stride(0), xs.data_ptr<float>(), xs.stride(0),
                                 stat_m.data_ptr<float>(), stat_l.data_ptr<float>(),
                                 c.data_ptr<float>(), dxs.data_ptr<float>(), dxs.stride(0),
                                 cur_stream(xd)));
}

// rows of da_part for a relation of R destination rows at width C (no device work)
int64_t gatv2_da_parts_op(int64_t R, int64_t C) {
  TORCH_CHECK(R >= 0 && C > 0 && C <= 256 && C % 4 == 0, "gatv2: bad (R, C) = (", R, ", ", C,
              ")");
  return gatv2_da_parts(R, static_cast<int>(C));
}

}  // namespace
}  // namespace dgraph

TORCH_LIBRARY_FRAGMENT(dgraph_amd, m) {
  m.def("gatv2_fwd_f32(Tensor rowptr, Tensor col, Tensor xd, Tensor xs, Tensor? xs2, "
        "int nsplit, Tensor att, Tensor(a!) out, float beta, Tensor(b!) stat_m, "
        "Tensor(c!) stat_l, int heads, float slope) -> ()");
  m.def("gatv2_bwd_dst_f32(Tensor rowptr, Tensor col, Tensor xd, Tensor xs, Tensor? xs2, "
        "int nsplit, Tensor att, Tensor stat_m, Tensor stat_l, Tensor g, Tensor c, "
        "Tensor(a!) dxd, Tensor(b!) da_part, int heads, float slope) -> ()");
  m.def("gatv2_bwd_src_f32(Tensor rowptr, Tensor col, Tensor xd, Tensor g, Tensor xs, "
        "Tensor att, Tensor stat_m, Tensor stat_l, Tensor c, Tensor(a!) dxs, int heads, "
        "float slope) -> ()");
  m.def("gatv2_da_parts(int R, int C) -> int", &dgraph::gatv2_da_parts_op);
}

TORCH_LIBRARY_IMPL(dgraph_amd, CUDA, m) {
  m.impl("gatv2_fwd_f32", &dgraph::gatv2_fwd_op);
  m.impl("gatv2_bwd_dst_f32", &dgraph::gatv2_bwd_dst_op);
  m.impl("gatv2_bwd_src_f32", &dgraph::gatv2_bwd_src_op);
}
