// dgraph_amd — dispatcher registration of the relation-attention kernels with bf16 storage
// (csrc/kernels/gat_bf16.hip; the bf16 lean RGAT layer, ops/gat.py). Every dtype, shape,
// stride and 16-B alignment the kernels rely on is checked here; column ids are checked
// against the operand rows once per pattern by the Python caller (ops/gat.py: GatPattern).
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <torch/library.h>

#include "attn_check.h"
#include "check.h"
#include "kernels/kernels.h"

namespace dgraph {
namespace {

constexpr const char* kOp = "gat_bf16";  // the prefix of every message

// int32 columns only: GatPattern builds nothing else
const int32_t* pattern32(const at::Tensor& rowptr, const at::Tensor& col,
                         const at::Tensor& ref) {
  pattern(kOp, rowptr, col, ref);
  TORCH_CHECK(col.scalar_type() == at::kInt,
              "gat_bf16: col must be int32 (GatPattern's index type), got ", col.scalar_type());
  return col.data_ptr<int32_t>();
}

int width(const at::Tensor& z, int64_t heads) {
  TORCH_CHECK(z.dim() == 2, "gat_bf16: z must be 2-D");
  const int C = static_cast<int>(z.size(1));
  TORCH_CHECK(gat_bf16_shape_ok(C, static_cast<int>(heads)), "gat_bf16: unsupported width ", C,
              " / heads ", heads, " (C in 64/128/256, heads in 1/2/4/8)");
  return C;
}

// contiguous [>= min_rows, heads] float32
void heads_f32(const at::Tensor& t, const at::Tensor& ref, int64_t min_rows, int64_t heads,
               const char* name) {
  per_head(kOp, t, ref, min_rows, heads, heads, name);
}

const float* att_vec(const at::Tensor& a_src, const at::Tensor& ref, int C) {
  TORCH_CHECK(a_src.is_cuda() && a_src.device() == ref.device() &&
                  a_src.scalar_type() == at::kFloat && a_src.dim() == 1 &&
                  a_src.is_contiguous() && a_src.numel() == C && al16(a_src.data_ptr()),
              "gat_bf16: a_src must be contiguous float32 [", C, "], 16-B aligned, on ",
              ref.device());
  return a_src.data_ptr<float>();
}

struct Sources {
  const uint16_t *z, *zh;
  int64_t ldz, ldzh, nsplit;
};

// z serves columns < nsplit (all of them without zh), zh the columns from nsplit on; row 0 of
// z must exist
Sources sources(const at::Tensor& z, const c10::optional<at::Tensor>& zh, int64_t nsplit,
                int C) {
  rows_bf16(kOp, z, z, 1, C, "z");
  TORCH_CHECK(nsplit >= 0 && nsplit < (int64_t(1) << 31), "gat_bf16: bad nsplit");
  Sources s{bf16_ptr(z), nullptr, z.stride(0), 0, 0};
  if (const at::Tensor* p = opt_t(zh)) {
    rows_bf16(kOp, *p, z, 0, C, "zh");
    TORCH_CHECK(z.size(0) >= nsplit, "gat_bf16: z has fewer rows than nsplit");
    if (p->size(0) > 0) {
      s.zh = bf16_ptr(*p);
      s.ldzh = p->stride(0);
      s.nsplit = nsplit;
    }
  }
  return s;
}

// sd / out rows = CSR rows; z (+ zh past nsplit) = the gathered rows
void gat_fwd_bf16_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& z,
                     const c10::optional<at::Tensor>& zh, int64_t nsplit,
                     const at::Tensor& a_src, const at::Tensor& sd, at::Tensor& out,
                     double beta, at::Tensor& stat_m, at::Tensor& stat_l, int64_t heads,
                     double slope) {
  const c10::DeviceGuard guard(z.device());
  const int C = width(z, heads);
  const int32_t* cp = pattern32(rowptr, col, z);
  const int64_t R = rowptr.numel() - 1;
  const Sources s = sources(z, zh, nsplit, C);
  const float* ap = att_vec(a_src, z, C);
  heads_f32(sd, z, R, heads, "sd");
  rows_bf16(kOp, out, z, R, C, "out");
  heads_f32(stat_m, z, R, heads, "stat_m");
  heads_f32(stat_l, z, R, heads, "stat_l");
  DG_HIP_CHECK(gat_fwd_bf16(rowptr.data_ptr<int64_t>(), cp, R, C, static_cast<int>(heads),
                            static_cast<float>(slope), s.z, s.ldz, s.zh, s.ldzh, s.nsplit, ap,
                            sd.data_ptr<float>(),
                            reinterpret_cast<uint16_t*>(out.data_ptr()), out.stride(0),
                            static_cast<float>(beta), stat_m.data_ptr<float>(),
                            stat_l.data_ptr<float>(), cur_stream(z)));
}

void gat_bwd_dst_bf16_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& z,
                         const c10::optional<at::Tensor>& zh, int64_t nsplit,
                         const at::Tensor& a_src, const at::Tensor& sd,
                         const at::Tensor& stat_m, const at::Tensor& stat_l,
                         const at::Tensor& g, at::Tensor& c_out, at::Tensor& gsd_out,
                         int64_t heads, double slope) {
  const c10::DeviceGuard guard(z.device());
  const int C = width(z, heads);
  const int32_t* cp = pattern32(rowptr, col, z);
  const int64_t R = rowptr.numel() - 1;
  const Sources s = sources(z, zh, nsplit, C);
  const float* ap = att_vec(a_src, z, C);
  heads_f32(sd, z, R, heads, "sd");
  heads_f32(stat_m, z, R, heads, "stat_m");
  heads_f32(stat_l, z, R, heads, "stat_l");
  rows_bf16(kOp, g, z, R, C, "g");
  heads_f32(c_out, z, R, heads, "c_out");
  heads_f32(gsd_out, z, R, heads, "gsd_out");
  DG_HIP_CHECK(gat_bwd_dst_bf16(rowptr.data_ptr<int64_t>(), cp, R, C, static_cast<int>(heads),
                                static_cast<float>(slope), s.z, s.ldz, s.zh, s.ldzh, s.nsplit,
                                ap, sd.data_ptr<float>(), stat_m.data_ptr<float>(),
                                stat_l.data_ptr<float>(), bf16_ptr(g), g.stride(0),
                                c_out.data_ptr<float>(), gsd_out.data_ptr<float>(),
                                cur_stream(z)));
}

// rows = source rows (the transposed pattern; z, gz, gss); col = destination rows (g, sd,
// m_dst, l_dst, c_dst). da_part: contiguous [gat_bf16_da_parts(R, C), C]; every row is written
void gat_bwd_src_bf16_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& g,
                         const at::Tensor& z, const at::Tensor& a_src, const at::Tensor& sd,
                         const at::Tensor& m_dst, const at::Tensor& l_dst,
                         const at::Tensor& c_dst, at::Tensor& gz, at::Tensor& gss,
                         at::Tensor& da_part, int64_t heads, double slope) {
  const c10::DeviceGuard guard(g.device());
  const int C = width(g, heads);
  const int32_t* cp = pattern32(rowptr, col, g);
  const int64_t R = rowptr.numel() - 1;
  const int64_t nd = g.size(0);
  rows_bf16(kOp, g, g, R > 0 ? 1 : 0, C, "g");
  rows_bf16(kOp, z, g, R, C, "z");
  const float* ap = att_vec(a_src, g, C);
  heads_f32(sd, g, nd, heads, "sd");
  heads_f32(m_dst, g, nd, heads, "m_dst");
  heads_f32(l_dst, g, nd, heads, "l_dst");
  heads_f32(c_dst, g, nd, heads, "c_dst");
  rows_bf16(kOp, gz, g, R, C, "gz");
  heads_f32(gss, g, R, heads, "gss");
  const int64_t P = gat_bf16_da_parts(R, C);
  TORCH_CHECK(da_part.is_cuda() && da_part.device() == g.device() &&
                  da_part.scalar_type() == at::kFloat && da_part.dim() == 2 &&
                  da_part.size(0) == P && da_part.size(1) == C &&
                  (P == 0 || (da_part.is_contiguous() && al16(da_part.data_ptr()))),
              "gat_bf16: da_part must be contiguous, 16-B aligned float32 [", P, ", ", C,
              "] on ", g.device(), ", got ", da_part.sizes());
  DG_HIP_CHECK(gat_bwd_src_bf16(rowptr.data_ptr<int64_t>(), cp, R, C, static_cast<int>(heads),
                                static_cast<float>(slope), bf16_ptr(g), g.stride(0),
                                bf16_ptr(z), z.stride(0), ap, sd.data_ptr<float>(),
                                m_dst.data_ptr<float>(), l_dst.data_ptr<float>(),
                                c_dst.data_ptr<float>(),
                                reinterpret_cast<uint16_t*>(gz.data_ptr()), gz.stride(0),
                                gss.data_ptr<float>(), da_part.data_ptr<float>(),
                                cur_stream(g)));
}

// rows of da_part for R source rows at width C (no device work)
int64_t gat_bf16_da_parts_op(int64_t R, int64_t C) {
  TORCH_CHECK(R >= 0 && C > 0 && C <= 256 && C % 8 == 0, "gat_bf16: bad (R, C) = (", R, ", ",
              C, ")");
  return gat_bf16_da_parts(R, static_cast<int>(C));
}

}  // namespace
}  // namespace dgraph

TORCH_LIBRARY_FRAGMENT(dgraph_amd, m) {
  m.def("gat_fwd_bf16(Tensor rowptr, Tensor col, Tensor z, Tensor? zh, int nsplit, "
        "Tensor a_src, Tensor sd, Tensor(a!) out, float beta, Tensor(b!) stat_m, "
        "Tensor(c!) stat_l, int heads, float slope) -> ()");
  m.def("gat_bwd_dst_bf16(Tensor rowptr, Tensor col, Tensor z, Tensor? zh, int nsplit, "
        "Tensor a_src, Tensor sd, Tensor stat_m, Tensor stat_l, Tensor g, Tensor(a!) c_out, "
        "Tensor(b!) gsd_out, int heads, float slope) -> ()");
  m.def("gat_bwd_src_bf16(Tensor rowptr, Tensor col, Tensor g, Tensor z, Tensor a_src, "
        "Tensor sd, Tensor m_dst, Tensor l_dst, Tensor c_dst, Tensor(a!) gz, Tensor(b!) gss, "
        "Tensor(c!) da_part, int heads, float slope) -> ()");
  m.def("gat_bf16_da_parts(int R, int C) -> int", &dgraph::gat_bf16_da_parts_op);
}

TORCH_LIBRARY_IMPL(dgraph_amd, CUDA, m) {
  m.impl("gat_fwd_bf16", &dgraph::gat_fwd_bf16_op);
  m.impl("gat_bwd_dst_bf16", &dgraph::gat_bwd_dst_bf16_op);
  m.impl("gat_bwd_src_bf16", &dgraph::gat_bwd_src_bf16_op);
}
