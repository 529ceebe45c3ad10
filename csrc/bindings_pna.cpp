// dgraph_amd — dispatcher registration of the fused PNA statistics kernels
// (csrc/kernels/spmm_pna.hip; ops/kernels.py: segment_pna / segment_pna_bwd). Every shape,
// dtype, device, stride and alignment contract the kernels rely on is checked here. The
// vector width follows from the row width: VEC = 4 (16-B accesses) when F is a multiple of
// 4, else 1; every array then needs a row stride that is a multiple of VEC and a base
// aligned to VEC elements, and one that is not raises here instead of running four times
// as many loads. Column ids are the caller's contract, as for segment_extreme.
//
// Zero rows and zero F return at once. A pattern with rows and no entries is legal (x may
// then have no rows): the launched kernel reads neither col nor x and writes the empty-row
// results, which a first-source pass owes its caller.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/library.h>

#include "check.h"
#include "kernels/kernels.h"

namespace dgraph {
namespace {

using OptT = c10::optional<at::Tensor>;

hipStream_t cur_stream(const at::Tensor& t) {
  return c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

const at::Tensor* opt_t(const OptT& t) { return (t.has_value() && t->defined()) ? &*t : nullptr; }

// [rows >= min_rows, F] of `type`, on ref's device, unit column stride, rows not overlapping
void rows_of(const at::Tensor& t, const at::Tensor& ref, at::ScalarType type, int64_t min_rows,
             int64_t F, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), "segment_pna: ", name, " must be on ",
              ref.device());
  TORCH_CHECK(t.scalar_type() == type, "segment_pna: ", name, " must be ", type, ", got ",
              t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.size(1) == F && t.size(0) >= min_rows, "segment_pna: ", name,
              " must be [>= ", min_rows, ", ", F, "], got ", t.sizes());
  if (t.size(0) == 0 || F == 0) return;
  TORCH_CHECK(t.stride(1) == 1 || F == 1, "segment_pna: ", name,
              " must have unit column stride, got strides ", t.strides());
  TORCH_CHECK(t.size(0) == 1 || t.stride(0) >= F, "segment_pna: ", name, " has a row stride ",
              t.stride(0), " below its width ", F);
  if (F % 4 == 0)
    TORCH_CHECK((t.size(0) == 1 || t.stride(0) % 4 == 0) &&
                    reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                "segment_pna: ", name, " (width ", F, ", a multiple of 4) needs a row stride "
                "divisible by 4 and a 16-B aligned base, got strides ", t.strides());
}

IType pattern(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& ref,
              const char* what) {
  TORCH_CHECK(rowptr.is_cuda() && rowptr.device() == ref.device() &&
                  rowptr.scalar_type() == at::kLong && rowptr.is_contiguous() &&
                  rowptr.dim() == 1 && rowptr.numel() >= 1,
              "segment_pna: ", what, " rowptr must be contiguous int64 on ", ref.device());
  TORCH_CHECK(col.is_cuda() && col.device() == ref.device() && col.is_contiguous() &&
                  col.dim() == 1 &&
                  (col.scalar_type() == at::kInt || col.scalar_type() == at::kLong),
              "segment_pna: ", what, " col must be contiguous int32/int64 on ", ref.device());
  return col.scalar_type() == at::kInt ? IType::I32 : IType::I64;
}

struct F32Rows {
  float* p = nullptr;
  int64_t ld = 0;
};
struct I32Rows {
  int32_t* p = nullptr;
  int64_t ld = 0;
};

F32Rows f32_rows(const at::Tensor* t, const at::Tensor& ref, int64_t min_rows, int64_t F,
                 const char* name) {
  if (t == nullptr) return {};
  rows_of(*t, ref, at::kFloat, min_rows, F, name);
  return {t->data_ptr<float>(), t->stride(0)};
}

I32Rows i32_rows(const at::Tensor* t, const at::Tensor& ref, int64_t min_rows, int64_t F,
                 const char* name) {
  if (t == nullptr) return {};
  rows_of(*t, ref, at::kInt, min_rows, F, name);
  return {t->data_ptr<int32_t>(), t->stride(0)};
}

void segment_pna_fwd_op(const at::Tensor& rowptr, const at::Tensor& col, const at::Tensor& x,
                        const OptT& mean, const OptT& sdev, const OptT& vmax, const OptT& amax,
                        const OptT& vmin, const OptT& amin, double eps, bool second, bool final,
                        const OptT& prev_rowptr, const OptT& row_map) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2, "segment_pna: x must be a 2-D GPU tensor");
  const c10::DeviceGuard guard(x.device());
  const int64_t F = x.size(1);
  rows_of(x, x, at::kFloat, 0, F, "x");
  const IType it = pattern(rowptr, col, x, "");
  const int64_t nrows = rowptr.numel() - 1;
  const at::Tensor *pm = opt_t(mean), *ps = opt_t(sdev), *px = opt_t(vmax), *pax = opt_t(amax),
                   *pn = opt_t(vmin), *pan = opt_t(amin);
  TORCH_CHECK((pm == nullptr) == (ps == nullptr), "segment_pna: mean and sdev come together");
  TORCH_CHECK((px == nullptr) == (pax == nullptr), "segment_pna: vmax and amax come together");
  TORCH_CHECK((pn == nullptr) == (pan == nullptr), "segment_pna: vmin and amin come together");
  TORCH_CHECK(eps >= 0.0, "segment_pna: eps must be >= 0");
  // output rows: the CSR rows, or wherever row_map sends them
  const int64_t* rmap = nullptr;
  int64_t min_rows = nrows;
  if (const at::Tensor* rm = opt_t(row_map)) {
    TORCH_CHECK(rm->is_cuda() && rm->device() == x.device() && rm->scalar_type() == at::kLong &&
                    rm->is_contiguous() && rm->numel() == nrows,
                "segment_pna: row_map must be contiguous int64 [nrows] on ", x.device());
    rmap = rm->data_ptr<int64_t>();
    min_rows = 0;  // the map's values are the caller's contract, as for segment_extreme
  }
  const F32Rows m = f32_rows(pm, x, min_rows, F, "mean");
  const F32Rows s = f32_rows(ps, x, min_rows, F, "sdev");
  const F32Rows vx = f32_rows(px, x, min_rows, F, "vmax");
  const F32Rows vn = f32_rows(pn, x, min_rows, F, "vmin");
  const I32Rows ax = i32_rows(pax, x, min_rows, F, "amax");
  const I32Rows an = i32_rows(pan, x, min_rows, F, "amin");
  const int64_t* prev = nullptr;
  if (second && pm != nullptr) {
    const at::Tensor* pr = opt_t(prev_rowptr);
    TORCH_CHECK(pr != nullptr, "segment_pna: a second pass over moments needs prev_rowptr");
    TORCH_CHECK(pr->is_cuda() && pr->device() == x.device() && pr->scalar_type() == at::kLong &&
                    pr->is_contiguous() && pr->dim() == 1 &&
                    pr->numel() == pm->size(0) + 1 && ps->size(0) == pm->size(0),
                "segment_pna: prev_rowptr must be contiguous int64 [output rows + 1] on ",
                x.device());
    prev = pr->data_ptr<int64_t>();
  }
  if (nrows <= 0 || F == 0) return;
  TORCH_CHECK(col.numel() == 0 || x.size(0) > 0, "segment_pna: entries but no source rows");
  // arg holds offsets within a row as int32 (and -2 - offset): every row must have fewer
  // than 2^31 - 2 entries. Certain when the whole CSR does; else look at the degrees.
  constexpr int64_t kMaxDeg = (int64_t(1) << 31) - 3;
  if (col.numel() > kMaxDeg) {
    const int64_t deg = (rowptr.slice(0, 1) - rowptr.slice(0, 0, nrows)).max().item<int64_t>();
    TORCH_CHECK(deg <= kMaxDeg, "segment_pna: a row of ", deg,
                " entries does not fit the int32 winner offset");
  }
  DG_HIP_CHECK(segment_pna_fwd(it, rowptr.data_ptr<int64_t>(), col.data_ptr(),
                               x.data_ptr<float>(), x.stride(0), m.p, m.ld, s.p, s.ld, vx.p,
                               vx.ld, ax.p, ax.ld, vn.p, vn.ld, an.p, an.ld, nrows,
                               static_cast<int>(F), static_cast<float>(eps), second, final, prev,
                               rmap, cur_stream(x)));
}

void segment_pna_bwd_op(const at::Tensor& t_rowptr, const at::Tensor& t_col,
                        const at::Tensor& rel, const at::Tensor& x, const OptT& inv_deg,
                        const OptT& g_mean, const OptT& g_std, const OptT& mean,
                        const OptT& sdev, const OptT& g_max, const OptT& amax,
                        const OptT& g_min, const OptT& amin, at::Tensor& out, bool halo,
                        double beta) {
  TORCH_CHECK(out.is_cuda() && out.dim() == 2, "segment_pna: out must be a 2-D GPU tensor");
  const c10::DeviceGuard guard(out.device());
  const int64_t F = out.size(1);
  const IType it = pattern(t_rowptr, t_col, out, "transposed");
  const int64_t nrows = t_rowptr.numel() - 1;
  TORCH_CHECK(rel.is_cuda() && rel.device() == out.device() && rel.scalar_type() == at::kInt &&
                  rel.is_contiguous() && rel.numel() == t_col.numel(),
              "segment_pna: rel must be contiguous int32, one per transposed entry");
  rows_of(out, out, at::kFloat, nrows, F, "out");
  rows_of(x, out, at::kFloat, nrows, F, "x");
  const at::Tensor *gm = opt_t(g_mean), *gs = opt_t(g_std), *gx = opt_t(g_max),
                   *gn = opt_t(g_min);
  // destination rows: every array the transposed column ids index has the same row count
  int64_t nd = -1;
  for (const at::Tensor* t : {gm, gs, gx, gn})
    if (t != nullptr) {
      TORCH_CHECK(nd < 0 || t->size(0) == nd, "segment_pna: g_* row counts differ");
      nd = t->size(0);
    }
  F32Rows a_gm = f32_rows(gm, out, 0, F, "g_mean"), a_gs = f32_rows(gs, out, 0, F, "g_std");
  F32Rows a_gx = f32_rows(gx, out, 0, F, "g_max"), a_gn = f32_rows(gn, out, 0, F, "g_min");
  F32Rows a_m, a_s;
  I32Rows a_ax, a_an;
  const float* inv = nullptr;
  if (gm != nullptr || gs != nullptr) {
    const at::Tensor* iv = opt_t(inv_deg);
    TORCH_CHECK(iv != nullptr && iv->is_cuda() && iv->device() == out.device() &&
                    iv->scalar_type() == at::kFloat && iv->is_contiguous() && iv->numel() == nd,
                "segment_pna: inv_deg must be contiguous float32, one per destination row");
    inv = iv->data_ptr<float>();
  }
  if (gs != nullptr) {
    TORCH_CHECK(opt_t(mean) && opt_t(sdev), "segment_pna: g_std needs mean and sdev");
    a_m = f32_rows(opt_t(mean), out, nd, F, "mean");
    a_s = f32_rows(opt_t(sdev), out, nd, F, "sdev");
  }
  if (gx != nullptr) {
    TORCH_CHECK(opt_t(amax), "segment_pna: g_max needs amax");
    a_ax = i32_rows(opt_t(amax), out, nd, F, "amax");
  }
  if (gn != nullptr) {
    TORCH_CHECK(opt_t(amin), "segment_pna: g_min needs amin");
    a_an = i32_rows(opt_t(amin), out, nd, F, "amin");
  }
  if (nrows <= 0 || F == 0) return;
  if (nd <= 0) {  // no destination rows (or no gradient at all): no entry contributes
    TORCH_CHECK(nd < 0 || t_col.numel() == 0, "segment_pna: entries but no destination rows");
    at::Tensor o = out.narrow(0, 0, nrows);
    if (beta == 0.0) o.zero_(); else o.mul_(beta);
    return;
  }
  DG_HIP_CHECK(segment_pna_bwd(it, t_rowptr.data_ptr<int64_t>(), t_col.data_ptr(),
                               rel.data_ptr<int32_t>(), x.data_ptr<float>(), x.stride(0), inv,
                               a_gm.p, a_gm.ld, a_gs.p, a_gs.ld, a_m.p, a_m.ld, a_s.p, a_s.ld,
                               a_gx.p, a_gx.ld, a_ax.p, a_ax.ld, a_gn.p, a_gn.ld, a_an.p,
                               a_an.ld, out.data_ptr<float>(), out.stride(0), nrows,
                               static_cast<int>(F), halo, static_cast<float>(beta),
                               cur_stream(out)));
}

}  // namespace
}  // namespace dgraph

TORCH_LIBRARY_FRAGMENT(dgraph_amd, m) {
  m.def("segment_pna_fwd(Tensor rowptr, Tensor col, Tensor x, Tensor(a!)? mean, "
        "Tensor(b!)? sdev, Tensor(c!)? vmax, Tensor(d!)? amax, Tensor(e!)? vmin, "
        "Tensor(f!)? amin, float eps, bool second, bool final, Tensor? prev_rowptr, "
        "Tensor? row_map) -> ()");
  m.def("segment_pna_bwd(Tensor t_rowptr, Tensor t_col, Tensor rel, Tensor x, Tensor? inv_deg, "
        "Tensor? g_mean, Tensor? g_std, Tensor? mean, Tensor? sdev, Tensor? g_max, "
        "Tensor? amax, Tensor? g_min, Tensor? amin, Tensor(a!) out, bool halo, float beta) "
        "-> ()");
}

TORCH_LIBRARY_IMPL(dgraph_amd, CUDA, m) {
  m.impl("segment_pna_fwd", &dgraph::segment_pna_fwd_op);
  m.impl("segment_pna_bwd", &dgraph::segment_pna_bwd_op);
}
