// dgraph_amd — fused gated neighbourhood aggregation with bf16 storage for gfx950.
// The contract is spmm_gated.hip's:
//
//   out[r, f] = sum_j s_j v[c_j, f],   s_j = sigmoid(k[r, f] + q[c_j, f])   over CSR row r
//   ds [r, f] = sum_j s_j (1 - s_j) v[c_j, f]                  (the saved state: dk = g * ds)
//   dv[c, f]  = sum_r s g[r, f],   dq[c, f] = v[c, f] sum_r s (1 - s) g[r, f]   (transposed)
//
// k, q, v, g are bf16; the outputs are bf16 or fp32 (a template parameter). All arithmetic and
// accumulation is fp32: a bf16 value is widened by a 16-bit shift and every stored value is
// rounded ONCE, to nearest even, at the store. The second pass of two sources (accumulate: the
// halo block after the interior block) therefore exists for fp32 outputs only: it reads the
// earlier sums, adds its own and the caller casts once at the end; an accumulated bf16 out
// would round twice and is refused (bindings_gated_bf16.cpp).
//
// This is not spmm_gated.hip with the type swapped:
//
// * Layout (gatv2_bf16.hip's and the bf16 row-group SpMM's): eight channels per lane, ONE 16-B
//   load per lane per gathered row; one group of LPR lanes (8 / 16 / 32 / 64, the smallest
//   that holds F / 8 lanes) owns an output row and a wave holds 64 / LPR rows, so a row's sum
//   never crosses lanes: no butterfly, no LDS, one summation order. The fp32 kernels give a
//   whole wave to a row, split its entries over the lane groups and add the groups by
//   shuffles. Widths above 8 LPR = 512 take column passes; lanes past F read column 0 and
//   store nothing. Every operand has its own row stride (a multiple of 8 elements), so k and
//   [q | v] stay column views of the layer's one [N, 3F] projection buffer.
// * Forward: k[r] is unpacked once per row and column pass and stays resident. The group's
//   lanes load LPR column ids at once and hand them round by shuffle; kU entries are in
//   flight, each a raw 16-B q vector and a raw 16-B v vector, unpacked on use. The groups of
//   a wave run to the wave's longest row: a slot past a row's end gathers row 0 (the loads of
//   a batch stay one straight run) and its arithmetic is predicated off, so whatever row 0
//   holds (an Inf, a NaN) reaches no other row and a finished group spends no lane cycles.
// * The gate is gate() of the fp32 file: e = exp(-|z|), r = 1 / (1 + e), s = z >= 0 ? r : e r
//   and s (1 - s) = e r^2, never s - s^2: one v_exp_f32 and one v_rcp_f32 per element, finite
//   for every finite z, the derivative exact in both tails.
// * Source-side backward: the same walk over the transposed pattern with q[c] resident, raw
//   k[r] and g[r] vectors in flight; dv += s g, a += s (1 - s) g; v[c] is read at the row's
//   end for dq = v[c] a. Every row c < nrows is written.
//
// No atomics, fixed summation order: two calls give equal bits, and int32 and int64 column
// ids give equal bits. An empty row stores exact zeros (and is not touched by an accumulate
// pass). The launchers need row 0 of the gathered arrays to exist; the bindings launch only
// when the pattern has entries.
//
// Compiler resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=
// kernel-resource-usage; the 48 instantiations at kU = 8, built without packed-fp32
// instructions; VGPRs / waves per SIMD; int32 ids, int64 within 2 VGPRs and at the same
// occupancy; bf16 and fp32 outputs within 1 VGPR; scratch 0 B, no AGPRs, no LDS in all 48):
//              LPR 8      LPR 16     LPR 32     LPR 64
//   fwd        124 / 4    115 / 4    115 / 4    110 / 4
//   fwd + ds   139 / 3    125 / 4    125 / 4    118 / 4
//   bwd src    141 / 3    132 / 3    132 / 3    120 / 4
// At kU = 4 the same table reads 93 / 5, 84 / 5, 83 / 5, 78 / 6 (fwd), 113 / 4 .. 88 / 5
// (fwd + ds) and 115 / 4 .. 90 / 5 (bwd src), without scratch. kU = 8 is chosen: occupancy x
// gathered 16-B vectors in flight per SIMD lane is 64 / 48-64 / 48-64 at kU = 8 against 40-48
// / 32-40 / 32-40 at kU = 4 (the fp32 kernels: 32), and at LPR 8 a batch is one whole chunk
// of column ids. With packed-fp32 instructions the same source takes 112-128 VGPRs in fwd
// (occupancy 4), 122-146 in fwd + ds (3 at LPR 8-32 with fp32 outputs, where the plain build
// has 4 at LPR 16 / 32) and 124-148 in bwd src (3 / 4): never fewer, so the file is built
// without them (_build.py: EXTRA_FLAGS). The timing does not favour that choice: one run of
// each build (PERFORMANCE.md) has the packed build faster or equal in 13 of 15 cases, by 3 %
// at F = 64 with bf16 outputs (3.46 / 4.07 / 4.12 ms against 3.56 / 4.19 / 4.23 ms), 4 % in
// fwd + ds at F = 128 (7.31 against 7.61 ms), 6 % at F = 64 with fp32 outputs (4.25 / 4.29
// against 4.51 / 4.56 ms), within 1 % at F = 256, and 2 % slower in fwd at F = 128 (7.00
// against 6.86 ms); the untouched fp32 kernels moved by up to 3.5 % between the two runs.
//
// Measured on an MI355X (python benchmarks/bench_gated_aggr_bf16.py --rounds 5, ogbn-products
// shape, 2.45 M rows, 123.7 M entries; PERFORMANCE.md, gated aggregation in bf16), bf16 rows and
// bf16 outputs against the fp32 kernels in the same run, F = 64 / 128 / 256:
//   fwd        3.56 /  6.86 / 14.84 ms   fp32  8.95 / 19.44 / 42.32 ms   ratio 0.40 / 0.35 / 0.35
//   fwd + ds   4.19 /  7.61 / 15.05 ms   fp32  9.42 / 20.73 / 45.11 ms   ratio 0.44 / 0.37 / 0.33
//   bwd src    4.23 /  8.06 / 15.47 ms   fp32  9.56 / 20.98 / 44.92 ms   ratio 0.44 / 0.38 / 0.34
// = 7.9 .. 9.5 TB/s of the bytes each pass must move (fp32: 5.8 .. 7.3). The ratios are below
// the 0.5 of the halved bytes: a row per lane group needs no cross-lane sums and keeps eight
// rows' gathers of a wave in flight at F = 64. fp32 outputs plus the cast to bf16 (what a
// partition with a halo block runs) cost 1.08 / 1.10 / 1.10 of the direct bf16 store in
// fwd + ds and 1.08 / 1.08 / 1.10 in bwd src.
#include "attn_device.h"
#include "kernels.h"

namespace dgraph {
namespace {

struct GatedBf16Fwd {
  const int64_t* rowptr;
  const uint16_t* k;
  int64_t ldk;
  const uint16_t* q;
  int64_t ldq;
  const uint16_t* v;
  int64_t ldv;
  void* out;
  int64_t ldo;
  void* ds;
  int64_t ldds;
  int64_t nrows;
  int F;
  bool accumulate;
};

struct GatedBf16Bwd {
  const int64_t* rowptr;
  const uint16_t* k;
  int64_t ldk;
  const uint16_t* q;
  int64_t ldq;
  const uint16_t* v;
  int64_t ldv;
  const uint16_t* g;
  int64_t ldg;
  void* dq;
  int64_t lddq;
  void* dv;
  int64_t lddv;
  int64_t nrows;
  int F;
};

constexpr int kU = 8;  // entries in flight per lane (two raw 16-B vectors each)

// s = sigmoid(z) and d = s (1 - s) from e = exp(-|z|) in (0, 1]: 1 + e is in [1, 2], so the
// reciprocal neither overflows nor meets a denormal; e underflows to 0 for |z| > 88 or so
// and the results go to their limits (1 or 0, and 0)
template <bool DS>
__device__ __forceinline__ void gate(float z, float& s, float& d) {
  const float e = __expf(-fabsf(z));
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  const float er = e * r;
  s = z >= 0.f ? r : er;
  if (DS) d = er * r;
}

// acc += s w and, with DS, dac += s (1 - s) w per channel, z = a + b
template <bool DS>
__device__ __forceinline__ void gate4(const float4& a, const float4& b, const float4& w,
                                      float4& acc, float4& dac) {
  float s, d;
  gate<DS>(a.x + b.x, s, d);
  acc.x = fmaf(s, w.x, acc.x);
  if (DS) dac.x = fmaf(d, w.x, dac.x);
  gate<DS>(a.y + b.y, s, d);
  acc.y = fmaf(s, w.y, acc.y);
  if (DS) dac.y = fmaf(d, w.y, dac.y);
  gate<DS>(a.z + b.z, s, d);
  acc.z = fmaf(s, w.z, acc.z);
  if (DS) dac.z = fmaf(d, w.z, dac.z);
  gate<DS>(a.w + b.w, s, d);
  acc.w = fmaf(s, w.w, acc.w);
  if (DS) dac.w = fmaf(d, w.w, dac.w);
}

template <bool DS>
__device__ __forceinline__ void gate8(const f32x8& a, const f32x8& b, const f32x8& w,
                                      f32x8& acc, f32x8& dac) {
  gate4<DS>(a.lo, b.lo, w.lo, acc.lo, dac.lo);
  gate4<DS>(a.hi, b.hi, w.hi, acc.hi, dac.hi);
}

// A batch's raw vectors are unpacked one entry at a time, in order, as each is consumed. Left
// alone the compiler unpacks the whole batch ahead of the gates and holds 16 kU fp32 values
// next to the raw ones; behind this barrier an entry is eight shifts / masks away from its
// raw vector and the batch costs its 8 kU raw registers.
__device__ __forceinline__ const uint4& on_use(uint4& r) {
  asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w));
  return r;
}

__device__ __forceinline__ float4 mul4(const float4& a, const float4& b) {
  return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}

// the lane's eight sums to out[f .. f + 8): one rounding to bf16 (one 16-B store), or fp32 as
// they are (two 16-B stores), added to what an earlier pass left when ADD
template <typename OutT, bool ADD>
__device__ __forceinline__ void store8(void* base, int64_t off, f32x8 v) {
  if constexpr (sizeof(OutT) == 2) {
    *reinterpret_cast<uint4*>(static_cast<uint16_t*>(base) + off) = pack_bf16x8(v);
  } else {
    float4* p = reinterpret_cast<float4*>(static_cast<float*>(base) + off);
    if (ADD) {  // the earlier pass's result comes first
      v.lo = add4(p[0], v.lo);
      v.hi = add4(p[1], v.hi);
    }
    p[0] = v.lo;
    p[1] = v.hi;
  }
}

// what every kernel knows of its lane and of the row its group handles in one step
template <typename IdxT, int LPR>
struct Walk {
  static constexpr int G = kWave / LPR;
  int g, l;
  int64_t ngroups, q0, qstep;
  int64_t r, rr, s;  // rr: r, or 0 for a group past the last row (reads row 0, writes nothing)
  int deg, maxdeg;
  bool has_row;
  __device__ explicit Walk(int64_t nrows) {
    const int lane = threadIdx.x & (kWave - 1);
    g = lane / LPR;
    l = lane % LPR;
    ngroups = (nrows + G - 1) / G;
    q0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    qstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  }
  __device__ void row(const int64_t* rowptr, int64_t nrows, int64_t q) {
    r = q * G + g;
    has_row = r < nrows;
    rr = has_row ? r : 0;
    s = has_row ? rowptr[r] : 0;
    deg = has_row ? static_cast<int>(rowptr[r + 1] - s) : 0;
    maxdeg = group_imax<LPR>(deg);
  }
  // this lane's column id of the chunk that starts at entry k0 (0 past the row's end)
  __device__ IdxT chunk_col(const IdxT* col, int k0) const {
    return k0 + l < deg ? col[s + k0 + l] : IdxT(0);
  }
  // entry k0 + j of the group's row: its column id (0 past the end) and whether it exists
  __device__ int64_t entry(IdxT mine, int k0, int j, bool& ok) const {
    const IdxT c = __shfl(mine, g * LPR + j, kWave);
    ok = k0 + j < deg;
    return ok ? static_cast<int64_t>(c) : 0;
  }
  // The row's sums, shared by both kernels: per entry c, z = res + a[c] and acc += s w[c],
  // dac += s (1 - s) w[c] (a, w: this lane's channels of the two gathered arrays; res: the
  // resident row). The lanes load LPR ids at once and hand them round by shuffle; kU entries
  // (a raw a and a raw w vector each) are in flight; a slot past the row's end gathers row 0
  // and its arithmetic is predicated off.
  template <bool DS>
  __device__ __forceinline__ void sum_row(const IdxT* col, const uint16_t* a, int64_t lda,
                                          const uint16_t* w, int64_t ldw, const f32x8& res,
                                          f32x8& acc, f32x8& dac) const {
    constexpr int U = kU;
    static_assert(U <= LPR, "a batch stays inside one chunk of ids");
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const IdxT mine = chunk_col(col, k0);
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += U) {
        uint4 ra[U], rw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          bool ok;
          const int64_t c = entry(mine, k0, j0 + u, ok);
          ra[u] = load16(a + c * lda);
          rw[u] = load16(w + c * ldw);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (k0 + j0 + u < deg)
            gate8<DS>(res, unpack_bf16x8(on_use(ra[u])), unpack_bf16x8(on_use(rw[u])), acc, dac);
        }
      }
    }
  }
};

// ------------------------------------------------------------------------------------ fwd
template <typename IdxT, int LPR, bool DS, typename OutT>
__global__ __launch_bounds__(256) void segment_gated_bf16_fwd_kernel(
    const IdxT* __restrict__ col, const GatedBf16Fwd p) {
  constexpr bool ADD = sizeof(OutT) == 4;  // an accumulate pass exists for fp32 outputs only
  Walk<IdxT, LPR> t(p.nrows);
  for (int64_t qi = t.q0; qi < t.ngroups; qi += t.qstep) {
    t.row(p.rowptr, p.nrows, qi);
    const bool add = ADD && p.accumulate;
    // an accumulate pass with no entry in this row leaves the earlier result alone
    const bool write = t.has_row && !(add && t.deg == 0);
    for (int fc = 0; fc < p.F; fc += 8 * LPR) {
      const int f = fc + 8 * t.l;
      const bool active = f < p.F;
      // lanes past F read column 0 (no branch around the loads) and write nothing
      const int fa = active ? f : 0;
      const f32x8 kv = unpack_bf16x8(load16(p.k + t.rr * p.ldk + fa));
      f32x8 acc = zero8(), dac = zero8();
      t.template sum_row<DS>(col, p.q + fa, p.ldq, p.v + fa, p.ldv, kv, acc, dac);
      if (!(write && active)) continue;
      if (add) {
        store8<OutT, true>(p.out, t.r * p.ldo + f, acc);
        if (DS) store8<OutT, true>(p.ds, t.r * p.ldds + f, dac);
      } else {
        store8<OutT, false>(p.out, t.r * p.ldo + f, acc);
        if (DS) store8<OutT, false>(p.ds, t.r * p.ldds + f, dac);
      }
    }
  }
}

// -------------------------------------------------------------------------------- bwd src
template <typename IdxT, int LPR, typename OutT>
__global__ __launch_bounds__(256) void segment_gated_bf16_bwd_src_kernel(
    const IdxT* __restrict__ col, const GatedBf16Bwd p) {
  Walk<IdxT, LPR> t(p.nrows);
  for (int64_t qi = t.q0; qi < t.ngroups; qi += t.qstep) {
    t.row(p.rowptr, p.nrows, qi);
    for (int fc = 0; fc < p.F; fc += 8 * LPR) {
      const int f = fc + 8 * t.l;
      const bool active = f < p.F;
      const int fa = active ? f : 0;
      const f32x8 qc = unpack_bf16x8(load16(p.q + t.rr * p.ldq + fa));
      f32x8 av = zero8(), aq = zero8();
      t.template sum_row<true>(col, p.k + fa, p.ldk, p.g + fa, p.ldg, qc, av, aq);
      if (!(t.has_row && active)) continue;
      const f32x8 vc = unpack_bf16x8(load16(p.v + t.r * p.ldv + f));
      aq.lo = mul4(aq.lo, vc.lo);
      aq.hi = mul4(aq.hi, vc.hi);
      store8<OutT, false>(p.dv, t.r * p.lddv + f, av);
      store8<OutT, false>(p.dq, t.r * p.lddq + f, aq);
    }
  }
}

// one row group per wave, four waves per workgroup, in row order; past the cap the waves
// stride over the row groups
inline unsigned row_blocks(int64_t nrows, int LPR) {
  const int64_t G = kWave / LPR;
  const int64_t ngroups = (nrows + G - 1) / G;
  return static_cast<unsigned>(cap_blocks((ngroups + 3) / 4, int64_t(1) << 22));
}

inline int lanes_per_row(int F) {
  const int lanes = (F + 7) / 8;
  return lanes <= 8 ? 8 : lanes <= 16 ? 16 : lanes <= 32 ? 32 : 64;
}

template <typename IdxT, bool DS, typename OutT>
hipError_t launch_fwd(const IdxT* col, const GatedBf16Fwd& a, hipStream_t st) {
  const int LPR = lanes_per_row(a.F);
  const dim3 grid(row_blocks(a.nrows, LPR)), block(256);
#define DG_FWD(LPR_)                                                                   \
  if (LPR == LPR_) {                                                                   \
    hipLaunchKernelGGL((segment_gated_bf16_fwd_kernel<IdxT, LPR_, DS, OutT>), grid,    \
                       block, 0, st, col, a);                                          \
    return hipGetLastError();                                                          \
  }
  DG_FWD(8) DG_FWD(16) DG_FWD(32) DG_FWD(64)
#undef DG_FWD
  return hipErrorInvalidValue;
}

template <typename IdxT, typename OutT>
hipError_t launch_bwd(const IdxT* col, const GatedBf16Bwd& a, hipStream_t st) {
  const int LPR = lanes_per_row(a.F);
  const dim3 grid(row_blocks(a.nrows, LPR)), block(256);
#define DG_BWD(LPR_)                                                                   \
  if (LPR == LPR_) {                                                                   \
    hipLaunchKernelGGL((segment_gated_bf16_bwd_src_kernel<IdxT, LPR_, OutT>), grid,    \
                       block, 0, st, col, a);                                          \
    return hipGetLastError();                                                          \
  }
  DG_BWD(8) DG_BWD(16) DG_BWD(32) DG_BWD(64)
#undef DG_BWD
  return hipErrorInvalidValue;
}

template <typename IdxT, typename OutT>
hipError_t dispatch_fwd(const IdxT* c, const GatedBf16Fwd& a, hipStream_t st) {
  return a.ds != nullptr ? launch_fwd<IdxT, true, OutT>(c, a, st)
                         : launch_fwd<IdxT, false, OutT>(c, a, st);
}

// a row array of 16-B vectors: a 16-B aligned base and a row stride that keeps every row so
inline bool rows16(const void* p, int64_t ld, int elem_bytes) {
  return p == nullptr ||
         ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld * elem_bytes) % 16 == 0);
}

}  // namespace

hipError_t segment_gated_bf16_fwd(IType it, DType out_dt, const int64_t* rowptr,
                                  const void* col, const uint16_t* k, int64_t ldk,
                                  const uint16_t* q, int64_t ldq, const uint16_t* v,
                                  int64_t ldv, void* out, int64_t ldo, void* ds, int64_t ldds,
                                  int64_t nrows, int F, bool accumulate, hipStream_t stream) {
  if (nrows <= 0 || F <= 0) return hipSuccess;
  const int ob = out_dt == DType::F32 ? 4 : 2;
  if (k == nullptr || q == nullptr || v == nullptr || out == nullptr || F % 8 != 0 ||
      (accumulate && out_dt != DType::F32))
    return hipErrorInvalidValue;
  if (!(rows16(k, ldk, 2) && rows16(q, ldq, 2) && rows16(v, ldv, 2) && rows16(out, ldo, ob) &&
        rows16(ds, ldds, ob)))
    return hipErrorInvalidValue;
  const GatedBf16Fwd a{rowptr, k, ldk, q, ldq, v, ldv, out, ldo, ds, ldds, nrows, F, accumulate};
  if (it == IType::I32) {
    const auto* c = static_cast<const int32_t*>(col);
    return out_dt == DType::F32 ? dispatch_fwd<int32_t, float>(c, a, stream)
                                : dispatch_fwd<int32_t, uint16_t>(c, a, stream);
  }
  const auto* c = static_cast<const int64_t*>(col);
  return out_dt == DType::F32 ? dispatch_fwd<int64_t, float>(c, a, stream)
                              : dispatch_fwd<int64_t, uint16_t>(c, a, stream);
}

hipError_t segment_gated_bf16_bwd_src(IType it, DType out_dt, const int64_t* t_rowptr,
                                      const void* t_col, const uint16_t* k, int64_t ldk,
                                      const uint16_t* q, int64_t ldq, const uint16_t* v,
                                      int64_t ldv, const uint16_t* g, int64_t ldg, void* dq,
                                      int64_t lddq, void* dv, int64_t lddv, int64_t nrows,
                                      int F, hipStream_t stream) {
  if (nrows <= 0 || F <= 0) return hipSuccess;
  const int ob = out_dt == DType::F32 ? 4 : 2;
  if (k == nullptr || q == nullptr || v == nullptr || g == nullptr || dq == nullptr ||
      dv == nullptr || F % 8 != 0)
    return hipErrorInvalidValue;
  if (!(rows16(k, ldk, 2) && rows16(q, ldq, 2) && rows16(v, ldv, 2) && rows16(g, ldg, 2) &&
        rows16(dq, lddq, ob) && rows16(dv, lddv, ob)))
    return hipErrorInvalidValue;
  const GatedBf16Bwd a{t_rowptr, k, ldk, q, ldq, v, ldv, g, ldg, dq, lddq, dv, lddv, nrows, F};
  if (it == IType::I32) {
    const auto* c = static_cast<const int32_t*>(t_col);
    return out_dt == DType::F32 ? launch_bwd<int32_t, float>(c, a, stream)
                                : launch_bwd<int32_t, uint16_t>(c, a, stream);
  }
  const auto* c = static_cast<const int64_t*>(t_col);
  return out_dt == DType::F32 ? launch_bwd<int64_t, float>(c, a, stream)
                              : launch_bwd<int64_t, uint16_t>(c, a, stream);
}

}  // namespace dgraph
