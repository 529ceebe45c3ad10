// dgraph_amd — fused gated neighbourhood aggregation (gfx950), fp32.
//
//   out[r, f] = sum_j sigmoid(k[r, f] + q[c_j, f]) v[c_j, f]     over the entries j of CSR row r
//
// The aggregation of the residual gated graph convolution (Bresson & Laurent; PyG's
// ResGatedGraphConv, GatedGCN): a sigmoid gate per channel that depends on both end points,
// so it is neither a per-vertex pre-pass nor an edge weight of the SpMM. One gather pass,
// nothing per edge. The skeleton is spmm_softmax.hip's: one wavefront owns an output row, the
// wave is cut into G = 64/LPR lane groups, group g walks slots g, g+G, ... of the row with
// VEC-wide (16 B) loads, kFwdDepth neighbour rows (a q and a v load each) in flight per group.
// Wider rows take column passes of LPR * VEC. No atomics, no LDS.
//
// Forward. k[r] is loaded once per row and column pass. Per gathered element, with
// z = k + q: e = exp(-|z|), r = 1 / (1 + e), s = z >= 0 ? r : e r, s (1 - s) = e r^2: one
// v_exp_f32 and one v_rcp_f32, finite for every finite z, and the derivative keeps its
// relative accuracy in both tails (it is never formed as s - s^2). Every lane sums s v (and,
// with DS, s (1 - s) v) over its group's entries; the groups are added in the xor butterfly.
// Stored: out, and ds when its pointer is given (a template parameter: the path without ds
// carries neither its accumulator nor its multiply). ds is the whole saved state of the
// destination side, dk = g * ds elementwise, so no destination-side backward kernel exists.
// An empty row gives exact zeros.
//
// Two sources (interior block, then halo block of a partition): the second pass
// (accumulate = true) adds its sums to the out / ds already there. A row with no entry in
// the second pass is not touched at all (bit-identical), so the pass may be run over all
// output rows.
//
// Backward, source side: a gather over the transposed pattern, one wave per source row c with
// q[c] and v[c] resident, two destination rows (a k and a g load each) in flight per group.
// Per entry (r = t_col[k]): dv[c] += s g[r], a[c] += s (1 - s) g[r]; stored dv and
// dq = v[c] a. Every row c < nrows is written. Fixed summation order in both directions =>
// bitwise reproducible.
//
// Resource usage reported by hipcc for gfx950 (-Rpass-analysis=kernel-resource-usage, int64
// column ids; int32 within 2 VGPRs and at the same occupancy; no scratch, no AGPRs and no LDS
// in any of the 48 instantiations):
//                     LPR 8         LPR 16        LPR 32        LPR 64
//   fwd      VEC 4   108 VGPR / 4   106 / 4       102 / 4       86 / 5   (VGPRs / waves per SIMD)
//   fwd + ds VEC 4   112 / 4        110 / 4       108 / 4       94 / 5
//   fwd      VEC 1    67 / 7         65 / 7        63 / 8       57 / 8
//   fwd + ds VEC 1    70 / 7         68 / 7        66 / 7       60 / 8
//   bwd src  VEC 4    84 / 5         82 / 5        80 / 6       74 / 6
//   bwd src  VEC 1    52 / 8         50 / 8        48 / 8       42 / 8
// The forward depth of four entries is chosen from this report: at VEC 4 a depth of 2 / 3 / 4
// takes 76 / 92 / 108 VGPRs (LPR 8, no ds), 6 / 5 / 4 waves per SIMD, which is 24 / 30 / 32
// 16-B gathers in flight per SIMD lane; ds adds its VEC accumulators and nothing in flight.
// Measured on an MI355X (python benchmarks/bench_gated_aggr.py --rounds 7, ogbn-products shape,
// 123.7 M entries; PERFORMANCE.md, gated aggregation): forward 8.86 / 19.24 / 41.98 ms at F =
// 64 / 128 / 256 = 7.3 / 6.7 / 6.2 TB/s of the bytes it must move (two gathered rows per
// entry), 1.8 / 2.1 / 1.9 of the softmax aggregation's one-row pass, whose skeleton it shares,
// and 3.9-4.5 x the fp32 sum SpMM (the row-group kernel, 14 TB/s) at 2.0 x its bytes. With ds:
// 9.44 / 20.67 / 44.71 ms, 6.5-7.4 % more. The v_exp_f32 and v_rcp_f32 per element do not
// show: the wave-per-row gather sets the time. Source-side backward 9.46 / 20.85 / 44.71 ms =
// 7.0 / 6.3 / 5.9 TB/s of two gathered rows per entry.
#include <initializer_list>

#include "../common.h"
#include "kernels.h"

namespace dgraph {
namespace {

struct GatedFwd {
  const int64_t* rowptr;
  const float* k;
  int64_t ldk;
  const float* q;
  int64_t ldq;
  const float* v;
  int64_t ldv;
  float* out;
  int64_t ldo;
  float* ds;
  int64_t ldds;
  int64_t nrows;
  int F;
  bool accumulate;
};

struct GatedBwd {
  const int64_t* rowptr;
  const float* k;
  int64_t ldk;
  const float* q;
  int64_t ldq;
  const float* v;
  int64_t ldv;
  const float* g;
  int64_t ldg;
  float* dq;
  int64_t lddq;
  float* dv;
  int64_t lddv;
  int64_t nrows;
  int F;
};

constexpr int kFwdDepth = 4;  // neighbour rows in flight per lane group (2 loads each)

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

template <typename IdxT, int VEC, int LPR, bool DS>
__global__ __launch_bounds__(256, 4) void segment_gated_fwd_kernel(
    const IdxT* __restrict__ col, const GatedFwd p) {
  constexpr int G = kWave / LPR;
  constexpr int U = kFwdDepth;
  using R = typename RawVec<VEC * sizeof(float)>::type;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR;
  const int l = lane % LPR;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;

  for (int64_t r = wave; r < p.nrows; r += nwaves) {
    const int64_t s = p.rowptr[r];
    const int64_t e = p.rowptr[r + 1];
    // an accumulate pass with no entry in this row leaves the earlier result alone
    if (p.accumulate && e == s) continue;
    for (int fc = 0; fc < p.F; fc += LPR * VEC) {
      const int f = fc + l * VEC;
      const bool active = f < p.F;
      // lanes past F read column 0 (no branch around the loads) and write nothing
      const int fa = active ? f : 0;
      const float* qf = p.q + fa;
      const float* vf = p.v + fa;
      float kr[VEC], acc[VEC], dac[VEC];
      load_vec_f32<float, VEC>(p.k + r * p.ldk + fa, kr);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = dac[i] = 0.f;

      int64_t j = s + g;
      for (; j + (U - 1) * G < e; j += U * G) {
        int64_t c[U];
#pragma unroll
        for (int u = 0; u < U; ++u) c[u] = static_cast<int64_t>(col[j + u * G]);
        R rq[U], rv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          rq[u] = *reinterpret_cast<const R*>(qf + c[u] * p.ldq);
          rv[u] = *reinterpret_cast<const R*>(vf + c[u] * p.ldv);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          float qe[VEC], ve[VEC];
          __builtin_memcpy(qe, &rq[u], sizeof(R));
          __builtin_memcpy(ve, &rv[u], sizeof(R));
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            float sg, dg;
            gate<DS>(kr[i] + qe[i], sg, dg);
            acc[i] = fmaf(sg, ve[i], acc[i]);
            if (DS) dac[i] = fmaf(dg, ve[i], dac[i]);
          }
        }
      }
      for (; j < e; j += G) {
        const int64_t c0 = static_cast<int64_t>(col[j]);
        float qe[VEC], ve[VEC];
        load_vec_f32<float, VEC>(qf + c0 * p.ldq, qe);
        load_vec_f32<float, VEC>(vf + c0 * p.ldv, ve);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          float sg, dg;
          gate<DS>(kr[i] + qe[i], sg, dg);
          acc[i] = fmaf(sg, ve[i], acc[i]);
          if (DS) dac[i] = fmaf(dg, ve[i], dac[i]);
        }
      }

      // the lane groups' sums, in the fixed order of the butterfly
#pragma unroll
      for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          acc[i] += __shfl_xor(acc[i], off, kWave);
          if (DS) dac[i] += __shfl_xor(dac[i], off, kWave);
        }

      if (g == 0 && active) {
        float* po = p.out + r * p.ldo + f;
        if (p.accumulate) {  // the earlier pass's result comes first
          float o[VEC];
          load_vec_f32<float, VEC>(po, o);
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] = o[i] + acc[i];
        }
        store_vec_f32<float, VEC>(po, acc);
        if (DS) {
          float* pd = p.ds + r * p.ldds + f;
          if (p.accumulate) {
            float o[VEC];
            load_vec_f32<float, VEC>(pd, o);
#pragma unroll
            for (int i = 0; i < VEC; ++i) dac[i] = o[i] + dac[i];
          }
          store_vec_f32<float, VEC>(pd, dac);
        }
      }
    }
  }
}

template <typename IdxT, int VEC, int LPR>
__global__ __launch_bounds__(256, 4) void segment_gated_bwd_src_kernel(
    const IdxT* __restrict__ col, const GatedBwd p) {
  constexpr int G = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR;
  const int l = lane % LPR;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;

  struct Ent {  // what one transposed entry reads from its destination row
    float kk[VEC], gg[VEC];
  };

  for (int64_t c = wave; c < p.nrows; c += nwaves) {
    const int64_t s = p.rowptr[c];
    const int64_t e = p.rowptr[c + 1];
    for (int fc = 0; fc < p.F; fc += LPR * VEC) {
      const int f = fc + l * VEC;
      const bool active = f < p.F;
      const int fa = active ? f : 0;
      const float* kf = p.k + fa;
      const float* gf = p.g + fa;
      float qc[VEC], av[VEC], aq[VEC];
      load_vec_f32<float, VEC>(p.q + c * p.ldq + fa, qc);
#pragma unroll
      for (int i = 0; i < VEC; ++i) av[i] = aq[i] = 0.f;

      auto load = [&](Ent& t, int64_t k) {
        const int64_t r = static_cast<int64_t>(col[k]);
        load_vec_f32<float, VEC>(kf + r * p.ldk, t.kk);
        load_vec_f32<float, VEC>(gf + r * p.ldg, t.gg);
      };
      auto add = [&](const Ent& t) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          float sg, dg;
          gate<true>(t.kk[i] + qc[i], sg, dg);
          av[i] = fmaf(sg, t.gg[i], av[i]);
          aq[i] = fmaf(dg, t.gg[i], aq[i]);
        }
      };

      int64_t j = s + g;
      for (; j + G < e; j += 2 * G) {
        Ent t0, t1;
        load(t0, j);
        load(t1, j + G);
        add(t0);
        add(t1);
      }
      for (; j < e; j += G) {
        Ent t0;
        load(t0, j);
        add(t0);
      }
#pragma unroll
      for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          av[i] += __shfl_xor(av[i], off, kWave);
          aq[i] += __shfl_xor(aq[i], off, kWave);
        }

      if (g == 0 && active) {
        float vc[VEC];
        load_vec_f32<float, VEC>(p.v + c * p.ldv + f, vc);
#pragma unroll
        for (int i = 0; i < VEC; ++i) aq[i] *= vc[i];
        store_vec_f32<float, VEC>(p.dv + c * p.lddv + f, av);
        store_vec_f32<float, VEC>(p.dq + c * p.lddq + f, aq);
      }
    }
  }
}

inline bool aligned_to(const void* p, int bytes) {
  return p == nullptr || (reinterpret_cast<uintptr_t>(p) % bytes) == 0;
}

inline int64_t row_blocks(int64_t nrows) { return cap_blocks((nrows + 3) / 4, 256 * 32); }

template <typename IdxT, int VEC, bool DS>
hipError_t launch_fwd(const IdxT* col, const GatedFwd& a, hipStream_t st) {
  const int lanes = (a.F + VEC - 1) / VEC;
  const dim3 grid(static_cast<unsigned>(row_blocks(a.nrows))), block(256);
#define DG_FWD(LPR_)                                                                      \
  hipLaunchKernelGGL((segment_gated_fwd_kernel<IdxT, VEC, LPR_, DS>), grid, block, 0, st, \
                     col, a);                                                             \
  return hipGetLastError();
  if (lanes <= 8) { DG_FWD(8) }
  if (lanes <= 16) { DG_FWD(16) }
  if (lanes <= 32) { DG_FWD(32) }
  DG_FWD(64)
#undef DG_FWD
}

template <typename IdxT, int VEC>
hipError_t launch_bwd(const IdxT* col, const GatedBwd& a, hipStream_t st) {
  const int lanes = (a.F + VEC - 1) / VEC;
  const dim3 grid(static_cast<unsigned>(row_blocks(a.nrows))), block(256);
#define DG_BWD(LPR_)                                                                      \
  hipLaunchKernelGGL((segment_gated_bwd_src_kernel<IdxT, VEC, LPR_>), grid, block, 0, st, \
                     col, a);                                                             \
  return hipGetLastError();
  if (lanes <= 8) { DG_BWD(8) }
  if (lanes <= 16) { DG_BWD(16) }
  if (lanes <= 32) { DG_BWD(32) }
  DG_BWD(64)
#undef DG_BWD
}

// a row array allows 16-B accesses: leading dimension a multiple of 4 elements and a 16-B
// aligned base
struct Arr {
  const void* p;
  int64_t ld;
};

inline bool vec4(int F, std::initializer_list<Arr> arrays) {
  if (F % 4 != 0) return false;
  for (const Arr& a : arrays)
    if (a.p != nullptr && (a.ld % 4 != 0 || !aligned_to(a.p, 16))) return false;
  return true;
}

template <typename IdxT>
hipError_t dispatch_fwd(const IdxT* c, const GatedFwd& a, bool v4, hipStream_t st) {
  if (a.ds != nullptr)
    return v4 ? launch_fwd<IdxT, 4, true>(c, a, st) : launch_fwd<IdxT, 1, true>(c, a, st);
  return v4 ? launch_fwd<IdxT, 4, false>(c, a, st) : launch_fwd<IdxT, 1, false>(c, a, st);
}

}  // namespace

hipError_t segment_gated_fwd(IType it, const int64_t* rowptr, const void* col, const float* k,
                             int64_t ldk, const float* q, int64_t ldq, const float* v,
                             int64_t ldv, float* out, int64_t ldo, float* ds, int64_t ldds,
                             int64_t nrows, int F, bool accumulate, hipStream_t stream) {
  if (nrows <= 0 || F <= 0) return hipSuccess;
  if (k == nullptr || out == nullptr) return hipErrorInvalidValue;
  const GatedFwd a{rowptr, k, ldk, q, ldq, v, ldv, out, ldo, ds, ldds, nrows, F, accumulate};
  const bool v4 = vec4(F, {{k, ldk}, {q, ldq}, {v, ldv}, {out, ldo}, {ds, ldds}});
  if (it == IType::I32) return dispatch_fwd(static_cast<const int32_t*>(col), a, v4, stream);
  return dispatch_fwd(static_cast<const int64_t*>(col), a, v4, stream);
}

hipError_t segment_gated_bwd_src(IType it, const int64_t* t_rowptr, const void* t_col,
                                 const float* k, int64_t ldk, const float* q, int64_t ldq,
                                 const float* v, int64_t ldv, const float* g, int64_t ldg,
                                 float* dq, int64_t lddq, float* dv, int64_t lddv,
                                 int64_t nrows, int F, hipStream_t stream) {
  if (nrows <= 0 || F <= 0) return hipSuccess;
  if (q == nullptr || v == nullptr || dq == nullptr || dv == nullptr)
    return hipErrorInvalidValue;
  const GatedBwd a{t_rowptr, k, ldk, q, ldq, v, ldv, g, ldg, dq, lddq, dv, lddv, nrows, F};
  const bool v4 = vec4(F, {{k, ldk}, {q, ldq}, {v, ldv}, {g, ldg}, {dq, lddq}, {dv, lddv}});
  if (it == IType::I32) {
    const auto* c = static_cast<const int32_t*>(t_col);
    return v4 ? launch_bwd<int32_t, 4>(c, a, stream) : launch_bwd<int32_t, 1>(c, a, stream);
  }
  const auto* c = static_cast<const int64_t*>(t_col);
  return v4 ? launch_bwd<int64_t, 4>(c, a, stream) : launch_bwd<int64_t, 1>(c, a, stream);
}

}  // namespace dgraph
