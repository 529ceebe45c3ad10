// dgraph_amd — fused softmax neighbourhood aggregation (gfx950), fp32.
//
//   out[r, f] = sum_j softmax_j(t_f x[c_j, f]) x[c_j, f]     over the entries j of CSR row r
//
// PyG's SoftmaxAggregation (the aggregator of DeeperGCN's GENConv): the softmax runs per
// CHANNEL and its score is the gathered value itself times a per-channel temperature t_f
// (t = 0: the mean; t -> +inf / -inf: the max / min). One gather pass, nothing per edge. The
// skeleton is spmm_pna.hip's: one wavefront owns an output row, the wave is cut into
// G = 64/LPR lane groups, group g walks slots g, g+G, ... of the row with VEC-wide (16 B)
// loads, four neighbour rows in flight per group. No atomics; no LDS but the one dt partial
// row per workgroup of the backward.
//
// Forward. Every lane keeps, per element, the online-softmax state of its group's entries
// with s = t_f v: m = max s, l = sum exp(s - m), acc = sum exp(s - m) v. The state is
// rescaled once per chunk of four in-flight entries (the chunk's maximum first, then ONE
// exp(m_old - m_new) and one exp per entry), not once per entry. The groups are merged in
// the xor butterfly by the two-state softmax merge; a group that scanned nothing holds
// (-inf, 0, 0), and no exp is taken of a difference of two equal values (so never of
// -inf - -inf). Stored: out = acc / l and lse = m + log l; an empty row gives 0 and -inf.
// (out, lse) is the whole state: every weight is exp(t_f x[c, f] - lse[r, f]).
//
// Two sources (interior block, then halo block of a partition): the second pass
// (second = true) seeds lane group 0 with the incumbent as (m, l, acc) = (lse, 1, out); an
// incumbent of lse = -inf counts as empty. A row with no entry in the second pass is not
// touched at all (bit-identical), so the pass may be run over all output rows.
//
// Backward: a gather over the transposed pattern, no atomics, one wave per source row c with
// x[c] and t resident, two destination rows in flight per group. Per entry (r = t_col[k]):
//   w = exp(t_f x[c, f] - lse[r, f]),  d = x[c, f] - out[r, f]
//   dx[c, f] += w g[r, f] (1 + t_f d),  pt[f] += w g[r, f] d^2
// with the deviation d formed per entry (never as a difference of accumulated sums). pt is
// kept per lane across the rows a wave handles, then reduced over the lane groups (butterfly)
// and the four waves of the workgroup (LDS, wave order) into ONE row of dt_part
// [gridDim.x, F]; the caller sums the rows (dt_f). The column passes are the outer loop of
// the backward so that this state is VEC registers. Fixed summation order in both directions
// => bitwise reproducible.
//
// Resource usage reported by hipcc for gfx950 (-Rpass-analysis=kernel-resource-usage, int64
// column ids; int32 within 1 VGPR except fwd VEC 4 LPR 64: 86 / 5; no scratch and no AGPRs
// in any instantiation; LDS: none in the forward, 1 KiB x VEC in the backward for the dt
// partial row):
//                 LPR 8        LPR 16       LPR 32       LPR 64
//   fwd VEC 4    90 VGPR / 5   88 / 5       86 / 5       80 / 6    (VGPRs / waves per SIMD)
//   fwd VEC 1    53 / 8        51 / 8       49 / 8       43 / 8
//   bwd VEC 4    92 / 5        86 / 5       84 / 5       84 / 5
//   bwd VEC 1    64 / 8        62 / 8       60 / 8       54 / 8
// The forward holds 3 state arrays + t (x VEC) plus four 16-B rows in flight and their four
// scores; the backward two entries in flight, each 3 arrays x VEC.
// Measured on an MI355X (benchmarks/bench_softmax_aggr.py, ogbn-products shape, 123.7 M
// entries; PERFORMANCE.md, softmax aggregation): forward 4.85 / 9.34 / 20.03 ms at F = 64 /
// 128 / 256 = 6.9 / 7.1 / 6.6 TB/s of the bytes it must move, 1.10 / 0.95 / 0.97 of one
// segment_extreme pass and 0.71 / 0.86 / 0.90 of the PNA pass, whose skeleton it shares, and
// 2.0-2.2 x the fp32 sum SpMM (the row-group kernel, 14 TB/s). The one v_exp_f32 per gathered
// element does not show: the wave-per-row gather sets the time, as for max / min. Backward
// 13.6 / 29.8 / 59.7 ms = 7.1 / 6.5 / 6.5 TB/s of three gathered rows per entry.
#include <initializer_list>

#include "../common.h"
#include "kernels.h"

namespace dgraph {
namespace {

struct SmxFwd {
  const int64_t* rowptr;
  const float* x;
  int64_t ldx;
  const float* t;
  float* out;
  int64_t ldo;
  float* lse;
  int64_t ldl;
  int64_t nrows;
  int F;
  bool second;
  const int64_t* row_map;
};

struct SmxBwd {
  const int64_t* rowptr;
  const float* x;
  int64_t ldx;
  const float* t;
  const float* g;
  int64_t ldg;
  const float* of;  // the forward's out
  int64_t ldof;
  const float* lse;
  int64_t ldl;
  float* dx;
  int64_t lddx;
  float* dt_part;  // [gridDim.x, F] or null
  int64_t nrows;
  int F;
};

constexpr float kNegInf = -__builtin_huge_valf();

// exp(a - b) for a <= b, the rescale of a softmax state of maximum a to the maximum b:
// equal maxima (two empty states at -inf included) give 1 without an exp
__device__ __forceinline__ float rescale(float a, float b) {
  return a == b ? 1.f : __expf(a - b);
}

template <typename IdxT, int VEC, int LPR>
__global__ __launch_bounds__(256, 4) void segment_softmax_fwd_kernel(
    const IdxT* __restrict__ col, const SmxFwd p) {
  constexpr int G = kWave / LPR;
  using R = typename RawVec<VEC * sizeof(float)>::type;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR;
  const int l = lane % LPR;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;

  for (int64_t r = wave; r < p.nrows; r += nwaves) {
    const int64_t s = p.rowptr[r];
    const int64_t e = p.rowptr[r + 1];
    // a second pass with no entry in this row leaves the incumbent alone
    if (p.second && e == s) continue;
    const int64_t orow = p.row_map ? p.row_map[r] : r;
    for (int fc = 0; fc < p.F; fc += LPR * VEC) {
      const int f = fc + l * VEC;
      const bool active = f < p.F;
      // lanes past F read column 0 (no branch around the loads) and write nothing
      const int fa = active ? f : 0;
      const float* xf = p.x + fa;
      float tv[VEC], m[VEC], ls[VEC], acc[VEC];
      load_vec_f32<float, VEC>(p.t + fa, tv);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        m[i] = kNegInf;
        ls[i] = acc[i] = 0.f;
      }
      if (p.second && g == 0) {  // the incumbent comes first: (lse, 1, out)
        float om[VEC], oo[VEC];
        load_vec_f32<float, VEC>(p.lse + orow * p.ldl + fa, om);
        load_vec_f32<float, VEC>(p.out + orow * p.ldo + fa, oo);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const bool has = om[i] != kNegInf;
          m[i] = om[i];
          ls[i] = has ? 1.f : 0.f;
          acc[i] = has ? oo[i] : 0.f;
        }
      }

      int64_t j = s + g;
      for (; j + 3 * G < e; j += 4 * G) {
        int64_t c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) c[u] = static_cast<int64_t>(col[j + u * G]);
        R v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const R*>(xf + c[u] * p.ldx);
        float ev[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) __builtin_memcpy(ev[u], &v[u], sizeof(R));
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          float sc[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) sc[u] = tv[i] * ev[u][i];
          const float mn = fmaxf(m[i], fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3])));
          const float k = rescale(m[i], mn);  // one rescale per chunk
          ls[i] *= k;
          acc[i] *= k;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float w = __expf(sc[u] - mn);
            ls[i] += w;
            acc[i] = fmaf(w, ev[u][i], acc[i]);
          }
          m[i] = mn;
        }
      }
      for (; j < e; j += G) {
        const int64_t c0 = static_cast<int64_t>(col[j]);
        const R v0 = *reinterpret_cast<const R*>(xf + c0 * p.ldx);
        float ev[VEC];
        __builtin_memcpy(ev, &v0, sizeof(R));
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float sc = tv[i] * ev[i];
          const float mn = fmaxf(m[i], sc);
          const float k = rescale(m[i], mn);
          const float w = rescale(sc, mn);
          ls[i] = fmaf(ls[i], k, w);
          acc[i] = fmaf(w, ev[i], acc[i] * k);
          m[i] = mn;
        }
      }

      // two-state merge of the lane groups; an empty group is (-inf, 0, 0)
#pragma unroll
      for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float om = __shfl_xor(m[i], off, kWave);
          const float ol = __shfl_xor(ls[i], off, kWave);
          const float oa = __shfl_xor(acc[i], off, kWave);
          const float mn = fmaxf(m[i], om);
          const float ka = rescale(m[i], mn);
          const float kb = rescale(om, mn);
          ls[i] = fmaf(ls[i], ka, ol * kb);
          acc[i] = fmaf(acc[i], ka, oa * kb);
          m[i] = mn;
        }

      if (g == 0 && active) {
        float o[VEC], le[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const bool has = ls[i] > 0.f;
          o[i] = has ? acc[i] / ls[i] : 0.f;
          le[i] = has ? m[i] + logf(ls[i]) : kNegInf;
        }
        store_vec_f32<float, VEC>(p.out + orow * p.ldo + f, o);
        store_vec_f32<float, VEC>(p.lse + orow * p.ldl + f, le);
      }
    }
  }
}

template <typename IdxT, int VEC, int LPR>
__global__ __launch_bounds__(256) void segment_softmax_bwd_kernel(const IdxT* __restrict__ col,
                                                                  const SmxBwd p) {
  constexpr int G = kWave / LPR;
  __shared__ float part[4][kWave * VEC];
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = threadIdx.x >> 6;
  const int g = lane / LPR;
  const int l = lane % LPR;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;

  struct Ent {  // what one transposed entry reads from its destination row
    float gg[VEC], le[VEC], oo[VEC];
  };

  for (int fc = 0; fc < p.F; fc += LPR * VEC) {
    const int f = fc + l * VEC;
    const bool active = f < p.F;
    const int fa = active ? f : 0;
    float tv[VEC], pt[VEC];
    load_vec_f32<float, VEC>(p.t + fa, tv);
#pragma unroll
    for (int i = 0; i < VEC; ++i) pt[i] = 0.f;

    for (int64_t c = wave; c < p.nrows; c += nwaves) {
      const int64_t s = p.rowptr[c];
      const int64_t e = p.rowptr[c + 1];
      float xc[VEC], sx[VEC], acc[VEC];
      load_vec_f32<float, VEC>(p.x + c * p.ldx + fa, xc);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        sx[i] = tv[i] * xc[i];
        acc[i] = 0.f;
      }

      auto load = [&](Ent& t, int64_t k) {
        const int64_t r = static_cast<int64_t>(col[k]);
        load_vec_f32<float, VEC>(p.g + r * p.ldg + fa, t.gg);
        load_vec_f32<float, VEC>(p.lse + r * p.ldl + fa, t.le);
        load_vec_f32<float, VEC>(p.of + r * p.ldof + fa, t.oo);
      };
      auto add = [&](const Ent& t) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float wg = __expf(sx[i] - t.le[i]) * t.gg[i];
          const float d = xc[i] - t.oo[i];  // per entry
          acc[i] = fmaf(wg, fmaf(tv[i], d, 1.f), acc[i]);
          pt[i] = fmaf(wg * d, d, pt[i]);
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
        for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off, kWave);

      if (g == 0 && active) store_vec_f32<float, VEC>(p.dx + c * p.lddx + f, acc);
    }

    if (p.dt_part != nullptr) {  // uniform over the grid
      // this workgroup's row of dt_part: lane groups by butterfly, then the waves in order
#pragma unroll
      for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
        for (int i = 0; i < VEC; ++i) pt[i] += __shfl_xor(pt[i], off, kWave);
      if (g == 0)
#pragma unroll
        for (int i = 0; i < VEC; ++i) part[wv][l * VEC + i] = pt[i];
      __syncthreads();
      if (wv == 0 && g == 0 && active) {
        float sum[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i)
          sum[i] = ((part[0][l * VEC + i] + part[1][l * VEC + i]) + part[2][l * VEC + i]) +
                   part[3][l * VEC + i];
        store_vec_f32<float, VEC>(p.dt_part + static_cast<int64_t>(blockIdx.x) * p.F + f, sum);
      }
      __syncthreads();  // part is reused by the next column pass
    }
  }
}

inline bool aligned_to(const void* p, int bytes) {
  return p == nullptr || (reinterpret_cast<uintptr_t>(p) % bytes) == 0;
}

inline int64_t row_blocks(int64_t nrows) { return cap_blocks((nrows + 3) / 4, 256 * 32); }

template <typename IdxT, int VEC>
hipError_t launch_fwd(const IdxT* col, const SmxFwd& a, hipStream_t st) {
  const int lanes = (a.F + VEC - 1) / VEC;
  const dim3 grid(static_cast<unsigned>(row_blocks(a.nrows))), block(256);
#define DG_FWD(LPR_)                                                                     \
  hipLaunchKernelGGL((segment_softmax_fwd_kernel<IdxT, VEC, LPR_>), grid, block, 0, st, col, \
                     a);                                                                 \
  return hipGetLastError();
  if (lanes <= 8) { DG_FWD(8) }
  if (lanes <= 16) { DG_FWD(16) }
  if (lanes <= 32) { DG_FWD(32) }
  DG_FWD(64)
#undef DG_FWD
}

template <typename IdxT, int VEC>
hipError_t launch_bwd(const IdxT* col, const SmxBwd& a, hipStream_t st) {
  const int lanes = (a.F + VEC - 1) / VEC;
  const dim3 grid(static_cast<unsigned>(row_blocks(a.nrows))), block(256);
#define DG_BWD(LPR_)                                                                     \
  hipLaunchKernelGGL((segment_softmax_bwd_kernel<IdxT, VEC, LPR_>), grid, block, 0, st, col, \
                     a);                                                                 \
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

}  // namespace

int64_t segment_softmax_dt_parts(int64_t nrows) { return nrows <= 0 ? 0 : row_blocks(nrows); }

hipError_t segment_softmax_fwd(IType it, const int64_t* rowptr, const void* col, const float* x,
                               int64_t ldx, const float* t, float* out, int64_t ldo, float* lse,
                               int64_t ldl, int64_t nrows, int F, bool second,
                               const int64_t* row_map, hipStream_t stream) {
  if (nrows <= 0 || F <= 0) return hipSuccess;
  if (t == nullptr || out == nullptr || lse == nullptr) return hipErrorInvalidValue;
  const SmxFwd a{rowptr, x, ldx, t, out, ldo, lse, ldl, nrows, F, second, row_map};
  const bool v4 = vec4(F, {{x, ldx}, {t, 4}, {out, ldo}, {lse, ldl}});
  if (it == IType::I32) {
    const auto* c = static_cast<const int32_t*>(col);
    return v4 ? launch_fwd<int32_t, 4>(c, a, stream) : launch_fwd<int32_t, 1>(c, a, stream);
  }
  const auto* c = static_cast<const int64_t*>(col);
  return v4 ? launch_fwd<int64_t, 4>(c, a, stream) : launch_fwd<int64_t, 1>(c, a, stream);
}

hipError_t segment_softmax_bwd(IType it, const int64_t* t_rowptr, const void* t_col,
                               const float* x, int64_t ldx, const float* t, const float* g,
                               int64_t ldg, const float* out_fwd, int64_t ldof,
                               const float* lse, int64_t ldl, float* dx, int64_t lddx,
                               float* dt_part, int64_t nrows, int F, hipStream_t stream) {
  if (nrows <= 0 || F <= 0) return hipSuccess;
  if (t == nullptr || dx == nullptr) return hipErrorInvalidValue;
  const SmxBwd a{t_rowptr, x, ldx, t, g, ldg, out_fwd, ldof, lse, ldl, dx, lddx, dt_part,
                 nrows, F};
  const bool v4 = vec4(F, {{x, ldx}, {t, 4}, {g, ldg}, {out_fwd, ldof}, {lse, ldl},
                           {dx, lddx}, {dt_part, F}});
  if (it == IType::I32) {
    const auto* c = static_cast<const int32_t*>(t_col);
    return v4 ? launch_bwd<int32_t, 4>(c, a, stream) : launch_bwd<int32_t, 1>(c, a, stream);
  }
  const auto* c = static_cast<const int64_t*>(t_col);
  return v4 ? launch_bwd<int64_t, 4>(c, a, stream) : launch_bwd<int64_t, 1>(c, a, stream);
}

}  // namespace dgraph
