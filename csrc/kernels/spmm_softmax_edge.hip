// dgraph_amd — fused softmax neighbourhood aggregation WITH edge features (gfx950), fp32.
//
//   z_k = x[col[k], f] + e[k, f]           per CSR slot k of row r: the source row plus the
//   m_k = (relu ? max(z_k, 0) : z_k) + eps slot's own edge row (GENConv's message with edge_dim)
//   out[r, f] = sum_k softmax_k(t_f m_k) m_k,   lse[r, f] = log sum_k exp(t_f m_k)
//
// PyG's GENConv(edge_dim=) with aggr="softmax": the message depends on the edge, so it cannot
// be formed once per vertex; it is formed here per slot in registers, between the gather and
// the online softmax of spmm_softmax.hip, whose skeleton this file keeps: one wavefront owns
// an output row, the wave is cut into G = 64/LPR lane groups, group g walks slots g, g+G, ...
// with VEC-wide (16 B) loads, four slots in flight per group. Slot j's edge row streams from
// e + j * lde with the same access width as the gathered row. No atomics; no LDS but the one
// dt partial row per workgroup of the backward.
//
// Forward: per element the online-softmax state (m, l, acc) over s = t_f m_k, rescaled once
// per chunk of four slots; the lane groups are merged in the xor butterfly by the two-state
// merge. out = acc / l, lse = m + log l; an empty row gives 0 and -inf. (out, lse) is the
// whole saved state. second = true seeds lane group 0 with the incumbent (lse, 1, out) of an
// earlier pass over another block of the entries (lse = -inf counts as empty) and leaves a
// row with no entry in this block bitwise alone. row_map as in spmm_softmax.hip.
//
// Backward, destination side: over the SAME pattern (not the transposed one), any block of the
// entries with the final (out, lse). One wave per destination row r with g[r], out[r],
// lse[r] and t resident; z and m are recomputed per slot:
//   w = exp(t_f m - lse[r, f]),  d = m - out[r, f],  dm = w g[r, f] (1 + t_f d)
//   de[k, f] = dm where !relu or z > 0 (strict, as torch.relu), else exactly 0
//   pt[f]   += w g[r, f] d^2
// Every slot's de row is written (F columns, own row stride). pt is kept per lane across the
// rows a wave handles, then reduced over the lane groups (butterfly) and the four waves of
// the workgroup (LDS, wave order) into ONE row of dt_part [gridDim.x, F]. The column passes
// are the outer loop so that this state is VEC registers. Fixed order => bitwise reproducible.
//
// Source side: no kernel here. dx[c] = sum_{k: col[k] = c} de[k] is the plain row-sum SpMM
// over the slot-transposed pattern with de as its [nnz, F] source matrix: de has to be
// written anyway (the edge projection's weight gradient reads it) and summing it reads one
// row per entry where a recomputing gather would read four (e, out, lse, g).
//
// Resource usage reported by hipcc for gfx950 (-Rpass-analysis=kernel-resource-usage, int64
// column ids; int32 within 2 VGPRs except fwd LPR 64: VEC 4 95 / 5, VEC 1 60 / 8; no scratch
// and no AGPRs in any instantiation; LDS: none in the forward, 1 KiB x VEC in the backward
// for the dt partial row):
//                 LPR 8        LPR 16       LPR 32       LPR 64
//   fwd VEC 4   106 VGPR / 4  104 / 4      102 / 4       98 / 4    (VGPRs / waves per SIMD)
//   fwd VEC 1    75 / 6        73 / 6       69 / 7       65 / 7
//   bwd VEC 4    92 / 5        92 / 5       92 / 5       90 / 5
//   bwd VEC 1    57 / 8        57 / 8       57 / 8       52 / 8
// The forward holds what spmm_softmax.hip's does plus four edge rows in flight (+16 VGPRs at
// VEC 4: one wave per SIMD fewer than the plain kernel, still within launch_bounds(256, 4));
// the backward four resident arrays + pt (x VEC) and two slots in flight, each a gathered
// row, an edge row and the de row it stores. Four slots in flight in the backward compile to
// 114 VGPRs / 4 waves without scratch and measured within the noise of two (below), which
// are kept.
// Measured on an MI355X (benchmarks/bench_softmax_aggr_edge.py, ogbn-products shape, 123.7 M
// entries; PERFORMANCE.md, softmax aggregation with edge features): forward 9.48 / 20.47 /
// 41.33 ms at F = 64 / 128 / 256 = 6.9 / 6.3 / 6.3 TB/s of the bytes it must move, 1.92 / 2.19
// / 1.96 of the plain forward where the bytes say 1.95: the stream of e (4 nnz F bytes) sets
// the time, not the gather. Backward 16.55 / 33.64 / 64.63 ms = 5.9 / 5.8 / 6.0 TB/s (four in
// flight: 16.39 / 32.01 / 66.11), the dx row sum of de 5.56 / 12.31 / 23.28 ms; together 1.59
// / 1.61 / 1.46 of the plain backward (1.35 by bytes). ogbn-proteins shape (132,534 rows,
// 79.1 M entries), F = 64: 5.13 ms forward (8.0 TB/s), 8.46 + 3.84 ms backward. Against the
// composed gather / add / relu / edge-softmax / scatter path on 2 GB edge tensors: 11.6-16.1 x
// forward, 8.9-12.6 x forward + backward, with de the only [E, F] temporary.
#include <initializer_list>

#include "../common.h"
#include "kernels.h"

namespace dgraph {
namespace {

struct SmxEdgeFwd {
  const int64_t* rowptr;
  const float* x;
  int64_t ldx;
  const float* e;
  int64_t lde;
  const float* t;
  float* out;
  int64_t ldo;
  float* lse;
  int64_t ldl;
  int64_t nrows;
  int F;
  bool relu;
  float eps;
  bool second;
  const int64_t* row_map;
};

struct SmxEdgeBwd {
  const int64_t* rowptr;
  const float* x;
  int64_t ldx;
  const float* e;
  int64_t lde;
  const float* t;
  const float* g;
  int64_t ldg;
  const float* of;  // the forward's out
  int64_t ldof;
  const float* lse;
  int64_t ldl;
  float* de;
  int64_t ldde;
  float* dt_part;  // [gridDim.x, F] or null
  int64_t nrows;
  int F;
  bool relu;
  float eps;
};

constexpr float kNegInf = -__builtin_huge_valf();

// exp(a - b) for a <= b: equal maxima (two empty states at -inf included) give 1 without an
// exp
__device__ __forceinline__ float rescale(float a, float b) {
  return a == b ? 1.f : __expf(a - b);
}

// the message of one element: (relu ? max(z, 0) : z) + eps
__device__ __forceinline__ float message(float z, bool relu, float eps) {
  return (relu ? fmaxf(z, 0.f) : z) + eps;
}

template <typename IdxT, int VEC, int LPR>
__global__ __launch_bounds__(256, 4) void segment_softmax_edge_fwd_kernel(
    const IdxT* __restrict__ col, const SmxEdgeFwd p) {
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
      const float* ef = p.e + fa;
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
        R v[4], w4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w4[u] = *reinterpret_cast<const R*>(ef + (j + u * G) * p.lde);
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const R*>(xf + c[u] * p.ldx);
        float mv[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float xv[VEC], ev[VEC];
          __builtin_memcpy(xv, &v[u], sizeof(R));
          __builtin_memcpy(ev, &w4[u], sizeof(R));
#pragma unroll
          for (int i = 0; i < VEC; ++i) mv[u][i] = message(xv[i] + ev[i], p.relu, p.eps);
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          float sc[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) sc[u] = tv[i] * mv[u][i];
          const float mn = fmaxf(m[i], fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3])));
          const float k = rescale(m[i], mn);  // one rescale per chunk
          ls[i] *= k;
          acc[i] *= k;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float w = __expf(sc[u] - mn);
            ls[i] += w;
            acc[i] = fmaf(w, mv[u][i], acc[i]);
          }
          m[i] = mn;
        }
      }
      for (; j < e; j += G) {
        const int64_t c0 = static_cast<int64_t>(col[j]);
        const R w0 = *reinterpret_cast<const R*>(ef + j * p.lde);
        const R v0 = *reinterpret_cast<const R*>(xf + c0 * p.ldx);
        float xv[VEC], ev[VEC];
        __builtin_memcpy(xv, &v0, sizeof(R));
        __builtin_memcpy(ev, &w0, sizeof(R));
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float mv = message(xv[i] + ev[i], p.relu, p.eps);
          const float sc = tv[i] * mv;
          const float mn = fmaxf(m[i], sc);
          const float k = rescale(m[i], mn);
          const float w = rescale(sc, mn);
          ls[i] = fmaf(ls[i], k, w);
          acc[i] = fmaf(w, mv, acc[i] * k);
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
__global__ __launch_bounds__(256) void segment_softmax_edge_bwd_kernel(
    const IdxT* __restrict__ col, const SmxEdgeBwd p) {
  constexpr int G = kWave / LPR;
  constexpr int U = 2;  // slots in flight per group
  using R = typename RawVec<VEC * sizeof(float)>::type;
  __shared__ float part[4][kWave * VEC];
  const int lane = threadIdx.x & (kWave - 1);
  const int wv = threadIdx.x >> 6;
  const int g = lane / LPR;
  const int l = lane % LPR;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;

  for (int fc = 0; fc < p.F; fc += LPR * VEC) {
    const int f = fc + l * VEC;
    const bool active = f < p.F;
    const int fa = active ? f : 0;
    const float* xf = p.x + fa;
    const float* ef = p.e + fa;
    float tv[VEC], pt[VEC];
    load_vec_f32<float, VEC>(p.t + fa, tv);
#pragma unroll
    for (int i = 0; i < VEC; ++i) pt[i] = 0.f;

    for (int64_t r = wave; r < p.nrows; r += nwaves) {
      const int64_t s = p.rowptr[r];
      const int64_t e = p.rowptr[r + 1];
      if (e == s) continue;
      float gg[VEC], oo[VEC], le[VEC];
      load_vec_f32<float, VEC>(p.g + r * p.ldg + fa, gg);
      load_vec_f32<float, VEC>(p.of + r * p.ldof + fa, oo);
      load_vec_f32<float, VEC>(p.lse + r * p.ldl + fa, le);

      // one slot: its message again, its de row out, its share of dt
      auto slot = [&](const R& vx, const R& ve, int64_t k) {
        float xv[VEC], ev[VEC], dv[VEC];
        __builtin_memcpy(xv, &vx, sizeof(R));
        __builtin_memcpy(ev, &ve, sizeof(R));
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float z = xv[i] + ev[i];
          const float mv = message(z, p.relu, p.eps);
          const float wg = __expf(tv[i] * mv - le[i]) * gg[i];
          const float d = mv - oo[i];  // per slot
          const float dm = wg * fmaf(tv[i], d, 1.f);
          dv[i] = (!p.relu || z > 0.f) ? dm : 0.f;
          pt[i] = fmaf(wg * d, d, pt[i]);
        }
        if (active) store_vec_f32<float, VEC>(p.de + k * p.ldde + f, dv);
      };

      int64_t j = s + g;
      for (; j + (U - 1) * G < e; j += U * G) {
        int64_t c[U];
#pragma unroll
        for (int u = 0; u < U; ++u) c[u] = static_cast<int64_t>(col[j + u * G]);
        R ve[U], vx[U];
#pragma unroll
        for (int u = 0; u < U; ++u) ve[u] = *reinterpret_cast<const R*>(ef + (j + u * G) * p.lde);
#pragma unroll
        for (int u = 0; u < U; ++u) vx[u] = *reinterpret_cast<const R*>(xf + c[u] * p.ldx);
#pragma unroll
        for (int u = 0; u < U; ++u) slot(vx[u], ve[u], j + u * G);
      }
      for (; j < e; j += G) {
        const int64_t c0 = static_cast<int64_t>(col[j]);
        const R ve = *reinterpret_cast<const R*>(ef + j * p.lde);
        const R vx = *reinterpret_cast<const R*>(xf + c0 * p.ldx);
        slot(vx, ve, j);
      }
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
hipError_t launch_fwd(const IdxT* col, const SmxEdgeFwd& a, hipStream_t st) {
  const int lanes = (a.F + VEC - 1) / VEC;
  const dim3 grid(static_cast<unsigned>(row_blocks(a.nrows))), block(256);
#define DG_FWD(LPR_)                                                                        \
  hipLaunchKernelGGL((segment_softmax_edge_fwd_kernel<IdxT, VEC, LPR_>), grid, block, 0, st, \
                     col, a);                                                               \
  return hipGetLastError();
  if (lanes <= 8) { DG_FWD(8) }
  if (lanes <= 16) { DG_FWD(16) }
  if (lanes <= 32) { DG_FWD(32) }
  DG_FWD(64)
#undef DG_FWD
}

template <typename IdxT, int VEC>
hipError_t launch_bwd(const IdxT* col, const SmxEdgeBwd& a, hipStream_t st) {
  const int lanes = (a.F + VEC - 1) / VEC;
  const dim3 grid(static_cast<unsigned>(row_blocks(a.nrows))), block(256);
#define DG_BWD(LPR_)                                                                        \
  hipLaunchKernelGGL((segment_softmax_edge_bwd_kernel<IdxT, VEC, LPR_>), grid, block, 0, st, \
                     col, a);                                                               \
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

int64_t segment_softmax_edge_dt_parts(int64_t nrows) {
  return nrows <= 0 ? 0 : row_blocks(nrows);
}

hipError_t segment_softmax_edge_fwd(IType it, const int64_t* rowptr, const void* col,
                                    const float* x, int64_t ldx, const float* e, int64_t lde,
                                    const float* t, float* out, int64_t ldo, float* lse,
                                    int64_t ldl, int64_t nrows, int F, bool relu, float eps,
                                    bool second, const int64_t* row_map, hipStream_t stream) {
  if (nrows <= 0 || F <= 0) return hipSuccess;
  if (t == nullptr || out == nullptr || lse == nullptr) return hipErrorInvalidValue;
  const SmxEdgeFwd a{rowptr, x,     ldx, e,    lde, t,      out,    ldo,
                     lse,    ldl,   nrows, F,  relu, eps,   second, row_map};
  const bool v4 = vec4(F, {{x, ldx}, {e, lde}, {t, 4}, {out, ldo}, {lse, ldl}});
  if (it == IType::I32) {
    const auto* c = static_cast<const int32_t*>(col);
    return v4 ? launch_fwd<int32_t, 4>(c, a, stream) : launch_fwd<int32_t, 1>(c, a, stream);
  }
  const auto* c = static_cast<const int64_t*>(col);
  return v4 ? launch_fwd<int64_t, 4>(c, a, stream) : launch_fwd<int64_t, 1>(c, a, stream);
}

hipError_t segment_softmax_edge_bwd(IType it, const int64_t* rowptr, const void* col,
                                    const float* x, int64_t ldx, const float* e, int64_t lde,
                                    const float* t, const float* g, int64_t ldg,
                                    const float* out_fwd, int64_t ldof, const float* lse,
                                    int64_t ldl, float* de, int64_t ldde, float* dt_part,
                                    int64_t nrows, int F, bool relu, float eps,
                                    hipStream_t stream) {
  if (nrows <= 0 || F <= 0) return hipSuccess;
  if (t == nullptr || de == nullptr) return hipErrorInvalidValue;
  const SmxEdgeBwd a{rowptr, x,   ldx, e,  lde,  t,       g,     ldg, out_fwd, ldof,
                     lse,    ldl, de,  ldde, dt_part, nrows, F,   relu,    eps};
  const bool v4 = vec4(F, {{x, ldx}, {e, lde}, {t, 4}, {g, ldg}, {out_fwd, ldof}, {lse, ldl},
                           {de, ldde}, {dt_part, F}});
  if (it == IType::I32) {
    const auto* c = static_cast<const int32_t*>(col);
    return v4 ? launch_bwd<int32_t, 4>(c, a, stream) : launch_bwd<int32_t, 1>(c, a, stream);
  }
  const auto* c = static_cast<const int64_t*>(col);
  return v4 ? launch_bwd<int64_t, 4>(c, a, stream) : launch_bwd<int64_t, 1>(c, a, stream);
}

}  // namespace dgraph
