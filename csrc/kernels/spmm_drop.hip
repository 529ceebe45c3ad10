// dgraph_amd — DropEdge fused into the CSR aggregation for gfx950 (contract: kernels.h).
//
// DropEdge (Rong et al., ICLR 2020; PyG's dropout_edge) aggregates over a fresh random
// subgraph every step. Filtering the edge list and rebuilding CSR, transpose and halo split
// per step would defeat the static pattern everything else here is built on, so the subgraph
// is never materialised: the keep decision of an entry is a pure function of (seed, dst id,
// src id) (philox.h: edge_keep), regenerated where it is needed. The transposed pass
// regenerates the same decisions from the transposed pattern, with no slot map.
//
// Data flow, the generic v2 SpMM (spmm.hip) with a compaction step in front of the gather:
//   * one wave owns a row; per chunk of 64 slots, lane j loads column id base + j with one
//     coalesced load and evaluates the keep decision of ITS slot: one Philox per entry;
//   * a ballot gives the 64-bit keep mask; its prefix popcount is each kept lane's rank, and
//     one ds_permute per word moves (column, weight) of the kept slots to lanes 0 .. kept-1
//     in slot order (the dropped slots go behind them, so the move is a permutation);
//   * the gather loop is v2's over the first `kept` lanes only: G = 64 / LPR lane groups, U
//     rows per group in flight, padding slots re-read kept slot 0 and are discarded by a
//     select (no branch around a load). A dropped entry's row is therefore never loaded:
//     that is the bandwidth DropEdge saves, and a NaN or Inf there cannot reach the output
//     (select-by-zero-weight, as v2 pads, would let it);
//   * a row wider than one column chunk (LPR x VEC) keeps up to NC chunks of accumulators, so
//     the mask is formed once per 64-slot chunk and not once per column chunk (rows wider
//     than NC chunks take another pass over the row's slots);
//   * fp32 accumulation in slot order per lane group, groups combined by an xor butterfly:
//     a fixed order, bitwise reproducible, the same for int32 and int64 columns.
// kept_degree is the same mask, counted.
//
// Not here: bf16 rows, edge weights, heads, hub splitting (a long row is simply walked by its
// wave), XCD row mapping and narrow column passes.
#include "../common.h"
#include "kernels.h"
#include "philox.h"

namespace dgraph {
namespace {

// the keep mask of the (up to 64) slots base .. base + n of a row whose id is rid; lane j's
// column goes to my_c (0 past n)
template <typename IdxT>
__device__ __forceinline__ uint64_t keep_mask(const SpmmDropArgs& a, uint64_t seed, int64_t rid,
                                              const IdxT* __restrict__ col, int64_t base, int n,
                                              int lane, int64_t& my_c) {
  my_c = 0;
  bool keep = false;
  if (lane < n) {
    my_c = static_cast<int64_t>(col[base + lane]);
    const int64_t cid = a.col_ids ? a.col_ids[my_c] : a.col_base + my_c;
    keep = edge_keep(seed, a.transposed ? cid : rid, a.transposed ? rid : cid, a.thr,
                     a.undirected);
  }
  return __ballot(keep);
}

// set bits of m below this lane
__device__ __forceinline__ int mask_rank(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                   __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0));
}

template <typename IdxT, int VEC, int LPR, int U, int NC>
__global__ __launch_bounds__(256) void spmm_drop_kernel(
    const SpmmDropArgs a, const float* __restrict__ col_scale,
    const float* __restrict__ row_scale, const float* __restrict__ x, int64_t ldx,
    float* __restrict__ out, int64_t ldo, int F, float beta) {
  constexpr int G = kWave / LPR;
  constexpr int kChunk = LPR * VEC;  // columns one sweep of the lanes covers
  using R = typename RawVec<VEC * sizeof(float)>::type;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR;
  const int l = lane % LPR;
  const IdxT* __restrict__ col = static_cast<const IdxT*>(a.col);
  const uint64_t seed = static_cast<uint64_t>(*a.seed);
  const int64_t r0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t rstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  for (int64_t r = r0; r < a.nrows; r += rstep) {
    const int64_t s = a.rowptr[r];
    const int64_t e = a.rowptr[r + 1];
    const int64_t orow = a.row_map ? a.row_map[r] : r;  // compacted CSR: output row
    const int64_t rid = a.row_ids ? a.row_ids[orow] : a.row_base + orow;
    for (int f0 = 0; f0 < F; f0 += NC * kChunk) {
      float acc[NC][VEC];
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[c][i] = 0.f;
      for (int64_t base = s; base < e; base += kWave) {
        const int n = (e - base) < kWave ? static_cast<int>(e - base) : kWave;
        int64_t my_c;
        const uint64_t mask = keep_mask<IdxT>(a, seed, rid, col, base, n, lane, my_c);
        const int nk = __popcll(mask);
        if (nk == 0) continue;  // wave-uniform
        const bool keep = (mask >> lane) & 1;
        float my_w = 1.f;
        if (col_scale && keep) my_w = col_scale[my_c];
        // compaction: kept slot of rank j -> lane j, dropped slots behind them
        const int below = mask_rank(mask);
        const int to = (keep ? below : nk + lane - below) << 2;
        int64_t cc = static_cast<uint32_t>(
            __builtin_amdgcn_ds_permute(to, static_cast<int>(static_cast<uint32_t>(my_c))));
        if constexpr (sizeof(IdxT) == 8)
          cc |= static_cast<int64_t>(
                    __builtin_amdgcn_ds_permute(to, static_cast<int>(my_c >> 32)))
                << 32;
        const float cw = __int_as_float(__builtin_amdgcn_ds_permute(to, __float_as_int(my_w)));
        // wave-uniform trip count: every lane stays active through the shuffles
        for (int k0 = 0; k0 < nk; k0 += G * U) {
          int64_t off[U];
          float w[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int kk = k0 + g + u * G;
            const int src = kk < nk ? kk : 0;  // padding re-reads kept slot 0
            off[u] = __shfl(cc, src, kWave) * ldx;
            w[u] = __shfl(cw, src, kWave);
          }
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            if (c > 0 && f0 + c * kChunk >= F) break;  // wave-uniform
            const int f = f0 + c * kChunk + l * VEC;
            const int fl = f < F ? f : 0;  // lanes past F read column 0
            R v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const R*>(x + off[u] + fl);
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const float* ev = reinterpret_cast<const float*>(&v[u]);
              const bool ok = k0 + g + u * G < nk;  // select, not a branch (inf * 0 safe)
#pragma unroll
              for (int i = 0; i < VEC; ++i) {
                const float t = fmaf(w[u], ev[i], acc[c][i]);
                acc[c][i] = ok ? t : acc[c][i];
              }
            }
          }
        }
      }
      const float rs = row_scale ? row_scale[orow] : 1.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c > 0 && f0 + c * kChunk >= F) break;
#pragma unroll
        for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[c][i] += __shfl_xor(acc[c][i], off, kWave);
        const int f = f0 + c * kChunk + l * VEC;
        if (g == 0 && f < F) {
          float* o = out + orow * ldo + f;
          if (beta != 0.f) {
            float old[VEC];
            load_vec_f32<float, VEC>(o, old);
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[c][i] = fmaf(acc[c][i], rs, beta * old[i]);
          } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[c][i] *= rs;
          }
          store_vec_f32<float, VEC>(o, acc[c]);
        }
      }
    }
  }
}

template <typename IdxT>
__global__ __launch_bounds__(256) void kept_degree_kernel(const SpmmDropArgs a,
                                                          int32_t* __restrict__ kept,
                                                          bool accumulate) {
  const int lane = threadIdx.x & (kWave - 1);
  const IdxT* __restrict__ col = static_cast<const IdxT*>(a.col);
  const uint64_t seed = static_cast<uint64_t>(*a.seed);
  const int64_t r0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t rstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  for (int64_t r = r0; r < a.nrows; r += rstep) {
    const int64_t s = a.rowptr[r];
    const int64_t e = a.rowptr[r + 1];
    const int64_t orow = a.row_map ? a.row_map[r] : r;
    const int64_t rid = a.row_ids ? a.row_ids[orow] : a.row_base + orow;
    int count = 0;
    for (int64_t base = s; base < e; base += kWave) {
      const int n = (e - base) < kWave ? static_cast<int>(e - base) : kWave;
      int64_t my_c;
      count += __popcll(keep_mask<IdxT>(a, seed, rid, col, base, n, lane, my_c));
    }
    if (lane == 0) kept[orow] = (accumulate ? kept[orow] : 0) + count;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) % 16) == 0; }

dim3 row_grid(int64_t nrows) {
  return dim3(static_cast<unsigned>(cap_blocks((nrows + 3) / 4, 256 * 32)));
}

template <typename IdxT, int VEC>
hipError_t launch_drop(const SpmmDropArgs& a, const float* cs, const float* rs, const float* x,
                       int64_t ldx, float* out, int64_t ldo, int F, float beta,
                       hipStream_t st) {
  const int lanes_needed = (F + VEC - 1) / VEC;
  const dim3 grid = row_grid(a.nrows), block(256);
  // U rows in flight per lane group: ~16 neighbour rows per wave, as the generic SpMM
#define DG_DROP(LPR_, U_, NC_)                                                              \
  hipLaunchKernelGGL((spmm_drop_kernel<IdxT, VEC, LPR_, U_, NC_>), grid, block, 0, st, a, cs, \
                     rs, x, ldx, out, ldo, F, beta);                                        \
  return hipGetLastError();
  if (lanes_needed <= 4) { DG_DROP(4, 2, 1) }
  if (lanes_needed <= 8) { DG_DROP(8, 2, 1) }
  if (lanes_needed <= 16) { DG_DROP(16, 4, 1) }
  if (lanes_needed <= 32) { DG_DROP(32, 8, 1) }
  if (lanes_needed <= 64) { DG_DROP(64, 8, 1) }
  DG_DROP(64, 4, 4)  // four chunks of accumulators: fewer rows in flight keep the registers
#undef DG_DROP
}

template <typename IdxT>
hipError_t launch_drop_vec(const SpmmDropArgs& a, const float* cs, const float* rs,
                           const float* x, int64_t ldx, float* out, int64_t ldo, int F,
                           float beta, hipStream_t st) {
  if (F % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && aligned16(x) && aligned16(out))
    return launch_drop<IdxT, 4>(a, cs, rs, x, ldx, out, ldo, F, beta, st);
  return launch_drop<IdxT, 1>(a, cs, rs, x, ldx, out, ldo, F, beta, st);
}

bool args_ok(const SpmmDropArgs& a) {
  return a.nrows >= 0 && a.nrows <= 0x7fffffff && a.rowptr && a.seed && (a.col || a.nrows == 0);
}

}  // namespace

hipError_t spmm_drop_f32(const SpmmDropArgs& a, const float* col_scale, const float* row_scale,
                         const float* x, int64_t ldx, float* out, int64_t ldo, int F, float beta,
                         hipStream_t st) {
  if (!args_ok(a) || F < 1 || !out) return hipErrorInvalidValue;
  if (a.nrows == 0) return hipSuccess;
  if (a.it == IType::I32)
    return launch_drop_vec<int32_t>(a, col_scale, row_scale, x, ldx, out, ldo, F, beta, st);
  return launch_drop_vec<int64_t>(a, col_scale, row_scale, x, ldx, out, ldo, F, beta, st);
}

hipError_t kept_degree(const SpmmDropArgs& a, int32_t* kept, bool accumulate, hipStream_t st) {
  if (!args_ok(a) || !kept) return hipErrorInvalidValue;
  if (a.nrows == 0) return hipSuccess;
  const dim3 grid = row_grid(a.nrows), block(256);
  if (a.it == IType::I32)
    hipLaunchKernelGGL(kept_degree_kernel<int32_t>, grid, block, 0, st, a, kept, accumulate);
  else
    hipLaunchKernelGGL(kept_degree_kernel<int64_t>, grid, block, 0, st, a, kept, accumulate);
  return hipGetLastError();
}

}  // namespace dgraph
