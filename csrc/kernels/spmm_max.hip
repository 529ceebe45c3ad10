// dgraph_amd — CSR segment max / min with a recorded winner, and its backward (gfx950).
//
// The non-linear sibling of the segment sum in spmm.hip (the reference aggregates by sum
// only). Same row-per-wave skeleton: one wavefront owns an output row, the wave is cut into
// G = 64/LPR lane groups, group g walks slots g, g+G, ... of the row with VEC-wide (up to
// 16 B) loads, four neighbour rows in flight per group.
//
// Forward: every lane keeps (best, slot) per element, slot = the entry's offset within its
// CSR row. A group scans its slots in increasing order with a strict comparison, and the
// groups are combined by an xor butterfly under "better value wins, lower slot wins on
// equality", so the winner is the FIRST slot in CSR order that attains the extremum,
// whatever G is. The winner is written to arg (int32): offset >= 0 for a first-source
// (interior) pass, -1 for an empty row. A second-source pass (the halo block of a
// partition) reads out / arg as the incumbent, replaces it only where its own winner is
// strictly better (or there is none), and records -2 - offset.
//
// Backward: a gather over the transposed pattern, no atomics. One wave owns a source row
// c; for each transposed slot it reads the destination r, that entry's forward offset
// rel, and adds g[r, f] where arg[r, f] names this entry. Fixed summation order (group
// scan, then the butterfly) => bitwise reproducible.
#include "../common.h"
#include "kernels.h"

namespace dgraph {
namespace {

template <int VEC>
__device__ __forceinline__ void load_vec_i32(const int32_t* __restrict__ p, int (&o)[VEC]) {
  if constexpr (VEC % 4 == 0) {
#pragma unroll
    for (int i = 0; i < VEC; i += 4) {
      const int4 r = *reinterpret_cast<const int4*>(p + i);
      o[i] = r.x, o[i + 1] = r.y, o[i + 2] = r.z, o[i + 3] = r.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = p[i];
  }
}

template <int VEC>
__device__ __forceinline__ void store_vec_i32(int32_t* __restrict__ p, const int (&v)[VEC]) {
  if constexpr (VEC % 4 == 0) {
#pragma unroll
    for (int i = 0; i < VEC; i += 4)
      *reinterpret_cast<int4*>(p + i) = make_int4(v[i], v[i + 1], v[i + 2], v[i + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) p[i] = v[i];
  }
}

template <bool MIN>
__device__ __forceinline__ bool better(float a, float b) {
  return MIN ? a < b : a > b;
}

template <typename T, typename IdxT, int VEC, int LPR, bool MIN>
__global__ __launch_bounds__(256) void segment_extreme_fwd_kernel(
    const int64_t* __restrict__ rowptr, const IdxT* __restrict__ col,
    const T* __restrict__ x, int64_t ldx, T* __restrict__ out, int64_t ldo,
    int32_t* __restrict__ arg, int64_t lda, int64_t nrows, int F, bool second,
    const int64_t* __restrict__ row_map) {
  constexpr int G = kWave / LPR;
  using R = typename RawVec<VEC * sizeof(T)>::type;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR;
  const int l = lane % LPR;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;

  for (int64_t r = wave; r < nrows; r += nwaves) {
    const int64_t s = rowptr[r];
    const int64_t e = rowptr[r + 1];
    const int64_t orow = row_map ? row_map[r] : r;  // compacted CSR: output row
    for (int fc = 0; fc < F; fc += LPR * VEC) {
      const int f = fc + l * VEC;
      const bool active = f < F;
      // lanes past F read column 0 (no branch around the loads) and write nothing
      const T* xf = x + (active ? f : 0);
      float best[VEC];
      int slot[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) best[i] = 0.f, slot[i] = -1;

      auto take = [&](const R& raw, int off) {
        const T* ev = reinterpret_cast<const T*>(&raw);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float v = Elem<T>::to_f32(ev[i]);
          const bool win = slot[i] < 0 || better<MIN>(v, best[i]);
          best[i] = win ? v : best[i];
          slot[i] = win ? off : slot[i];
        }
      };

      int64_t j = s + g;
      for (; j + 3 * G < e; j += 4 * G) {
        int64_t c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) c[u] = static_cast<int64_t>(col[j + u * G]);
        R v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const R*>(xf + c[u] * ldx);
#pragma unroll
        for (int u = 0; u < 4; ++u) take(v[u], static_cast<int>(j + u * G - s));
      }
      for (; j < e; j += G) {
        const int64_t c0 = static_cast<int64_t>(col[j]);
        const R v0 = *reinterpret_cast<const R*>(xf + c0 * ldx);
        take(v0, static_cast<int>(j - s));
      }
      // Combine the G lane groups: the better value wins, the lower slot on equality
      // (so +0.0 and -0.0 tie); a group with no entry never wins.
#pragma unroll
      for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float ov = __shfl_xor(best[i], off, kWave);
          const int os = __shfl_xor(slot[i], off, kWave);
          const bool win = os >= 0 && (slot[i] < 0 || better<MIN>(ov, best[i]) ||
                                       (ov == best[i] && os < slot[i]));
          best[i] = win ? ov : best[i];
          slot[i] = win ? os : slot[i];
        }

      if (g == 0 && active) {
        T* o = out + orow * ldo + f;
        int32_t* a = arg + orow * lda + f;
        if (second) {
          float old[VEC];
          int oa[VEC];
          load_vec_f32<T, VEC>(o, old);
          load_vec_i32<VEC>(a, oa);
#pragma unroll
          for (int i = 0; i < VEC; ++i) {
            const bool win = slot[i] >= 0 && (oa[i] == -1 || better<MIN>(best[i], old[i]));
            best[i] = win ? best[i] : old[i];
            slot[i] = win ? -2 - slot[i] : oa[i];
          }
        }
        store_vec_f32<T, VEC>(o, best);  // a selected input value: exact in T
        store_vec_i32<VEC>(a, slot);
      }
    }
  }
}

template <typename T, typename IdxT, int VEC, int LPR>
__global__ __launch_bounds__(256) void segment_extreme_bwd_kernel(
    const int64_t* __restrict__ rowptr, const IdxT* __restrict__ col,
    const int32_t* __restrict__ rel, const T* __restrict__ gin, int64_t ldg,
    const int32_t* __restrict__ arg, int64_t lda, T* __restrict__ out, int64_t ldo,
    int64_t nrows, int F, bool halo, float beta) {
  constexpr int G = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR;
  const int l = lane % LPR;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;

  for (int64_t c = wave; c < nrows; c += nwaves) {
    const int64_t s = rowptr[c];
    const int64_t e = rowptr[c + 1];
    for (int fc = 0; fc < F; fc += LPR * VEC) {
      const int f = fc + l * VEC;
      const bool active = f < F;
      const int fa = active ? f : 0;
      float acc[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;

      int64_t j = s + g;
      for (; j + 1 * G < e; j += 2 * G) {
        int64_t r[2];
        int key[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          r[u] = static_cast<int64_t>(col[j + u * G]);
          const int q = rel[j + u * G];
          key[u] = halo ? -2 - q : q;
        }
        float v[2][VEC];
        int a[2][VEC];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          load_vec_f32<T, VEC>(gin + r[u] * ldg + fa, v[u]);
          load_vec_i32<VEC>(arg + r[u] * lda + fa, a[u]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] += a[u][i] == key[u] ? v[u][i] : 0.f;
      }
      for (; j < e; j += G) {
        const int64_t r0 = static_cast<int64_t>(col[j]);
        const int q = rel[j];
        const int key = halo ? -2 - q : q;
        float v[VEC];
        int a[VEC];
        load_vec_f32<T, VEC>(gin + r0 * ldg + fa, v);
        load_vec_i32<VEC>(arg + r0 * lda + fa, a);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += a[i] == key ? v[i] : 0.f;
      }
#pragma unroll
      for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += __shfl_xor(acc[i], off, kWave);

      if (g == 0 && active) {
        T* o = out + c * ldo + f;
        if (beta != 0.f) {
          float old[VEC];
          load_vec_f32<T, VEC>(o, old);
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] = fmaf(beta, old[i], acc[i]);
        }
        store_vec_f32<T, VEC>(o, acc);
      }
    }
  }
}

inline bool aligned_to(const void* p, int bytes) {
  return (reinterpret_cast<uintptr_t>(p) % bytes) == 0;
}

inline dim3 row_grid(int64_t nrows) {
  return dim3(static_cast<unsigned>(cap_blocks((nrows + 3) / 4, 256 * 32)));
}

template <typename T, typename IdxT, int VEC, bool MIN>
hipError_t launch_fwd(const int64_t* rowptr, const IdxT* col, const T* x, int64_t ldx, T* out,
                      int64_t ldo, int32_t* arg, int64_t lda, int64_t nrows, int F, bool second,
                      const int64_t* row_map, hipStream_t st) {
  const int lanes = (F + VEC - 1) / VEC;
  const dim3 grid = row_grid(nrows), block(256);
#define DG_FWD(LPR_)                                                                        \
  hipLaunchKernelGGL((segment_extreme_fwd_kernel<T, IdxT, VEC, LPR_, MIN>), grid, block, 0, \
                     st, rowptr, col, x, ldx, out, ldo, arg, lda, nrows, F, second, row_map); \
  return hipGetLastError();
  if (lanes <= 8) { DG_FWD(8) }
  if (lanes <= 16) { DG_FWD(16) }
  if (lanes <= 32) { DG_FWD(32) }
  DG_FWD(64)
#undef DG_FWD
}

template <typename T, typename IdxT, bool MIN>
hipError_t launch_fwd_vec(const int64_t* rowptr, const IdxT* col, const T* x, int64_t ldx,
                          T* out, int64_t ldo, int32_t* arg, int64_t lda, int64_t nrows, int F,
                          bool second, const int64_t* row_map, hipStream_t st) {
  // widest vector that divides the row width and every leading dimension and matches the
  // base pointers (arg is int32: VEC of them span 4 * VEC bytes, read as 16-B pieces)
  constexpr int kMaxVec = 16 / sizeof(T);
  auto ok = [&](int v) {
    return F % v == 0 && ldx % v == 0 && ldo % v == 0 && lda % v == 0 &&
           aligned_to(x, v * sizeof(T)) && aligned_to(out, v * sizeof(T)) &&
           aligned_to(arg, v % 4 == 0 ? 16 : 4);
  };
#define DG_ARGS rowptr, col, x, ldx, out, ldo, arg, lda, nrows, F, second, row_map, st
  if (ok(kMaxVec)) return launch_fwd<T, IdxT, kMaxVec, MIN>(DG_ARGS);
  if (ok(4)) return launch_fwd<T, IdxT, 4, MIN>(DG_ARGS);
  return launch_fwd<T, IdxT, 1, MIN>(DG_ARGS);
#undef DG_ARGS
}

template <typename T, typename IdxT, int VEC>
hipError_t launch_bwd(const int64_t* rowptr, const IdxT* col, const int32_t* rel, const T* g,
                      int64_t ldg, const int32_t* arg, int64_t lda, T* out, int64_t ldo,
                      int64_t nrows, int F, bool halo, float beta, hipStream_t st) {
  const int lanes = (F + VEC - 1) / VEC;
  const dim3 grid = row_grid(nrows), block(256);
#define DG_BWD(LPR_)                                                                         \
  hipLaunchKernelGGL((segment_extreme_bwd_kernel<T, IdxT, VEC, LPR_>), grid, block, 0, st,   \
                     rowptr, col, rel, g, ldg, arg, lda, out, ldo, nrows, F, halo, beta);    \
  return hipGetLastError();
  if (lanes <= 8) { DG_BWD(8) }
  if (lanes <= 16) { DG_BWD(16) }
  if (lanes <= 32) { DG_BWD(32) }
  DG_BWD(64)
#undef DG_BWD
}

template <typename T, typename IdxT>
hipError_t launch_bwd_vec(const int64_t* rowptr, const IdxT* col, const int32_t* rel,
                          const T* g, int64_t ldg, const int32_t* arg, int64_t lda, T* out,
                          int64_t ldo, int64_t nrows, int F, bool halo, float beta,
                          hipStream_t st) {
  constexpr int kMaxVec = 16 / sizeof(T);
  auto ok = [&](int v) {
    return F % v == 0 && ldg % v == 0 && ldo % v == 0 && lda % v == 0 &&
           aligned_to(g, v * sizeof(T)) && aligned_to(out, v * sizeof(T)) &&
           aligned_to(arg, v % 4 == 0 ? 16 : 4);
  };
#define DG_ARGS rowptr, col, rel, g, ldg, arg, lda, out, ldo, nrows, F, halo, beta, st
  if (ok(kMaxVec)) return launch_bwd<T, IdxT, kMaxVec>(DG_ARGS);
  if (ok(4)) return launch_bwd<T, IdxT, 4>(DG_ARGS);
  return launch_bwd<T, IdxT, 1>(DG_ARGS);
#undef DG_ARGS
}

}  // namespace

hipError_t segment_extreme_fwd(DType dt, IType it, bool minimum, const int64_t* rowptr,
                               const void* col, const void* x, int64_t ldx, void* out,
                               int64_t ldo, int32_t* arg, int64_t lda, int64_t nrows, int F,
                               bool second, const int64_t* row_map, hipStream_t stream) {
  if (nrows <= 0 || F <= 0) return hipSuccess;
#define DG_CALL(T, I, M)                                                                      \
  return launch_fwd_vec<T, I, M>(rowptr, static_cast<const I*>(col), static_cast<const T*>(x), \
                                 ldx, static_cast<T*>(out), ldo, arg, lda, nrows, F, second,   \
                                 row_map, stream);
#define DG_IDX(T, M)                                 \
  if (it == IType::I32) { DG_CALL(T, int32_t, M) }   \
  DG_CALL(T, int64_t, M)
  if (dt == DType::F32) {
    if (minimum) { DG_IDX(float, true) }
    DG_IDX(float, false)
  }
  if (minimum) { DG_IDX(uint16_t, true) }
  DG_IDX(uint16_t, false)
#undef DG_IDX
#undef DG_CALL
}

hipError_t segment_extreme_bwd(DType dt, IType it, const int64_t* t_rowptr, const void* t_col,
                               const int32_t* rel, const void* g, int64_t ldg,
                               const int32_t* arg, int64_t lda, void* out, int64_t ldo,
                               int64_t nrows, int F, bool halo, float beta,
                               hipStream_t stream) {
  if (nrows <= 0 || F <= 0) return hipSuccess;
#define DG_CALL(T, I)                                                                        \
  return launch_bwd_vec<T, I>(t_rowptr, static_cast<const I*>(t_col), rel,                   \
                              static_cast<const T*>(g), ldg, arg, lda, static_cast<T*>(out), \
                              ldo, nrows, F, halo, beta, stream);
  if (dt == DType::F32) {
    if (it == IType::I32) { DG_CALL(float, int32_t) }
    DG_CALL(float, int64_t)
  }
  if (it == IType::I32) { DG_CALL(uint16_t, int32_t) }
  DG_CALL(uint16_t, int64_t)
#undef DG_CALL
}

}  // namespace dgraph
