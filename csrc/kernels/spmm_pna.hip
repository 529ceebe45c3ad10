// dgraph_amd — fused multi-aggregator neighbourhood statistics for PNA (gfx950), fp32.
//
// Mean, standard deviation, max and min of the same neighbour rows in ONE gather pass (the
// separate reductions gather x[col] four to five times), and the matching backward. The
// skeleton is spmm_max.hip's: one wavefront owns an output row, the wave is cut into
// G = 64/LPR lane groups, group g walks slots g, g+G, ... of the row with VEC-wide (16 B)
// loads, four neighbour rows in flight per group.
//
// Forward. Every lane keeps, per element: a pivot (its group's first value), S1 = sum d and
// S2 = sum d*d with d = v - pivot, and (best, slot) for the maximum and for the minimum.
// After the scan a group holds (n_g, mean_g, M2_g) with n_g = the number of the row's slots
// congruent to g (from the degree, no counter), mean_g = pivot + S1/n_g and
// M2_g = S2 - S1*S1/n_g: the cancellation is relative to the spread about the pivot, not to
// the offset of the values. The groups are merged in the xor butterfly by the pairwise
// (Chan) formula, with each mean kept split as (pivot, mean - pivot) until the last merge so
// that the difference of two group means does not round at the magnitude of the values;
// the extremes by "better value wins, lower slot wins on equality" as in
// spmm_max.hip. M2 is clamped at 0 before the square root. Everything is computed whatever
// outputs are requested (the kernel is gather-bound); null output pairs are not stored.
//
// Two sources (interior block, then halo block of a partition): the first pass (final =
// false) stores mean and M2 (in sdev); the second pass (second = true, final = true) merges
// its own (n_b, mean_b, M2_b) with that incumbent, whose count is read from prev_rowptr,
// then finalises sdev = sqrt(max(M2, 0) / max(n, 1) + eps). A pass finalises only the rows
// it visits, so the host runs the second pass over ALL output rows (the uncompacted halo
// block; a row with no halo entry costs one read and one write of its moments and nothing
// else) rather than over the row-compacted block plus a finalise launch for the rest.
//
// Backward: a gather over the transposed pattern, no atomics, one wave per source row c,
// two destination rows in flight per group. The deviation (x[c] - mean[r]) / sdev[r] is
// formed per entry (the factored form x_c * sum b - sum b * mean loses the bound).
// Fixed summation order in both directions => bitwise reproducible.
//
// Resource usage reported by hipcc for gfx950 (-Rpass-analysis=kernel-resource-usage, int64
// column ids; int32 within 1 VGPR except fwd VEC 4 LPR 64: 87 / 5; no scratch, no LDS, no
// AGPRs in any instantiation):
//                 LPR 8        LPR 16       LPR 32       LPR 64
//   fwd VEC 4   113 VGPR / 4  113 / 4      110 / 4      103 / 4    (VGPRs / waves per SIMD)
//   fwd VEC 1    81 / 5        77 / 6       77 / 6       63 / 8
//   bwd VEC 4   157 / 3       156 / 3      155 / 3      151 / 3
//   bwd VEC 1    86 / 5        84 / 5       82 / 5       76 / 6
// The forward holds 7 accumulators x VEC plus four 16-B rows in flight; without the
// 4-waves-per-SIMD launch bound its VEC 4 instantiations take 126-130 VGPRs (3 waves at
// LPR 16). The backward holds two entries in flight, each 8 arrays x VEC.
#include <initializer_list>

#include "../common.h"
#include "kernels.h"

namespace dgraph {
namespace {

struct PnaFwd {
  const int64_t* rowptr;
  const float* x;
  int64_t ldx;
  float* mean;
  int64_t ld_mean;
  float* sdev;
  int64_t ld_sdev;
  float* vmax;
  int64_t ld_vmax;
  int32_t* amax;
  int64_t ld_amax;
  float* vmin;
  int64_t ld_vmin;
  int32_t* amin;
  int64_t ld_amin;
  int64_t nrows;
  int F;
  float eps;
  bool second, final;
  const int64_t* prev_rowptr;
  const int64_t* row_map;
};

struct PnaBwd {
  const int64_t* rowptr;
  const int32_t* rel;
  const float* x;
  int64_t ldx;
  const float* inv_deg;
  const float* g_mean;
  int64_t ld_gmean;
  const float* g_std;
  int64_t ld_gstd;
  const float* mean;
  int64_t ld_mean;
  const float* sdev;
  int64_t ld_sdev;
  const float* g_max;
  int64_t ld_gmax;
  const int32_t* amax;
  int64_t ld_amax;
  const float* g_min;
  int64_t ld_gmin;
  const int32_t* amin;
  int64_t ld_amin;
  float* out;
  int64_t ldo;
  int64_t nrows;
  int F;
  bool halo;
  float beta;
};

template <int VEC>
__device__ __forceinline__ void ld_i32(const int32_t* __restrict__ p, int (&o)[VEC]) {
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
__device__ __forceinline__ void st_i32(int32_t* __restrict__ p, const int (&v)[VEC]) {
  if constexpr (VEC % 4 == 0) {
#pragma unroll
    for (int i = 0; i < VEC; i += 4)
      *reinterpret_cast<int4*>(p + i) = make_int4(v[i], v[i + 1], v[i + 2], v[i + 3]);
  } else {
#pragma unroll
    for (int i = 0; i < VEC; ++i) p[i] = v[i];
  }
}

// (best, slot) of one extreme over the lane groups, then against a second-source incumbent
template <int VEC, int LPR, bool MIN>
__device__ __forceinline__ void combine_extreme(float (&best)[VEC], int (&slot)[VEC]) {
#pragma unroll
  for (int off = LPR; off < kWave; off <<= 1)
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const float ov = __shfl_xor(best[i], off, kWave);
      const int os = __shfl_xor(slot[i], off, kWave);
      const bool better = MIN ? ov < best[i] : ov > best[i];
      const bool win = os >= 0 && (slot[i] < 0 || better || (ov == best[i] && os < slot[i]));
      best[i] = win ? ov : best[i];
      slot[i] = win ? os : slot[i];
    }
}

template <int VEC, bool MIN>
__device__ __forceinline__ void store_extreme(float* __restrict__ o, int32_t* __restrict__ a,
                                              float (&best)[VEC], int (&slot)[VEC],
                                              bool second) {
  if (second) {
    float old[VEC];
    int oa[VEC];
    load_vec_f32<float, VEC>(o, old);
    ld_i32<VEC>(a, oa);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const bool better = MIN ? best[i] < old[i] : best[i] > old[i];
      const bool win = slot[i] >= 0 && (oa[i] == -1 || better);
      best[i] = win ? best[i] : old[i];
      slot[i] = win ? -2 - slot[i] : oa[i];
    }
  }
  store_vec_f32<float, VEC>(o, best);  // a selected input value: exact
  st_i32<VEC>(a, slot);
}

template <typename IdxT, int VEC, int LPR>
__global__ __launch_bounds__(256, 4) void segment_pna_fwd_kernel(const IdxT* __restrict__ col,
                                                              const PnaFwd p) {
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
    const int64_t deg = e - s;
    const int64_t orow = p.row_map ? p.row_map[r] : r;
    // slots of this row that group g scans: g, g + G, ...
    const float cnt_g = g < deg ? static_cast<float>((deg - g + G - 1) / G) : 0.f;
    const float inv_g = g < deg ? 1.f / cnt_g : 0.f;
    for (int fc = 0; fc < p.F; fc += LPR * VEC) {
      const int f = fc + l * VEC;
      const bool active = f < p.F;
      // lanes past F read column 0 (no branch around the loads) and write nothing
      const float* xf = p.x + (active ? f : 0);
      float pv[VEC], s1[VEC], s2[VEC], bmx[VEC], bmn[VEC];
      int smx[VEC], smn[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        pv[i] = s1[i] = s2[i] = bmx[i] = bmn[i] = 0.f;
        smx[i] = smn[i] = -1;
      }

      // The next entry is this group's first (its pivot). One flag per lane, and the loaded
      // row copied out with memcpy: a version that derived `first` per element from
      // slot < 0 and read the raw vector through a float pointer recorded, on gfx950, the
      // group's first slot for element 0 where its second entry won (values were right).
      bool first = true;
      auto take = [&](const R& raw, int off) {
        float ev[VEC];
        __builtin_memcpy(ev, &raw, sizeof(raw));
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float v = ev[i];
          pv[i] = first ? v : pv[i];
          const float d = v - pv[i];
          s1[i] += d;
          s2[i] = fmaf(d, d, s2[i]);
          const bool wx = first || v > bmx[i];
          bmx[i] = wx ? v : bmx[i];
          smx[i] = wx ? off : smx[i];
          const bool wn = first || v < bmn[i];
          bmn[i] = wn ? v : bmn[i];
          smn[i] = wn ? off : smn[i];
        }
        first = false;
      };

      int64_t j = s + g;
      float seen = 0.f;  // entries this group has accumulated
      for (; j + 3 * G < e; j += 4 * G) {
        int64_t c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) c[u] = static_cast<int64_t>(col[j + u * G]);
        R v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const R*>(xf + c[u] * p.ldx);
#pragma unroll
        for (int u = 0; u < 4; ++u) take(v[u], static_cast<int>(j + u * G - s));
        // Re-centre: move the pivot to the running mean, so that S1 stays near 0 however
        // long the row is (with one lane group a hub row is one chain of thousands of
        // entries, and S1 * S1 / n about a first value 2 sigma out loses the bound). The
        // sums follow the shift actually applied, cs = new pivot - old pivot:
        // S2' = S2 - cs (2 S1 - n cs), S1' = S1 - n cs.
        seen += 4.f;
        const float rseen = __builtin_amdgcn_rcpf(seen);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float np = fmaf(s1[i], rseen, pv[i]);
          const float cs = np - pv[i];
          s2[i] = fmaf(-cs, fmaf(-seen, cs, 2.f * s1[i]), s2[i]);
          s1[i] = fmaf(-seen, cs, s1[i]);
          pv[i] = np;
        }
      }
      for (; j < e; j += G) {
        const int64_t c0 = static_cast<int64_t>(col[j]);
        const R v0 = *reinterpret_cast<const R*>(xf + c0 * p.ldx);
        take(v0, static_cast<int>(j - s));
      }

      // this group's (n, mean, M2) about its pivot; an empty group holds (0, 0, 0). The
      // mean stays split as pivot + rl through the merges: the pivots of two groups differ
      // by an exactly representable amount, so delta keeps the precision of the spread and
      // does not round at the magnitude of the values.
      float cnt = cnt_g;
      float rl[VEC], m2[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        rl[i] = s1[i] * inv_g;
        m2[i] = fmaf(-s1[i], rl[i], s2[i]);
      }
      // pairwise merge of the lane groups (Chan et al.): n = n_a + n_b, delta = mean_b -
      // mean_a, mean = mean_a + delta n_b / n, M2 = M2_a + M2_b + delta^2 n_a n_b / n
#pragma unroll
      for (int off = LPR; off < kWave; off <<= 1) {
        const float ocnt = __shfl_xor(cnt, off, kWave);
        const float tot = cnt + ocnt;
        const float w = tot > 0.f ? ocnt / tot : 0.f;
        const float cw = cnt * w;
        const bool adopt = cnt == 0.f;  // nothing here yet: take the partner's pivot too
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          const float opv = __shfl_xor(pv[i], off, kWave);
          const float orl = __shfl_xor(rl[i], off, kWave);
          const float om2 = __shfl_xor(m2[i], off, kWave);
          const float dl = (opv - pv[i]) + (orl - rl[i]);
          rl[i] = adopt ? orl : fmaf(dl, w, rl[i]);
          pv[i] = adopt ? opv : pv[i];
          m2[i] = adopt ? om2 : (m2[i] + om2) + dl * dl * cw;
        }
        cnt = tot;
      }
      float mu[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) mu[i] = pv[i] + rl[i];
      combine_extreme<VEC, LPR, false>(bmx, smx);
      combine_extreme<VEC, LPR, true>(bmn, smn);

      if (g == 0 && active) {
        if (p.mean != nullptr) {
          float* pm = p.mean + orow * p.ld_mean + f;
          float* ps = p.sdev + orow * p.ld_sdev + f;
          if (p.second) {  // the incumbent comes first: (n_a, mean_a, M2_a)
            float ma[VEC], qa[VEC];
            load_vec_f32<float, VEC>(pm, ma);
            load_vec_f32<float, VEC>(ps, qa);
            const float na = static_cast<float>(p.prev_rowptr[orow + 1] - p.prev_rowptr[orow]);
            const float tot = na + cnt;
            const float w = tot > 0.f ? cnt / tot : 0.f;
            const float cw = na * w;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
              const float dl = mu[i] - ma[i];
              mu[i] = fmaf(dl, w, ma[i]);
              m2[i] = (qa[i] + m2[i]) + dl * dl * cw;
            }
            cnt = tot;
          }
          if (p.final) {
            const float n = fmaxf(cnt, 1.f);
#pragma unroll
            for (int i = 0; i < VEC; ++i) m2[i] = sqrtf(fmaxf(m2[i], 0.f) / n + p.eps);
          }
          store_vec_f32<float, VEC>(pm, mu);
          store_vec_f32<float, VEC>(ps, m2);
        }
        // a second pass with no entry in this row leaves the incumbent extremes alone
        const bool ext = !(p.second && deg == 0);
        if (p.vmax != nullptr && ext)
          store_extreme<VEC, false>(p.vmax + orow * p.ld_vmax + f,
                                    p.amax + orow * p.ld_amax + f, bmx, smx, p.second);
        if (p.vmin != nullptr && ext)
          store_extreme<VEC, true>(p.vmin + orow * p.ld_vmin + f,
                                   p.amin + orow * p.ld_amin + f, bmn, smn, p.second);
      }
    }
  }
}

template <typename IdxT, int VEC, int LPR>
__global__ __launch_bounds__(256) void segment_pna_bwd_kernel(const IdxT* __restrict__ col,
                                                              const PnaBwd p) {
  constexpr int G = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR;
  const int l = lane % LPR;
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const bool hm = p.g_mean != nullptr, hs = p.g_std != nullptr;
  const bool hx = p.g_max != nullptr, hn = p.g_min != nullptr;

  struct Ent {  // everything one transposed entry reads from its destination row
    float w;
    int key;
    float gm[VEC], gs[VEC], m[VEC], sd[VEC], gx[VEC], gn[VEC];
    int ax[VEC], an[VEC];
  };

  for (int64_t c = wave; c < p.nrows; c += nwaves) {
    const int64_t s = p.rowptr[c];
    const int64_t e = p.rowptr[c + 1];
    for (int fc = 0; fc < p.F; fc += LPR * VEC) {
      const int f = fc + l * VEC;
      const bool active = f < p.F;
      const int fa = active ? f : 0;
      float xc[VEC], acc[VEC];
      load_vec_f32<float, VEC>(p.x + c * p.ldx + fa, xc);
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[i] = 0.f;

      auto load = [&](Ent& t, int64_t k) {
        const int64_t r = static_cast<int64_t>(col[k]);
        const int q = p.rel[k];
        t.key = p.halo ? -2 - q : q;
        if (hm || hs) t.w = p.inv_deg[r];
        if (hm) load_vec_f32<float, VEC>(p.g_mean + r * p.ld_gmean + fa, t.gm);
        if (hs) {
          load_vec_f32<float, VEC>(p.g_std + r * p.ld_gstd + fa, t.gs);
          load_vec_f32<float, VEC>(p.mean + r * p.ld_mean + fa, t.m);
          load_vec_f32<float, VEC>(p.sdev + r * p.ld_sdev + fa, t.sd);
        }
        if (hx) {
          load_vec_f32<float, VEC>(p.g_max + r * p.ld_gmax + fa, t.gx);
          ld_i32<VEC>(p.amax + r * p.ld_amax + fa, t.ax);
        }
        if (hn) {
          load_vec_f32<float, VEC>(p.g_min + r * p.ld_gmin + fa, t.gn);
          ld_i32<VEC>(p.amin + r * p.ld_amin + fa, t.an);
        }
      };
      auto add = [&](const Ent& t) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          if (hm || hs) {
            float b = hm ? t.gm[i] : 0.f;
            if (hs) b += t.gs[i] * ((xc[i] - t.m[i]) / t.sd[i]);
            acc[i] = fmaf(t.w, b, acc[i]);
          }
          if (hx) acc[i] += t.ax[i] == t.key ? t.gx[i] : 0.f;
          if (hn) acc[i] += t.an[i] == t.key ? t.gn[i] : 0.f;
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

      if (g == 0 && active) {
        float* o = p.out + c * p.ldo + f;
        if (p.beta != 0.f) {
          float old[VEC];
          load_vec_f32<float, VEC>(o, old);
#pragma unroll
          for (int i = 0; i < VEC; ++i) acc[i] = fmaf(p.beta, old[i], acc[i]);
        }
        store_vec_f32<float, VEC>(o, acc);
      }
    }
  }
}

inline bool aligned_to(const void* p, int bytes) {
  return p == nullptr || (reinterpret_cast<uintptr_t>(p) % bytes) == 0;
}

inline dim3 row_grid(int64_t nrows) {
  return dim3(static_cast<unsigned>(cap_blocks((nrows + 3) / 4, 256 * 32)));
}

template <typename IdxT, int VEC>
hipError_t launch_fwd(const IdxT* col, const PnaFwd& a, hipStream_t st) {
  const int lanes = (a.F + VEC - 1) / VEC;
  const dim3 grid = row_grid(a.nrows), block(256);
#define DG_FWD(LPR_)                                                                       \
  hipLaunchKernelGGL((segment_pna_fwd_kernel<IdxT, VEC, LPR_>), grid, block, 0, st, col, a); \
  return hipGetLastError();
  if (lanes <= 8) { DG_FWD(8) }
  if (lanes <= 16) { DG_FWD(16) }
  if (lanes <= 32) { DG_FWD(32) }
  DG_FWD(64)
#undef DG_FWD
}

template <typename IdxT, int VEC>
hipError_t launch_bwd(const IdxT* col, const PnaBwd& a, hipStream_t st) {
  const int lanes = (a.F + VEC - 1) / VEC;
  const dim3 grid = row_grid(a.nrows), block(256);
#define DG_BWD(LPR_)                                                                       \
  hipLaunchKernelGGL((segment_pna_bwd_kernel<IdxT, VEC, LPR_>), grid, block, 0, st, col, a); \
  return hipGetLastError();
  if (lanes <= 8) { DG_BWD(8) }
  if (lanes <= 16) { DG_BWD(16) }
  if (lanes <= 32) { DG_BWD(32) }
  DG_BWD(64)
#undef DG_BWD
}

// a present array allows 16-B accesses: leading dimension a multiple of 4 elements and a
// 16-B aligned base (float and int32 are both 4 bytes wide)
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

hipError_t segment_pna_fwd(IType it, const int64_t* rowptr, const void* col, const float* x,
                           int64_t ldx, float* mean, int64_t ld_mean, float* sdev,
                           int64_t ld_sdev, float* vmax, int64_t ld_vmax, int32_t* amax,
                           int64_t ld_amax, float* vmin, int64_t ld_vmin, int32_t* amin,
                           int64_t ld_amin, int64_t nrows, int F, float eps, bool second,
                           bool final, const int64_t* prev_rowptr, const int64_t* row_map,
                           hipStream_t stream) {
  if (nrows <= 0 || F <= 0) return hipSuccess;
  if ((mean == nullptr) != (sdev == nullptr) || (vmax == nullptr) != (amax == nullptr) ||
      (vmin == nullptr) != (amin == nullptr) || (second && mean && prev_rowptr == nullptr))
    return hipErrorInvalidValue;
  const PnaFwd a{rowptr, x,       ldx,  mean,    ld_mean, sdev, ld_sdev, vmax,
                 ld_vmax, amax,   ld_amax, vmin, ld_vmin, amin, ld_amin, nrows,
                 F,      eps,     second, final, prev_rowptr, row_map};
  // widest vector that divides the row width and every leading dimension and matches every
  // base pointer, as in spmm_max.hip
  const bool v4 = vec4(F, {{x, ldx}, {mean, ld_mean}, {sdev, ld_sdev},
                                       {vmax, ld_vmax}, {amax, ld_amax}, {vmin, ld_vmin},
                                       {amin, ld_amin}});
  if (it == IType::I32) {
    const auto* c = static_cast<const int32_t*>(col);
    return v4 ? launch_fwd<int32_t, 4>(c, a, stream) : launch_fwd<int32_t, 1>(c, a, stream);
  }
  const auto* c = static_cast<const int64_t*>(col);
  return v4 ? launch_fwd<int64_t, 4>(c, a, stream) : launch_fwd<int64_t, 1>(c, a, stream);
}

hipError_t segment_pna_bwd(IType it, const int64_t* t_rowptr, const void* t_col,
                           const int32_t* rel, const float* x, int64_t ldx,
                           const float* inv_deg, const float* g_mean, int64_t ld_gmean,
                           const float* g_std, int64_t ld_gstd, const float* mean,
                           int64_t ld_mean, const float* sdev, int64_t ld_sdev,
                           const float* g_max, int64_t ld_gmax, const int32_t* amax,
                           int64_t ld_amax, const float* g_min, int64_t ld_gmin,
                           const int32_t* amin, int64_t ld_amin, float* out, int64_t ldo,
                           int64_t nrows, int F, bool halo, float beta, hipStream_t stream) {
  if (nrows <= 0 || F <= 0) return hipSuccess;
  if ((g_std && !(mean && sdev)) || ((g_mean || g_std) && !inv_deg) || (g_max && !amax) ||
      (g_min && !amin))
    return hipErrorInvalidValue;
  // arrays whose gradient is absent are never read
  if (!g_std) mean = sdev = nullptr;
  if (!g_max) amax = nullptr;
  if (!g_min) amin = nullptr;
  const PnaBwd a{t_rowptr, rel,    x,       ldx,  inv_deg, g_mean, ld_gmean, g_std, ld_gstd,
                 mean,     ld_mean, sdev,   ld_sdev, g_max, ld_gmax, amax,  ld_amax, g_min,
                 ld_gmin,  amin,   ld_amin, out,  ldo,     nrows,  F,        halo,  beta};
  const bool v4 = vec4(F, {{x, ldx}, {g_mean, ld_gmean}, {g_std, ld_gstd},
                                       {mean, ld_mean}, {sdev, ld_sdev}, {g_max, ld_gmax},
                                       {amax, ld_amax}, {g_min, ld_gmin}, {amin, ld_amin},
                                       {out, ldo}});
  if (it == IType::I32) {
    const auto* c = static_cast<const int32_t*>(t_col);
    return v4 ? launch_bwd<int32_t, 4>(c, a, stream) : launch_bwd<int32_t, 1>(c, a, stream);
  }
  const auto* c = static_cast<const int64_t*>(t_col);
  return v4 ? launch_bwd<int64_t, 4>(c, a, stream) : launch_bwd<int64_t, 1>(c, a, stream);
}

}  // namespace dgraph
