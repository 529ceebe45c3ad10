// dgraph_amd — fused fp32 scaled dot-product graph attention for gfx950 (TransformerConv).
//
// For one relation, per destination row i and head h (channels [hD, (h+1)D) of C = heads D):
//
//   e_ij  = scale <q_i^h, k_j^h>
//   alpha = softmax_j(e_ij)                                  (max-subtracted)
//   out_i^h = beta out_i^h + sum_j alpha_ij v_j^h
//
// Composed from gather_rows + edge_softmax + the weighted SpMM this is [E, C] tensors for
// q_i, k_j, the products and v_j; here it is three row-parallel kernels and nothing per edge
// is ever written:
//
// * dot_attn_fwd: per destination row with q_i resident, ONE pass over the row's edges that
//   gathers k_j and v_j once each. The score needs the whole k_j row, so there is no cheap
//   statistics pass as in gat_f32.hip: a running maximum is kept instead, and the
//   accumulator and the running sum are rescaled once per chunk of kU edges (not per edge).
//   Writes out, stat_m (the row maximum of e) and stat_l (1 / sum exp(e - m); 0 for an
//   empty row, whose stat_m is unspecified). Its CARRY instantiations (dot_attn_fwd_carry)
//   start the running maximum, sum and accumulator from an earlier pass's (out, stat_m,
//   stat_l) instead of (0, -inf, 0): a softmax over a union of edge sets, one set per launch
//   (interior edges while the halo is on the links, then the halo edges; several relations
//   with their own q / k / v). The backward kernels need nothing new: they recompute alpha
//   from the final statistics and so work on any subset of the edges.
// * dot_attn_bwd_dst: per destination row with g_i = dL/dout_i and q_i resident: gathers
//   k_j and v_j, ga = <g^h, v_j^h>, de = alpha (ga - c), dq_i = scale sum_j de k_j.
//   c_i^h = sum_j alpha ga = <g_i^h, o_i^h> is an input (the caller has the forward's own
//   output): de is formed per edge, never as a difference of two accumulated sums.
// * dot_attn_bwd_src: per SOURCE row over the transposed pattern with k_j and v_j resident:
//   gathers q_i, g_i and the destinations' m, 1/l, c, recomputes alpha, and accumulates
//   dv_j = sum_i alpha g_i and dk_j = scale sum_i de q_i.
//
// Two sources (k / v for columns < nsplit, k2 / v2 for columns >= nsplit: local rows and
// received halo rows, never concatenated). Every feature array has its own row stride, so k
// and v may be the column halves of one [N, 2C] buffer; the per-head arrays share the row
// stride lds. Layout as gat_f32.hip: one LPR-lane group per row (LPR = C / 4, 16-B fp32
// vectors), the heads as contiguous blocks of LH = LPR / heads lanes, the per-head dot
// product by xor shuffles inside a block (every lane of a head holds the same sum). No LDS,
// no atomics, fixed summation orders: bitwise deterministic.
//
// Padding lanes / slots (a wave's groups run to the longest row of the wave) gather row 0
// of the first source with weight 0; the callers guarantee that row exists whenever a
// kernel is launched (bindings_dot_attn.cpp).
//
// Compiler resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=
// kernel-resource-usage; smallest .. largest of the 24 instantiations of each kernel at
// kU = 8; no LDS, no AGPRs; 512 VGPRs per SIMD lane, so waves per SIMD = 512 / VGPRs):
//   dot_attn_fwd      102 .. 122 VGPRs   scratch 0 B   occupancy 4     (2 kU gathered vectors)
//   dot_attn_fwd, CARRY  104 .. 130 VGPRs   scratch 0 B   occupancy 3 .. 4
//     (the carried state is loaded under two branches before the loop; the 24 plain
//     instantiations compile to the same figures, SGPRs included, as without the template
//     parameter)
//   dot_attn_bwd_dst  109 .. 128 VGPRs   scratch 0 B   occupancy 4
//   dot_attn_bwd_src  149 .. 178 VGPRs   scratch 0 B   occupancy 2 .. 3
//     (4 resident / accumulator vectors, 2 kU gathered ones and 3 kU gathered statistics)
// At kU = 4 the three take 70 .. 75 / 77 .. 82 / 102 .. 114 VGPRs (occupancy 6-7 / 5-6 / 4):
// the gathered vectors in flight per SIMD (occupancy x 2 kU) are about the same either way,
// and on an MI355X the two measure the same within 1 % in all three kernels
// (PERFORMANCE.md); kU = 8 halves the rescales of the forward and matches gat_f32.hip.
#include "../common.h"
#include "kernels.h"

namespace dgraph {
namespace {

constexpr int kU = 8;  // edges in flight per lane: 2 kU gathered 16-B vectors

struct DotArgs {
  const int64_t* rowptr;
  const void* col;
  int64_t nrows;
  int C;
  float scale;
  int64_t lds;       // row stride (floats) of stat_m / stat_l / c
  const float* q;    // fwd / bwd_dst: the rows' own q; bwd_src: gathered by destination id
  int64_t ldq;
  const float* k;    // fwd / bwd_dst: gathered (columns < nsplit); bwd_src: the rows' own
  int64_t ldk;
  const float* v;
  int64_t ldv;
  const float* k2;   // second source (columns >= nsplit) or nullptr
  int64_t ldk2;
  const float* v2;
  int64_t ldv2;
  int64_t nsplit;
  float* out;        // fwd
  int64_t ldo;
  float beta;
  float* stat_m;     // [*, heads] written by fwd, read by the backward kernels
  float* stat_l;
  const float* g;    // dL/dout: bwd_dst the rows' own, bwd_src gathered
  int64_t ldg;
  const float* c;    // [*, heads] <g_i^h, o_i^h>
  float* dq;         // bwd_dst
  int64_t lddq;
  float* dk;         // bwd_src
  int64_t lddk;
  float* dv;
  int64_t lddv;
};

template <typename IdxT>
__device__ __forceinline__ int64_t load_col(const DotArgs& a, int64_t pos) {
  return static_cast<int64_t>(static_cast<const IdxT*>(a.col)[pos]);
}

// sum over the LH lanes of one head (contiguous, aligned lane blocks); the same in all of them
template <int LH>
__device__ __forceinline__ float head_sum(float v) {
#pragma unroll
  for (int off = LH / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// the longest row among the wave's row groups
template <int LPR>
__device__ __forceinline__ int group_imax(int v) {
#pragma unroll
  for (int off = LPR; off < kWave; off <<= 1) {
    const int o = __shfl_xor(v, off, kWave);
    v = o > v ? o : v;
  }
  return v;
}

// this lane's four terms of <a, b>; one fixed order in all three kernels, so the backward
// recomputes the forward's scores bitwise
__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
  float p = a.x * b.x;
  p = fmaf(a.y, b.y, p);
  p = fmaf(a.z, b.z, p);
  return fmaf(a.w, b.w, p);
}

__device__ __forceinline__ void axpy4(float w, const float4& x, float4& acc) {
  acc.x = fmaf(w, x.x, acc.x);
  acc.y = fmaf(w, x.y, acc.y);
  acc.z = fmaf(w, x.z, acc.z);
  acc.w = fmaf(w, x.w, acc.w);
}

__device__ __forceinline__ const float4* vec(const float* p) {
  return reinterpret_cast<const float4*>(p);
}

// ------------------------------------------------------------------------------------ fwd
// CARRY: the softmax state of the rows starts from an earlier pass's (out, stat_m, stat_l)
// instead of (0, -inf, 0), so the result is the softmax over the union of the passes' edge
// sets. stat_l == 0 on entry: nothing accumulated yet, out and stat_m are not read (they may
// hold anything). A row without entries in this pass is left bitwise untouched and its q is
// not loaded (its lanes still serve the wave's shuffles, with weight 0).
template <typename IdxT, int LPR, int HH, bool CARRY>
__global__ __launch_bounds__(256) void dot_attn_fwd_kernel(DotArgs a) {
  constexpr int G = kWave / LPR;
  constexpr int LH = LPR / HH;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, l = lane % LPR, hk = l / LH;
  const int f = 4 * l;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  const int64_t q0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t qstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const int64_t ns = a.nsplit;
  for (int64_t q = q0; q < ngroups; q += qstep) {
    const int64_t r = q * G + g;
    const bool has_row = r < a.nrows;
    const int64_t rr = has_row ? r : 0;
    const int64_t s = has_row ? a.rowptr[r] : 0;
    const int deg = has_row ? static_cast<int>(a.rowptr[r + 1] - s) : 0;
    const int maxdeg = group_imax<LPR>(deg);
    float4 qv;
    float m = -INFINITY, lsum = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (CARRY) {
      qv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (deg > 0) {
        qv = *vec(a.q + r * a.ldq + f);
        const float L = a.stat_l[r * a.lds + hk];
        if (L > 0.f) {  // out is normalised: acc = out * sum, sum = 1 / L
          m = a.stat_m[r * a.lds + hk];
          lsum = 1.f / L;
          const float4 old = *vec(a.out + r * a.ldo + f);
          acc = make_float4(old.x * lsum, old.y * lsum, old.z * lsum, old.w * lsum);
        }
      }
    } else {
      qv = *vec(a.q + rr * a.ldq + f);
    }
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int64_t my_c = kk < deg ? load_col<IdxT>(a, s + kk) : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 kv[kU], vv[kU];
        float e[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int64_t cj = __shfl(my_c, g * LPR + (j < LPR ? j : 0), kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t c = ok ? cj : 0;
          const bool second = a.k2 && c >= ns;
          kv[u] = *vec(second ? a.k2 + (c - ns) * a.ldk2 + f : a.k + c * a.ldk + f);
          vv[u] = *vec(second ? a.v2 + (c - ns) * a.ldv2 + f : a.v + c * a.ldv + f);
        }
        // the chunk's scores and the new running maximum
        float mc = m;
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          e[u] = ok ? a.scale * head_sum<LH>(dot4(qv, kv[u])) : -INFINITY;
          mc = fmaxf(mc, e[u]);
        }
        // one rescale per chunk (mc = -inf: nothing seen yet, acc and lsum are 0)
        const float rs = mc == -INFINITY ? 1.f : __expf(m - mc);
        m = mc;
        lsum *= rs;
        acc.x *= rs;
        acc.y *= rs;
        acc.z *= rs;
        acc.w *= rs;
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const float p = e[u] == -INFINITY ? 0.f : __expf(e[u] - mc);
          lsum += p;
          axpy4(p, vv[u], acc);
        }
      }
    }
    if (!has_row) continue;
    if constexpr (CARRY) {
      if (deg == 0) continue;  // the carried state of the row is its result
    }
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
    acc.x *= inv;
    acc.y *= inv;
    acc.z *= inv;
    acc.w *= inv;
    float* o = a.out + r * a.ldo + f;
    if (!CARRY && a.beta != 0.f) {
      const float4 old = *vec(o);
      acc.x = fmaf(a.beta, old.x, acc.x);
      acc.y = fmaf(a.beta, old.y, acc.y);
      acc.z = fmaf(a.beta, old.z, acc.z);
      acc.w = fmaf(a.beta, old.w, acc.w);
    }
    *reinterpret_cast<float4*>(o) = acc;
    if (l % LH == 0) {
      a.stat_m[r * a.lds + hk] = m;
      a.stat_l[r * a.lds + hk] = inv;  // 1 / sum (0 for an empty row)
    }
  }
}

// -------------------------------------------------------------------------------- bwd dst
template <typename IdxT, int LPR, int HH>
__global__ __launch_bounds__(256) void dot_attn_bwd_dst_kernel(DotArgs a) {
  constexpr int G = kWave / LPR;
  constexpr int LH = LPR / HH;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, l = lane % LPR, hk = l / LH;
  const int f = 4 * l;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  const int64_t q0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t qstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const int64_t ns = a.nsplit;
  for (int64_t q = q0; q < ngroups; q += qstep) {
    const int64_t r = q * G + g;
    const bool has_row = r < a.nrows;
    const int64_t rr = has_row ? r : 0;
    const int64_t s = has_row ? a.rowptr[r] : 0;
    const int deg = has_row ? static_cast<int>(a.rowptr[r + 1] - s) : 0;
    const int maxdeg = group_imax<LPR>(deg);
    const float4 qv = *vec(a.q + rr * a.ldq + f);
    const float4 gv = *vec(a.g + rr * a.ldg + f);
    const float my_m = a.stat_m[rr * a.lds + hk];
    const float my_inv = a.stat_l[rr * a.lds + hk];
    const float my_c = a.c[rr * a.lds + hk];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int64_t my_col = kk < deg ? load_col<IdxT>(a, s + kk) : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 kv[kU], vv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int64_t cj = __shfl(my_col, g * LPR + (j < LPR ? j : 0), kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t c = ok ? cj : 0;
          const bool second = a.k2 && c >= ns;
          kv[u] = *vec(second ? a.k2 + (c - ns) * a.ldk2 + f : a.k + c * a.ldk + f);
          vv[u] = *vec(second ? a.v2 + (c - ns) * a.ldv2 + f : a.v + c * a.ldv + f);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          const float e = a.scale * head_sum<LH>(dot4(qv, kv[u]));
          const float ga = head_sum<LH>(dot4(gv, vv[u]));
          const float de = ok ? __expf(e - my_m) * my_inv * (ga - my_c) : 0.f;
          axpy4(de, kv[u], acc);
        }
      }
    }
    if (!has_row) continue;
    acc.x *= a.scale;
    acc.y *= a.scale;
    acc.z *= a.scale;
    acc.w *= a.scale;
    *reinterpret_cast<float4*>(a.dq + r * a.lddq + f) = acc;
  }
}

// -------------------------------------------------------------------------------- bwd src
template <typename IdxT, int LPR, int HH>
__global__ __launch_bounds__(256) void dot_attn_bwd_src_kernel(DotArgs a) {
  constexpr int G = kWave / LPR;
  constexpr int LH = LPR / HH;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, l = lane % LPR, hk = l / LH;
  const int f = 4 * l;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  const int64_t q0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t qstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  for (int64_t q = q0; q < ngroups; q += qstep) {
    const int64_t r = q * G + g;
    const bool has_row = r < a.nrows;
    const int64_t rr = has_row ? r : 0;
    const int64_t s = has_row ? a.rowptr[r] : 0;
    const int deg = has_row ? static_cast<int>(a.rowptr[r + 1] - s) : 0;
    const int maxdeg = group_imax<LPR>(deg);
    const float4 kv = *vec(a.k + rr * a.ldk + f);
    const float4 vv = *vec(a.v + rr * a.ldv + f);
    float4 dk = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 dv = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int64_t my_i = kk < deg ? load_col<IdxT>(a, s + kk) : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 qg[kU], gg[kU];
        float m[kU], il[kU], c[kU];
        bool ok[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int64_t i = __shfl(my_i, g * LPR + (j < LPR ? j : 0), kWave);
          ok[u] = j < LPR && k0 + j < deg;
          const int64_t ii = ok[u] ? i : 0;
          qg[u] = *vec(a.q + ii * a.ldq + f);
          gg[u] = *vec(a.g + ii * a.ldg + f);
          m[u] = a.stat_m[ii * a.lds + hk];
          il[u] = a.stat_l[ii * a.lds + hk];
          c[u] = a.c[ii * a.lds + hk];
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const float e = a.scale * head_sum<LH>(dot4(qg[u], kv));
          const float ga = head_sum<LH>(dot4(gg[u], vv));
          const float al = ok[u] ? __expf(e - m[u]) * il[u] : 0.f;
          const float de = ok[u] ? al * (ga - c[u]) : 0.f;
          axpy4(al, gg[u], dv);
          axpy4(de, qg[u], dk);
        }
      }
    }
    if (!has_row) continue;
    dk.x *= a.scale;
    dk.y *= a.scale;
    dk.z *= a.scale;
    dk.w *= a.scale;
    *reinterpret_cast<float4*>(a.dk + r * a.lddk + f) = dk;
    *reinterpret_cast<float4*>(a.dv + r * a.lddv + f) = dv;
  }
}

template <int KIND, typename IdxT, int LPR, int HH>
void launch_one(const DotArgs& a, int64_t blocks, hipStream_t st) {
  dim3 grid(static_cast<unsigned>(blocks)), block(256);
  if constexpr (KIND == 0)
    hipLaunchKernelGGL((dot_attn_fwd_kernel<IdxT, LPR, HH, false>), grid, block, 0, st, a);
  else if constexpr (KIND == 3)
    hipLaunchKernelGGL((dot_attn_fwd_kernel<IdxT, LPR, HH, true>), grid, block, 0, st, a);
  else if constexpr (KIND == 1)
    hipLaunchKernelGGL((dot_attn_bwd_dst_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((dot_attn_bwd_src_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
}

template <int KIND, typename IdxT>
hipError_t launch_kind(const DotArgs& a, int heads, hipStream_t st) {
  const int LPR = a.C / 4;
  const int64_t G = kWave / LPR;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  int64_t blocks = (ngroups + 3) / 4;  // one row group per wave, in order
  if (blocks < 1) blocks = 1;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
#define DG_DOT(L_, H_)                                   \
  if (LPR == L_ && heads == H_) {                        \
    launch_one<KIND, IdxT, L_, H_>(a, blocks, st);       \
    return hipGetLastError();                            \
  }
  DG_DOT(16, 1) DG_DOT(16, 2) DG_DOT(16, 4) DG_DOT(16, 8)
  DG_DOT(32, 1) DG_DOT(32, 2) DG_DOT(32, 4) DG_DOT(32, 8)
  DG_DOT(64, 1) DG_DOT(64, 2) DG_DOT(64, 4) DG_DOT(64, 8)
#undef DG_DOT
  return hipErrorInvalidValue;
}

template <int KIND>
hipError_t launch(const DotArgs& a, IType it, int heads, hipStream_t st) {
  if (a.nrows <= 0) return hipSuccess;
  if (!dot_attn_f32_shape_ok(a.C, heads)) return hipErrorInvalidValue;
  return it == IType::I32 ? launch_kind<KIND, int32_t>(a, heads, st)
                          : launch_kind<KIND, int64_t>(a, heads, st);
}

}  // namespace

bool dot_attn_f32_shape_ok(int C, int heads) { return gat_f32_shape_ok(C, heads); }

hipError_t dot_attn_fwd_f32(IType it, const int64_t* rowptr, const void* col, int64_t nrows,
                            int C, int heads, int64_t lds, float scale, const float* q,
                            int64_t ldq, const float* k, int64_t ldk, const float* v,
                            int64_t ldv, const float* k2, int64_t ldk2, const float* v2,
                            int64_t ldv2, int64_t nsplit, float* out, int64_t ldo, float beta,
                            float* stat_m, float* stat_l, hipStream_t st) {
  DotArgs a{};
  a.rowptr = rowptr;
  a.col = col;
  a.nrows = nrows;
  a.C = C;
  a.lds = lds;
  a.scale = scale;
  a.q = q;
  a.ldq = ldq;
  a.k = k;
  a.ldk = ldk;
  a.v = v;
  a.ldv = ldv;
  a.k2 = k2;
  a.ldk2 = ldk2;
  a.v2 = v2;
  a.ldv2 = ldv2;
  a.nsplit = nsplit;
  a.out = out;
  a.ldo = ldo;
  a.beta = beta;
  a.stat_m = stat_m;
  a.stat_l = stat_l;
  return launch<0>(a, it, heads, st);
}

hipError_t dot_attn_fwd_carry_f32(IType it, const int64_t* rowptr, const void* col,
                                  int64_t nrows, int C, int heads, int64_t lds, float scale,
                                  const float* q, int64_t ldq, const float* k, int64_t ldk,
                                  const float* v, int64_t ldv, const float* k2, int64_t ldk2,
                                  const float* v2, int64_t ldv2, int64_t nsplit, float* out,
                                  int64_t ldo, float* stat_m, float* stat_l, hipStream_t st) {
  DotArgs a{};
  a.rowptr = rowptr;
  a.col = col;
  a.nrows = nrows;
  a.C = C;
  a.lds = lds;
  a.scale = scale;
  a.q = q;
  a.ldq = ldq;
  a.k = k;
  a.ldk = ldk;
  a.v = v;
  a.ldv = ldv;
  a.k2 = k2;
  a.ldk2 = ldk2;
  a.v2 = v2;
  a.ldv2 = ldv2;
  a.nsplit = nsplit;
  a.out = out;
  a.ldo = ldo;
  a.stat_m = stat_m;
  a.stat_l = stat_l;
  return launch<3>(a, it, heads, st);
}

hipError_t dot_attn_bwd_dst_f32(IType it, const int64_t* rowptr, const void* col,
                                int64_t nrows, int C, int heads, int64_t lds, float scale,
                                const float* q, int64_t ldq, const float* k, int64_t ldk,
                                const float* v, int64_t ldv, const float* k2, int64_t ldk2,
                                const float* v2, int64_t ldv2, int64_t nsplit,
                                const float* stat_m, const float* stat_l, const float* g,
                                int64_t ldg, const float* c, float* dq, int64_t lddq,
                                hipStream_t st) {
  DotArgs a{};
  a.rowptr = rowptr;
  a.col = col;
  a.nrows = nrows;
  a.C = C;
  a.lds = lds;
  a.scale = scale;
  a.q = q;
  a.ldq = ldq;
  a.k = k;
  a.ldk = ldk;
  a.v = v;
  a.ldv = ldv;
  a.k2 = k2;
  a.ldk2 = ldk2;
  a.v2 = v2;
  a.ldv2 = ldv2;
  a.nsplit = nsplit;
  a.stat_m = const_cast<float*>(stat_m);
  a.stat_l = const_cast<float*>(stat_l);
  a.g = g;
  a.ldg = ldg;
  a.c = c;
  a.dq = dq;
  a.lddq = lddq;
  return launch<1>(a, it, heads, st);
}

hipError_t dot_attn_bwd_src_f32(IType it, const int64_t* rowptr, const void* col,
                                int64_t nrows, int C, int heads, int64_t lds, float scale,
                                const float* q, int64_t ldq, const float* g, int64_t ldg,
                                const float* k, int64_t ldk, const float* v, int64_t ldv,
                                const float* stat_m, const float* stat_l, const float* c,
                                float* dk, int64_t lddk, float* dv, int64_t lddv,
                                hipStream_t st) {
  DotArgs a{};
  a.rowptr = rowptr;
  a.col = col;
  a.nrows = nrows;
  a.C = C;
  a.lds = lds;
  a.scale = scale;
  a.q = q;
  a.ldq = ldq;
  a.g = g;
  a.ldg = ldg;
  a.k = k;
  a.ldk = ldk;
  a.v = v;
  a.ldv = ldv;
  a.stat_m = const_cast<float*>(stat_m);
  a.stat_l = const_cast<float*>(stat_l);
  a.c = c;
  a.dk = dk;
  a.lddk = lddk;
  a.dv = dv;
  a.lddv = lddv;
  return launch<2>(a, it, heads, st);
}

}  // namespace dgraph
