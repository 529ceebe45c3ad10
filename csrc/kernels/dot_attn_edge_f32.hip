// dgraph_amd — fused fp32 scaled dot-product graph attention with edge features for gfx950
// (TransformerConv with edge_dim: the same per-edge row is added to the key and the value).
//
// ee [E, C] holds one fp32 row per CSR slot p of the relation's pattern (the order of col);
// edge (i, j) sits at slot p. Per destination row i and head h (channels [hD, (h+1)D)):
//
//   kk = k_j + ee_p          vv = v_j + ee_p          (one fp32 add each)
//   e_ij  = scale <q_i^h, kk^h>     alpha = softmax_j(e_ij)     out_i^h = beta out_i^h + sum_j alpha vv^h
//   ga    = <g_i^h, vv^h>           c_i^h = <g_i^h, o_i^h>      (an input, as in dot_attn_f32.hip)
//   de    = alpha (ga - c_i^h)
//   dq_i  = scale sum_j de kk       dk_j = scale sum_i de q_i   dv_j = sum_i alpha g_i
//   dee_p = alpha g_i^h + scale de q_i^h
//
// * dot_attn_edge_fwd: dot_attn_fwd with ee_p loaded for slot p = rowptr[r] + k0 + j and
//   added into the gathered k and v vectors. A row's slots are consecutive rows of ee, so ee
//   is streamed once in slot order, not gathered.
// * dot_attn_edge_bwd_dst: dot_attn_bwd_dst with the same operand. Per real slot it also
//   stores dee_p (one 16-B store per lane) and, from the first lane of each head block, the
//   two scalars w[p, h] = alpha and w[p, heads + h] = de (without scale). Every real slot has
//   exactly one writer, so dee and w need no initialisation.
// * dot_attn_edge_bwd_src: per SOURCE row over the transposed pattern: gathers q_i, g_i and
//   the two scalars w[t_slot[p']] of each transposed entry p' and accumulates dv_j += alpha
//   g_i, dk_j += de q_i, scale applied at the end. It reads neither k, v, ee nor the softmax
//   statistics: the weights were formed once, by the destination side. Recomputing alpha
//   here would need a third random [C] gather (ee by forward slot) in what is the widest of
//   the plain kernels; w costs 8 heads bytes per edge next to the 4 C bytes of dee.
//
// Layout, sources, strides, index types and shapes as dot_attn_f32.hip: LPR = C / 4 lanes
// per row, the heads as lane blocks, dot4 / head_sum in the same fixed order (the backward
// recomputes the forward's scores bitwise), two gathered sources, a row stride per operand,
// no LDS, no atomics: bitwise deterministic. The small device helpers are duplicated from
// dot_attn_f32.hip so that file compiles exactly as before.
//
// Padding lanes / slots gather row 0 of the first source, slot 0 of ee and of w, with weight
// 0; the callers launch only when those rows exist (bindings_dot_attn_edge.cpp).
//
// Compiler resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=
// kernel-resource-usage; smallest .. largest of the 24 instantiations of each kernel; no
// LDS, no AGPRs; occupancy in waves per SIMD), at the kU = 8 that is kept:
//   dot_attn_edge_fwd      137 .. 158 VGPRs   scratch 0 B   occupancy 3   (3 kU 16-B vectors)
//   dot_attn_edge_bwd_dst  166 .. 223 VGPRs   scratch 0 B   occupancy 2 .. 3
//     (6 .. 12 SGPRs spilled to VGPR lanes at C = 128 and 256; nothing spilled to memory)
//   dot_attn_edge_bwd_src  100 .. 108 VGPRs   scratch 0 B   occupancy 4
//     (2 kU gathered vectors and 2 kU gathered scalars; nothing resident but dk, dv)
// At kU = 4 the three take 89 .. 99 / 123 .. 142 / 90 .. 102 VGPRs (occupancy 4-5 / 3-4 /
// 4-5), scratch 0 B as well. On an MI355X the two measure within 2 % of each other in all
// three kernels, kU = 8 ahead by 0.6-1.7 % on the destination side (PERFORMANCE.md), so all
// three keep 8, as dot_attn_f32.hip does.
#include "../common.h"
#include "kernels.h"

namespace dgraph {
namespace {

// edges in flight per lane: 3 kU 16-B vectors (k_j, v_j, ee_p) in fwd and bwd_dst, 2 kU
// gathered vectors and 2 kU scalars in bwd_src
constexpr int kU = 8;

struct EdgeArgs {
  const int64_t* rowptr;
  const void* col;
  const void* t_slot;  // bwd_src: forward slot of each transposed entry (col's index type)
  int64_t nrows;
  int C;
  float scale;
  int64_t lds;       // row stride (floats) of stat_m / stat_l / c
  const float* q;    // fwd / bwd_dst: the rows' own q; bwd_src: gathered by destination id
  int64_t ldq;
  const float* k;    // gathered (columns < nsplit)
  int64_t ldk;
  const float* v;
  int64_t ldv;
  const float* k2;   // second source (columns >= nsplit) or nullptr
  int64_t ldk2;
  const float* v2;
  int64_t ldv2;
  int64_t nsplit;
  const float* ee;   // [E, C] by CSR slot
  int64_t ldee;
  float* out;        // fwd
  int64_t ldo;
  float beta;
  float* stat_m;     // [*, heads] written by fwd, read by bwd_dst
  float* stat_l;
  const float* g;    // dL/dout: bwd_dst the rows' own, bwd_src gathered
  int64_t ldg;
  const float* c;    // [*, heads] <g_i^h, o_i^h>
  float* dq;         // bwd_dst
  int64_t lddq;
  float* dee;        // bwd_dst: [E, C] by CSR slot
  int64_t lddee;
  float* w;          // [E, 2 heads] (alpha | de): written by bwd_dst, read by bwd_src
  int64_t ldw;
  float* dk;         // bwd_src
  int64_t lddk;
  float* dv;
  int64_t lddv;
};

template <typename IdxT>
__device__ __forceinline__ int64_t load_idx(const void* p, int64_t pos) {
  return static_cast<int64_t>(static_cast<const IdxT*>(p)[pos]);
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

// this lane's four terms of <a, b>; the order of dot_attn_f32.hip, the same in fwd and bwd_dst
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

__device__ __forceinline__ float4 add4(const float4& a, const float4& b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

__device__ __forceinline__ const float4* vec(const float* p) {
  return reinterpret_cast<const float4*>(p);
}

// ------------------------------------------------------------------------------------ fwd
template <typename IdxT, int LPR, int HH>
__global__ __launch_bounds__(256) void dot_attn_edge_fwd_kernel(EdgeArgs a) {
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
    float m = -INFINITY, lsum = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int64_t my_c = kk < deg ? load_idx<IdxT>(a.col, s + kk) : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 kv[kU], vv[kU];
        float e[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int64_t cj = __shfl(my_c, g * LPR + (j < LPR ? j : 0), kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t c = ok ? cj : 0;
          const int64_t p = ok ? s + k0 + j : 0;  // the entry's slot: consecutive rows of ee
          const bool second = a.k2 && c >= ns;
          const float4 ev = *vec(a.ee + p * a.ldee + f);
          kv[u] = add4(*vec(second ? a.k2 + (c - ns) * a.ldk2 + f : a.k + c * a.ldk + f), ev);
          vv[u] = add4(*vec(second ? a.v2 + (c - ns) * a.ldv2 + f : a.v + c * a.ldv + f), ev);
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
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
    acc.x *= inv;
    acc.y *= inv;
    acc.z *= inv;
    acc.w *= inv;
    float* o = a.out + r * a.ldo + f;
    if (a.beta != 0.f) {
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
__global__ __launch_bounds__(256) void dot_attn_edge_bwd_dst_kernel(EdgeArgs a) {
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
      const int64_t my_col = kk < deg ? load_idx<IdxT>(a.col, s + kk) : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 kv[kU], vv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int64_t cj = __shfl(my_col, g * LPR + (j < LPR ? j : 0), kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t c = ok ? cj : 0;
          const int64_t p = ok ? s + k0 + j : 0;
          const bool second = a.k2 && c >= ns;
          const float4 ev = *vec(a.ee + p * a.ldee + f);
          kv[u] = add4(*vec(second ? a.k2 + (c - ns) * a.ldk2 + f : a.k + c * a.ldk + f), ev);
          vv[u] = add4(*vec(second ? a.v2 + (c - ns) * a.ldv2 + f : a.v + c * a.ldv + f), ev);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          const float e = a.scale * head_sum<LH>(dot4(qv, kv[u]));
          const float ga = head_sum<LH>(dot4(gv, vv[u]));
          const float al = ok ? __expf(e - my_m) * my_inv : 0.f;
          const float de = ok ? al * (ga - my_c) : 0.f;
          axpy4(de, kv[u], acc);
          if (ok) {  // this slot's only writer
            const int64_t p = s + k0 + j;
            const float t = a.scale * de;
            float4 d;
            d.x = fmaf(t, qv.x, al * gv.x);
            d.y = fmaf(t, qv.y, al * gv.y);
            d.z = fmaf(t, qv.z, al * gv.z);
            d.w = fmaf(t, qv.w, al * gv.w);
            *reinterpret_cast<float4*>(a.dee + p * a.lddee + f) = d;
            if (l % LH == 0) {
              a.w[p * a.ldw + hk] = al;
              a.w[p * a.ldw + HH + hk] = de;
            }
          }
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
__global__ __launch_bounds__(256) void dot_attn_edge_bwd_src_kernel(EdgeArgs a) {
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
    const int64_t s = has_row ? a.rowptr[r] : 0;
    const int deg = has_row ? static_cast<int>(a.rowptr[r + 1] - s) : 0;
    const int maxdeg = group_imax<LPR>(deg);
    float4 dk = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 dv = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int64_t my_i = kk < deg ? load_idx<IdxT>(a.col, s + kk) : 0;
      const int64_t my_p = kk < deg ? load_idx<IdxT>(a.t_slot, s + kk) : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 qg[kU], gg[kU];
        float al[kU], de[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int src_lane = g * LPR + (j < LPR ? j : 0);
          const int64_t i = __shfl(my_i, src_lane, kWave);
          const int64_t p = __shfl(my_p, src_lane, kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t ii = ok ? i : 0;
          const int64_t pp = ok ? p : 0;
          qg[u] = *vec(a.q + ii * a.ldq + f);
          gg[u] = *vec(a.g + ii * a.ldg + f);
          const float wa = a.w[pp * a.ldw + hk];
          const float wd = a.w[pp * a.ldw + HH + hk];
          al[u] = ok ? wa : 0.f;
          de[u] = ok ? wd : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          axpy4(al[u], gg[u], dv);
          axpy4(de[u], qg[u], dk);
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
void launch_one(const EdgeArgs& a, int64_t blocks, hipStream_t st) {
  dim3 grid(static_cast<unsigned>(blocks)), block(256);
  if constexpr (KIND == 0)
    hipLaunchKernelGGL((dot_attn_edge_fwd_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
  else if constexpr (KIND == 1)
    hipLaunchKernelGGL((dot_attn_edge_bwd_dst_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((dot_attn_edge_bwd_src_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
}

template <int KIND, typename IdxT>
hipError_t launch_kind(const EdgeArgs& a, int heads, hipStream_t st) {
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
hipError_t launch(const EdgeArgs& a, IType it, int heads, hipStream_t st) {
  if (a.nrows <= 0) return hipSuccess;
  if (!dot_attn_f32_shape_ok(a.C, heads)) return hipErrorInvalidValue;
  return it == IType::I32 ? launch_kind<KIND, int32_t>(a, heads, st)
                          : launch_kind<KIND, int64_t>(a, heads, st);
}

}  // namespace

hipError_t dot_attn_edge_fwd_f32(IType it, const int64_t* rowptr, const void* col,
                                 int64_t nrows, int C, int heads, int64_t lds, float scale,
                                 const float* q, int64_t ldq, const float* k, int64_t ldk,
                                 const float* v, int64_t ldv, const float* k2, int64_t ldk2,
                                 const float* v2, int64_t ldv2, int64_t nsplit,
                                 const float* ee, int64_t ldee, float* out, int64_t ldo,
                                 float beta, float* stat_m, float* stat_l, hipStream_t st) {
  EdgeArgs a{};
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
  a.ee = ee;
  a.ldee = ldee;
  a.out = out;
  a.ldo = ldo;
  a.beta = beta;
  a.stat_m = stat_m;
  a.stat_l = stat_l;
  return launch<0>(a, it, heads, st);
}

hipError_t dot_attn_edge_bwd_dst_f32(IType it, const int64_t* rowptr, const void* col,
                                     int64_t nrows, int C, int heads, int64_t lds, float scale,
                                     const float* q, int64_t ldq, const float* k, int64_t ldk,
                                     const float* v, int64_t ldv, const float* k2,
                                     int64_t ldk2, const float* v2, int64_t ldv2,
                                     int64_t nsplit, const float* ee, int64_t ldee,
                                     const float* stat_m, const float* stat_l, const float* g,
                                     int64_t ldg, const float* c, float* dq, int64_t lddq,
                                     float* dee, int64_t lddee, float* w, int64_t ldw,
                                     hipStream_t st) {
  EdgeArgs a{};
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
  a.ee = ee;
  a.ldee = ldee;
  a.stat_m = const_cast<float*>(stat_m);
  a.stat_l = const_cast<float*>(stat_l);
  a.g = g;
  a.ldg = ldg;
  a.c = c;
  a.dq = dq;
  a.lddq = lddq;
  a.dee = dee;
  a.lddee = lddee;
  a.w = w;
  a.ldw = ldw;
  return launch<1>(a, it, heads, st);
}

hipError_t dot_attn_edge_bwd_src_f32(IType it, const int64_t* rowptr, const void* col,
                                     const void* t_slot, int64_t nrows, int C, int heads,
                                     float scale, const float* q, int64_t ldq, const float* g,
                                     int64_t ldg, const float* w, int64_t ldw, float* dk,
                                     int64_t lddk, float* dv, int64_t lddv, hipStream_t st) {
  EdgeArgs a{};
  a.rowptr = rowptr;
  a.col = col;
  a.t_slot = t_slot;
  a.nrows = nrows;
  a.C = C;
  a.scale = scale;
  a.q = q;
  a.ldq = ldq;
  a.g = g;
  a.ldg = ldg;
  a.w = const_cast<float*>(w);
  a.ldw = ldw;
  a.dk = dk;
  a.lddk = lddk;
  a.dv = dv;
  a.lddv = lddv;
  return launch<2>(a, it, heads, st);
}

}  // namespace dgraph
