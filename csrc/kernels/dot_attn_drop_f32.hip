// dgraph_amd — fused fp32 scaled dot-product graph attention with dropout on the attention
// coefficients for gfx950 (PyG's TransformerConv(..., dropout=p) in training).
//
// Dropout is applied after the softmax. With keep(p', h) the Philox4x32-10 decision of
// philox.h for the edge's CSR slot p' and head h, and mm = keep / (1 - p) (0 or inv_keep):
//
//   e_ij  = scale <q_i^h, k_j^h>     alpha = softmax_j(e_ij)   over ALL edges of the row
//   out_i^h = sum_j alpha mm v_j^h
//   ga    = <g_i^h, v_j^h>           c_i^h = <g_i^h, o_i^h>    (an input, as in dot_attn_f32.hip)
//   de    = alpha (mm ga - c_i^h)
//   dq_i  = scale sum_j de k_j       dk_j = scale sum_i de q_i       dv_j = sum_i alpha mm g_i
//
// stat_m / stat_l are those of the plain forward: dropout does not enter the softmax
// statistics. A row whose edges are all dropped gives out = 0, hence c = 0 and every de = 0.
//
// * dot_attn_drop_fwd: dot_attn_fwd (no beta, no carry). The lane that loads the column id of
//   slot s + k0 + l also evaluates the slot's keep bits (one Philox call per lane per LPR
//   edges, two at 8 heads); the bits travel with the column id through one more __shfl. The
//   running sum takes every edge, the accumulator only the kept ones, times inv_keep.
// * dot_attn_drop_bwd_dst: dot_attn_bwd_dst with the same bits and de as above.
// * dot_attn_drop_bwd_src: dot_attn_bwd_src over the transposed pattern; the lane that loads
//   the transposed entry's destination id also loads its forward slot from t_slot (col's
//   index type, indexed by absolute position as col is) and evaluates the bits from it.
//
// The mask is never stored: all three kernels regenerate it from (seed, slot, head). seed is
// a pointer to ONE int64 in device memory, read by the kernels, so a step captured into a
// HIP graph draws a fresh mask per replay when the caller refreshes that value inside the
// captured region. thr = floor(p 2^32), inv_keep = 1 / (1 - p) formed once on the host.
//
// Layout, sources, strides, index types and shapes as dot_attn_f32.hip: LPR = C / 4 lanes
// per row, the heads as lane blocks, dot4 / head_sum in the same fixed order (the backward
// recomputes the forward's scores bitwise), two gathered sources, a row stride per operand,
// no LDS, no atomics: bitwise deterministic for a fixed seed. The small device helpers are
// duplicated from dot_attn_f32.hip so that file compiles exactly as before.
//
// Padding lanes / slots gather row 0 of the first source with weight 0 and evaluate no
// Philox call (bits 0); the callers launch only when that row exists
// (bindings_dot_attn_drop.cpp).
//
// Compiler resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=
// kernel-resource-usage; smallest .. largest of the 24 instantiations of each kernel at
// kU = 8; no LDS, no AGPRs; occupancy in waves per SIMD):
//   dot_attn_drop_fwd      114 .. 133 VGPRs   scratch 0 B   occupancy 3 .. 4
//   dot_attn_drop_bwd_dst  121 .. 141 VGPRs   scratch 0 B   occupancy 3 .. 4
//   dot_attn_drop_bwd_src  159 .. 186 VGPRs   scratch 0 B   occupancy 2 .. 3
// (0 .. 10 SGPRs spilled to VGPR lanes in fwd and bwd_dst; nothing spilled to memory.) That
// is 8 .. 13 VGPRs over dot_attn_f32.hip: the kU keep factors of a chunk and the bits that
// travel with the column id. Occupancy 3 is the C = 64 instantiations of fwd and bwd_dst
// (132 .. 141 VGPRs, the 8-head forward at 128 excepted; the plain ones sit at or under the
// 128 of occupancy 4), occupancy 2 the C = 64 source side at 2 .. 8 heads, as in the plain
// file. Keeping the chunk's keep flags
// packed in one register instead of kU floats was tried and compiles to 1 .. 2 VGPRs MORE.
#include "../common.h"
#include "kernels.h"
#include "philox.h"

namespace dgraph {
namespace {

constexpr int kU = 8;  // edges in flight per lane: 2 kU gathered 16-B vectors

struct DropArgs {
  const int64_t* rowptr;
  const void* col;
  const void* t_slot;  // bwd_src: forward slot of each transposed entry (col's index type)
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
  const int64_t* seed;  // one int64 in device memory
  uint32_t thr;         // keep when the head's Philox word >= thr
  float inv_keep;       // 1 / (1 - p)
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

// this lane's four terms of <a, b>; the order of dot_attn_f32.hip, the same in all three
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
template <typename IdxT, int LPR, int HH>
__global__ __launch_bounds__(256) void dot_attn_drop_fwd_kernel(DropArgs a) {
  constexpr int G = kWave / LPR;
  constexpr int LH = LPR / HH;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, l = lane % LPR, hk = l / LH;
  const int f = 4 * l;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  const int64_t q0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t qstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const int64_t ns = a.nsplit;
  const uint64_t seed = static_cast<uint64_t>(*a.seed);
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
      // the keep bits of this lane's slot, all heads (a padding slot: nothing evaluated)
      const uint32_t my_b = kk < deg ? attn_keep_bits(seed, s + kk, a.thr, HH) : 0u;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 kv[kU], vv[kU];
        float e[kU], mm[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int src_lane = g * LPR + (j < LPR ? j : 0);
          const int64_t cj = __shfl(my_c, src_lane, kWave);
          const uint32_t bj = __shfl(my_b, src_lane, kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t c = ok ? cj : 0;
          const bool second = a.k2 && c >= ns;
          kv[u] = *vec(second ? a.k2 + (c - ns) * a.ldk2 + f : a.k + c * a.ldk + f);
          vv[u] = *vec(second ? a.v2 + (c - ns) * a.ldv2 + f : a.v + c * a.ldv + f);
          mm[u] = ok && ((bj >> hk) & 1u) ? a.inv_keep : 0.f;
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
          lsum += p;                     // every edge
          axpy4(p * mm[u], vv[u], acc);  // the kept ones, times 1 / (1 - p)
        }
      }
    }
    if (!has_row) continue;
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
    acc.x *= inv;
    acc.y *= inv;
    acc.z *= inv;
    acc.w *= inv;
    *reinterpret_cast<float4*>(a.out + r * a.ldo + f) = acc;
    if (l % LH == 0) {
      a.stat_m[r * a.lds + hk] = m;
      a.stat_l[r * a.lds + hk] = inv;  // 1 / sum (0 for an empty row)
    }
  }
}

// -------------------------------------------------------------------------------- bwd dst
template <typename IdxT, int LPR, int HH>
__global__ __launch_bounds__(256) void dot_attn_drop_bwd_dst_kernel(DropArgs a) {
  constexpr int G = kWave / LPR;
  constexpr int LH = LPR / HH;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, l = lane % LPR, hk = l / LH;
  const int f = 4 * l;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  const int64_t q0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t qstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const int64_t ns = a.nsplit;
  const uint64_t seed = static_cast<uint64_t>(*a.seed);
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
      const uint32_t my_b = kk < deg ? attn_keep_bits(seed, s + kk, a.thr, HH) : 0u;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 kv[kU], vv[kU];
        float mm[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int src_lane = g * LPR + (j < LPR ? j : 0);
          const int64_t cj = __shfl(my_col, src_lane, kWave);
          const uint32_t bj = __shfl(my_b, src_lane, kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t c = ok ? cj : 0;
          const bool second = a.k2 && c >= ns;
          kv[u] = *vec(second ? a.k2 + (c - ns) * a.ldk2 + f : a.k + c * a.ldk + f);
          vv[u] = *vec(second ? a.v2 + (c - ns) * a.ldv2 + f : a.v + c * a.ldv + f);
          mm[u] = ok && ((bj >> hk) & 1u) ? a.inv_keep : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          const float e = a.scale * head_sum<LH>(dot4(qv, kv[u]));
          const float ga = head_sum<LH>(dot4(gv, vv[u]));
          const float de = ok ? __expf(e - my_m) * my_inv * (mm[u] * ga - my_c) : 0.f;
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
__global__ __launch_bounds__(256) void dot_attn_drop_bwd_src_kernel(DropArgs a) {
  constexpr int G = kWave / LPR;
  constexpr int LH = LPR / HH;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, l = lane % LPR, hk = l / LH;
  const int f = 4 * l;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  const int64_t q0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t qstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const uint64_t seed = static_cast<uint64_t>(*a.seed);
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
      const int64_t my_i = kk < deg ? load_idx<IdxT>(a.col, s + kk) : 0;
      // the entry's forward slot keys the same bits as the destination side's
      const uint32_t my_b =
          kk < deg ? attn_keep_bits(seed, load_idx<IdxT>(a.t_slot, s + kk), a.thr, HH) : 0u;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 qg[kU], gg[kU];
        float m[kU], il[kU], c[kU], mm[kU];
        bool ok[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int src_lane = g * LPR + (j < LPR ? j : 0);
          const int64_t i = __shfl(my_i, src_lane, kWave);
          const uint32_t bj = __shfl(my_b, src_lane, kWave);
          ok[u] = j < LPR && k0 + j < deg;
          const int64_t ii = ok[u] ? i : 0;
          qg[u] = *vec(a.q + ii * a.ldq + f);
          gg[u] = *vec(a.g + ii * a.ldg + f);
          m[u] = a.stat_m[ii * a.lds + hk];
          il[u] = a.stat_l[ii * a.lds + hk];
          c[u] = a.c[ii * a.lds + hk];
          mm[u] = ok[u] && ((bj >> hk) & 1u) ? a.inv_keep : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const float e = a.scale * head_sum<LH>(dot4(qg[u], kv));
          const float ga = head_sum<LH>(dot4(gg[u], vv));
          const float al = ok[u] ? __expf(e - m[u]) * il[u] : 0.f;
          const float de = ok[u] ? al * (mm[u] * ga - c[u]) : 0.f;
          axpy4(al * mm[u], gg[u], dv);
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
void launch_one(const DropArgs& a, int64_t blocks, hipStream_t st) {
  dim3 grid(static_cast<unsigned>(blocks)), block(256);
  if constexpr (KIND == 0)
    hipLaunchKernelGGL((dot_attn_drop_fwd_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
  else if constexpr (KIND == 1)
    hipLaunchKernelGGL((dot_attn_drop_bwd_dst_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((dot_attn_drop_bwd_src_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
}

template <int KIND, typename IdxT>
hipError_t launch_kind(const DropArgs& a, int heads, hipStream_t st) {
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
hipError_t launch(const DropArgs& a, IType it, int heads, hipStream_t st) {
  if (a.nrows <= 0) return hipSuccess;
  if (!dot_attn_f32_shape_ok(a.C, heads) || a.seed == nullptr) return hipErrorInvalidValue;
  return it == IType::I32 ? launch_kind<KIND, int32_t>(a, heads, st)
                          : launch_kind<KIND, int64_t>(a, heads, st);
}

}  // namespace

hipError_t dot_attn_drop_fwd_f32(IType it, const int64_t* rowptr, const void* col,
                                 int64_t nrows, int C, int heads, int64_t lds, float scale,
                                 const float* q, int64_t ldq, const float* k, int64_t ldk,
                                 const float* v, int64_t ldv, const float* k2, int64_t ldk2,
                                 const float* v2, int64_t ldv2, int64_t nsplit, float* out,
                                 int64_t ldo, float* stat_m, float* stat_l,
                                 const int64_t* seed, uint32_t thr, float inv_keep,
                                 hipStream_t st) {
  DropArgs a{};
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
  a.seed = seed;
  a.thr = thr;
  a.inv_keep = inv_keep;
  return launch<0>(a, it, heads, st);
}

hipError_t dot_attn_drop_bwd_dst_f32(IType it, const int64_t* rowptr, const void* col,
                                     int64_t nrows, int C, int heads, int64_t lds, float scale,
                                     const float* q, int64_t ldq, const float* k, int64_t ldk,
                                     const float* v, int64_t ldv, const float* k2,
                                     int64_t ldk2, const float* v2, int64_t ldv2,
                                     int64_t nsplit, const float* stat_m, const float* stat_l,
                                     const float* g, int64_t ldg, const float* c, float* dq,
                                     int64_t lddq, const int64_t* seed, uint32_t thr,
                                     float inv_keep, hipStream_t st) {
  DropArgs a{};
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
  a.seed = seed;
  a.thr = thr;
  a.inv_keep = inv_keep;
  return launch<1>(a, it, heads, st);
}

hipError_t dot_attn_drop_bwd_src_f32(IType it, const int64_t* rowptr, const void* col,
                                     const void* t_slot, int64_t nrows, int C, int heads,
                                     int64_t lds, float scale, const float* q, int64_t ldq,
                                     const float* g, int64_t ldg, const float* k, int64_t ldk,
                                     const float* v, int64_t ldv, const float* stat_m,
                                     const float* stat_l, const float* c, float* dk,
                                     int64_t lddk, float* dv, int64_t lddv,
                                     const int64_t* seed, uint32_t thr, float inv_keep,
                                     hipStream_t st) {
  DropArgs a{};
  a.rowptr = rowptr;
  a.col = col;
  a.t_slot = t_slot;
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
  a.seed = seed;
  a.thr = thr;
  a.inv_keep = inv_keep;
  return launch<2>(a, it, heads, st);
}

}  // namespace dgraph
