// dgraph_amd — fused scaled dot-product graph attention with bf16 storage for gfx950
// (TransformerConv in bf16). Per destination row i, head h (channels [hD, (h+1)D) of
// C = heads D):
//
//   e_ij  = scale <q_i[head h], k_j[head h]>
//   alpha = softmax_j(e_ij)                      max-subtracted, over the row's entries
//   out_i = bf16_rne(sum_j alpha_ij v_j[head h])         (an empty row gives 0)
//
// q, k, v, the second source k2 / v2 (columns >= nsplit), out, g = dL/dout, dq, dk, dv are
// bf16; stat_m, stat_l (= 1 / sum, 0 for an empty row) and c are fp32 [rows, heads]. All
// arithmetic and accumulation is fp32: a bf16 value is widened by a 16-bit shift and narrowed
// once, at the store, by round-to-nearest-even (Inf / NaN pass through).
//
// This is not dot_attn_f32.h with the type swapped:
//
// * Layout (gat_bf16.hip's): one group of LPR = C / 8 lanes per row (8 / 16 / 32), eight
//   channels per lane, ONE 16-B load per lane per gathered row; 64 / LPR row groups per wave;
//   the heads as contiguous blocks of LH = LPR / heads >= 1 lanes. Every feature array has
//   its own row stride (elements, a multiple of 8): with k and v the column halves of one
//   [N, 2C] buffer both gathers of an edge come from one contiguous 4C-byte row.
// * score(): scale * head_sum(dot8(q, k)), ONE function, one order, compiled without
//   contraction of its last product. All three kernels call it, so the backward kernels
//   recompute the forward's scores (and with stat_m / stat_l its alpha) bit for bit.
// * dot_attn_bf16_fwd: q_i unpacked once and resident; ONE pass with a running maximum:
//   column ids loaded lane-parallel and broadcast by shuffle, kU edges = 2 kU raw 16-B
//   vectors (k_j and v_j) in flight; per batch its maximum, one rescale of the accumulator
//   and the running sum, then the accumulation. Writes out, stat_m and stat_l. No beta and
//   no carry-in: a carried accumulator would round-trip through bf16.
// * dot_attn_bf16_bwd_dst: g_i and q_i resident, TWO passes over the row's entries. The
//   fp32 op forms c_i^h = <g_i^h, out_i^h> from the saved output; from an output rounded to
//   bf16 that c is off by about 2^-9 sqrt(D) |g| |out|, and a row of degree 1 (alpha = 1,
//   c = ga exactly, de = 0, dq = 0) would get a dq of that error times scale |k_j|. So pass 1
//   gathers k_j and v_j, recomputes alpha and accumulates c_i^h = sum_j alpha_ij <g_i^h,
//   v_j^h> in fp32 in CSR order; pass 2 gathers the same rows again (the wave has just read
//   them), forms de = alpha (ga - c) per edge and accumulates dq_i = scale sum_j de k_j.
//   dq is never a difference of two accumulated sums. Writes c (fp32) and dq (bf16).
// * dot_attn_bf16_bwd_src: over the transposed pattern with k_j and v_j resident; gathers
//   q_i, g_i (bf16) and m, 1 / l, c (fp32) of the destination, recomputes alpha and de;
//   dv_j = sum_i alpha g_i and dk_j = scale sum_i de q_i, both bf16.
//
// Column ids are int32. No atomics, no LDS, no scratch; fixed summation orders: two calls
// give equal bits. Padding lanes / slots (a wave's groups run to the longest row of the
// wave) gather row 0 with weight 0: of k / v — of k2 / v2 when nsplit == 0 and they are
// given, so a relation whose sources are all halo rows never touches the empty first source
// — and in bwd_src of q, g and the destination arrays. The launchers refuse a launch that
// has no such source; the callers launch only when that row exists
// (bindings_dot_attn_bf16.cpp).
//
// Compiler resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=
// kernel-resource-usage; the 12 (LPR, heads) instantiations of each kernel at kU = 8; no LDS,
// no AGPRs; 512 VGPRs per SIMD lane, so waves per SIMD = min(8, 512 / VGPRs)):
//                     LPR = 8          LPR = 16         LPR = 32
//   heads             1   2   4   8    1   2   4   8    1   2   4   8
//   fwd      VGPRs    120 123 122 123  112 115 114 113  113 116 115 114   occupancy 4
//   bwd_dst  VGPRs    138 139 138 137  132 132 130 129  133 135 132 130   occupancy 3
//   bwd_src  VGPRs    236 236 233 189  229 229 228 225  230 230 229 228   occupancy 2
// Scratch 0 B, no VGPR and no SGPR spilled in all 36. At kU = 4 the same table reads 91 .. 96
// (occupancy 5), 97 .. 121 (4) and 128 .. 150 (3; 8 / 8: 4), also without scratch. kU = 8 is
// chosen: the kernels are gather-bound, and occupancy x 2 kU gathered 16-B vectors in flight
// per SIMD lane is 64 / 48 / 32 at kU = 8 against 40 / 32 / 24 at kU = 4. The forward holds
// 2 kU raw rows (64 VGPRs) and unpacks each on use rather than keeping 16 kU fp32 values; the
// source side holds four resident / accumulator vectors of eight (k_j, v_j, dk, dv), 2 kU
// raw rows and 3 kU gathered destination scalars. The file is compiled without packed-fp32
// instructions (_build.py: EXTRA_FLAGS).
#include "attn_device.h"
#include "kernels.h"

namespace dgraph {
namespace {

constexpr int kU = 8;  // edges in flight per lane: 2 kU gathered 16-B vectors

// e_ij[head of this lane]: the ONE definition all three kernels use. Contraction is off so
// that the product is rounded before the row maximum is subtracted from it, in every caller.
template <int LH>
__device__ __forceinline__ float score(const f32x8& qv, const f32x8& kv, float scale) {
#pragma clang fp contract(off)
  return scale * head_sum<LH>(dot8(qv, kv));
}

// <g_i, v_j>[head of this lane], the same in bwd_dst's two passes and in bwd_src
template <int LH>
__device__ __forceinline__ float gdot(const f32x8& gv, const f32x8& vv) {
  return head_sum<LH>(dot8(gv, vv));
}

// what every kernel knows of its lane and of the row its group handles in this step
template <int LPR, int HH>
struct Lane {
  static constexpr int G = kWave / LPR;
  int g, l, hk, f;
  int64_t ngroups, q0, qstep;
  __device__ explicit Lane(int64_t nrows) {
    const int lane = threadIdx.x & (kWave - 1);
    g = lane / LPR;
    l = lane % LPR;
    hk = l / (LPR / HH);
    f = 8 * l;
    ngroups = (nrows + G - 1) / G;
    q0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    qstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  }
};

struct Row {
  int64_t r, rr, s;  // rr: r, or 0 for a group past the last row (reads row 0, writes nothing)
  int deg, maxdeg;
  bool has_row;
  template <int LPR, int HH>
  __device__ Row(const DotAttnBf16Args& a, const Lane<LPR, HH>& t, int64_t q) {
    r = q * Lane<LPR, HH>::G + t.g;
    has_row = r < a.nrows;
    rr = has_row ? r : 0;
    s = has_row ? a.rowptr[r] : 0;
    deg = has_row ? static_cast<int>(a.rowptr[r + 1] - s) : 0;
    maxdeg = group_imax<LPR>(deg);
  }
};

// this lane's column id of chunk k0 (0 past the row's end)
__device__ __forceinline__ int chunk_col(const DotAttnBf16Args& a, const Row& row, int kk) {
  return kk < row.deg ? a.col[row.s + kk] : 0;
}

// the batch's kU (k_j, v_j) pairs, raw; a slot past the row's end reads column 0
template <int LPR>
__device__ __forceinline__ void gather_kv(const DotAttnBf16Args& a, int my_c, int g, int f,
                                          int k0, int j0, int deg, uint4 (&kr)[kU],
                                          uint4 (&vr)[kU]) {
#pragma unroll
  for (int u = 0; u < kU; ++u) {
    const int j = j0 + u;
    const int cj = __shfl(my_c, g * LPR + (j < LPR ? j : 0), kWave);
    const bool ok = j < LPR && k0 + j < deg;
    const int64_t c = ok ? cj : 0;
    if (a.k2 && c >= a.nsplit) {
      kr[u] = load16(a.k2 + (c - a.nsplit) * a.ldk2 + f);
      vr[u] = load16(a.v2 + (c - a.nsplit) * a.ldv2 + f);
    } else {
      kr[u] = load16(a.k + c * a.ldk + f);
      vr[u] = load16(a.v + c * a.ldv + f);
    }
  }
}

// ------------------------------------------------------------------------------------ fwd
template <int LPR, int HH>
__global__ __launch_bounds__(256) void dot_attn_bf16_fwd_kernel(DotAttnBf16Args a) {
  constexpr int LH = LPR / HH;
  const Lane<LPR, HH> t(a.nrows);
  const int g = t.g, l = t.l, hk = t.hk, f = t.f;
  for (int64_t q = t.q0; q < t.ngroups; q += t.qstep) {
    const Row row(a, t, q);
    const int deg = row.deg, maxdeg = row.maxdeg;
    const f32x8 qv = unpack_bf16x8(load16(a.q + row.rr * a.ldq + f));
    float m = -INFINITY, lsum = 0.f;
    f32x8 acc = zero8();
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int my_c = chunk_col(a, row, k0 + l);
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        uint4 kr[kU], vr[kU];
        float e[kU];
        gather_kv<LPR>(a, my_c, g, f, k0, j0, deg, kr, vr);
        // the batch's scores and the new running maximum
        float mc = m;
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          const float sc = score<LH>(qv, unpack_bf16x8(kr[u]), a.scale);
          e[u] = ok ? sc : -INFINITY;
          mc = fmaxf(mc, e[u]);
        }
        // one rescale per batch (mc = -inf: nothing seen yet, acc and lsum are 0)
        const float rs = mc == -INFINITY ? 1.f : __expf(m - mc);
        m = mc;
        lsum *= rs;
        scale8(rs, acc);
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const float p = e[u] == -INFINITY ? 0.f : __expf(e[u] - mc);
          lsum += p;
          axpy8(p, unpack_bf16x8(vr[u]), acc);
        }
      }
    }
    if (!row.has_row) continue;
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
    scale8(inv, acc);
    *reinterpret_cast<uint4*>(a.out + row.r * a.ldo + f) = pack_bf16x8(acc);
    if (l % LH == 0) {
      a.stat_m[row.r * HH + hk] = m;
      a.stat_l[row.r * HH + hk] = inv;  // 1 / sum (0 for an empty row)
    }
  }
}

// -------------------------------------------------------------------------------- bwd dst
template <int LPR, int HH>
__global__ __launch_bounds__(256) void dot_attn_bf16_bwd_dst_kernel(DotAttnBf16Args a) {
  constexpr int LH = LPR / HH;
  const Lane<LPR, HH> t(a.nrows);
  const int g = t.g, l = t.l, hk = t.hk, f = t.f;
  for (int64_t q = t.q0; q < t.ngroups; q += t.qstep) {
    const Row row(a, t, q);
    const int deg = row.deg, maxdeg = row.maxdeg;
    const f32x8 qv = unpack_bf16x8(load16(a.q + row.rr * a.ldq + f));
    const f32x8 gv = unpack_bf16x8(load16(a.g + row.rr * a.ldg + f));
    const float my_m = a.stat_m[row.rr * HH + hk];
    const float my_inv = a.stat_l[row.rr * HH + hk];
    // pass 1: c = sum_j alpha_ij <g_i, v_j> per head, in CSR order
    float cacc = 0.f;
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int my_c = chunk_col(a, row, k0 + l);
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        uint4 kr[kU], vr[kU];
        gather_kv<LPR>(a, my_c, g, f, k0, j0, deg, kr, vr);
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          const float e = score<LH>(qv, unpack_bf16x8(kr[u]), a.scale);
          const float ga = gdot<LH>(gv, unpack_bf16x8(vr[u]));
          const float al = ok ? __expf(e - my_m) * my_inv : 0.f;
          cacc = fmaf(al, ok ? ga : 0.f, cacc);
        }
      }
    }
    // pass 2: the same rows again; de per edge from the finished c
    f32x8 acc = zero8();
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int my_c = chunk_col(a, row, k0 + l);
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        uint4 kr[kU], vr[kU];
        gather_kv<LPR>(a, my_c, g, f, k0, j0, deg, kr, vr);
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          const f32x8 kv = unpack_bf16x8(kr[u]);
          const float e = score<LH>(qv, kv, a.scale);
          const float ga = gdot<LH>(gv, unpack_bf16x8(vr[u]));
          const float de = ok ? __expf(e - my_m) * my_inv * (ga - cacc) : 0.f;
          axpy8(de, kv, acc);
        }
      }
    }
    if (!row.has_row) continue;
    scale8(a.scale, acc);
    *reinterpret_cast<uint4*>(a.dq + row.r * a.lddq + f) = pack_bf16x8(acc);
    if (l % LH == 0) a.c[row.r * HH + hk] = cacc;
  }
}

// -------------------------------------------------------------------------------- bwd src
template <int LPR, int HH>
__global__ __launch_bounds__(256) void dot_attn_bf16_bwd_src_kernel(DotAttnBf16Args a) {
  constexpr int LH = LPR / HH;
  const Lane<LPR, HH> t(a.nrows);
  const int g = t.g, l = t.l, hk = t.hk, f = t.f;
  for (int64_t q = t.q0; q < t.ngroups; q += t.qstep) {
    const Row row(a, t, q);
    const int deg = row.deg, maxdeg = row.maxdeg;
    const f32x8 kv = unpack_bf16x8(load16(a.k + row.rr * a.ldk + f));
    const f32x8 vv = unpack_bf16x8(load16(a.v + row.rr * a.ldv + f));
    f32x8 dk = zero8(), dv = zero8();
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int my_i = chunk_col(a, row, k0 + l);
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        uint4 qr[kU], gr[kU];
        float m[kU], il[kU], c[kU];
        bool ok[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int i = __shfl(my_i, g * LPR + (j < LPR ? j : 0), kWave);
          ok[u] = j < LPR && k0 + j < deg;
          const int64_t ii = ok[u] ? i : 0;
          qr[u] = load16(a.q + ii * a.ldq + f);
          gr[u] = load16(a.g + ii * a.ldg + f);
          m[u] = a.stat_m[ii * HH + hk];
          il[u] = a.stat_l[ii * HH + hk];
          c[u] = a.c[ii * HH + hk];
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const f32x8 qg = unpack_bf16x8(qr[u]);
          const f32x8 gg = unpack_bf16x8(gr[u]);
          const float e = score<LH>(qg, kv, a.scale);
          const float ga = gdot<LH>(gg, vv);
          const float al = ok[u] ? __expf(e - m[u]) * il[u] : 0.f;
          const float de = ok[u] ? al * (ga - c[u]) : 0.f;
          axpy8(al, gg, dv);
          axpy8(de, qg, dk);
        }
      }
    }
    if (!row.has_row) continue;
    scale8(a.scale, dk);
    *reinterpret_cast<uint4*>(a.dk + row.r * a.lddk + f) = pack_bf16x8(dk);
    *reinterpret_cast<uint4*>(a.dv + row.r * a.lddv + f) = pack_bf16x8(dv);
  }
}

template <int KIND, int LPR, int HH>
void launch_one(const DotAttnBf16Args& a, int64_t blocks, hipStream_t st) {
  dim3 grid(static_cast<unsigned>(blocks)), block(256);
  if constexpr (KIND == 0)
    hipLaunchKernelGGL((dot_attn_bf16_fwd_kernel<LPR, HH>), grid, block, 0, st, a);
  else if constexpr (KIND == 1)
    hipLaunchKernelGGL((dot_attn_bf16_bwd_dst_kernel<LPR, HH>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((dot_attn_bf16_bwd_src_kernel<LPR, HH>), grid, block, 0, st, a);
}

template <int KIND>
hipError_t launch(const DotAttnBf16Args& a, int heads, hipStream_t st) {
  if (a.nrows <= 0) return hipSuccess;
  if (!dot_attn_bf16_shape_ok(a.C, heads)) return hipErrorInvalidValue;
  // row 0 of what the padding slots gather must exist: the first source, or the second one
  // when it serves every column
  if (KIND != 2) {
    const bool second_only = a.k2 && a.v2 && a.nsplit == 0;
    if (!second_only && !(a.k && a.v)) return hipErrorInvalidValue;
    if ((a.k2 == nullptr) != (a.v2 == nullptr) || a.nsplit < 0) return hipErrorInvalidValue;
  } else if (!(a.q && a.g && a.stat_m && a.stat_l && a.c)) {
    return hipErrorInvalidValue;
  }
  const int LPR = a.C / 8;
  const int64_t G = kWave / LPR;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  const int64_t blocks = (ngroups + 3) / 4;  // one row group per wave, in order
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
#define DG_DOTB(L_, H_)                        \
  if (LPR == L_ && heads == H_) {              \
    launch_one<KIND, L_, H_>(a, blocks, st);   \
    return hipGetLastError();                  \
  }
  DG_DOTB(8, 1) DG_DOTB(8, 2) DG_DOTB(8, 4) DG_DOTB(8, 8)
  DG_DOTB(16, 1) DG_DOTB(16, 2) DG_DOTB(16, 4) DG_DOTB(16, 8)
  DG_DOTB(32, 1) DG_DOTB(32, 2) DG_DOTB(32, 4) DG_DOTB(32, 8)
#undef DG_DOTB
  return hipErrorInvalidValue;
}

}  // namespace

bool dot_attn_bf16_shape_ok(int C, int heads) {
  if (C != 64 && C != 128 && C != 256) return false;
  return heads == 1 || heads == 2 || heads == 4 || heads == 8;  // LH = C / 8 / heads >= 1
}

hipError_t dot_attn_fwd_bf16(const DotAttnBf16Args& a, int heads, hipStream_t st) {
  return launch<0>(a, heads, st);
}

hipError_t dot_attn_bwd_dst_bf16(const DotAttnBf16Args& a, int heads, hipStream_t st) {
  return launch<1>(a, heads, st);
}

hipError_t dot_attn_bwd_src_bf16(const DotAttnBf16Args& a, int heads, hipStream_t st) {
  return launch<2>(a, heads, st);
}

}  // namespace dgraph
