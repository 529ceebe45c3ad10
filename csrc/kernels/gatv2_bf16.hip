// dgraph_amd — fused GATv2 graph attention with bf16 storage for gfx950 (GATv2Conv in bf16).
// The contract is gatv2_f32.hip's. Per destination row i and head h (channels [hD, (h+1)D) of
// C = heads D), with l = the destination-transformed rows (xd), r = the source-transformed
// rows (xs):
//
//   pre_ijc = l_ic + r_jc                                   (one fp32 add)
//   act     = pre > 0 ? pre : slope pre      lam = pre > 0 ? 1 : slope   (slope at pre == 0)
//   e_ij    = sum_{c in head h} a_c act_ijc
//   alpha   = softmax_j(e_ij)                               (max-subtracted)
//   out_i^h = bf16_rne(sum_j alpha_ij r_j^h)                (an empty row gives 0)
//
// xd, xs, the second source xs2 (columns >= nsplit), out, g = dL/dout, dxd, dxs are bf16; att
// is fp32 [C]; stat_m, stat_l (= 1 / sum, 0 for an empty row) and c are fp32 [rows, heads]
// with one shared row stride; da_part is fp32 [P, C]. All arithmetic and accumulation is fp32:
// a bf16 value is widened by a 16-bit shift and narrowed once, at the store, by
// round-to-nearest-even (Inf / NaN pass through). No beta: an accumulated out would round-trip
// through bf16. Column ids are int32.
//
// This is not gatv2_f32.hip with the type swapped:
//
// * Layout (gat_bf16.hip's and dot_attn_bf16.hip's): one group of LPR = C / 8 lanes per row
//   (8 / 16 / 32), eight channels per lane, ONE 16-B load per lane per gathered row; 64 / LPR
//   row groups per wave; the heads as contiguous blocks of LH = LPR / heads >= 1 lanes. Every
//   feature array has its own row stride (elements, a multiple of 8), so xd and xs can be the
//   halves of the layer's one [N, 2C] buffer. Each lane keeps its eight att values (the
//   backward kernels also slope att) in registers.
// * score(): head_sum(dot8(att, leaky(l + r))), ONE function, one order, compiled without
//   contraction. All three kernels call it, so the backward kernels recompute the forward's
//   scores bit for bit and exp(e - m) <= 1.
// * gatv2_fwd_bf16: l_i unpacked once and resident; ONE pass with a running maximum: column
//   ids loaded lane-parallel and broadcast by shuffle, kU raw 16-B r_j vectors in flight, each
//   unpacked on use (the same vector feeds the score and the message); per batch its maximum,
//   one rescale of the accumulator and the running sum, then the accumulation. Writes out,
//   stat_m and stat_l.
// * gatv2_bwd_dst_bf16: l_i, g_i, m, 1 / l resident, ONE pass. The fp32 op forms
//   c_i^h = <g_i^h, out_i^h> from the saved output; from an output rounded to bf16 that c is
//   off by about 2^-9 sqrt(D) |g| |out|. Two passes (c first, then de = alpha (ga - c) per
//   edge; dot_attn_bf16.hip) gather every row twice. Here, per edge with alpha recomputed,
//   ga = <g_i^h, r_j^h> and w = alpha ga, one pass accumulates in fp32
//     per head     c  = sum alpha ga
//     per channel  T1 = sum w (a lam)   T2 = sum alpha (a lam)
//                  U1 = sum w act       U2 = sum alpha act
//   and at the row's end dl_i = T1 - c T2 (bf16) and the lane's da += U1 - c U2; c is written
//   in fp32 for the source side and never comes from the rounded out. c T2 and c U2 are
//   products rounded on their own (no contraction into the subtraction): a row of degree 1
//   has alpha = 1, c = ga, T1 = fl(ga a lam) = fl(c T2), so its dl is exactly 0. Each
//   workgroup combines its lanes' da through LDS in thread order and writes ONE row of
//   da_part [P, C]; the grid (and so P, gatv2_bf16_da_parts) depends on (rows, C) only: at
//   most kMaxParts workgroups that stride over the row groups.
// * gatv2_bwd_src_bf16: over the transposed pattern with r_j resident; gathers l_i, g_i (raw
//   16-B bf16 vectors) and m, 1 / l, c (fp32) of each destination, recomputes alpha, forms
//   de = alpha (ga - c) directly and writes dr_j = sum_i (alpha g_i + de a lam) in bf16.
//
// No atomics, fixed summation orders: two calls give equal bits. Padding lanes / slots (a
// wave's groups run to the longest row of the wave) gather row 0 with weight 0: of xs — of
// xs2 when nsplit == 0 and it is given, so a relation whose sources are all halo rows never
// touches the empty first source — and in bwd_src of xd, g and the destination arrays. The
// launchers refuse a launch that has no such row; the callers launch only when it exists
// (bindings_gatv2_bf16.cpp).
//
// Compiler resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=
// kernel-resource-usage; the 12 (LPR, heads) instantiations of each kernel at kU = 8; no
// AGPRs; 512 VGPRs per SIMD lane, so waves per SIMD = min(8, 512 / VGPRs)):
//                     LPR = 8          LPR = 16         LPR = 32
//   heads             1   2   4   8    1   2   4   8    1   2   4   8
//   fwd      VGPRs    108 111 109 107  102 105 104 102  103 106 105 104   occupancy 4
//   bwd_dst  VGPRs    163 166 162 157  155 158 157 153  156 159 158 157   occupancy 3
//   bwd_src  VGPRs    182 187 186 168  166 181 180 170  167 181 180 179   occupancy 2 (3 at
//                                                          <= 168: 8 / 8, 16 / 1 and 32 / 1)
// Scratch 0 B and no VGPR spilled in all 36; bwd_dst holds 8 KiB of LDS (the da combine);
// bwd_src keeps 79 .. 92 scalar registers in VGPR lanes (no scratch), as gatv2_f32.hip's
// backward kernels do. At kU = 4 the same table reads 82 .. 95 (occupancy 5), 133 .. 143 (3)
// and 119 .. 127 (4), at kU = 16 109 .. 159 (4 / 3), 175 .. 206 (2) and 186 .. 256 with AGPRs
// (2 / 1), all without scratch. One kU = 8 is chosen for all three: the kernels are
// gather-bound, and occupancy x gathered 16-B vectors in flight per SIMD lane is 32 / 24 /
// 32 .. 48 at kU = 8 against 20 / 12 / 32 at kU = 4; kU = 16 would put 48 in flight in the
// forward at LPR 16 / 32 but half of an LPR = 8 batch would be padding slots, and it halves
// the occupancy of both backward kernels. The source side stays off scratch and at
// occupancy >= 2 at kU = 8, so it needs no kU of its own. bwd_dst holds five accumulator
// vectors of eight (T1, T2, U1, U2, da), l_i, g_i, a and slope a (72 VGPRs) and kU raw rows;
// bwd_src r_j, dr, a, slope a, 2 kU raw rows and 3 kU gathered destination scalars. The file
// is compiled without packed-fp32 instructions (_build.py: EXTRA_FLAGS): with them the same
// source takes 146 .. 186 VGPRs in fwd (occupancy 3 / 2) and 256 VGPRs plus 14 .. 20 AGPRs
// in bwd_dst (occupancy 1).
#include "attn_device.h"
#include "kernels.h"

namespace dgraph {
namespace {

constexpr int kU = 8;            // edges in flight per lane (bwd_src: 2 kU gathered vectors)
constexpr int kMaxParts = 4096;  // workgroups of gatv2_bwd_dst_bf16 = rows of da_part, at most

// pre = l + r: one add per channel, the same bits whichever operand is the resident one
__device__ __forceinline__ f32x8 add8(const f32x8& a, const f32x8& b) {
  f32x8 v;
  v.lo = add4(a.lo, b.lo);
  v.hi = add4(a.hi, b.hi);
  return v;
}

__device__ __forceinline__ float4 leaky4(const float4& p, float slope) {
#pragma clang fp contract(off)
  return make_float4(p.x > 0.f ? p.x : slope * p.x, p.y > 0.f ? p.y : slope * p.y,
                     p.z > 0.f ? p.z : slope * p.z, p.w > 0.f ? p.w : slope * p.w);
}

__device__ __forceinline__ f32x8 leaky8(const f32x8& pre, float slope) {
  f32x8 v;
  v.lo = leaky4(pre.lo, slope);
  v.hi = leaky4(pre.hi, slope);
  return v;
}

// a lam per channel (av or its slope multiple; slope at pre == 0)
__device__ __forceinline__ float4 alam4(const float4& p, const float4& av, const float4& as) {
  return make_float4(p.x > 0.f ? av.x : as.x, p.y > 0.f ? av.y : as.y,
                     p.z > 0.f ? av.z : as.z, p.w > 0.f ? av.w : as.w);
}

__device__ __forceinline__ f32x8 alam8(const f32x8& pre, const f32x8& av, const f32x8& as) {
  f32x8 v;
  v.lo = alam4(pre.lo, av.lo, as.lo);
  v.hi = alam4(pre.hi, av.hi, as.hi);
  return v;
}

// e_ij[head of this lane] from act = leaky(l_i + r_j): the ONE definition all three kernels
// use. Contraction is off here and in leaky4, so every caller rounds the same products.
template <int LH>
__device__ __forceinline__ float score(const f32x8& av, const f32x8& act) {
#pragma clang fp contract(off)
  return head_sum<LH>(dot8(av, act));
}

// <g_i, r_j>[head of this lane], the same in bwd_dst and in bwd_src
template <int LH>
__device__ __forceinline__ float gdot(const f32x8& gv, const f32x8& rv) {
  return head_sum<LH>(dot8(gv, rv));
}

// x - c y per channel with c y rounded on its own: never one fma
__device__ __forceinline__ float4 sub_scaled4(const float4& x, float c, const float4& y) {
#pragma clang fp contract(off)
  const float px = c * y.x, py = c * y.y, pz = c * y.z, pw = c * y.w;
  return make_float4(x.x - px, x.y - py, x.z - pz, x.w - pw);
}

// The forward uses a gathered row twice, for the score and then for the message. Left alone
// the compiler keeps the batch's 8 kU unpacked values between the two (133 .. 157 VGPRs,
// occupancy 3); behind this barrier it unpacks the raw vector again (8 VALU shifts / masks
// per row) and the kernel fits occupancy 4.
__device__ __forceinline__ const uint4& reread(uint4& r) {
  asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w));
  return r;
}

__device__ __forceinline__ f32x8 att8(const float* att, int f) {
  f32x8 v;
  v.lo = *vec(att + f);
  v.hi = *vec(att + f + 4);
  return v;
}

// what every kernel knows of its lane
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

// the row this lane's group handles in one step
struct Row {
  int64_t r, rr, s;  // rr: r, or 0 for a group past the last row (reads row 0, writes nothing)
  int deg, maxdeg;
  bool has_row;
  template <int LPR, int HH>
  __device__ Row(const GatV2Bf16Args& a, const Lane<LPR, HH>& t, int64_t q) {
    r = q * Lane<LPR, HH>::G + t.g;
    has_row = r < a.nrows;
    rr = has_row ? r : 0;
    s = has_row ? a.rowptr[r] : 0;
    deg = has_row ? static_cast<int>(a.rowptr[r + 1] - s) : 0;
    maxdeg = group_imax<LPR>(deg);
  }
};

// this lane's column id of the chunk (0 past the row's end)
__device__ __forceinline__ int chunk_col(const GatV2Bf16Args& a, const Row& row, int kk) {
  return kk < row.deg ? a.col[row.s + kk] : 0;
}

// the batch's U r_j rows, raw; a slot past the row's end reads column 0
template <int LPR, int U>
__device__ __forceinline__ void gather_r(const GatV2Bf16Args& a, int my_c, int g, int f, int k0,
                                         int j0, int deg, uint4 (&rr)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = j0 + u;
    const int cj = __shfl(my_c, g * LPR + (j < LPR ? j : 0), kWave);
    const bool ok = j < LPR && k0 + j < deg;
    const int64_t c = ok ? cj : 0;
    if (a.xs2 && c >= a.nsplit)
      rr[u] = load16(a.xs2 + (c - a.nsplit) * a.ldxs2 + f);
    else
      rr[u] = load16(a.xs + c * a.ldxs + f);
  }
}

// ------------------------------------------------------------------------------------ fwd
template <int LPR, int HH>
__global__ __launch_bounds__(256) void gatv2_fwd_bf16_kernel(GatV2Bf16Args a) {
  constexpr int LH = LPR / HH;
  constexpr int U = kU;
  const Lane<LPR, HH> t(a.nrows);
  const int g = t.g, l = t.l, hk = t.hk, f = t.f;
  const f32x8 av = att8(a.att, f);
  for (int64_t q = t.q0; q < t.ngroups; q += t.qstep) {
    const Row row(a, t, q);
    const int deg = row.deg, maxdeg = row.maxdeg;
    const f32x8 lv = unpack_bf16x8(load16(a.xd + row.rr * a.ldxd + f));
    float m = -INFINITY, lsum = 0.f;
    f32x8 acc = zero8();
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int my_c = chunk_col(a, row, k0 + l);
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += U) {
        uint4 rr[U];
        float e[U];
        gather_r<LPR, U>(a, my_c, g, f, k0, j0, deg, rr);
        // the batch's scores and the new running maximum
        float mc = m;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          const float sc = score<LH>(av, leaky8(add8(lv, unpack_bf16x8(rr[u])), a.slope));
          e[u] = ok ? sc : -INFINITY;
          mc = fmaxf(mc, e[u]);
        }
        // one rescale per batch (mc = -inf: nothing seen yet, acc and lsum are 0)
        const float rs = mc == -INFINITY ? 1.f : __expf(m - mc);
        m = mc;
        lsum *= rs;
        scale8(rs, acc);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float p = e[u] == -INFINITY ? 0.f : __expf(e[u] - mc);
          lsum += p;
          axpy8(p, unpack_bf16x8(reread(rr[u])), acc);
        }
      }
    }
    if (!row.has_row) continue;
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
    scale8(inv, acc);
    *reinterpret_cast<uint4*>(a.out + row.r * a.ldo + f) = pack_bf16x8(acc);
    if (l % LH == 0) {
      a.stat_m[row.r * a.lds + hk] = m;
      a.stat_l[row.r * a.lds + hk] = inv;  // 1 / sum (0 for an empty row)
    }
  }
}

// -------------------------------------------------------------------------------- bwd dst
template <int LPR, int HH>
__global__ __launch_bounds__(256) void gatv2_bwd_dst_bf16_kernel(GatV2Bf16Args a) {
  constexpr int LH = LPR / HH;
  constexpr int U = kU;
  __shared__ float4 part[2][256];
  const Lane<LPR, HH> t(a.nrows);
  const int g = t.g, l = t.l, hk = t.hk, f = t.f;
  const f32x8 av = att8(a.att, f);
  f32x8 as = av;
  scale8(a.slope, as);
  f32x8 da = zero8();  // this lane's channels, over all its rows
  for (int64_t q = t.q0; q < t.ngroups; q += t.qstep) {
    const Row row(a, t, q);
    const int deg = row.deg, maxdeg = row.maxdeg;
    const f32x8 lv = unpack_bf16x8(load16(a.xd + row.rr * a.ldxd + f));
    const f32x8 gv = unpack_bf16x8(load16(a.g + row.rr * a.ldg + f));
    const float my_m = a.stat_m[row.rr * a.lds + hk];
    const float my_inv = a.stat_l[row.rr * a.lds + hk];
    float cacc = 0.f;
    f32x8 t1 = zero8(), t2 = zero8(), u1 = zero8(), u2 = zero8();
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int my_c = chunk_col(a, row, k0 + l);
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += U) {
        uint4 rr[U];
        gather_r<LPR, U>(a, my_c, g, f, k0, j0, deg, rr);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          const f32x8 rv = unpack_bf16x8(rr[u]);
          const f32x8 pre = add8(lv, rv);
          const f32x8 act = leaky8(pre, a.slope);
          const float e = score<LH>(av, act);
          const float ga = gdot<LH>(gv, rv);
          const float al = ok ? __expf(e - my_m) * my_inv : 0.f;
          const float w = ok ? al * ga : 0.f;
          const f32x8 al8 = alam8(pre, av, as);
          cacc += w;
          axpy8(w, al8, t1);
          axpy8(al, al8, t2);
          axpy8(w, act, u1);
          axpy8(al, act, u2);
        }
      }
    }
    // the row's end (a group past the last row holds zeros and adds them)
    da.lo = add4(da.lo, sub_scaled4(u1.lo, cacc, u2.lo));
    da.hi = add4(da.hi, sub_scaled4(u1.hi, cacc, u2.hi));
    if (!row.has_row) continue;
    f32x8 dl;
    dl.lo = sub_scaled4(t1.lo, cacc, t2.lo);
    dl.hi = sub_scaled4(t1.hi, cacc, t2.hi);
    *reinterpret_cast<uint4*>(a.dxd + row.r * a.lddxd + f) = pack_bf16x8(dl);
    if (l % LH == 0) a.c[row.r * a.lds + hk] = cacc;
  }
  // one row of da_part per workgroup: the 256 / LPR lanes that hold the same eight channels,
  // in thread order
  part[0][threadIdx.x] = da.lo;
  part[1][threadIdx.x] = da.hi;
  __syncthreads();
  if (threadIdx.x < 2 * LPR) {
    const int half = threadIdx.x / LPR, ll = threadIdx.x % LPR;
    float4 sum = part[half][ll];
    for (int k = ll + LPR; k < 256; k += LPR) sum = add4(sum, part[half][k]);
    *reinterpret_cast<float4*>(a.da_part + static_cast<int64_t>(blockIdx.x) * a.C + 8 * ll +
                               4 * half) = sum;
  }
}

// -------------------------------------------------------------------------------- bwd src
template <int LPR, int HH>
__global__ __launch_bounds__(256) void gatv2_bwd_src_bf16_kernel(GatV2Bf16Args a) {
  constexpr int LH = LPR / HH;
  constexpr int U = kU;
  const Lane<LPR, HH> t(a.nrows);
  const int g = t.g, l = t.l, hk = t.hk, f = t.f;
  const f32x8 av = att8(a.att, f);
  f32x8 as = av;
  scale8(a.slope, as);
  for (int64_t q = t.q0; q < t.ngroups; q += t.qstep) {
    const Row row(a, t, q);
    const int deg = row.deg, maxdeg = row.maxdeg;
    const f32x8 rv = unpack_bf16x8(load16(a.xs + row.rr * a.ldxs + f));
    f32x8 dr = zero8();
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int my_i = chunk_col(a, row, k0 + l);
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += U) {
        uint4 lr[U], gr[U];
        float m[U], il[U], c[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int j = j0 + u;
          const int i = __shfl(my_i, g * LPR + (j < LPR ? j : 0), kWave);
          ok[u] = j < LPR && k0 + j < deg;
          const int64_t ii = ok[u] ? i : 0;
          lr[u] = load16(a.xd + ii * a.ldxd + f);
          gr[u] = load16(a.g + ii * a.ldg + f);
          m[u] = a.stat_m[ii * a.lds + hk];
          il[u] = a.stat_l[ii * a.lds + hk];
          c[u] = a.c[ii * a.lds + hk];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const f32x8 gg = unpack_bf16x8(gr[u]);
          const f32x8 pre = add8(unpack_bf16x8(lr[u]), rv);
          const float e = score<LH>(av, leaky8(pre, a.slope));
          const float ga = gdot<LH>(gg, rv);
          const float al = ok[u] ? __expf(e - m[u]) * il[u] : 0.f;
          const float de = ok[u] ? al * (ga - c[u]) : 0.f;
          axpy8(al, gg, dr);
          axpy8(de, alam8(pre, av, as), dr);
        }
      }
    }
    if (!row.has_row) continue;
    *reinterpret_cast<uint4*>(a.dxs + row.r * a.lddxs + f) = pack_bf16x8(dr);
  }
}

template <int KIND, int LPR, int HH>
void launch_one(const GatV2Bf16Args& a, int64_t blocks, hipStream_t st) {
  dim3 grid(static_cast<unsigned>(blocks)), block(256);
  if constexpr (KIND == 0)
    hipLaunchKernelGGL((gatv2_fwd_bf16_kernel<LPR, HH>), grid, block, 0, st, a);
  else if constexpr (KIND == 1)
    hipLaunchKernelGGL((gatv2_bwd_dst_bf16_kernel<LPR, HH>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((gatv2_bwd_src_bf16_kernel<LPR, HH>), grid, block, 0, st, a);
}

template <int KIND>
hipError_t launch(const GatV2Bf16Args& a, int heads, hipStream_t st) {
  if (a.nrows <= 0) return hipSuccess;
  if (!gatv2_bf16_shape_ok(a.C, heads) || !a.att || a.lds < heads) return hipErrorInvalidValue;
  // row 0 of what the padding slots gather must exist: the first source, or the second one
  // when it serves every column
  if (KIND != 2) {
    const bool second_only = a.xs2 && a.nsplit == 0;
    if ((!second_only && !a.xs) || a.nsplit < 0 || !a.xd) return hipErrorInvalidValue;
  } else if (!(a.xd && a.g && a.xs && a.stat_m && a.stat_l && a.c)) {
    return hipErrorInvalidValue;
  }
  const int LPR = a.C / 8;
  const int64_t G = kWave / LPR;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  int64_t blocks = (ngroups + 3) / 4;  // one row group per wave, in order
  if (KIND == 1) blocks = gatv2_bf16_da_parts(a.nrows, a.C);  // strided: one da_part row each
  if (blocks < 1 || blocks > 0x7fffffff) return hipErrorInvalidValue;
#define DG_V2B(L_, H_)                        \
  if (LPR == L_ && heads == H_) {             \
    launch_one<KIND, L_, H_>(a, blocks, st);  \
    return hipGetLastError();                 \
  }
  DG_V2B(8, 1) DG_V2B(8, 2) DG_V2B(8, 4) DG_V2B(8, 8)
  DG_V2B(16, 1) DG_V2B(16, 2) DG_V2B(16, 4) DG_V2B(16, 8)
  DG_V2B(32, 1) DG_V2B(32, 2) DG_V2B(32, 4) DG_V2B(32, 8)
#undef DG_V2B
  return hipErrorInvalidValue;
}

}  // namespace

bool gatv2_bf16_shape_ok(int C, int heads) {
  if (C != 64 && C != 128 && C != 256) return false;
  return heads == 1 || heads == 2 || heads == 4 || heads == 8;  // LH = C / 8 / heads >= 1
}

int64_t gatv2_bf16_da_parts(int64_t nrows, int C) {
  if (nrows <= 0 || C < 8 || C > 8 * kWave || kWave % (C / 8)) return 0;
  const int64_t G = kWave / (C / 8);
  const int64_t ngroups = (nrows + G - 1) / G;
  const int64_t blocks = (ngroups + 3) / 4;
  return blocks < kMaxParts ? blocks : kMaxParts;
}

hipError_t gatv2_fwd_bf16(const GatV2Bf16Args& a, int heads, hipStream_t st) {
  return launch<0>(a, heads, st);
}

hipError_t gatv2_bwd_dst_bf16(const GatV2Bf16Args& a, int heads, hipStream_t st) {
  return launch<1>(a, heads, st);
}

hipError_t gatv2_bwd_src_bf16(const GatV2Bf16Args& a, int heads, hipStream_t st) {
  return launch<2>(a, heads, st);
}

}  // namespace dgraph
