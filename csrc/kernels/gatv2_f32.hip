// dgraph_amd — fused fp32 GATv2 graph attention for gfx950 (GATv2Conv; Brody et al.).
//
// For one relation, per destination row i and head h (channels [hD, (h+1)D) of C = heads D),
// with l = the destination-transformed rows (xd) and r = the source-transformed rows (xs):
//
//   pre_ijc = l_ic + r_jc                                   (one fp32 add)
//   act     = pre > 0 ? pre : slope pre      lam = pre > 0 ? 1 : slope
//   e_ij    = sum_{c in head h} a_c act_ijc
//   alpha   = softmax_j(e_ij)                               (max-subtracted)
//   out_i^h = beta out_i^h + sum_j alpha_ij r_j^h
//
// The score does not separate into a destination scalar plus a source scalar (gat_f32.hip),
// it needs the whole r_j row per edge — and that row is also the message. Three row-parallel
// kernels in the layout of dot_attn_f32.hip, nothing per edge is ever written:
//
// * gatv2_fwd: per destination row with l_i and a resident, ONE pass over the row's edges
//   that gathers r_j once: the same vector feeds the score and the message. A running
//   maximum is kept; the accumulator and the running sum are rescaled once per chunk of kU
//   edges. Writes out, stat_m (the row maximum of e) and stat_l (1 / sum exp(e - m); 0 for
//   an empty row, whose stat_m is unspecified).
// * gatv2_bwd_dst: per destination row with l_i, g_i = dL/dout_i, a, m, 1/l and
//   c_i^h = <g_i^h, out_i^h> resident: gathers r_j, recomputes e with the forward's per-lane
//   operation order (bitwise the forward's score, so exp(e - m) <= 1), ga = <g^h, r_j^h>,
//   de = alpha (ga - c) per edge, dl_i = sum_j de a lam. Each lane also accumulates its four
//   channels of da = sum_ij de act over the rows it handles; a workgroup combines its lanes
//   through LDS in a fixed order and writes ONE row of da_part [P, C]. The grid (and so P,
//   gatv2_da_parts) depends on (rows, C) only: at most kMaxParts workgroups that stride over
//   the row groups. The caller sums da_part's rows (col_sum_partial, elementwise.hip).
// * gatv2_bwd_src: per SOURCE row over the transposed pattern with r_j and a resident:
//   gathers l_i, g_i and the destinations' m, 1/l, c, recomputes alpha and de and
//   accumulates the single dr_j = sum_i (alpha g_i + de a lam).
//
// Two sources (xs for columns < nsplit, xs2 for columns >= nsplit: local rows and received
// halo rows, never concatenated). Every feature array has its own row stride, so xd and xs
// may be the column halves of one [N, 2C] buffer; the per-head arrays share the row stride
// lds. a is a contiguous 16-B aligned [C] vector; each lane keeps its four values (and
// slope a) in registers. One LPR-lane group per row (LPR = C / 4, 16-B fp32 vectors), the
// heads as contiguous blocks of LH = LPR / heads lanes, the per-head sum by xor shuffles
// inside a block. No atomics, fixed summation orders: bitwise deterministic.
//
// Padding lanes / slots (a wave's groups run to the longest row of the wave) gather row 0
// of the first source with weight 0; the callers guarantee that row exists whenever a
// kernel is launched (bindings_gatv2.cpp).
//
// Compiler resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=
// kernel-resource-usage; smallest .. largest of the 24 instantiations of each kernel at
// kU = 8; no AGPRs; 512 VGPRs per SIMD lane, so waves per SIMD = 512 / VGPRs):
//   gatv2_fwd       84 .. 106 VGPRs   scratch 0 B   occupancy 4 .. 5   (kU gathered vectors)
//   gatv2_bwd_dst  112 .. 153 VGPRs   scratch 0 B   occupancy 3 .. 4   4 KiB LDS (da combine)
//   gatv2_bwd_src  137 .. 163 VGPRs   scratch 0 B   occupancy 3
//     (2 resident / accumulator vectors, 2 kU gathered ones and 3 kU gathered statistics)
// The two backward kernels keep 14 .. 46 scalar registers in VGPR lanes (no scratch). With
// kU = 4 in gatv2_bwd_dst alone it takes 88 .. 97 VGPRs (occupancy 4 .. 5, no scalar
// register moved) and on an MI355X measures the same within 2 % (PERFORMANCE.md): the depth
// is not what bounds it, so one kU = 8 stays for all three, as in dot_attn_f32.hip.
#include "attn_device.h"
#include "kernels.h"

namespace dgraph {
namespace {

constexpr int kU = 8;            // edges in flight per lane: kU gathered 16-B vectors
constexpr int kMaxParts = 4096;  // workgroups of gatv2_bwd_dst = rows of da_part, at most

struct V2Args {
  const int64_t* rowptr;
  const void* col;
  int64_t nrows;
  int C;
  float slope;
  int64_t lds;        // row stride (floats) of stat_m / stat_l / c
  const float* att;   // [C]
  const float* xd;    // l: fwd / bwd_dst the rows' own; bwd_src gathered by destination id
  int64_t ldxd;
  const float* xs;    // r: fwd / bwd_dst gathered (columns < nsplit); bwd_src the rows' own
  int64_t ldxs;
  const float* xs2;   // second source (columns >= nsplit) or nullptr
  int64_t ldxs2;
  int64_t nsplit;
  float* out;         // fwd
  int64_t ldo;
  float beta;
  float* stat_m;      // [*, heads] written by fwd, read by the backward kernels
  float* stat_l;
  const float* g;     // dL/dout: bwd_dst the rows' own, bwd_src gathered
  int64_t ldg;
  const float* c;     // [*, heads] <g_i^h, out_i^h>
  float* dxd;         // bwd_dst
  int64_t lddxd;
  float* da_part;     // bwd_dst: [gridDim.x, C]
  float* dxs;         // bwd_src
  int64_t lddxs;
};

template <typename IdxT>
__device__ __forceinline__ int64_t load_col(const V2Args& a, int64_t pos) {
  return static_cast<int64_t>(static_cast<const IdxT*>(a.col)[pos]);
}

__device__ __forceinline__ float4 leaky4(const float4& pre, float slope) {
  return make_float4(pre.x > 0.f ? pre.x : slope * pre.x, pre.y > 0.f ? pre.y : slope * pre.y,
                     pre.z > 0.f ? pre.z : slope * pre.z, pre.w > 0.f ? pre.w : slope * pre.w);
}

// a lam per channel (av or its slope multiple; slope at pre == 0)
__device__ __forceinline__ float4 alam4(const float4& pre, const float4& av, const float4& as) {
  return make_float4(pre.x > 0.f ? av.x : as.x, pre.y > 0.f ? av.y : as.y,
                     pre.z > 0.f ? av.z : as.z, pre.w > 0.f ? av.w : as.w);
}

// this lane's four terms of <a, LeakyReLU(pre)>; one fixed order in all three kernels, so
// the backward recomputes the forward's scores bitwise
__device__ __forceinline__ float score4(const float4& av, const float4& pre, float slope) {
  return dot4(av, leaky4(pre, slope));
}

// ------------------------------------------------------------------------------------ fwd
template <typename IdxT, int LPR, int HH>
__global__ __launch_bounds__(256) void gatv2_fwd_kernel(V2Args a) {
  constexpr int G = kWave / LPR;
  constexpr int LH = LPR / HH;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, l = lane % LPR, hk = l / LH;
  const int f = 4 * l;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  const int64_t q0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t qstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const int64_t ns = a.nsplit;
  const float4 av = *vec(a.att + f);
  for (int64_t q = q0; q < ngroups; q += qstep) {
    const int64_t r = q * G + g;
    const bool has_row = r < a.nrows;
    const int64_t rr = has_row ? r : 0;
    const int64_t s = has_row ? a.rowptr[r] : 0;
    const int deg = has_row ? static_cast<int>(a.rowptr[r + 1] - s) : 0;
    const int maxdeg = group_imax<LPR>(deg);
    const float4 lv = *vec(a.xd + rr * a.ldxd + f);
    float m = -INFINITY, lsum = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int64_t my_c = kk < deg ? load_col<IdxT>(a, s + kk) : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 rv[kU];
        float e[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int64_t cj = __shfl(my_c, g * LPR + (j < LPR ? j : 0), kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t c = ok ? cj : 0;
          const bool second = a.xs2 && c >= ns;
          rv[u] = *vec(second ? a.xs2 + (c - ns) * a.ldxs2 + f : a.xs + c * a.ldxs + f);
        }
        // the chunk's scores and the new running maximum
        float mc = m;
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          e[u] = ok ? head_sum<LH>(score4(av, add4(lv, rv[u]), a.slope)) : -INFINITY;
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
          axpy4(p, rv[u], acc);
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
__global__ __launch_bounds__(256) void gatv2_bwd_dst_kernel(V2Args a) {
  constexpr int G = kWave / LPR;
  constexpr int LH = LPR / HH;
  __shared__ float4 part[256];
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, l = lane % LPR, hk = l / LH;
  const int f = 4 * l;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  const int64_t q0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t qstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const int64_t ns = a.nsplit;
  const float4 av = *vec(a.att + f);
  const float4 as = make_float4(a.slope * av.x, a.slope * av.y, a.slope * av.z, a.slope * av.w);
  float4 da = make_float4(0.f, 0.f, 0.f, 0.f);  // this lane's channels, over all its rows
  for (int64_t q = q0; q < ngroups; q += qstep) {
    const int64_t r = q * G + g;
    const bool has_row = r < a.nrows;
    const int64_t rr = has_row ? r : 0;
    const int64_t s = has_row ? a.rowptr[r] : 0;
    const int deg = has_row ? static_cast<int>(a.rowptr[r + 1] - s) : 0;
    const int maxdeg = group_imax<LPR>(deg);
    const float4 lv = *vec(a.xd + rr * a.ldxd + f);
    const float4 gv = *vec(a.g + rr * a.ldg + f);
    const float my_m = a.stat_m[rr * a.lds + hk];
    const float my_inv = a.stat_l[rr * a.lds + hk];
    const float my_c = a.c[rr * a.lds + hk];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int64_t my_col = kk < deg ? load_col<IdxT>(a, s + kk) : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 rv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int64_t cj = __shfl(my_col, g * LPR + (j < LPR ? j : 0), kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t c = ok ? cj : 0;
          const bool second = a.xs2 && c >= ns;
          rv[u] = *vec(second ? a.xs2 + (c - ns) * a.ldxs2 + f : a.xs + c * a.ldxs + f);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          const float4 pre = add4(lv, rv[u]);
          const float4 act = leaky4(pre, a.slope);
          const float e = head_sum<LH>(dot4(av, act));
          const float ga = head_sum<LH>(dot4(gv, rv[u]));
          const float de = ok ? __expf(e - my_m) * my_inv * (ga - my_c) : 0.f;
          axpy4(de, alam4(pre, av, as), acc);
          axpy4(de, act, da);
        }
      }
    }
    if (!has_row) continue;
    *reinterpret_cast<float4*>(a.dxd + r * a.lddxd + f) = acc;
  }
  // one row of da_part per workgroup: the 256 / LPR lanes that hold the same four channels,
  // in thread order
  part[threadIdx.x] = da;
  __syncthreads();
  if (threadIdx.x < LPR) {
    float4 sum = part[threadIdx.x];
    for (int t = threadIdx.x + LPR; t < 256; t += LPR) {
      const float4 p = part[t];
      sum.x += p.x;
      sum.y += p.y;
      sum.z += p.z;
      sum.w += p.w;
    }
    *reinterpret_cast<float4*>(a.da_part + static_cast<int64_t>(blockIdx.x) * a.C +
                               4 * threadIdx.x) = sum;
  }
}

// -------------------------------------------------------------------------------- bwd src
template <typename IdxT, int LPR, int HH>
__global__ __launch_bounds__(256) void gatv2_bwd_src_kernel(V2Args a) {
  constexpr int G = kWave / LPR;
  constexpr int LH = LPR / HH;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, l = lane % LPR, hk = l / LH;
  const int f = 4 * l;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  const int64_t q0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t qstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const float4 av = *vec(a.att + f);
  const float4 as = make_float4(a.slope * av.x, a.slope * av.y, a.slope * av.z, a.slope * av.w);
  for (int64_t q = q0; q < ngroups; q += qstep) {
    const int64_t r = q * G + g;
    const bool has_row = r < a.nrows;
    const int64_t rr = has_row ? r : 0;
    const int64_t s = has_row ? a.rowptr[r] : 0;
    const int deg = has_row ? static_cast<int>(a.rowptr[r + 1] - s) : 0;
    const int maxdeg = group_imax<LPR>(deg);
    const float4 rv = *vec(a.xs + rr * a.ldxs + f);
    float4 dr = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int64_t my_i = kk < deg ? load_col<IdxT>(a, s + kk) : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 lg[kU], gg[kU];
        float m[kU], il[kU], c[kU];
        bool ok[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int64_t i = __shfl(my_i, g * LPR + (j < LPR ? j : 0), kWave);
          ok[u] = j < LPR && k0 + j < deg;
          const int64_t ii = ok[u] ? i : 0;
          lg[u] = *vec(a.xd + ii * a.ldxd + f);
          gg[u] = *vec(a.g + ii * a.ldg + f);
          m[u] = a.stat_m[ii * a.lds + hk];
          il[u] = a.stat_l[ii * a.lds + hk];
          c[u] = a.c[ii * a.lds + hk];
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const float4 pre = add4(lg[u], rv);
          const float e = head_sum<LH>(score4(av, pre, a.slope));
          const float ga = head_sum<LH>(dot4(gg[u], rv));
          const float al = ok[u] ? __expf(e - m[u]) * il[u] : 0.f;
          const float de = ok[u] ? al * (ga - c[u]) : 0.f;
          axpy4(al, gg[u], dr);
          axpy4(de, alam4(pre, av, as), dr);
        }
      }
    }
    if (!has_row) continue;
    *reinterpret_cast<float4*>(a.dxs + r * a.lddxs + f) = dr;
  }
}

template <int KIND, typename IdxT, int LPR, int HH>
void launch_one(const V2Args& a, int64_t blocks, hipStream_t st) {
  dim3 grid(static_cast<unsigned>(blocks)), block(256);
  if constexpr (KIND == 0)
    hipLaunchKernelGGL((gatv2_fwd_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
  else if constexpr (KIND == 1)
    hipLaunchKernelGGL((gatv2_bwd_dst_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((gatv2_bwd_src_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
}

template <int KIND, typename IdxT>
hipError_t launch_kind(const V2Args& a, int heads, hipStream_t st) {
  const int LPR = a.C / 4;
  const int64_t G = kWave / LPR;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  int64_t blocks = (ngroups + 3) / 4;  // one row group per wave, in order
  if (KIND == 1) blocks = gatv2_da_parts(a.nrows, a.C);  // strided: one da_part row each
  if (blocks < 1) blocks = 1;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
#define DG_V2(L_, H_)                                    \
  if (LPR == L_ && heads == H_) {                        \
    launch_one<KIND, IdxT, L_, H_>(a, blocks, st);       \
    return hipGetLastError();                            \
  }
  DG_V2(16, 1) DG_V2(16, 2) DG_V2(16, 4) DG_V2(16, 8)
  DG_V2(32, 1) DG_V2(32, 2) DG_V2(32, 4) DG_V2(32, 8)
  DG_V2(64, 1) DG_V2(64, 2) DG_V2(64, 4) DG_V2(64, 8)
#undef DG_V2
  return hipErrorInvalidValue;
}

template <int KIND>
hipError_t launch(const V2Args& a, IType it, int heads, hipStream_t st) {
  if (a.nrows <= 0) return hipSuccess;
  if (!gatv2_f32_shape_ok(a.C, heads)) return hipErrorInvalidValue;
  return it == IType::I32 ? launch_kind<KIND, int32_t>(a, heads, st)
                          : launch_kind<KIND, int64_t>(a, heads, st);
}

}  // namespace

bool gatv2_f32_shape_ok(int C, int heads) { return gat_f32_shape_ok(C, heads); }

int64_t gatv2_da_parts(int64_t nrows, int C) {
  if (nrows <= 0 || C < 4 || C > 4 * kWave) return 0;
  const int64_t G = kWave / (C / 4);
  const int64_t ngroups = (nrows + G - 1) / G;
  const int64_t blocks = (ngroups + 3) / 4;
  return blocks < kMaxParts ? blocks : kMaxParts;
}

hipError_t gatv2_fwd_f32(IType it, const int64_t* rowptr, const void* col, int64_t nrows, int C,
                         int heads, int64_t lds, float slope, const float* att, const float* xd,
                         int64_t ldxd, const float* xs, int64_t ldxs, const float* xs2,
                         int64_t ldxs2, int64_t nsplit, float* out, int64_t ldo, float beta,
                         float* stat_m, float* stat_l, hipStream_t st) {
  V2Args a{};
  a.rowptr = rowptr;
  a.col = col;
  a.nrows = nrows;
  a.C = C;
  a.lds = lds;
  a.slope = slope;
  a.att = att;
  a.xd = xd;
  a.ldxd = ldxd;
  a.xs = xs;
  a.ldxs = ldxs;
  a.xs2 = xs2;
  a.ldxs2 = ldxs2;
  a.nsplit = nsplit;
  a.out = out;
  a.ldo = ldo;
  a.beta = beta;
  a.stat_m = stat_m;
  a.stat_l = stat_l;
  return launch<0>(a, it, heads, st);
}

hipError_t gatv2_bwd_dst_f32(IType it, const int64_t* rowptr, const void* col, int64_t nrows,
                             int C, int heads, int64_t lds, float slope, const float* att,
                             const float* xd, int64_t ldxd, const float* xs, int64_t ldxs,
                             const float* xs2, int64_t ldxs2, int64_t nsplit,
                             const float* stat_m, const float* stat_l, const float* g,
                             int64_t ldg, const float* c, float* dxd, int64_t lddxd,
                             float* da_part, hipStream_t st) {
  V2Args a{};
  a.rowptr = rowptr;
  a.col = col;
  a.nrows = nrows;
  a.C = C;
  a.lds = lds;
  a.slope = slope;
  a.att = att;
  a.xd = xd;
  a.ldxd = ldxd;
  a.xs = xs;
  a.ldxs = ldxs;
  a.xs2 = xs2;
  a.ldxs2 = ldxs2;
  a.nsplit = nsplit;
  a.stat_m = const_cast<float*>(stat_m);
  a.stat_l = const_cast<float*>(stat_l);
  a.g = g;
  a.ldg = ldg;
  a.c = c;
  a.dxd = dxd;
  a.lddxd = lddxd;
  a.da_part = da_part;
  return launch<1>(a, it, heads, st);
}

hipError_t gatv2_bwd_src_f32(IType it, const int64_t* rowptr, const void* col, int64_t nrows,
                             int C, int heads, int64_t lds, float slope, const float* att,
                             const float* xd, int64_t ldxd, const float* g, int64_t ldg,
                             const float* xs, int64_t ldxs, const float* stat_m,
                             const float* stat_l, const float* c, float* dxs, int64_t lddxs,
                             hipStream_t st) {
  V2Args a{};
  a.rowptr = rowptr;
  a.col = col;
  a.nrows = nrows;
  a.C = C;
  a.lds = lds;
  a.slope = slope;
  a.att = att;
  a.xd = xd;
  a.ldxd = ldxd;
  a.g = g;
  a.ldg = ldg;
  a.xs = xs;
  a.ldxs = ldxs;
  a.stat_m = const_cast<float*>(stat_m);
  a.stat_l = const_cast<float*>(stat_l);
  a.c = c;
  a.dxs = dxs;
  a.lddxs = lddxs;
  return launch<2>(a, it, heads, st);
}

}  // namespace dgraph
