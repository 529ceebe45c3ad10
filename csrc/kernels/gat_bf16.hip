// dgraph_amd — fused relation attention with bf16 storage for gfx950 (the bf16 lean RGAT
// layer). Per destination row i, head k (channels [kD, (k+1)D) of C = heads D):
//
//   ss_j  = <z_j[head k], a_src[k]>             computed HERE, from the gathered bf16 row
//   e_ij  = leaky_relu(sd_i[k] + ss_j, slope)
//   alpha = softmax_j(e_ij)                      max-subtracted, over the row's entries
//   out_i = bf16_rne(beta out_i + sum_j alpha_ij z_j[head k])
//
// z, the halo rows (second source: columns >= nsplit), out, g = dL/dout, gz are bf16; sd,
// stat_m, stat_l (= 1 / sum, 0 for an empty row), c, gsd, gss, a_src and the da partial rows
// are fp32. All arithmetic and accumulation is fp32: a bf16 value is widened by a 16-bit
// shift and narrowed once, at the store, by round-to-nearest-even (Inf / NaN pass through).
//
// This is not gat_f32.hip with the type swapped:
//
// * Layout: one group of LPR = C / 8 lanes per row (8 / 16 / 32), eight channels per lane,
//   ONE 16-B load per lane per gathered row; 64 / LPR row groups per wave; the heads as
//   contiguous blocks of LH = LPR / heads >= 1 lanes (LH = 1: the head sum is the identity).
//   The lane's eight a_src values stay in registers.
// * The score comes from the gathered row: the same 16 bytes feed ss_j (dot8 with the
//   resident a_src, then head_sum) and the message. There is no ss / ss2 operand and no
//   source-side score GEMM (the fp32 forward reads ss[j] three times per edge from cache
//   lines of its own). All three kernels call score() — one function, one order — so the
//   backward kernels recompute the forward's scores bit for bit.
// * gat_bf16_fwd: ONE pass with a running maximum (as dot_attn_f32.h; the fp32 GAT runs a
//   max pass, a sum pass and a gather pass): column ids loaded lane-parallel and broadcast by
//   shuffle, kU = 8 rows in flight; per batch its maximum, one rescale of the accumulator
//   and the running sum, then the accumulation. Writes stat_m and stat_l.
// * gat_bf16_bwd_dst: g_i unpacked once and resident; per entry gathers z_j, recomputes
//   ss_j and alpha, ga = head_sum(<g, z_j>); accumulates c and gsd = A - c B as the fp32
//   kernel does.
// * gat_bf16_bwd_src: over the transposed pattern with z_j resident and ss_j computed once
//   per row; gathers g_i (bf16) and sd, m, 1/l, c of the destination;
//   dz_j = bf16_rne(sum alpha g_i + gss_j a_src) and gss_j. In the same pass every lane
//   accumulates its eight channels of da[k, d] = sum_j gss_j[k] z_j[kD + d] over the rows it
//   handles; a workgroup is ONE wave here, which folds its row groups by xor shuffles and
//   writes one row of da_part [P, C]. P (gat_bf16_da_parts) is a function of (nrows, C)
//   only: the grid is capped at kMaxParts workgroups that stride over the row groups. The
//   caller sums the rows; no [heads, rows] x [rows, C] GEMM and no fp32 copy of z.
//
// Column ids are int32. Every feature array has its own row stride (elements, a multiple of
// 8), so z may be a column view of a wider GEMM output; the per-head arrays are contiguous
// [rows, heads]. No atomics, no LDS, no scratch; fixed summation orders: two calls give
// equal bits. Padding lanes / slots (a wave's groups run to the longest row of the wave)
// gather row 0 of the first source (bwd_src: of g and the destination arrays) with weight
// 0; the callers launch only when that row exists (bindings_gat_bf16.cpp).
//
// Compiler resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=
// kernel-resource-usage; the 12 (LPR, heads) instantiations of each kernel at kU = 8; no
// LDS, no AGPRs; 512 VGPRs per SIMD lane, so waves per SIMD = min(8, 512 / VGPRs)):
//                     LPR = 8          LPR = 16         LPR = 32
//   heads             1   2   4   8    1   2   4   8    1   2   4   8
//   fwd      VGPRs    125 127 125 125  127 127 127 127  118 120 119 118   occupancy 4
//   bwd_dst  VGPRs     90  91  90  79   96  96  95  95   84  83  82  82   occupancy 5 (8/8: 6)
//   bwd_src  VGPRs    167 167 167 140  185 187 186 185  162 164 163 162   occupancy 3 (LPR 16: 2)
// Scratch 0 B, no VGPR and no SGPR spilled in all 36. The forward holds kU raw 16-B rows
// (32 VGPRs), their kU scores, and unpacks each row twice (score, then message: two VALU ops
// per pair of channels) rather than keeping 8 kU fp32 values. The source side holds four
// resident / accumulator vectors of eight (z_j, a_src, dz, da), kU raw rows and 4 kU gathered
// destination scalars; as a one-wave workgroup its register budget is not capped by the
// 256-thread bound of the other two. The file is compiled without packed-fp32 instructions
// (_build.py: EXTRA_FLAGS).
#include "attn_device.h"
#include "kernels.h"

namespace dgraph {
namespace {

constexpr int kU = 8;            // gathered 16-B rows in flight per lane
constexpr int kMaxParts = 8192;  // waves of gat_bf16_bwd_src = rows of da_part, at most
                                 // (256 CUs x 4 SIMDs x 8 waves: never the occupancy bound)

struct GatBf16Args {
  const int64_t* rowptr;
  const int32_t* col;
  int64_t nrows;
  float slope;
  const float* a_src;   // [C]
  const uint16_t* x;    // gathered rows (z: fwd / bwd_dst; g of the destinations: bwd_src)
  int64_t ldx;
  const uint16_t* x2;   // second source (columns >= nsplit) or nullptr
  int64_t ldx2;
  int64_t nsplit;
  const float* sd;      // [rows or destinations, HH]
  float* stat_m;        // [*, HH] written by fwd, read by the backward kernels
  float* stat_l;
  // fwd
  uint16_t* out;
  int64_t ldo;
  float beta;
  // bwd_dst
  const uint16_t* g;    // the rows' own dL/dout
  int64_t ldg;
  float* c_out;         // [nrows, HH]
  float* gsd_out;
  // bwd_src (rows = sources, col = destination ids)
  const uint16_t* z;    // the rows' own features
  int64_t ldz;
  const float* c_dst;   // [destinations, HH]
  uint16_t* gz;
  int64_t ldgz;
  float* gss;           // [nrows, HH]
  float* da_part;       // [gridDim.x, C]
};

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// ss_j[head of this lane] from a gathered row: the ONE definition all three kernels use
template <int LH>
__device__ __forceinline__ float score(const f32x8& zv, const f32x8& av) {
  return head_sum<LH>(dot8(zv, av));
}

__device__ __forceinline__ f32x8 load_a(const float* a_src, int f) {
  f32x8 av;
  av.lo = *vec(a_src + f);
  av.hi = *vec(a_src + f + 4);
  return av;
}

// ------------------------------------------------------------------------------------ fwd
template <int LPR, int HH>
__global__ __launch_bounds__(256) void gat_bf16_fwd_kernel(GatBf16Args a) {
  constexpr int G = kWave / LPR;
  constexpr int LH = LPR / HH;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, l = lane % LPR, hk = l / LH;
  const int f = 8 * l;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  const int64_t q0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t qstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const int64_t ns = a.nsplit;
  const f32x8 av = load_a(a.a_src, f);
  for (int64_t q = q0; q < ngroups; q += qstep) {
    const int64_t r = q * G + g;
    const bool has_row = r < a.nrows;
    const int64_t s = has_row ? a.rowptr[r] : 0;
    const int deg = has_row ? static_cast<int>(a.rowptr[r + 1] - s) : 0;
    const int maxdeg = group_imax<LPR>(deg);
    const float my_sd = has_row ? a.sd[r * HH + hk] : 0.f;
    float m = -INFINITY, lsum = 0.f;
    f32x8 acc = zero8();
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int my_c = kk < deg ? a.col[s + kk] : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        uint4 raw[kU];
        float e[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int cj = __shfl(my_c, g * LPR + (j < LPR ? j : 0), kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t c = ok ? cj : 0;
          const bool second = a.x2 && c >= ns;
          raw[u] = load16(second ? a.x2 + (c - ns) * a.ldx2 + f : a.x + c * a.ldx + f);
        }
        // the batch's scores, from the rows just gathered, and the new running maximum
        float mc = m;
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          const float ss = score<LH>(unpack_bf16x8(raw[u]), av);
          e[u] = ok ? lrelu(my_sd + ss, a.slope) : -INFINITY;
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
          axpy8(p, unpack_bf16x8(raw[u]), acc);
        }
      }
    }
    if (!has_row) continue;
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
    scale8(inv, acc);
    uint16_t* o = a.out + r * a.ldo + f;
    if (a.beta != 0.f) {
      axpy8(a.beta, unpack_bf16x8(load16(o)), acc);  // one fma per channel
    }
    *reinterpret_cast<uint4*>(o) = pack_bf16x8(acc);
    if (l % LH == 0) {
      a.stat_m[r * HH + hk] = m;
      a.stat_l[r * HH + hk] = inv;  // 1 / sum (0 for an empty row)
    }
  }
}

// -------------------------------------------------------------------------------- bwd dst
template <int LPR, int HH>
__global__ __launch_bounds__(256) void gat_bf16_bwd_dst_kernel(GatBf16Args a) {
  constexpr int G = kWave / LPR;
  constexpr int LH = LPR / HH;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, l = lane % LPR, hk = l / LH;
  const int f = 8 * l;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  const int64_t q0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t qstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  const int64_t ns = a.nsplit;
  const f32x8 av = load_a(a.a_src, f);
  for (int64_t q = q0; q < ngroups; q += qstep) {
    const int64_t r = q * G + g;
    const bool has_row = r < a.nrows;
    const int64_t rr = has_row ? r : 0;
    const int64_t s = has_row ? a.rowptr[r] : 0;
    const int deg = has_row ? static_cast<int>(a.rowptr[r + 1] - s) : 0;
    const int maxdeg = group_imax<LPR>(deg);
    const f32x8 gv = unpack_bf16x8(load16(a.g + rr * a.ldg + f));
    const float my_sd = a.sd[rr * HH + hk];
    const float my_m = a.stat_m[rr * HH + hk];
    const float my_inv = a.stat_l[rr * HH + hk];
    float cacc = 0.f, aacc = 0.f, bacc = 0.f;
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int my_c = kk < deg ? a.col[s + kk] : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        uint4 raw[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int cj = __shfl(my_c, g * LPR + (j < LPR ? j : 0), kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t c = ok ? cj : 0;
          const bool second = a.x2 && c >= ns;
          raw[u] = load16(second ? a.x2 + (c - ns) * a.ldx2 + f : a.x + c * a.ldx + f);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          const f32x8 zv = unpack_bf16x8(raw[u]);
          const float e = my_sd + score<LH>(zv, av);
          const float p = head_sum<LH>(dot8(gv, zv));
          const float lam = e > 0.f ? 1.f : a.slope;
          const float al = ok ? __expf(lrelu(e, a.slope) - my_m) * my_inv : 0.f;
          cacc = fmaf(al, p, cacc);
          aacc = fmaf(lam * al, p, aacc);
          bacc = fmaf(lam, al, bacc);
        }
      }
    }
    if (has_row && l % LH == 0) {
      a.c_out[r * HH + hk] = cacc;
      a.gsd_out[r * HH + hk] = aacc - cacc * bacc;
    }
  }
}

// -------------------------------------------------------------------------------- bwd src
// one wave per workgroup: its row of da_part is folded by shuffles, without LDS
template <int LPR, int HH>
__global__ __launch_bounds__(kWave) void gat_bf16_bwd_src_kernel(GatBf16Args a) {
  constexpr int G = kWave / LPR;
  constexpr int LH = LPR / HH;
  const int lane = threadIdx.x;
  const int g = lane / LPR, l = lane % LPR, hk = l / LH;
  const int f = 8 * l;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  const f32x8 av = load_a(a.a_src, f);
  f32x8 da = zero8();  // this lane's channels, over all its rows
  for (int64_t q = blockIdx.x; q < ngroups; q += gridDim.x) {
    const int64_t r = q * G + g;
    const bool has_row = r < a.nrows;
    const int64_t rr = has_row ? r : 0;
    const int64_t s = has_row ? a.rowptr[r] : 0;
    const int deg = has_row ? static_cast<int>(a.rowptr[r + 1] - s) : 0;
    const int maxdeg = group_imax<LPR>(deg);
    const f32x8 zv = unpack_bf16x8(load16(a.z + rr * a.ldz + f));
    const float my_ss = score<LH>(zv, av);
    f32x8 acc = zero8();
    float gss = 0.f;
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int my_i = kk < deg ? a.col[s + kk] : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        uint4 raw[kU];
        float e[kU], m[kU], il[kU], c[kU];
        bool ok[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int i = __shfl(my_i, g * LPR + (j < LPR ? j : 0), kWave);
          ok[u] = j < LPR && k0 + j < deg;
          const int64_t ii = ok[u] ? i : 0;
          raw[u] = load16(a.x + ii * a.ldx + f);
          e[u] = a.sd[ii * HH + hk] + my_ss;
          m[u] = a.stat_m[ii * HH + hk];
          il[u] = a.stat_l[ii * HH + hk];
          c[u] = a.c_dst[ii * HH + hk];
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const f32x8 gv = unpack_bf16x8(raw[u]);
          const float p = head_sum<LH>(dot8(gv, zv));
          const float lam = e[u] > 0.f ? 1.f : a.slope;
          const float al = ok[u] ? __expf(lrelu(e[u], a.slope) - m[u]) * il[u] : 0.f;
          axpy8(al, gv, acc);
          gss = fmaf(lam * al, p - c[u], gss);
        }
      }
    }
    if (!has_row) continue;
    axpy8(gss, av, acc);  // ss_j = <z_j, a_src>: its gradient flows back into z_j
    *reinterpret_cast<uint4*>(a.gz + r * a.ldgz + f) = pack_bf16x8(acc);
    if (l % LH == 0) a.gss[r * HH + hk] = gss;
    axpy8(gss, zv, da);
  }
  // the wave's row groups hold the same eight channels LPR lanes apart
#pragma unroll
  for (int off = LPR; off < kWave; off <<= 1) {
    da.lo.x += __shfl_xor(da.lo.x, off, kWave);
    da.lo.y += __shfl_xor(da.lo.y, off, kWave);
    da.lo.z += __shfl_xor(da.lo.z, off, kWave);
    da.lo.w += __shfl_xor(da.lo.w, off, kWave);
    da.hi.x += __shfl_xor(da.hi.x, off, kWave);
    da.hi.y += __shfl_xor(da.hi.y, off, kWave);
    da.hi.z += __shfl_xor(da.hi.z, off, kWave);
    da.hi.w += __shfl_xor(da.hi.w, off, kWave);
  }
  if (lane < LPR) {
    float* d = a.da_part + static_cast<int64_t>(blockIdx.x) * (8 * LPR) + f;
    *reinterpret_cast<float4*>(d) = da.lo;
    *reinterpret_cast<float4*>(d + 4) = da.hi;
  }
}

template <int KIND, int LPR, int HH>
void launch_one(const GatBf16Args& a, int64_t blocks, hipStream_t st) {
  dim3 grid(static_cast<unsigned>(blocks));
  if constexpr (KIND == 0)
    hipLaunchKernelGGL((gat_bf16_fwd_kernel<LPR, HH>), grid, dim3(256), 0, st, a);
  else if constexpr (KIND == 1)
    hipLaunchKernelGGL((gat_bf16_bwd_dst_kernel<LPR, HH>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((gat_bf16_bwd_src_kernel<LPR, HH>), grid, dim3(kWave), 0, st, a);
}

template <int KIND>
hipError_t launch(const GatBf16Args& a, int C, int heads, hipStream_t st) {
  if (a.nrows <= 0) return hipSuccess;
  if (!gat_bf16_shape_ok(C, heads)) return hipErrorInvalidValue;
  const int LPR = C / 8;
  const int64_t G = kWave / LPR;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  int64_t blocks = (ngroups + 3) / 4;  // one row group per wave, in order
  if (KIND == 2) blocks = gat_bf16_da_parts(a.nrows, C);  // strided: one da_part row each
  if (blocks < 1 || blocks > 0x7fffffff) return hipErrorInvalidValue;
#define DG_GATB(L_, H_)                        \
  if (LPR == L_ && heads == H_) {              \
    launch_one<KIND, L_, H_>(a, blocks, st);   \
    return hipGetLastError();                  \
  }
  DG_GATB(8, 1) DG_GATB(8, 2) DG_GATB(8, 4) DG_GATB(8, 8)
  DG_GATB(16, 1) DG_GATB(16, 2) DG_GATB(16, 4) DG_GATB(16, 8)
  DG_GATB(32, 1) DG_GATB(32, 2) DG_GATB(32, 4) DG_GATB(32, 8)
#undef DG_GATB
  return hipErrorInvalidValue;
}

}  // namespace

bool gat_bf16_shape_ok(int C, int heads) {
  if (C != 64 && C != 128 && C != 256) return false;
  return heads == 1 || heads == 2 || heads == 4 || heads == 8;  // LH = C / 8 / heads >= 1
}

int64_t gat_bf16_da_parts(int64_t nrows, int C) {
  if (nrows <= 0 || C < 8 || C > 8 * kWave) return 0;
  const int64_t G = kWave / (C / 8);
  const int64_t ngroups = (nrows + G - 1) / G;
  return ngroups < kMaxParts ? ngroups : kMaxParts;
}

hipError_t gat_fwd_bf16(const int64_t* rowptr, const int32_t* col, int64_t nrows, int C,
                        int heads, float slope, const uint16_t* z, int64_t ldz,
                        const uint16_t* zh, int64_t ldzh, int64_t nsplit, const float* a_src,
                        const float* sd, uint16_t* out, int64_t ldo, float beta, float* stat_m,
                        float* stat_l, hipStream_t st) {
  GatBf16Args a{};
  a.rowptr = rowptr;
  a.col = col;
  a.nrows = nrows;
  a.slope = slope;
  a.a_src = a_src;
  a.x = z;
  a.ldx = ldz;
  a.x2 = zh;
  a.ldx2 = ldzh;
  a.nsplit = nsplit;
  a.sd = sd;
  a.out = out;
  a.ldo = ldo;
  a.beta = beta;
  a.stat_m = stat_m;
  a.stat_l = stat_l;
  return launch<0>(a, C, heads, st);
}

hipError_t gat_bwd_dst_bf16(const int64_t* rowptr, const int32_t* col, int64_t nrows, int C,
                            int heads, float slope, const uint16_t* z, int64_t ldz,
                            const uint16_t* zh, int64_t ldzh, int64_t nsplit,
                            const float* a_src, const float* sd, const float* stat_m,
                            const float* stat_l, const uint16_t* g, int64_t ldg, float* c_out,
                            float* gsd_out, hipStream_t st) {
  GatBf16Args a{};
  a.rowptr = rowptr;
  a.col = col;
  a.nrows = nrows;
  a.slope = slope;
  a.a_src = a_src;
  a.x = z;
  a.ldx = ldz;
  a.x2 = zh;
  a.ldx2 = ldzh;
  a.nsplit = nsplit;
  a.sd = sd;
  a.stat_m = const_cast<float*>(stat_m);
  a.stat_l = const_cast<float*>(stat_l);
  a.g = g;
  a.ldg = ldg;
  a.c_out = c_out;
  a.gsd_out = gsd_out;
  return launch<1>(a, C, heads, st);
}

hipError_t gat_bwd_src_bf16(const int64_t* rowptr, const int32_t* col, int64_t nrows, int C,
                            int heads, float slope, const uint16_t* g, int64_t ldg,
                            const uint16_t* z, int64_t ldz, const float* a_src,
                            const float* sd, const float* m_dst, const float* l_dst,
                            const float* c_dst, uint16_t* gz, int64_t ldgz, float* gss,
                            float* da_part, hipStream_t st) {
  GatBf16Args a{};
  a.rowptr = rowptr;
  a.col = col;
  a.nrows = nrows;
  a.slope = slope;
  a.a_src = a_src;
  a.x = g;
  a.ldx = ldg;
  a.z = z;
  a.ldz = ldz;
  a.sd = sd;
  a.stat_m = const_cast<float*>(m_dst);
  a.stat_l = const_cast<float*>(l_dst);
  a.c_dst = c_dst;
  a.gz = gz;
  a.ldgz = ldgz;
  a.gss = gss;
  a.da_part = da_part;
  return launch<2>(a, C, heads, st);
}

}  // namespace dgraph
