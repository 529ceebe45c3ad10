// dgraph_amd — fused fp32 GATv2 graph attention WITH EDGE FEATURES for gfx950 (PyG's
// GATv2Conv with edge_dim): the edge row enters the score, the message stays r_j.
//
// For one relation, per destination row i, source column j, CSR slot p of the pair and head h
// (channels [hD, (h+1)D) of C = heads D), with l = xd, r = xs / xs2 and ee one row per slot:
//
//   pre_p   = (l_i + r_j) + ee_p                  two fp32 adds, this order in every kernel
//   act     = pre > 0 ? pre : slope pre           lam = pre > 0 ? 1 : slope
//   e_p     = sum_{c in head h} a_c act_pc
//   alpha_p = softmax over the row's slots of e_p                      (max-subtracted)
//   out_i^h = beta out_i^h + sum_p alpha_p r_j^h
//   de_p    = alpha_p (<g_i^h, r_j^h> - c_i^h)    c_i^h = <g_i^h, out_i^h>  (c is an input)
//   dee_p   = de_p a lam                          [E, C]: the gradient of ee
//   dl_i    = sum_p dee_p       dr_j = sum_{p: col[p] = j} (alpha_p g_i + dee_p)
//   da      = sum_p de_p act_p
//
// Three row-parallel kernels in the layout of gatv2_f32.hip (attn_device.h): one LPR-lane
// group per row (LPR = C / 4, 16-B fp32 vectors), the heads as contiguous blocks of
// LH = LPR / heads lanes, the per-head sum by xor shuffles inside a block.
//
// * gatv2_edge_fwd: the one-pass forward of gatv2_fwd. Resident: l_i, a, the running
//   maximum / sum and the accumulator. Per slot it gathers r_j ONCE (the same vector feeds
//   score and message) and STREAMS ee_p: slots s + k of a row are consecutive rows of ee, so
//   a lane group reads consecutive 16-B vectors (coalesced, not gathered). One rescale per
//   chunk of kU slots. Writes out, stat_m and stat_l (= 1 / sum; 0 for an empty row, whose
//   stat_m is unspecified and whose out is beta out).
// * gatv2_edge_bwd_dst: per destination row. Resident: l_i, g_i, a, slope a, m, 1 / l, c_i,
//   the dl accumulator and this lane's four channels of da. Gathers r_j, streams ee_p and
//   recomputes e with the forward's per-lane operation order (bitwise the forward's score, so
//   exp(e - m) <= 1). Writes dl_i and, per real slot — exactly one writer each, so neither
//   array needs initialising — dee_p (one 16-B store per lane) and w[p, h] = alpha_p (the
//   first lane of each head block). da leaves as ONE row of da_part [P, C] per workgroup,
//   combined through LDS in thread order; the grid is gatv2_da_parts(rows, C) workgroups
//   that stride over the row groups, exactly as gatv2_bwd_dst.
// * gatv2_edge_bwd_src: per SOURCE row j over the transposed pattern. Resident: the dr
//   accumulator only. Per entry it reads the destination id from t_col and the forward slot
//   from t_slot, gathers g_i, the dee[slot] row and the one scalar w[slot, h] of the lane's
//   head: dr_j = sum (w g_i + dee). It takes no a, l, r, ee, m, 1 / l or c and recomputes no
//   score, no exp and no shuffle reduction: everything per edge was formed once, by the
//   destination side. (The plain gatv2_bwd_src gathers two vectors and three statistics per
//   entry and recomputes the score: two head_sums and an exp.)
//
// Two gathered sources (xs for columns < nsplit, xs2 from nsplit on), a row stride per
// operand (ee, dee and w included), no atomics, fixed summation orders: bitwise deterministic.
//
// Memory safety. Padding lanes / slots (a wave's groups run to the longest row of the wave)
// gather row 0 of the first source and read slot 0 of ee / dee / w — a slot that exists
// whenever a kernel is launched — with weight 0, and store nothing. Real slots are
// s + k < rowptr[r + 1] <= E. The callers launch only with E > 0 and with row 0 of every
// gathered array present (bindings_gatv2.cpp); nrows <= 0 launches nothing.
//
// Compiler resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=
// kernel-resource-usage; smallest .. largest of the 24 instantiations of each kernel; no
// AGPRs; 512 VGPRs per SIMD lane, so waves per SIMD = 512 / VGPRs), at kU = 8 and kU = 4:
//                         kU = 8                          kU = 4
//   gatv2_edge_fwd        112 .. 134 VGPRs  occupancy 3 .. 4   78 ..  92 VGPRs  occupancy 5 .. 6
//   gatv2_edge_bwd_dst    149 .. 230 VGPRs  occupancy 2 .. 3  130 .. 148 VGPRs  occupancy 3
//   gatv2_edge_bwd_src     86 .. 126 VGPRs  occupancy 4 .. 5   78 ..  81 VGPRs  occupancy 5 .. 6
// Scratch 0 B and no VGPR spilled in all 144; the destination side has 4 KiB of LDS (the da
// combine) and at kU = 8 keeps 0 .. 14 scalar registers in VGPR lanes (none at kU = 4).
// Chosen: kU = 8 for all three. What hides the gather latency is the 16-B vectors in flight
// per SIMD, occupancy x 2 kU: 48 .. 64 against 40 .. 48 in the forward, 32 .. 48 against 24
// on the destination side, 64 .. 80 against 40 .. 48 on the source side. kU = 8 is ahead or
// level in every instantiation, halves the forward's rescales and matches gatv2_f32.hip.
#include "gatv2_device.h"
#include "kernels.h"

namespace dgraph {
namespace {

constexpr int kU = 8;  // slots in flight per lane: 2 kU 16-B vectors (the header comment)

template <int LPR>
struct Row {
  int64_t r, rr, s;
  bool has_row;
  int deg, maxdeg;
  __device__ __forceinline__ Row(const int64_t* rowptr, int64_t nrows, int64_t q, int g) {
    r = q * (kWave / LPR) + g;
    has_row = r < nrows;
    rr = has_row ? r : 0;
    s = has_row ? rowptr[r] : 0;
    deg = has_row ? static_cast<int>(rowptr[r + 1] - s) : 0;
    maxdeg = group_imax<LPR>(deg);
  }
};

// ------------------------------------------------------------------------------------ fwd
template <typename IdxT, int LPR, int HH>
__global__ __launch_bounds__(256) void gatv2_edge_fwd_kernel(GatV2EdgeArgs a) {
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
    const Row<LPR> row(a.rowptr, a.nrows, q, g);
    const int64_t s = row.s;
    const int deg = row.deg, maxdeg = row.maxdeg;
    const float4 lv = *vec(a.xd + row.rr * a.ldxd + f);
    float m = -INFINITY, lsum = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int64_t my_c = kk < deg ? load_idx<IdxT>(a.col, s + kk) : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 rv[kU], ev[kU];
        float e[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int64_t cj = __shfl(my_c, g * LPR + (j < LPR ? j : 0), kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t c = ok ? cj : 0;
          const int64_t p = ok ? s + k0 + j : 0;  // the slot: consecutive rows of ee
          const bool second = a.xs2 && c >= ns;
          rv[u] = *vec(second ? a.xs2 + (c - ns) * a.ldxs2 + f : a.xs + c * a.ldxs + f);
          ev[u] = *vec(a.ee + p * a.ldee + f);
        }
        // the chunk's scores and the new running maximum
        float mc = m;
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          const float4 pre = add4(add4(lv, rv[u]), ev[u]);
          e[u] = ok ? head_sum<LH>(score4(av, pre, a.slope)) : -INFINITY;
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
    if (!row.has_row) continue;
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
    acc.x *= inv;
    acc.y *= inv;
    acc.z *= inv;
    acc.w *= inv;
    float* o = a.out + row.r * a.ldo + f;
    if (a.beta != 0.f) {
      const float4 old = *vec(o);
      acc.x = fmaf(a.beta, old.x, acc.x);
      acc.y = fmaf(a.beta, old.y, acc.y);
      acc.z = fmaf(a.beta, old.z, acc.z);
      acc.w = fmaf(a.beta, old.w, acc.w);
    }
    *reinterpret_cast<float4*>(o) = acc;
    if (l % LH == 0) {
      a.stat_m[row.r * a.lds + hk] = m;
      a.stat_l[row.r * a.lds + hk] = inv;  // 1 / sum (0 for an empty row)
    }
  }
}

// -------------------------------------------------------------------------------- bwd dst
template <typename IdxT, int LPR, int HH>
__global__ __launch_bounds__(256) void gatv2_edge_bwd_dst_kernel(GatV2EdgeArgs a) {
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
    const Row<LPR> row(a.rowptr, a.nrows, q, g);
    const int64_t rr = row.rr, s = row.s;
    const int deg = row.deg, maxdeg = row.maxdeg;
    const float4 lv = *vec(a.xd + rr * a.ldxd + f);
    const float4 gv = *vec(a.g + rr * a.ldg + f);
    const float my_m = a.stat_m[rr * a.lds + hk];
    const float my_inv = a.stat_l[rr * a.lds + hk];
    const float my_c = a.c[rr * a.lds + hk];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int64_t my_col = kk < deg ? load_idx<IdxT>(a.col, s + kk) : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 rv[kU], ev[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int64_t cj = __shfl(my_col, g * LPR + (j < LPR ? j : 0), kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t c = ok ? cj : 0;
          const int64_t p = ok ? s + k0 + j : 0;
          const bool second = a.xs2 && c >= ns;
          rv[u] = *vec(second ? a.xs2 + (c - ns) * a.ldxs2 + f : a.xs + c * a.ldxs + f);
          ev[u] = *vec(a.ee + p * a.ldee + f);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          const float4 pre = add4(add4(lv, rv[u]), ev[u]);
          const float4 act = leaky4(pre, a.slope);
          const float e = head_sum<LH>(dot4(av, act));
          const float ga = head_sum<LH>(dot4(gv, rv[u]));
          const float al = ok ? __expf(e - my_m) * my_inv : 0.f;
          const float de = ok ? al * (ga - my_c) : 0.f;
          const float4 al4 = alam4(pre, av, as);
          const float4 d = make_float4(de * al4.x, de * al4.y, de * al4.z, de * al4.w);
          acc = add4(acc, d);
          axpy4(de, act, da);
          if (ok) {  // this slot's only writer
            const int64_t p = s + k0 + j;
            *reinterpret_cast<float4*>(a.dee + p * a.lddee + f) = d;
            if (l % LH == 0) a.w[p * a.ldw + hk] = al;
          }
        }
      }
    }
    if (!row.has_row) continue;
    *reinterpret_cast<float4*>(a.dxd + row.r * a.lddxd + f) = acc;
  }
  // one row of da_part per workgroup: the 256 / LPR lanes that hold the same four channels,
  // in thread order
  part[threadIdx.x] = da;
  __syncthreads();
  if (threadIdx.x < LPR) {
    float4 sum = part[threadIdx.x];
    for (int t = threadIdx.x + LPR; t < 256; t += LPR) sum = add4(sum, part[t]);
    *reinterpret_cast<float4*>(a.da_part + static_cast<int64_t>(blockIdx.x) * a.C +
                               4 * threadIdx.x) = sum;
  }
}

// -------------------------------------------------------------------------------- bwd src
// rowptr / col / t_slot: the transposed pattern (rows = source rows, col = destination ids,
// t_slot = the forward slot of each entry, both indexed by absolute position)
template <typename IdxT, int LPR, int HH>
__global__ __launch_bounds__(256) void gatv2_edge_bwd_src_kernel(GatV2EdgeArgs a) {
  constexpr int G = kWave / LPR;
  constexpr int LH = LPR / HH;
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, l = lane % LPR, hk = l / LH;
  const int f = 4 * l;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  const int64_t q0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t qstep = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
  for (int64_t q = q0; q < ngroups; q += qstep) {
    const Row<LPR> row(a.rowptr, a.nrows, q, g);
    const int64_t s = row.s;
    const int deg = row.deg, maxdeg = row.maxdeg;
    float4 dr = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int64_t my_i = kk < deg ? load_idx<IdxT>(a.col, s + kk) : 0;
      const int64_t my_p = kk < deg ? load_idx<IdxT>(a.t_slot, s + kk) : 0;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 gg[kU], dv[kU];
        float al[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int src_lane = g * LPR + (j < LPR ? j : 0);
          const int64_t i = __shfl(my_i, src_lane, kWave);
          const int64_t p = __shfl(my_p, src_lane, kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t ii = ok ? i : 0;
          const int64_t pp = ok ? p : 0;
          gg[u] = *vec(a.g + ii * a.ldg + f);
          dv[u] = *vec(a.dee + pp * a.lddee + f);
          const float wa = a.w[pp * a.ldw + hk];
          al[u] = ok ? wa : 0.f;
          if (!ok) dv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          axpy4(al[u], gg[u], dr);
          dr = add4(dr, dv[u]);
        }
      }
    }
    if (!row.has_row) continue;
    *reinterpret_cast<float4*>(a.dxs + row.r * a.lddxs + f) = dr;
  }
}

template <int KIND, typename IdxT, int LPR, int HH>
void launch_one(const GatV2EdgeArgs& a, int64_t blocks, hipStream_t st) {
  dim3 grid(static_cast<unsigned>(blocks)), block(256);
  if constexpr (KIND == 0)
    hipLaunchKernelGGL((gatv2_edge_fwd_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
  else if constexpr (KIND == 1)
    hipLaunchKernelGGL((gatv2_edge_bwd_dst_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((gatv2_edge_bwd_src_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
}

template <int KIND, typename IdxT>
hipError_t launch_kind(const GatV2EdgeArgs& a, int heads, hipStream_t st) {
  const int LPR = a.C / 4;
  const int64_t G = kWave / LPR;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  int64_t blocks = (ngroups + 3) / 4;  // one row group per wave, in order
  if (KIND == 1) blocks = gatv2_da_parts(a.nrows, a.C);  // strided: one da_part row each
  if (blocks < 1) blocks = 1;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
#define DG_V2E(L_, H_)                                   \
  if (LPR == L_ && heads == H_) {                        \
    launch_one<KIND, IdxT, L_, H_>(a, blocks, st);       \
    return hipGetLastError();                            \
  }
  DG_V2E(16, 1) DG_V2E(16, 2) DG_V2E(16, 4) DG_V2E(16, 8)
  DG_V2E(32, 1) DG_V2E(32, 2) DG_V2E(32, 4) DG_V2E(32, 8)
  DG_V2E(64, 1) DG_V2E(64, 2) DG_V2E(64, 4) DG_V2E(64, 8)
#undef DG_V2E
  return hipErrorInvalidValue;
}

template <int KIND>
hipError_t launch(const GatV2EdgeArgs& a, IType it, int heads, hipStream_t st) {
  if (a.nrows <= 0) return hipSuccess;
  if (!gatv2_f32_shape_ok(a.C, heads)) return hipErrorInvalidValue;
  return it == IType::I32 ? launch_kind<KIND, int32_t>(a, heads, st)
                          : launch_kind<KIND, int64_t>(a, heads, st);
}

}  // namespace

hipError_t gatv2_edge_fwd_f32(const GatV2EdgeArgs& a, IType it, int heads, hipStream_t st) {
  return launch<0>(a, it, heads, st);
}

hipError_t gatv2_edge_bwd_dst_f32(const GatV2EdgeArgs& a, IType it, int heads, hipStream_t st) {
  return launch<1>(a, it, heads, st);
}

hipError_t gatv2_edge_bwd_src_f32(const GatV2EdgeArgs& a, IType it, int heads, hipStream_t st) {
  return launch<2>(a, it, heads, st);
}

}  // namespace dgraph
