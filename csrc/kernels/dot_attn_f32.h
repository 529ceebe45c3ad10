// dgraph_amd — fused fp32 scaled dot-product graph attention for gfx950 (TransformerConv):
// the kernel templates of the whole family. dot_attn_f32.hip, dot_attn_edge_f32.hip and
// dot_attn_drop_f32.hip instantiate one variant each (so the three compile side by side).
//
// For one relation, per destination row i and head h (channels [hD, (h+1)D) of C = heads D),
// with p the CSR slot of edge (i, j):
//
//   kk = k_j (+ ee_p)        vv = v_j (+ ee_p)                 EDGE: one fp32 add each
//   e_ij  = scale <q_i^h, kk^h>
//   alpha = softmax_j(e_ij)                  max-subtracted, over ALL edges of the row
//   mm    = 1, DROP: keep(p, h) / (1 - p)    0 or inv_keep; philox.h decides keep
//   out_i^h = beta out_i^h + sum_j alpha mm vv^h
//   ga    = <g_i^h, vv^h>     c_i^h = sum_j alpha mm ga = <g_i^h, o_i^h>     (c is an input)
//   de    = alpha (mm ga - c_i^h)
//   dq_i  = scale sum_j de kk     dk_j = scale sum_i de q_i     dv_j = sum_i alpha mm g_i
//   EDGE: dee_p = alpha g_i^h + scale de q_i^h
//
// Composed from gather_rows + edge_softmax + the weighted SpMM this is [E, C] tensors for
// q_i, k_j, the products and v_j; here it is three row-parallel kernels and nothing per edge
// is written but what EDGE asks for (dee, w):
//
// * dot_attn_fwd: per destination row with q_i resident, ONE pass over the row's edges that
//   gathers k_j and v_j once each. The score needs the whole k_j row, so there is no cheap
//   statistics pass as in gat_f32.hip: a running maximum is kept instead, and the
//   accumulator and the running sum are rescaled once per chunk of kU edges (not per edge).
//   Writes out, stat_m (the row maximum of e) and stat_l (1 / sum exp(e - m); 0 for an
//   empty row, whose stat_m is unspecified).
//   - CARRY starts the running maximum, sum and accumulator from an earlier pass's (out,
//     stat_m, stat_l) instead of (0, -inf, 0): a softmax over a union of edge sets, one set
//     per launch (interior edges while the halo is on the links, then the halo edges;
//     several relations with their own q / k / v). The backward kernels need nothing new:
//     they recompute alpha from the final statistics and so work on any subset of the edges.
//   - EDGE loads ee_p for slot p = rowptr[r] + k0 + j and adds it into the gathered k and v
//     vectors. A row's slots are consecutive rows of ee, so ee is streamed, not gathered.
//   - DROP: the lane that loads the column id of slot s + k0 + l also evaluates the slot's
//     keep bits (one Philox call per lane per LPR edges, two at 8 heads); the bits travel
//     with the column id through one more __shfl. The running sum takes every edge, the
//     accumulator only the kept ones, times inv_keep: dropout does not enter stat_m /
//     stat_l. A row whose edges are all dropped gives out = 0, hence c = 0 and every de = 0.
//     No beta and no carry.
// * dot_attn_bwd_dst: per destination row with g_i and q_i resident: gathers k_j and v_j as
//   the forward does and accumulates dq_i. de is formed per edge from the input c, never as
//   a difference of two accumulated sums. EDGE also stores, per real slot, dee_p (one 16-B
//   store per lane) and, from the first lane of each head block, the two scalars w[p, h] =
//   alpha and w[p, heads + h] = de (without scale). Every real slot has exactly one writer,
//   so dee and w need no initialisation.
// * dot_attn_bwd_src: per SOURCE row over the transposed pattern with k_j and v_j resident:
//   gathers q_i, g_i and the destinations' m, 1/l, c, recomputes alpha, and accumulates dv_j
//   and dk_j. DROP finds the forward slot of transposed entry p' at t_slot[p'] (col's index
//   type, indexed by absolute position as col is) and evaluates the bits from it.
// * dot_attn_edge_bwd_src: the EDGE source side gathers q_i, g_i and the two scalars
//   w[t_slot[p']] and recomputes nothing; it reads neither k, v, ee nor the statistics: the
//   weights were formed once, by the destination side. Recomputing alpha here would need a
//   third random [C] gather (ee by forward slot) in what is the widest of the plain kernels;
//   w costs 8 heads bytes per edge next to the 4 C bytes of dee. It shares the helpers and
//   the row prologue with the others and is kept as its own short body.
//
// The DROP mask is never stored: all three kernels regenerate it from (seed, slot, head).
// seed is a pointer to ONE int64 in device memory, read by the kernels, so a step captured
// into a HIP graph draws a fresh mask per replay when the caller refreshes that value inside
// the captured region. thr = floor(p 2^32), inv_keep = 1 / (1 - p) formed once on the host.
//
// Two sources (k / v for columns < nsplit, k2 / v2 for columns >= nsplit: local rows and
// received halo rows, never concatenated). Every feature array has its own row stride, so k
// and v may be the column halves of one [N, 2C] buffer; the per-head arrays share the row
// stride lds. Layout as gat_f32.hip (attn_device.h): one LPR-lane group per row, the heads
// as lane blocks, the per-head dot product by xor shuffles inside a block (every lane of a
// head holds the same sum). No LDS, no atomics, fixed summation orders: bitwise
// deterministic (DROP: for a fixed seed). The variants' statements stand under
// `if constexpr` in one body; no variant pays for another's (plain is never multiplied by a
// keep factor of 1).
//
// Padding lanes / slots (a wave's groups run to the longest row of the wave) gather row 0
// of the first source, EDGE slot 0 of ee and of w, with weight 0, and evaluate no Philox
// call (bits 0); the callers launch only when those rows exist (bindings_dot_attn.cpp).
//
// Compiler resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=
// kernel-resource-usage; smallest .. largest of the 24 instantiations of each kernel at
// kU = 8; no LDS, no AGPRs; 512 VGPRs per SIMD lane, so waves per SIMD = 512 / VGPRs):
//                      plain        CARRY       EDGE          DROP
//   dot_attn_fwd       101 .. 120   103 .. 128  137 .. 158    113 .. 133   VGPRs
//                      4            4           3             3 .. 4       occupancy
//   dot_attn_bwd_dst   109 .. 128               166 .. 223    121 .. 141
//                      4                        2 .. 3        3 .. 4
//   dot_attn_bwd_src   149 .. 174               100 .. 108    159 .. 186
//                      2 .. 3                   4             2 .. 3
// Scratch 0 B and no VGPR spilled in all 240; SGPRs spilled to VGPR lanes: 0 .. 12 in EDGE
// bwd_dst (at C = 128 and 256), 0 .. 4 in DROP fwd and bwd_dst, none elsewhere. The plain
// source side holds 4 resident / accumulator vectors, 2 kU gathered ones and 3 kU gathered
// statistics; the EDGE one nothing resident but dk, dv. DROP is 8 .. 13 VGPRs over plain: the
// kU keep factors of a chunk and the bits that travel with the column id. Against the three
// separate sources this family was folded from, no instantiation takes more VGPRs or has a
// lower occupancy, and the kernels open as those did: the work-group size from one scalar
// load, rowptr fetched next (PERFORMANCE.md has the table and what the shared helpers below
// must not do).
// At kU = 4 the plain three take 70 .. 75 / 77 .. 82 / 102 .. 114 VGPRs (occupancy 6-7 / 5-6
// / 4) and the EDGE three 89 .. 99 / 123 .. 142 / 90 .. 102 (occupancy 4-5 / 3-4 / 4-5): the
// gathered vectors in flight per SIMD (occupancy x 2 kU) are about the same either way. On
// an MI355X the two measure the same within 1 % in the plain kernels and within 2 % in the
// EDGE ones, kU = 8 ahead by 0.6-1.7 % on the EDGE destination side (PERFORMANCE.md); kU = 8
// halves the rescales of the forward and matches gat_f32.hip. Keeping a DROP chunk's keep
// flags packed in one register instead of kU floats was tried and compiles to 1 .. 2 VGPRs
// MORE.
#pragma once

#include "attn_device.h"
#include "kernels.h"
#include "philox.h"

namespace dgraph {

// edges in flight per lane: 2 kU gathered 16-B vectors in fwd / bwd_dst (EDGE: a third, ee_p),
// 2 kU gathered vectors and 3 kU (EDGE: 2 kU) gathered scalars in bwd_src
constexpr int kDotU = 8;

constexpr int kDotPlain = static_cast<int>(DotVariant::Plain);
constexpr int kDotCarry = static_cast<int>(DotVariant::Carry);
constexpr int kDotEdge = static_cast<int>(DotVariant::Edge);
constexpr int kDotDrop = static_cast<int>(DotVariant::Drop);

// this lane's place in its wave's row groups, and the row groups of its wave
template <int LPR, int HH>
struct DotLane {
  static constexpr int G = kWave / LPR;
  static constexpr int LH = LPR / HH;
  int g, l, hk, f;
  int64_t ngroups, q0, qstep;
  // block_dim, grid_dim: blockDim.x and gridDim.x, read in the kernel's own body. Read in
  // here, the compiler no longer folds the uniform work-group size and every wave opens with
  // a dependent vector-memory load of the remainder group size before it fetches rowptr.
  __device__ __forceinline__ DotLane(int64_t nrows, unsigned block_dim, unsigned grid_dim) {
    const int lane = threadIdx.x & (kWave - 1);
    g = lane / LPR, l = lane % LPR, hk = l / LH;
    f = 4 * l;
    ngroups = (nrows + G - 1) / G;
    q0 = (static_cast<int64_t>(blockIdx.x) * block_dim + threadIdx.x) >> 6;
    qstep = (static_cast<int64_t>(grid_dim) * block_dim) >> 6;
  }
};

// the row of this lane's group in row group q: rr is a row that exists (0 past the end), s
// its first slot, maxdeg the longest row of the wave. It takes rowptr and nrows by value: with
// a reference to the kernel's argument struct instead, the EDGE and DROP kernels compile to
// 2 .. 4 VGPRs more (and two DROP instantiations lose a wave of occupancy).
struct DotRow {
  int64_t r, rr, s;
  bool has_row;
  int deg, maxdeg;
  template <int LPR, int HH>
  __device__ __forceinline__ DotRow(const int64_t* rowptr, int64_t nrows,
                                    const DotLane<LPR, HH>& t, int64_t q) {
    r = q * t.G + t.g;
    has_row = r < nrows;
    rr = has_row ? r : 0;
    s = has_row ? rowptr[r] : 0;
    deg = has_row ? static_cast<int>(rowptr[r + 1] - s) : 0;
    maxdeg = group_imax<LPR>(deg);
  }
};

// ------------------------------------------------------------------------------------ fwd
// CARRY: stat_l == 0 on entry: nothing accumulated yet, out and stat_m are not read (they
// may hold anything). A row without entries in this pass is left bitwise untouched and its q
// is not loaded (its lanes still serve the wave's shuffles, with weight 0).
template <typename IdxT, int LPR, int HH, int V>
__global__ __launch_bounds__(256) void dot_attn_fwd_kernel(DotAttnArgs a) {
  constexpr int kU = kDotU;
  constexpr int LH = LPR / HH;
  constexpr bool CARRY = V == kDotCarry, EDGE = V == kDotEdge, DROP = V == kDotDrop;
  const DotLane<LPR, HH> t(a.nrows, blockDim.x, gridDim.x);
  const int g = t.g, l = t.l, hk = t.hk, f = t.f;
  const int64_t ns = a.nsplit;
  uint64_t seed = 0;
  if constexpr (DROP) seed = static_cast<uint64_t>(*a.seed);
  for (int64_t q = t.q0; q < t.ngroups; q += t.qstep) {
    const DotRow row(a.rowptr, a.nrows, t, q);
    const int64_t r = row.r, s = row.s;
    const int deg = row.deg, maxdeg = row.maxdeg;
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
      qv = *vec(a.q + row.rr * a.ldq + f);
    }
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int64_t my_c = kk < deg ? load_idx<IdxT>(a.col, s + kk) : 0;
      // DROP: the keep bits of this lane's slot, all heads (a padding slot: nothing evaluated)
      uint32_t my_b = 0u;
      if constexpr (DROP) my_b = kk < deg ? attn_keep_bits(seed, s + kk, a.thr, HH) : 0u;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 kv[kU], vv[kU];
        float e[kU], mm[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int src_lane = g * LPR + (j < LPR ? j : 0);
          const int64_t cj = __shfl(my_c, src_lane, kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t c = ok ? cj : 0;
          const bool second = a.k2 && c >= ns;
          // (the two-source gather is written out: as a helper taking the pointers and strides
          // the carry kernels compile to 1 .. 2 % more instructions, 10 .. 28 address adds)
          if constexpr (EDGE) {
            const int64_t p = ok ? s + k0 + j : 0;  // the entry's slot: consecutive rows of ee
            const float4 ev = *vec(a.ee + p * a.ldee + f);
            kv[u] = add4(*vec(second ? a.k2 + (c - ns) * a.ldk2 + f : a.k + c * a.ldk + f), ev);
            vv[u] = add4(*vec(second ? a.v2 + (c - ns) * a.ldv2 + f : a.v + c * a.ldv + f), ev);
          } else {
            kv[u] = *vec(second ? a.k2 + (c - ns) * a.ldk2 + f : a.k + c * a.ldk + f);
            vv[u] = *vec(second ? a.v2 + (c - ns) * a.ldv2 + f : a.v + c * a.ldv + f);
          }
          if constexpr (DROP) {
            const uint32_t bj = __shfl(my_b, src_lane, kWave);
            mm[u] = ok && ((bj >> hk) & 1u) ? a.inv_keep : 0.f;
          }
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
          lsum += p;  // every edge
          if constexpr (DROP)
            axpy4(p * mm[u], vv[u], acc);  // the kept ones, times 1 / (1 - p)
          else
            axpy4(p, vv[u], acc);
        }
      }
    }
    if (!row.has_row) continue;
    if constexpr (CARRY) {
      if (deg == 0) continue;  // the carried state of the row is its result
    }
    const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
    acc.x *= inv;
    acc.y *= inv;
    acc.z *= inv;
    acc.w *= inv;
    float* o = a.out + r * a.ldo + f;
    if constexpr (!CARRY && !DROP) {
      if (a.beta != 0.f) {
        const float4 old = *vec(o);
        acc.x = fmaf(a.beta, old.x, acc.x);
        acc.y = fmaf(a.beta, old.y, acc.y);
        acc.z = fmaf(a.beta, old.z, acc.z);
        acc.w = fmaf(a.beta, old.w, acc.w);
      }
    }
    *reinterpret_cast<float4*>(o) = acc;
    if (l % LH == 0) {
      a.stat_m[r * a.lds + hk] = m;
      a.stat_l[r * a.lds + hk] = inv;  // 1 / sum (0 for an empty row)
    }
  }
}

// -------------------------------------------------------------------------------- bwd dst
template <typename IdxT, int LPR, int HH, int V>
__global__ __launch_bounds__(256) void dot_attn_bwd_dst_kernel(DotAttnArgs a) {
  constexpr int kU = kDotU;
  constexpr int LH = LPR / HH;
  constexpr bool EDGE = V == kDotEdge, DROP = V == kDotDrop;
  const DotLane<LPR, HH> t(a.nrows, blockDim.x, gridDim.x);
  const int g = t.g, l = t.l, hk = t.hk, f = t.f;
  const int64_t ns = a.nsplit;
  uint64_t seed = 0;
  if constexpr (DROP) seed = static_cast<uint64_t>(*a.seed);
  for (int64_t q = t.q0; q < t.ngroups; q += t.qstep) {
    const DotRow row(a.rowptr, a.nrows, t, q);
    const int64_t r = row.r, rr = row.rr, s = row.s;
    const int deg = row.deg, maxdeg = row.maxdeg;
    const float4 qv = *vec(a.q + rr * a.ldq + f);
    const float4 gv = *vec(a.g + rr * a.ldg + f);
    const float my_m = a.stat_m[rr * a.lds + hk];
    const float my_inv = a.stat_l[rr * a.lds + hk];
    const float my_c = a.c[rr * a.lds + hk];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int64_t my_col = kk < deg ? load_idx<IdxT>(a.col, s + kk) : 0;
      uint32_t my_b = 0u;
      if constexpr (DROP) my_b = kk < deg ? attn_keep_bits(seed, s + kk, a.thr, HH) : 0u;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 kv[kU], vv[kU];
        float mm[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int src_lane = g * LPR + (j < LPR ? j : 0);
          const int64_t cj = __shfl(my_col, src_lane, kWave);
          const bool ok = j < LPR && k0 + j < deg;
          const int64_t c = ok ? cj : 0;
          const bool second = a.k2 && c >= ns;
          if constexpr (EDGE) {
            const int64_t p = ok ? s + k0 + j : 0;
            const float4 ev = *vec(a.ee + p * a.ldee + f);
            kv[u] = add4(*vec(second ? a.k2 + (c - ns) * a.ldk2 + f : a.k + c * a.ldk + f), ev);
            vv[u] = add4(*vec(second ? a.v2 + (c - ns) * a.ldv2 + f : a.v + c * a.ldv + f), ev);
          } else {
            kv[u] = *vec(second ? a.k2 + (c - ns) * a.ldk2 + f : a.k + c * a.ldk + f);
            vv[u] = *vec(second ? a.v2 + (c - ns) * a.ldv2 + f : a.v + c * a.ldv + f);
          }
          if constexpr (DROP) {
            const uint32_t bj = __shfl(my_b, src_lane, kWave);
            mm[u] = ok && ((bj >> hk) & 1u) ? a.inv_keep : 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const bool ok = j < LPR && k0 + j < deg;
          const float e = a.scale * head_sum<LH>(dot4(qv, kv[u]));
          const float ga = head_sum<LH>(dot4(gv, vv[u]));
          const float al = ok ? __expf(e - my_m) * my_inv : 0.f;
          float de;
          if constexpr (DROP)
            de = ok ? al * (mm[u] * ga - my_c) : 0.f;
          else
            de = ok ? al * (ga - my_c) : 0.f;
          axpy4(de, kv[u], acc);
          if constexpr (EDGE) {
            if (ok) {  // this slot's only writer
              const int64_t p = s + k0 + j;
              const float ts = a.scale * de;
              float4 d;
              d.x = fmaf(ts, qv.x, al * gv.x);
              d.y = fmaf(ts, qv.y, al * gv.y);
              d.z = fmaf(ts, qv.z, al * gv.z);
              d.w = fmaf(ts, qv.w, al * gv.w);
              *reinterpret_cast<float4*>(a.dee + p * a.lddee + f) = d;
              if (l % LH == 0) {
                a.w[p * a.ldw + hk] = al;
                a.w[p * a.ldw + HH + hk] = de;
              }
            }
          }
        }
      }
    }
    if (!row.has_row) continue;
    acc.x *= a.scale;
    acc.y *= a.scale;
    acc.z *= a.scale;
    acc.w *= a.scale;
    *reinterpret_cast<float4*>(a.dq + r * a.lddq + f) = acc;
  }
}

// -------------------------------------------------------------------------------- bwd src
// plain and DROP: alpha recomputed from the destinations' statistics
template <typename IdxT, int LPR, int HH, int V>
__global__ __launch_bounds__(256) void dot_attn_bwd_src_kernel(DotAttnArgs a) {
  constexpr int kU = kDotU;
  constexpr int LH = LPR / HH;
  constexpr bool DROP = V == kDotDrop;
  const DotLane<LPR, HH> t(a.nrows, blockDim.x, gridDim.x);
  const int g = t.g, l = t.l, hk = t.hk, f = t.f;
  uint64_t seed = 0;
  if constexpr (DROP) seed = static_cast<uint64_t>(*a.seed);
  for (int64_t q = t.q0; q < t.ngroups; q += t.qstep) {
    const DotRow row(a.rowptr, a.nrows, t, q);
    const int64_t r = row.r, rr = row.rr, s = row.s;
    const int deg = row.deg, maxdeg = row.maxdeg;
    const float4 kv = *vec(a.k + rr * a.ldk + f);
    const float4 vv = *vec(a.v + rr * a.ldv + f);
    float4 dk = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 dv = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = 0; k0 < maxdeg; k0 += LPR) {
      const int kk = k0 + l;
      const int64_t my_i = kk < deg ? load_idx<IdxT>(a.col, s + kk) : 0;
      // DROP: the entry's forward slot keys the same bits as the destination side's
      uint32_t my_b = 0u;
      if constexpr (DROP)
        my_b = kk < deg ? attn_keep_bits(seed, load_idx<IdxT>(a.t_slot, s + kk), a.thr, HH) : 0u;
      for (int j0 = 0; j0 < LPR && k0 + j0 < maxdeg; j0 += kU) {
        float4 qg[kU], gg[kU];
        float m[kU], il[kU], c[kU], mm[kU];
        bool ok[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int j = j0 + u;
          const int src_lane = g * LPR + (j < LPR ? j : 0);
          const int64_t i = __shfl(my_i, src_lane, kWave);
          ok[u] = j < LPR && k0 + j < deg;
          const int64_t ii = ok[u] ? i : 0;
          qg[u] = *vec(a.q + ii * a.ldq + f);
          gg[u] = *vec(a.g + ii * a.ldg + f);
          m[u] = a.stat_m[ii * a.lds + hk];
          il[u] = a.stat_l[ii * a.lds + hk];
          c[u] = a.c[ii * a.lds + hk];
          if constexpr (DROP) {
            const uint32_t bj = __shfl(my_b, src_lane, kWave);
            mm[u] = ok[u] && ((bj >> hk) & 1u) ? a.inv_keep : 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const float e = a.scale * head_sum<LH>(dot4(qg[u], kv));
          const float ga = head_sum<LH>(dot4(gg[u], vv));
          const float al = ok[u] ? __expf(e - m[u]) * il[u] : 0.f;
          if constexpr (DROP) {
            const float de = ok[u] ? al * (mm[u] * ga - c[u]) : 0.f;
            axpy4(al * mm[u], gg[u], dv);
            axpy4(de, qg[u], dk);
          } else {
            const float de = ok[u] ? al * (ga - c[u]) : 0.f;
            axpy4(al, gg[u], dv);
            axpy4(de, qg[u], dk);
          }
        }
      }
    }
    if (!row.has_row) continue;
    dk.x *= a.scale;
    dk.y *= a.scale;
    dk.z *= a.scale;
    dk.w *= a.scale;
    *reinterpret_cast<float4*>(a.dk + r * a.lddk + f) = dk;
    *reinterpret_cast<float4*>(a.dv + r * a.lddv + f) = dv;
  }
}

// EDGE: the weights w written by the destination side, nothing recomputed
template <typename IdxT, int LPR, int HH>
__global__ __launch_bounds__(256) void dot_attn_edge_bwd_src_kernel(DotAttnArgs a) {
  constexpr int kU = kDotU;
  const DotLane<LPR, HH> t(a.nrows, blockDim.x, gridDim.x);
  const int g = t.g, l = t.l, hk = t.hk, f = t.f;
  for (int64_t q = t.q0; q < t.ngroups; q += t.qstep) {
    const DotRow row(a.rowptr, a.nrows, t, q);
    const int64_t r = row.r, s = row.s;
    const int deg = row.deg, maxdeg = row.maxdeg;
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
    if (!row.has_row) continue;
    dk.x *= a.scale;
    dk.y *= a.scale;
    dk.z *= a.scale;
    dk.w *= a.scale;
    *reinterpret_cast<float4*>(a.dk + r * a.lddk + f) = dk;
    *reinterpret_cast<float4*>(a.dv + r * a.lddv + f) = dv;
  }
}

// ---------------------------------------------------------------------------------- launch
template <int V, int KIND, typename IdxT, int LPR, int HH>
void dot_attn_launch_one(const DotAttnArgs& a, int64_t blocks, hipStream_t st) {
  dim3 grid(static_cast<unsigned>(blocks)), block(256);
  if constexpr (KIND == 0)
    hipLaunchKernelGGL((dot_attn_fwd_kernel<IdxT, LPR, HH, V>), grid, block, 0, st, a);
  else if constexpr (KIND == 1)
    hipLaunchKernelGGL((dot_attn_bwd_dst_kernel<IdxT, LPR, HH, V>), grid, block, 0, st, a);
  else if constexpr (V == kDotEdge)
    hipLaunchKernelGGL((dot_attn_edge_bwd_src_kernel<IdxT, LPR, HH>), grid, block, 0, st, a);
  else
    hipLaunchKernelGGL((dot_attn_bwd_src_kernel<IdxT, LPR, HH, V>), grid, block, 0, st, a);
}

template <int V, int KIND, typename IdxT>
hipError_t dot_attn_launch_kind(const DotAttnArgs& a, int heads, hipStream_t st) {
  const int LPR = a.C / 4;
  const int64_t G = kWave / LPR;
  const int64_t ngroups = (a.nrows + G - 1) / G;
  int64_t blocks = (ngroups + 3) / 4;  // one row group per wave, in order
  if (blocks < 1) blocks = 1;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
#define DG_DOT(L_, H_)                                          \
  if (LPR == L_ && heads == H_) {                               \
    dot_attn_launch_one<V, KIND, IdxT, L_, H_>(a, blocks, st);  \
    return hipGetLastError();                                   \
  }
  DG_DOT(16, 1) DG_DOT(16, 2) DG_DOT(16, 4) DG_DOT(16, 8)
  DG_DOT(32, 1) DG_DOT(32, 2) DG_DOT(32, 4) DG_DOT(32, 8)
  DG_DOT(64, 1) DG_DOT(64, 2) DG_DOT(64, 4) DG_DOT(64, 8)
#undef DG_DOT
  return hipErrorInvalidValue;
}

// every kernel of variant V; a translation unit instantiates it for its variant
// (dot_attn_f32.hip holds dot_attn_launch, which picks the variant)
template <int V>
hipError_t dot_attn_launch_variant(DotKind kind, IType it, int heads, const DotAttnArgs& a,
                                   hipStream_t st) {
  if (a.nrows <= 0) return hipSuccess;
  if (!dot_attn_f32_shape_ok(a.C, heads)) return hipErrorInvalidValue;
  if (V == kDotDrop && a.seed == nullptr) return hipErrorInvalidValue;
  const bool i32 = it == IType::I32;
  if (kind == DotKind::Fwd)
    return i32 ? dot_attn_launch_kind<V, 0, int32_t>(a, heads, st)
               : dot_attn_launch_kind<V, 0, int64_t>(a, heads, st);
  if constexpr (V != kDotCarry) {  // the carried state is the forward's alone
    if (kind == DotKind::BwdDst)
      return i32 ? dot_attn_launch_kind<V, 1, int32_t>(a, heads, st)
                 : dot_attn_launch_kind<V, 1, int64_t>(a, heads, st);
    if (kind == DotKind::BwdSrc)
      return i32 ? dot_attn_launch_kind<V, 2, int32_t>(a, heads, st)
                 : dot_attn_launch_kind<V, 2, int64_t>(a, heads, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace dgraph
