// dgraph_amd — Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
// SC'11; the generator of Random123, cuRAND and torch) and the attention-dropout keep
// decision built on it. Stateless and counter-based: the bits of an edge are a pure function
// of (seed, CSR slot, head), so the forward, both backward kernels, the host and the torch
// implementation (dgraph_amd/ops/philox.py) regenerate the same mask and none is ever stored.
//
//   words = philox4x32_10(counter = (slot & 0xffffffff, slot >> 32, h >> 2, 0),
//                         key     = (seed & 0xffffffff, seed >> 32))
//   keep(slot, h) = words[h & 3] >= thr          thr = floor(p 2^32),  0 <= p < 1
//
// One call serves four heads. The DropEdge decision (edge_keep, below) is keyed by the two
// vertex ids of an edge instead of its slot. Host and device compile the same text; the only dependency is
// <cstdint>. The 32 x 32 -> 64 products become v_mul_lo_u32 / v_mul_hi_u32 on the device.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define DG_PHILOX_HD __host__ __device__ inline
#else
#define DG_PHILOX_HD inline
#endif

namespace dgraph {

struct Philox4 {
  uint32_t w[4];
};

DG_PHILOX_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                   uint32_t k0, uint32_t k1) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
  constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = static_cast<uint64_t>(kM0) * c0;
    const uint64_t p1 = static_cast<uint64_t>(kM1) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<uint32_t>(p1);
    c3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c2 = n2;
    k0 += kW0;
    k1 += kW1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// floor(p 2^32) for 0 <= p < 1 (exact in double)
inline uint32_t attn_keep_threshold(double p) {
  return static_cast<uint32_t>(p * 4294967296.0);
}

// bit h of the result: head h of the edge at CSR slot `slot` is kept. heads <= 32.
DG_PHILOX_HD uint32_t attn_keep_bits(uint64_t seed, int64_t slot, uint32_t thr, int heads) {
  const uint64_t s = static_cast<uint64_t>(slot);
  uint32_t bits = 0;
  for (int h0 = 0; h0 < heads; h0 += 4) {
    const Philox4 r = philox4x32_10(static_cast<uint32_t>(s), static_cast<uint32_t>(s >> 32),
                                    static_cast<uint32_t>(h0 >> 2), 0u,
                                    static_cast<uint32_t>(seed),
                                    static_cast<uint32_t>(seed >> 32));
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (h0 + i < heads && r.w[i] >= thr) bits |= 1u << (h0 + i);
  }
  return bits;
}

// DropEdge (spmm_drop.hip): the keep decision of the edge dst <- src. It depends on the
// seed and the two vertex ids alone, never on a CSR slot, so it is the same in the forward
// pass and over the transposed pattern (no slot map), the same on every partition when the
// ids are global, and parallel entries with equal (dst, src) share one fate. `undirected`
// orders the pair first, so both directions of an edge share it too (PyG's
// force_undirected). Ids are non-negative int64.
//
//   (a, b) = undirected ? (min(dst, src), max(dst, src)) : (dst, src)
//   words  = philox4x32_10(counter = (a & 0xffffffff, a >> 32, b & 0xffffffff, b >> 32),
//                          key     = (seed & 0xffffffff, seed >> 32))
//   keep   = words[0] >= thr          thr = floor(p 2^32),  0 <= p < 1  (p = 0 keeps all)
inline uint32_t edge_keep_threshold(double p) { return attn_keep_threshold(p); }

DG_PHILOX_HD bool edge_keep(uint64_t seed, int64_t dst, int64_t src, uint32_t thr,
                            bool undirected) {
  const bool swap = undirected && src < dst;
  const uint64_t a = static_cast<uint64_t>(swap ? src : dst);
  const uint64_t b = static_cast<uint64_t>(swap ? dst : src);
  const Philox4 r = philox4x32_10(static_cast<uint32_t>(a), static_cast<uint32_t>(a >> 32),
                                  static_cast<uint32_t>(b), static_cast<uint32_t>(b >> 32),
                                  static_cast<uint32_t>(seed),
                                  static_cast<uint32_t>(seed >> 32));
  return r.w[0] >= thr;
}

}  // namespace dgraph
