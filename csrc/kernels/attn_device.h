// dgraph_amd — device helpers shared by the row-parallel fp32 attention kernels
// (gat_f32.hip, gatv2_f32.hip, dot_attn_f32.h). All of them lay a row out the same way: one
// group of LPR = C / 4 lanes per row (16-B fp32 vectors), kWave / LPR row groups per wave,
// the heads as contiguous blocks of LH = LPR / heads lanes.
#pragma once

#include "../common.h"

namespace dgraph {

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

// this lane's four terms of <a, b>; one fixed order everywhere, so a backward kernel
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

// one add per channel, the same bits whichever operand is the resident one
__device__ __forceinline__ float4 add4(const float4& a, const float4& b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

__device__ __forceinline__ const float4* vec(const float* p) {
  return reinterpret_cast<const float4*>(p);
}

}  // namespace dgraph
