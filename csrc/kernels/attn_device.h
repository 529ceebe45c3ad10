// dgraph_amd — device helpers shared by the row-parallel fp32 attention kernels
// (gat_f32.hip, gatv2_f32.hip, dot_attn_f32.h). All of them lay a row out the same way: one
// group of LPR = C / 4 lanes per row (16-B fp32 vectors), kWave / LPR row groups per wave,
// the heads as contiguous blocks of LH = LPR / heads lanes. gat_bf16.hip keeps the layout
// with eight bf16 channels per lane (LPR = C / 8): its unpack / pack and 8-term helpers are
// at the end.
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

// ---- bf16 storage (gat_bf16.hip, dot_attn_bf16.hip): a lane's eight channels are one 16-B vector of bf16,
// widened to fp32 by a 16-bit shift (exact) and narrowed once, at the store, by
// round-to-nearest-even (Inf and NaN pass through). LPR = C / 8 there.
struct f32x8 {
  float4 lo, hi;
};

__device__ __forceinline__ uint4 load16(const uint16_t* p) {
  return *reinterpret_cast<const uint4*>(p);
}

__device__ __forceinline__ f32x8 zero8() {
  f32x8 v;
  v.lo = make_float4(0.f, 0.f, 0.f, 0.f);
  v.hi = make_float4(0.f, 0.f, 0.f, 0.f);
  return v;
}

__device__ __forceinline__ f32x8 unpack_bf16x8(const uint4& r) {
  f32x8 v;
  v.lo.x = __uint_as_float(r.x << 16);
  v.lo.y = __uint_as_float(r.x & 0xffff0000u);
  v.lo.z = __uint_as_float(r.y << 16);
  v.lo.w = __uint_as_float(r.y & 0xffff0000u);
  v.hi.x = __uint_as_float(r.z << 16);
  v.hi.y = __uint_as_float(r.z & 0xffff0000u);
  v.hi.z = __uint_as_float(r.w << 16);
  v.hi.w = __uint_as_float(r.w & 0xffff0000u);
  return v;
}

__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b) {
  return static_cast<uint32_t>(f32_to_bf16(a)) | (static_cast<uint32_t>(f32_to_bf16(b)) << 16);
}

__device__ __forceinline__ uint4 pack_bf16x8(const f32x8& v) {
  return make_uint4(pack_bf16x2(v.lo.x, v.lo.y), pack_bf16x2(v.lo.z, v.lo.w),
                    pack_bf16x2(v.hi.x, v.hi.y), pack_bf16x2(v.hi.z, v.hi.w));
}

// this lane's eight terms of <a, b>, one fixed order (see dot4)
__device__ __forceinline__ float dot8(const f32x8& a, const f32x8& b) {
  float p = a.lo.x * b.lo.x;
  p = fmaf(a.lo.y, b.lo.y, p);
  p = fmaf(a.lo.z, b.lo.z, p);
  p = fmaf(a.lo.w, b.lo.w, p);
  p = fmaf(a.hi.x, b.hi.x, p);
  p = fmaf(a.hi.y, b.hi.y, p);
  p = fmaf(a.hi.z, b.hi.z, p);
  return fmaf(a.hi.w, b.hi.w, p);
}

__device__ __forceinline__ void axpy8(float w, const f32x8& x, f32x8& acc) {
  axpy4(w, x.lo, acc.lo);
  axpy4(w, x.hi, acc.hi);
}

__device__ __forceinline__ void scale8(float w, f32x8& acc) {
  acc.lo = make_float4(acc.lo.x * w, acc.lo.y * w, acc.lo.z * w, acc.lo.w * w);
  acc.hi = make_float4(acc.hi.x * w, acc.hi.y * w, acc.hi.z * w, acc.hi.w * w);
}

}  // namespace dgraph
