// dgraph_amd — the per-lane LeakyReLU / score helpers of the fp32 GATv2 kernels
// (gatv2_f32.hip, gatv2_edge_f32.hip). One definition, so every kernel of the two files
// rounds a score's terms in the same order and a backward recomputes its forward bitwise.
#pragma once

#include "attn_device.h"

namespace dgraph {

__device__ __forceinline__ float4 leaky4(const float4& pre, float slope) {
  return make_float4(pre.x > 0.f ? pre.x : slope * pre.x, pre.y > 0.f ? pre.y : slope * pre.y,
                     pre.z > 0.f ? pre.z : slope * pre.z, pre.w > 0.f ? pre.w : slope * pre.w);
}

// a lam per channel (av or its slope multiple; slope at pre == 0)
__device__ __forceinline__ float4 alam4(const float4& pre, const float4& av, const float4& as) {
  return make_float4(pre.x > 0.f ? av.x : as.x, pre.y > 0.f ? av.y : as.y,
                     pre.z > 0.f ? av.z : as.z, pre.w > 0.f ? av.w : as.w);
}

// this lane's four terms of <a, LeakyReLU(pre)>; one fixed order in every kernel, so the
// backward recomputes the forward's scores bitwise
__device__ __forceinline__ float score4(const float4& av, const float4& pre, float slope) {
  return dot4(av, leaky4(pre, slope));
}

}  // namespace dgraph
