// dgraph_amd — fused fp32 dot-product graph attention (dot_attn_f32.h): the plain and the
// carry-in kernels, and the family's entry point.
#include "dot_attn_f32.h"

namespace dgraph {

template hipError_t dot_attn_launch_variant<kDotPlain>(DotKind, IType, int, const DotAttnArgs&,
                                                       hipStream_t);
template hipError_t dot_attn_launch_variant<kDotCarry>(DotKind, IType, int, const DotAttnArgs&,
                                                       hipStream_t);
// dot_attn_edge_f32.hip, dot_attn_drop_f32.hip
extern template hipError_t dot_attn_launch_variant<kDotEdge>(DotKind, IType, int,
                                                             const DotAttnArgs&, hipStream_t);
extern template hipError_t dot_attn_launch_variant<kDotDrop>(DotKind, IType, int,
                                                             const DotAttnArgs&, hipStream_t);

bool dot_attn_f32_shape_ok(int C, int heads) { return gat_f32_shape_ok(C, heads); }

hipError_t dot_attn_launch(DotKind kind, DotVariant variant, IType it, int heads,
                           const DotAttnArgs& a, hipStream_t st) {
  switch (variant) {
    case DotVariant::Plain: return dot_attn_launch_variant<kDotPlain>(kind, it, heads, a, st);
    case DotVariant::Carry: return dot_attn_launch_variant<kDotCarry>(kind, it, heads, a, st);
    case DotVariant::Edge: return dot_attn_launch_variant<kDotEdge>(kind, it, heads, a, st);
    case DotVariant::Drop: return dot_attn_launch_variant<kDotDrop>(kind, it, heads, a, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace dgraph
