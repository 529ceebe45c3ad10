// dgraph_amd — fused fp32 dot-product graph attention (dot_attn_f32.h): the kernels with
// dropout on the attention coefficients (TransformerConv(dropout=p) in training).
#include "dot_attn_f32.h"

namespace dgraph {

template hipError_t dot_attn_launch_variant<kDotDrop>(DotKind, IType, int, const DotAttnArgs&,
                                                      hipStream_t);

}  // namespace dgraph
