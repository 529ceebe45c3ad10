def __getattr__(name):
    # ``from dgraph_amd.ops import dot_attention`` (imported on first use: the op modules
    # import each other and the native loader)
    if name == "dot_attention":
        from .dot_attn import dot_attention
        return dot_attention
    if name in ("dot_attention_parts", "dot_attention_halo", "HaloPlan"):
        from . import dot_attn
        return getattr(dot_attn, name)
    if name == "edge_dot":  # next to aggregate (ops/aggregate.py)
        from .aggregate import edge_dot
        return edge_dot
    if name == "EdgeDrop":  # the DropEdge spec of aggregate(..., drop=)
        from .aggregate import EdgeDrop
        return EdgeDrop
    if name == "softmax_aggregate_edge":  # softmax aggregation of per-edge messages
        from .aggregate import softmax_aggregate_edge
        return softmax_aggregate_edge
    if name == "gated_aggregate":  # per-channel sigmoid-gated neighbourhood sum
        from .aggregate import gated_aggregate
        return gated_aggregate
    if name == "gatv2_attention":
        from .gatv2 import gatv2_attention
        return gatv2_attention
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
