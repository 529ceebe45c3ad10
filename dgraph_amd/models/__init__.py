def __getattr__(name):
    # ``from dgraph_amd.models import CommAwarePNAConv`` (imported on first use: the model
    # modules import the op library and the native loader)
    if name == "CommAwarePNAConv":
        from .pna import CommAwarePNAConv
        return CommAwarePNAConv
    if name == "CommAwareGATv2Conv":
        from .gatv2_conv import CommAwareGATv2Conv
        return CommAwareGATv2Conv
    if name == "CommAwareGENConv":
        from .genconv import CommAwareGENConv
        return CommAwareGENConv
    if name == "CommAwareResGatedGraphConv":
        from .resgated import CommAwareResGatedGraphConv
        return CommAwareResGatedGraphConv
    if name in ("InnerProductDecoder", "recon_loss", "negative_pattern"):
        from . import link_pred
        return getattr(link_pred, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
