from bem.archs import CrossFusionBlock, FusedTunedModel, SEBlock, SpatialAttention  # noqa: F401
