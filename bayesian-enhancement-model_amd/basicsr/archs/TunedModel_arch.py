from bem.archs import CrossFusionBlock, SEBlock, SpatialAttention, TunedModel  # noqa: F401
