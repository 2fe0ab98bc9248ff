from bem.archs import VMUNet  # noqa: F401
