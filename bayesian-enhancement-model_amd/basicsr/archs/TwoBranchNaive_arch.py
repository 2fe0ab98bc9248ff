from bem.archs import NaiveVMUNetTwoBranch  # noqa: F401
