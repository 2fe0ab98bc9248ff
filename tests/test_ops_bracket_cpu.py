"""CPU: the launch-timing seam of bem.ops that bench.py reads -- the profile keys, the ops they bracket, and the off state.
Needs no GPU and no library: ops loads libbem_hip.so lazily."""
import inspect

import pytest

from bem import ops

KEYS = {"pw_x6_res<3,2,1>", "pw_x6_stream<2>", "pw_gemm", "gdmlp_x6<3>", "gdmlp_x6<5>", "conv2d", "dwconv3x3", "ss2d_scan", "transpose_planes",
        "up_fuse", "pw_wgrad", "conv_wgrad", "ss2d_scan_bwd", "dwact_bwd", "ln_bwd"}


def test_key_set():
    assert set(ops._KEYS) == KEYS
    for op, bound, symbol, pred in ops._KEYS.values():
        assert bound in ("hbm", "mfma", "mfma_bf16") and symbol and (pred is None or callable(pred))


def test_every_key_names_a_bracketed_op():
    for key, (name, _, _, pred) in ops._KEYS.items():
        fn = getattr(ops, name)
        inner = getattr(fn, "__wrapped__", None)
        assert inner is not None and getattr(inner, "__wrapped__", None) is None, f"{key}: ops.{name} must carry exactly one bracket"
        assert fn.__name__ == name and fn.__doc__ == inner.__doc__ and inspect.signature(fn) == inspect.signature(inner)
        assert "kw" not in inspect.signature(fn).parameters


def test_a_key_with_a_predicate_needs_an_op_that_says_what_it_sees():
    """Such a key calls the op's ``sees``; an op bracketed without one is refused where it is defined, not under the first profile."""
    def pw_gemm(x1, Wp, M):
        return x1
    with pytest.raises(TypeError):
        ops._bracket(lambda **_: (0.0, 0.0))(pw_gemm)
    assert ops._bracket(lambda **_: (0.0, 0.0), lambda **_: ())(pw_gemm)(1, 2, 3) == 1


def test_unbracketed_neighbours_stay_unbracketed():
    """Keys count one op each: the other scan and transpose forms launch outside every key."""
    for name in ("ss2d_scan_n", "ss2d_scan_rm", "ss2d_scan_n_bwd", "transpose_plane_slice", "transpose_planes_into"):
        assert not hasattr(getattr(ops, name), "__wrapped__")


def test_start_and_stop_off_state():
    assert ops._PROF is None
    with pytest.raises(ValueError):
        ops.profile_start("nope")
    assert ops._PROF is None
    assert ops.profile_stop() is None
    assert ops._PROF is None
