"""CPU: the Stage-II archs without a decomposition (VMUNet, NaiveVMUNetTwoBranch, TunedModel, FusedTunedModel): the oracle
restatements against the reference's recorded outputs (g15), the option files build through the registry with the reference's keys and
shapes, unsupported settings are refused by name, and the fused output head's C ABI rejects bad arguments before any HIP call."""
import os

import pytest
import torch

import twobranch_ref as T
from conftest import PKG, ROOT
from oracle import bem_oracle as O

NAMES = list(T.REFS)


def _case(golden, tag):
    g = golden(f"g15_twobranch_{tag}")
    return {k: v.float() for k, v in g["sd"].items()}, g


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(golden, name):
    sd, g = _case(golden, T.TAGS[name])
    y = T.REFS[name](sd, g["x"], O.selective_scan_ref)
    assert float((y - g["y"]).abs().max()) <= 2e-5, float((y - g["y"]).abs().max())


def test_restatement_d_state_1_4_16(golden):
    sd, g = _case(golden, "tuned_n1_4_16")
    assert [sd[f"{p}.0.op.A_logs"].shape[1] for p in ("encoders.0", "encoders.1", "bottleneck")] == [1, 4, 16]
    y = T.tunedmodel_ref(sd, g["x"], O.selective_scan_ref)
    assert float((y - g["y"]).abs().max()) <= 2e-5


@pytest.mark.parametrize("tag", ["tuned", "fused"])
def test_fusion_head_restatement(golden, tag):
    sd, g = _case(golden, tag)
    fin = g["fusion_in"]
    assert tuple(fin.shape) == (2, 6, 32, 32)
    y = T.fusion_ref(sd, fin[:, :3], fin[:, 3:])
    assert float((y - g["fusion_out"]).abs().max()) <= 1e-6
    assert torch.equal(g["fusion_out"], g["y"])


@pytest.mark.parametrize("name", NAMES)
def test_arch_keys_shapes_and_order(golden, name):
    """Full width (n_feat 40, [2,2,2]): the reference's keys and shapes; the reduced-width state dict of g15 loads strictly; the modules
    register in the reference's order (parameters() order); no decomposition is built."""
    ref = golden("g15_twobranch_contract")[T.TAGS[name]].tolist()
    net = T.build(name)
    mine = [f"{k}|{','.join(map(str, v.shape))}" for k, v in net.state_dict().items()]
    assert sorted(mine) == sorted(ref)
    tops = lambda keys: list(dict.fromkeys(k.split("|")[0].split(".")[0] for k in keys))
    assert tops(mine) == tops(ref)
    assert not any(k.startswith("decomp.") for k in net.state_dict()) and not hasattr(net, "decomp")
    sd, _ = _case(golden, T.TAGS[name])
    T.build(name, n_feat=16, num_blocks=(1, 1, 1)).load_state_dict(sd, strict=True)


def test_tuned_d_state_1_4_16_loads(golden):
    sd, _ = _case(golden, "tuned_n1_4_16")
    T.build("TunedModel", n_feat=16, num_blocks=(1, 1, 1), d_state=(1, 4, 16)).load_state_dict(sd, strict=True)


@pytest.mark.parametrize("yml,arch", [("TwoBranch_1.yml", "TunedModel"), ("TwoBranch_3.yml", "FusedTunedModel")])
def test_option_file_builds_through_registry(golden, yml, arch):
    from basicsr.models import build_model
    from basicsr.utils.options import parse
    opt = parse(os.path.join(PKG, "Options", yml), is_train=False)
    assert opt["network_g"]["type"] == arch and "decomp_model" not in opt["network_g"]
    opt["num_gpu"] = 0
    net = build_model(opt).net_g
    assert type(net).__name__ == arch
    ref = golden("g15_twobranch_contract")[T.TAGS[arch]].tolist()
    assert sorted(f"{k}|{','.join(map(str, v.shape))}" for k, v in net.state_dict().items()) == sorted(ref)


def test_registry_and_mirrors():
    import importlib
    from basicsr.utils.registry import ARCH_REGISTRY
    import bem.archs as A
    for name, mod in (("VMUNet", "VMUnet_arch"), ("NaiveVMUNetTwoBranch", "TwoBranchNaive_arch"), ("TunedModel", "TunedModel_arch"),
                      ("FusedTunedModel", "FusedModel_arch")):
        assert ARCH_REGISTRY.get(name) is getattr(A, name)
        assert getattr(importlib.import_module(f"basicsr.archs.{mod}"), name) is getattr(A, name)


def test_build_nets_without_decomposition():
    from bem.pipeline import build_nets
    _, net2 = build_nets(n_feat=16, num_blocks=(1, 1, 1), device="cpu", stage2="FusedTunedModel")
    assert type(net2).__name__ == "FusedTunedModel" and not hasattr(net2, "decomp")


@pytest.mark.parametrize("name", NAMES)
def test_last_act_refused(name):
    import bem.archs as A
    with pytest.raises(NotImplementedError, match="last_act"):
        getattr(A, name)(in_channels=6, n_feat=16, num_blocks=[1, 1, 1], last_act="relu")


@pytest.mark.parametrize("name", ["NaiveVMUNetTwoBranch", "TunedModel", "FusedTunedModel"])
def test_head_width_other_than_3_refused(name):
    import bem.archs as A
    with pytest.raises(NotImplementedError, match="out_channels=4"):
        getattr(A, name)(in_channels=6, out_channels=4, n_feat=16, num_blocks=[1, 1, 1])
    with pytest.raises(NotImplementedError, match="out_channels=4"):
        A.FusionHead(4)


def test_ops_refuse_cpu_tensors():
    from bem import ops
    from bem.native import BemNativeError
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(BemNativeError):
        ops.fusion_head(x, x, mean=True)


def _lib():
    from bem import native
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


def test_fusion_head_abi_rejects_before_any_hip_call():
    lib = _lib()
    p = 16   # any non-null value: the checks below reject before a pointer is touched
    B, H, W = 2, 5, 7
    fwd = lambda o1=p, o2=p, w=p, out=p, Cin=6, Cout=3, H=H, W=W, mode=0, bs1=0, bs2=0: lib.bem_fusion_head_f32(
        o1, bs1, o2, bs2, w, w, w, w, out, B, Cin, Cout, H, W, mode, None)
    assert fwd(o1=None) == 1 and b"null" in lib.bem_last_error()
    assert fwd(out=None) == 1 and b"null" in lib.bem_last_error()
    assert fwd(w=None) == 1 and b"null weight" in lib.bem_last_error()
    assert fwd(Cout=4) == 1 and b"C_out=4" in lib.bem_last_error()
    assert fwd(Cin=8) == 1 and b"C_in=8" in lib.bem_last_error()
    assert fwd(mode=2) == 1 and b"mode" in lib.bem_last_error()
    assert fwd(H=-1) == 1 and b"bad shape" in lib.bem_last_error()
    assert fwd(bs1=3 * H * W - 1) == 1 and b"batch strides" in lib.bem_last_error()
    nws = lib.bem_fusion_head_bwd_ws_elems(B, H, W)
    assert nws == 249 * B * 1 * 1 and lib.bem_fusion_head_bwd_ws_elems(1, 448, 640) == 249 * 10 * 56
    bwd = lambda ptrs, ws=nws, Cin=6, Cout=3, mode=0: lib.bem_fusion_head_bwd_f32(ptrs[0], 0, ptrs[1], 0, *ptrs[2:], ws, B, Cin, Cout, H, W, mode,
                                                                                  None)
    assert bwd([None] + [p] * 12) == 1 and b"null" in lib.bem_last_error()
    assert bwd([p] * 12 + [None]) == 1 and b"null" in lib.bem_last_error()
    assert bwd([p] * 13, Cout=1) == 1 and b"C_out=1" in lib.bem_last_error()
    assert bwd([p] * 13, ws=nws - 1) == 1 and b"workspace" in lib.bem_last_error()


def test_fusion_head_entries_in_header_and_signature_table():
    from bem import native
    hdr = open(os.path.join(ROOT, "include", "bem_hip.h")).read()
    for name in ("bem_fusion_head_f32", "bem_fusion_head_bwd_ws_elems", "bem_fusion_head_bwd_f32"):
        assert name + "(" in hdr and name in native.SIGNATURES
    assert "TunedModel_arch.py:315-319,406" in hdr and "FusedModel_arch.py:234-238,330" in hdr
