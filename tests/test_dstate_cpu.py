"""CPU: SS2D with d_state N > 1 (VMamba's ssm_d_state, vmamba.py:251-253,345-346,442): the module builds the reference's parameters,
every arch builds from an option file with d_state > 1, N > 16 is refused by name, and the N-state C ABI entries reject bad arguments
before any HIP call."""
import math
import os

import pytest
import torch

from conftest import GOLDEN, PKG


def _vss(N, C=40):
    from bem.modules import VSSBlock
    return VSSBlock(hidden_dim=C, drop_path=0, channel_first=True, ssm_d_state=N, ssm_ratio=1, ssm_dt_rank="auto", ssm_conv=3,
                    ssm_conv_bias=False, ssm_drop_rate=0, ssm_init="v0", forward_type="v05_noz", mlp_ratio=4, mlp_type="gdmlp")


@pytest.mark.parametrize("N", [4, 16])
def test_vssblock_keys_and_shapes_equal_reference(golden, N):
    ref = golden("g14_dstate")[f"sd_n{N}"]
    blk = _vss(N)
    mine = {k: tuple(v.shape) for k, v in blk.state_dict().items()}
    assert mine == {k: tuple(v.shape) for k, v in ref.items()}
    R = math.ceil(40 / 16)
    assert mine["op.x_proj_weight"] == (4, R + 2 * N, 40) and mine["op.A_logs"] == (160, N)
    blk.load_state_dict({k: v for k, v in ref.items()}, strict=True)


@pytest.mark.parametrize("N", [2, 4, 16])
def test_a_logs_init_is_log_arange(N):
    blk = _vss(N)
    want = torch.log(torch.arange(1, N + 1, dtype=torch.float32))
    A = blk.op.A_logs.detach()
    assert A.shape == (160, N)
    assert torch.equal(A, want.expand(160, N))
    assert torch.equal(blk.op.Ds.detach(), torch.ones(160))


def test_d_state_one_initialisation_unchanged():
    """N = 1 draws the same random numbers in the same order as before: two seeded builds agree and A_logs is zero."""
    torch.manual_seed(5)
    a = _vss(1).state_dict()
    torch.manual_seed(5)
    b = _vss(1).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert a["op.x_proj_weight"].shape == (4, 5, 40) and torch.equal(a["op.A_logs"], torch.zeros(160, 1))


def test_d_state_above_limit_is_refused_by_name():
    with pytest.raises(NotImplementedError, match="16"):
        _vss(17)
    with pytest.raises(NotImplementedError, match="16"):
        _vss(0)


def test_ddwavelet_mixed_d_state_key_contract(golden):
    """d_state = [1, 4, 16] per level: the full-width DecompDualBranchDDWavelet has the reference's keys and shapes."""
    from bem.archs import DecompDualBranchDDWavelet
    ref = golden("g14_dstate")["contract_ddw_1_4_16"].tolist()
    net = DecompDualBranchDDWavelet(in_channels=6, out_channels=3, n_feat=40, stage=1, num_blocks=[2, 2, 2], d_state=[1, 4, 16], ssm_ratio=1,
                                    mlp_ratio=4, mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, decomp_model="model4")
    mine = [f"{k}|{','.join(map(str, v.shape))}" for k, v in net.state_dict().items()]
    assert sorted(mine) == sorted(ref)


_OPTION_FILES = ["CG_UNet_LOLv1.yml", "DecompDualBranch2DDWavelet_4.yml", "DecompDualBranch2DD_4.yml", "DecompDualBranch2_1.yml",
                 "DecompDualBranch_4.yml", "DecompSingleBranchDD_1.yml", "DecompSingleBranch_1.yml"]


@pytest.mark.parametrize("yml", _OPTION_FILES)
def test_option_file_with_d_state_4_builds(tmp_path, yml):
    """A copy of each shipped option file with d_state: [4,4,4] builds its net; every SS2D has 4 states."""
    from basicsr.models import build_model
    from basicsr.utils.options import parse
    from bem.modules import SS2D
    text = open(os.path.join(PKG, "Options", yml)).read()
    assert "d_state: [1,1,1]" in text
    p = tmp_path / yml
    p.write_text(text.replace("d_state: [1,1,1]", "d_state: [4,4,4]"))
    opt = parse(str(p), is_train=False)
    opt["num_gpu"] = 0
    net = build_model(opt).net_g
    ss = [m for m in net.modules() if isinstance(m, SS2D)]
    assert ss and all(m.d_state == 4 and m.A_logs.shape[1] == 4 and m.x_proj_weight.shape[1] == m.dt_rank + 8 for m in ss)


def _lib():
    from bem import native
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


def test_scan_n_supported_query():
    lib = _lib()
    assert [lib.bem_ss2d_scan_n_supported(n) for n in (0, 1, 2, 16, 17)] == [0, 1, 1, 1, 0]


def test_scan_n_entries_reject_before_any_hip_call():
    lib = _lib()
    p = 16   # any non-null value: the checks below reject before a pointer is touched
    B, C, L, R = 2, 40, 192, 3
    # forward: x0 x1 xd0 xd1 dtw dtb A Ds y0 y1, B C L R N, strides, stream
    fwd = lambda ptrs, N=4, R=R, s0=0, s1=0: lib.bem_ss2d_scan_n_f32(*ptrs, B, C, L, R, N, s0, s1, None)
    assert fwd([None] + [p] * 9) == 1 and b"null" in lib.bem_last_error()
    assert fwd([p] * 9 + [None]) == 1 and b"null" in lib.bem_last_error()
    for N in (0, 17):
        assert fwd([p] * 10, N=N) == 1 and b"d_state" in lib.bem_last_error()
    assert fwd([p] * 10, R=17) == 1 and b"dt_rank" in lib.bem_last_error()
    assert fwd([p] * 10, s0=2 * (R + 8) * L - 4) == 1 and b"strides" in lib.bem_last_error()
    assert fwd([p] * 10, s1=2 * (R + 8) * L + 2) == 1 and b"strides" in lib.bem_last_error()
    # backward: 18 tensors + ws, ws_elems, B C L R N, strides, stream
    nws = lib.bem_ss2d_scan_n_bwd_ws_elems(B, C, L, 4)
    assert nws == 2 * B * C * 1 * 4 and lib.bem_ss2d_scan_n_bwd_ws_elems(B, C, L, 17) == 0
    bwd = lambda ptrs, N=4, ws=nws, s0=0, s1=0: lib.bem_ss2d_scan_n_bwd_f32(*ptrs, ws, B, C, L, R, N, s0, s1, None)
    assert bwd([p] * 18 + [None]) == 1 and b"null" in lib.bem_last_error()
    assert bwd([p] * 5 + [None] + [p] * 13) == 1 and b"null" in lib.bem_last_error()
    for N in (0, 17):
        assert bwd([p] * 19, N=N) == 1 and b"d_state" in lib.bem_last_error()
    assert bwd([p] * 19, s0=4) == 1 and b"strides" in lib.bem_last_error()
    assert bwd([p] * 19, ws=nws - 1) == 1 and b"workspace" in lib.bem_last_error()


def test_scan_n_entries_in_header_and_signature_table():
    from bem import native
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "bem_hip.h")).read()
    for name in ("bem_ss2d_scan_n_supported", "bem_ss2d_scan_n_f32", "bem_ss2d_scan_n_bwd_ws_elems", "bem_ss2d_scan_n_bwd_f32"):
        assert name + "(" in hdr and name in native.SIGNATURES
