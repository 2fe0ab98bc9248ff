"""The eval kernels on tensors that cross 2^29, 2^30, 2^31 and 2^32 elements: the four places where a signed or unsigned 32-bit byte
offset or element index breaks.  tests/large_rows.py describes the method: rows are small planes and the row count makes the tensor large,
the rows are filled periodically (period P = 5) except the marker rows at the boundaries, every row of the output is compared with the base
row of its residue class on the device, and only the P base rows and the ~14 marker rows are compared with a reference: torch in float64
on the CPU, with the tolerance of the op's own float64 test (tests/test_ops_gpu.py, test_tile_kernels_edges_gpu.py, test_upfuse_gpu.py,
test_selection_gpu.py), and the op called on that row alone.  Outputs are allocated inside canary margins.

Each case chooses the shape that selects the kernel form, as tests/test_ops_gpu.py does; nothing is forced by a switch.  The second
tier runs the tile kernels with 32-bit lane offsets on one huge image, at the last plane set below 2^30 elements and the first above.

Every op has a case at the 2^32 tier: its largest row-scaled tensor crosses 2^32 elements.  bilinear_up and cond_dwt have no second case in
which their small input crosses it: the output would be 16 and 171 times 16 GiB.  Where an op reads two tensors of the largest size and writes
one or two (gdmlp_x6 with pre, the scans) one tensor is passed for both inputs there, to stay within 64 GiB; a second case at the 2^31 tier
(crossing 2^29, 2^30 and 2^31) has two different ones.  A whole VSSBlock runs on the first wide plane set.  Measured on the MI355X: the
whole module takes about 70 s, the slowest case 6.7 s (most of it the float64 reference on the CPU), most cases under 0.5 s; nothing skips."""
import time

import pytest
import torch
import torch.nn.functional as F

import large_rows as LR
from test_tile_kernels_edges_gpu import _gd_case, _gd_ref64, ln64

pytestmark = pytest.mark.gpu
NOLIMIT = 1 << 31


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bem import ops as o
    return o


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """A kernel fault leaves the device unusable for the process: nothing more is started on it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error after this test, nothing more is run on it: {e}", returncode=3)


def dev(t):
    return None if t is None else t.cuda().contiguous()


def d64(t):
    return None if t is None else t.detach().cpu().double()


def close(a, b, rtol, atol, what):
    a, b = d64(a), d64(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a - b).abs().max().item()
    print(f"{what}: max abs err {err:.3e} (ref max {b.abs().max():.3e})")
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{what}: max abs err {err:.3e} (ref max {b.abs().max():.3e})"


def unit(gen, n, shape):
    return torch.rand(n, *shape, generator=gen)


def dyadic(gen, n, shape):
    """multiples of 1/8 in [-4, 4]: sums, halves and products of a few of them are exact in float32, so an op that only adds and multiplies
    must meet the float64 reference to the bit, whatever the order of its operations"""
    return torch.randint(-32, 33, (n, *shape), generator=gen).float() / 8


def wide_unit(gen, n, shape):
    """images with values on both sides of the clamp to [0, 1]"""
    return torch.rand(n, *shape, generator=gen) * 1.4 - 0.2


class Case:
    """One op at one shape.  ins: name -> row shape, or (row shape, fresh) -- the tensors with one row per batch row (a 'row' may be a group
    of rows where the op ties rows together: run and ref flatten it themselves).  params(gen): the shared small tensors (CPU).  run(ops, ins on
    the device, params on the device) -> tuple of outputs, each with the rows of the inputs.  ref(ins in float64 on the CPU, params on the CPU)
    -> the same in float64.  tol: (rtol, atol) of the op's float64 test; or, with ref None, a function of (what, outputs, ins as float32 on the CPU,
    params) that applies the criterion of the op's own test (selection_ref, mc_stream_ref, niqe_ref, uiqm_ref, dstate_ref ...).  exact: the periodic
    comparison and the call on one row alone are bit for bit.  limit: rows per call.  cross: the tensor (input name or 'out0', ...) that must
    cross the target; default the largest.  ptol: the periodic comparison's (rtol, atol) where it is not exact and differs from tol.  scratch:
    elements per row the op allocates besides its results (state planes), for need_bytes."""

    def __init__(self, name, ins, params, run, ref, tol, exact=True, alone=True, limit=LR.ROW_LIMIT, target=1 << 32, cross=None, ptol=None, scratch=0):
        self.name, self.params, self.run, self.ref, self.tol, self.exact, self.alone, self.ptol = name, params, run, ref, tol, exact, alone, ptol
        self.ins = {k: (v if isinstance(v[0], tuple) else (v, LR.fresh_normal)) for k, v in ins.items()}
        self.limit, self.target, self.cross, self.scratch = limit, target, cross, scratch


CASES = []


def case(*a, **kw):
    CASES.append(Case(*a, **kw))


def none(gen):
    return {}


# ------------------------------------------------------------------------------------------------ layout and channel helpers
def _dst_then(fn, shape_of, fill=-1.0):
    """ops that write into a tensor of the caller: allocated here (inside the canary margins), filled, then handed to the op"""
    def run(ops, i, p):
        dst = torch.empty(*shape_of(i), device="cuda", dtype=torch.float32)
        dst.fill_(fill)
        fn(ops, i, dst)
        return (dst,)
    return run


def _ref_copy(i, p):
    d = torch.full((i["src"].shape[0], 10, 96, 96), -1.0, dtype=torch.float64)
    d[:, 2:8] = i["src"]
    return (d,)


case("copy_channels", {"src": (6, 96, 96)}, none, _dst_then(lambda ops, i, d: ops.copy_channels(i["src"], d, 2), lambda i: (i["src"].shape[0], 10, 96, 96)),
     _ref_copy, (0, 0), limit=NOLIMIT)


def _ref_copy_slice(i, p):
    d = torch.full((i["src"].shape[0], 10, 96, 96), -1.0, dtype=torch.float64)
    d[:, 1:4] = i["src"][:, 2:5]
    return (d,)


case("copy_channels-src_slice", {"src": (6, 96, 96)}, none,
     _dst_then(lambda ops, i, d: ops.copy_channels(i["src"], d, 1, src_c0=2, C=3), lambda i: (i["src"].shape[0], 10, 96, 96)), _ref_copy_slice, (0, 0), limit=NOLIMIT)


def _run_copy_rep(ops, i, p):
    n = i["src"].shape[0]
    dst = torch.empty(3 * n, 6, 72, 96, device="cuda", dtype=torch.float32)
    dst.fill_(-1.0)
    ops.copy_channels_rep(i["src"], dst, 1, 3)
    return (dst.view(n, 3, 6, 72, 96),)


def _ref_copy_rep(i, p):
    d = torch.full((i["src"].shape[0], 3, 6, 72, 96), -1.0, dtype=torch.float64)
    d[:, :, 1:5] = i["src"][:, None]
    return (d,)


case("copy_channels_rep", {"src": (4, 72, 96)}, none, _run_copy_rep, _ref_copy_rep, (0, 0), limit=NOLIMIT)


def _run_add_channels(ops, i, p):
    dst = torch.empty_like(i["dst0"])
    dst.copy_(i["dst0"])
    ops.add_channels(i["src"], dst, 2, src_c0=1, C=3)
    return (dst,)


def _ref_add_channels(i, p):
    d = i["dst0"].clone()
    d[:, 2:5] += i["src"][:, 1:4]
    return (d,)


case("add_channels", {"src": ((5, 96, 96), dyadic), "dst0": ((8, 96, 96), dyadic)}, none, _run_add_channels, _ref_add_channels, (0, 0), limit=NOLIMIT)
case("add", {"a": ((10, 96, 96), dyadic), "b": ((10, 96, 96), dyadic)}, none, lambda ops, i, p: (ops.add(i["a"], i["b"], 0.5),), lambda i, p: (i["a"] + 0.5 * i["b"],),
     (0, 0), limit=NOLIMIT)


def _ref_s2d(i, p):
    x = i["x"]
    return (torch.cat([x[:, :, 0::2, 0::2], x[:, :, 1::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 1::2]], 1),)


case("space_to_depth", {"x": (10, 96, 96)}, none, lambda ops, i, p: (ops.space_to_depth(i["x"]),), _ref_s2d, (0, 0), limit=NOLIMIT)
case("pixel_shuffle2", {"x": (40, 48, 48)}, none, lambda ops, i, p: (ops.pixel_shuffle2(i["x"]),), lambda i, p: (F.pixel_shuffle(i["x"], 2),), (0, 0), limit=NOLIMIT)
case("bilinear_up", {"src": (3, 24, 24)}, none, lambda ops, i, p: (ops.bilinear_up(i["src"], 4),),
     lambda i, p: (F.interpolate(i["src"], scale_factor=4, mode="bilinear", align_corners=False),), (1e-5, 1e-6), limit=NOLIMIT)
# 1 677 840 planes: 26 launches of transpose_planes' split at 65535 planes
case("transpose_planes", {"x": (40, 64, 40)}, none, lambda ops, i, p: (ops.transpose_planes(i["x"]),), lambda i, p: (i["x"].transpose(2, 3),), (0, 0), limit=NOLIMIT)
# the x_dbl planes of the column-major scan directions, as SS2D.forward_fused takes them: 14 planes of each of 33 290 rows, more than one launch holds
case("transpose_plane_slice", {"x": (28, 64, 72)}, none, lambda ops, i, p: (ops.transpose_plane_slice(i["x"], 14, 14),),
     lambda i, p: (i["x"][:, 14:].transpose(2, 3),), (0, 0), limit=NOLIMIT)


def _ref_tinto(i, p):
    d = torch.full((i["src"].shape[0], 20, 72, 64), -1.0, dtype=torch.float64)
    d[:, 3:17] = i["src"].transpose(2, 3)
    return (d,)


case("transpose_planes_into", {"src": (14, 64, 72)}, none,
     _dst_then(lambda ops, i, d: ops.transpose_planes_into(i["src"], d, 3), lambda i: (i["src"].shape[0], 20, 72, 64)), _ref_tinto, (0, 0), limit=NOLIMIT)


# ------------------------------------------------------------------------------------------------ quaternion / Haar
# references: oracle.bem_oracle on the float32 values, at the bounds of tests/test_ops_gpu.py (test_haar_quaternion_golden,
# test_quat_dwt_and_iwt_hamilton); cond_dwt: the chain quat_dwt(bilinear_up()) bit for bit, as tests/test_stage2_entry.py holds it
def _oracle(fn, rtol, atol):
    def verify(what, got, i, p):
        from oracle import bem_oracle as O
        close(got[0], fn(O, i), rtol, atol, what + " vs the oracle")
    return verify


def _cond_dwt_verify(what, got, i, p):
    from bem import ops
    want = ops.quat_dwt(ops.bilinear_up(i["c"].cuda(), 8))
    assert torch.equal(got[0], want), f"{what}: differs from quat_dwt(bilinear_up()) by {float((got[0] - want).abs().max()):.3e}"


case("quat_dwt", {"x": ((5, 96, 96), unit)}, none, lambda ops, i, p: (ops.quat_dwt(i["x"], 1),), None,
     _oracle(lambda O, i: O.dwt_ref(O.quaternion_stack_ref(i["x"][:, 1:4])), 0, 1e-6))
case("cond_dwt", {"c": ((3, 6, 6), lambda g, n, s: torch.rand(n, *s, generator=g) * 1.2 - 0.1)}, none, lambda ops, i, p: (ops.cond_dwt(i["c"], 8),), None,
     _cond_dwt_verify, limit=NOLIMIT)
case("dwt", {"x": ((10, 96, 96), dyadic)}, none, lambda ops, i, p: (ops.dwt(i["x"]),), None, _oracle(lambda O, i: O.dwt_ref(i["x"]), 0, 1e-6), limit=NOLIMIT)
case("iwt", {"x": ((40, 48, 48), dyadic)}, none, lambda ops, i, p: (ops.iwt(i["x"]),), None, _oracle(lambda O, i: O.iwt_ref(i["x"]), 0, 1e-6), limit=NOLIMIT)
case("iwt_hamilton", {"a": ((16, 72, 72), dyadic), "b": ((16, 72, 72), dyadic)}, none, lambda ops, i, p: (ops.iwt_hamilton(i["a"], i["b"]),), None,
     _oracle(lambda O, i: O.hamilton_ref(O.iwt_ref(i["a"]), O.iwt_ref(i["b"]))[:, 1:], 1e-6, 1e-6), limit=NOLIMIT)
case("hamilton", {"q": ((8, 96, 96), dyadic)}, none, lambda ops, i, p: (ops.hamilton(i["q"]),), None,
     _oracle(lambda O, i: O.hamilton_ref(i["q"][:, :4], i["q"][:, 4:])[:, 1:], 0, 1e-6), limit=NOLIMIT)


# ------------------------------------------------------------------------------------------------ dense convolutions
def _conv_params(Cout, Cin, K, scale=None):
    def params(gen):
        return {"w": torch.randn(Cout, Cin, K, K, generator=gen) * (scale or (Cin * K * K) ** -0.5), "b": 0.3 * torch.randn(Cout, generator=gen)}
    return params


CONV_TOL = (1e-4, 2e-5)
# 3x3 row form (W a power of two), relu + res2
case("conv2d-3x3-rows-relu-res2", {"x": (8, 32, 64), "r2": (40, 32, 64)}, _conv_params(40, 8, 3),
     lambda ops, i, p: (ops.conv2d(i["x"], p["w"], p["b"], relu=True, res2=i["r2"]),),
     lambda i, p: (F.relu(F.conv2d(i["x"], p["w"].double(), p["b"].double(), padding=1)) + i["r2"],), CONV_TOL)
# 3x3 tap form (even W, no power of two), res1 shared by three rows: a row here is a group of three samples of one image
case("conv2d-3x3-taps-res1_rep3", {"x": (3, 8, 36, 48), "r1": (1, 40, 36, 48)}, _conv_params(40, 8, 3),
     lambda ops, i, p: (ops.conv2d(i["x"].flatten(0, 1), p["w"], p["b"], res1=i["r1"].flatten(0, 1), res1_rep=3).unflatten(0, (-1, 3)),),
     lambda i, p: (F.conv2d(i["x"].flatten(0, 1), p["w"].double(), p["b"].double(), padding=1).unflatten(0, (-1, 3)) + i["r1"],), CONV_TOL,
     limit=LR.ROW_LIMIT // 3)
# f32-MFMA form (odd W) on a channel slice: x_bstride = 12 H W, Cin = 8
case("conv2d-3x3-mfma-cin_slice", {"x": (12, 36, 47)}, _conv_params(40, 8, 3),
     lambda ops, i, p: (ops.conv2d(i["x"], p["w"], p["b"], cin_slice=(3, 8)),),
     lambda i, p: (F.conv2d(i["x"][:, 3:11], p["w"].double(), p["b"].double(), padding=1),), CONV_TOL)
# 4x4 stride 2: coalesced-row form (Wo = 32) and f32-MFMA form (Wo = 24); the input is the larger tensor
case("conv2d-4x4s2-rows", {"x": (24, 48, 64)}, _conv_params(48, 24, 4), lambda ops, i, p: (ops.conv2d(i["x"], p["w"], p["b"], stride=2),),
     lambda i, p: (F.conv2d(i["x"], p["w"].double(), p["b"].double(), stride=2, padding=1),), CONV_TOL)
case("conv2d-4x4s2-mfma", {"x": (24, 64, 48)}, _conv_params(48, 24, 4), lambda ops, i, p: (ops.conv2d(i["x"], p["w"], p["b"], stride=2),),
     lambda i, p: (F.conv2d(i["x"], p["w"].double(), p["b"].double(), stride=2, padding=1),), CONV_TOL)
# the direct kernel: more than 160 output channels at an odd width
case("conv2d-3x3-direct", {"x": (3, 20, 21)}, _conv_params(168, 3, 3), lambda ops, i, p: (ops.conv2d(i["x"], p["w"], p["b"]),),
     lambda i, p: (F.conv2d(i["x"], p["w"].double(), p["b"].double(), padding=1),), CONV_TOL)


# ------------------------------------------------------------------------------------------------ pointwise GEMM and depthwise
def _pw_params(M, K, ln=False, prelu=False):
    def params(gen):
        p = {"w": torch.randn(M, K, generator=gen) * K ** -0.5, "b": 0.3 * torch.randn(M, generator=gen)}
        if ln:
            p["lw"], p["lb"] = 1 + 0.2 * torch.randn(K, generator=gen), 0.1 * torch.randn(K, generator=gen)
        if prelu:
            p["a"] = torch.tensor([0.2])
        return p
    return params


def _pw64(x, p, ln=False, prelu=False):
    if ln:
        x = ln64(x, p["lw"], p["lb"], 1e-5)
    y = F.conv2d(x, p["w"].double()[:, :, None, None], p["b"].double())
    return torch.where(y >= 0, y, p["a"].double() * y) if prelu else y


PW_TOL, PWLN_TOL = (1e-4, 2e-5), (1e-4, 3e-5)
case("pw_gemm-plain", {"x": (40, 64, 64)}, _pw_params(40, 40), lambda ops, i, p: (ops.pw_gemm(i["x"], ops.pack_pw_weight(p["w"]), 40, bias=p["b"]),),
     lambda i, p: (_pw64(i["x"], p),), PW_TOL)
case("pw_gemm-ln-k40", {"x": (40, 64, 64)}, _pw_params(40, 40, ln=True),
     lambda ops, i, p: (ops.pw_gemm(i["x"], ops.pack_pw_weight(p["w"]), 40, ln=(p["lw"], p["lb"]), bias=p["b"]),), lambda i, p: (_pw64(i["x"], p, ln=True),), PWLN_TOL)
# K = 160 -> M = 320 with many pixel waves: an M-tile's weights through LDS (pw_x6_res_lds_kernel); one row alone takes the per-wave form
case("pw_gemm-ln-k160", {"x": (160, 16, 16)}, _pw_params(320, 160, ln=True),
     lambda ops, i, p: (ops.pw_gemm(i["x"], ops.pack_pw_weight(p["w"]), 320, ln=(p["lw"], p["lb"]), bias=p["b"]),), lambda i, p: (_pw64(i["x"], p, ln=True),), PWLN_TOL,
     alone=False)
case("pw_gemm-sum-ln-res", {"x1": (40, 64, 64), "x2": (40, 64, 64)}, _pw_params(40, 40, ln=True),
     lambda ops, i, p: (ops.pw_gemm(i["x1"], ops.pack_pw_weight(p["w"]), 40, x2=i["x2"], in_mode=1, ln=(p["lw"], p["lb"]), bias=p["b"], res=i["x1"]),),
     lambda i, p: (_pw64(i["x1"] + i["x2"], p, ln=True) + i["x1"],), PWLN_TOL)
case("pw_gemm-cat-prelu", {"x1": (24, 64, 64), "x2": (16, 64, 64)}, _pw_params(40, 40, prelu=True),
     lambda ops, i, p: (ops.pw_gemm(i["x1"], ops.pack_pw_weight(p["w"]), 40, x2=i["x2"], in_mode=2, bias=p["b"], prelu=p["a"]),),
     lambda i, p: (_pw64(torch.cat([i["x1"], i["x2"]], 1), p, prelu=True),), PW_TOL)


def _ref_convT(i, p):
    x, Co = i["x"], 20
    y = _pw64(x, p)                                                               # row = q * Co + co, q = 2 dy + dx
    return (F.pixel_shuffle(y.unflatten(1, (4, Co)).transpose(1, 2).flatten(1, 2), 2),)


case("pw_gemm-convT", {"x": (40, 32, 32)}, _pw_params(80, 40),
     lambda ops, i, p: (ops.pw_gemm(i["x"], ops.pack_pw_weight(p["w"]), 80, bias=p["b"], convT_Win=32),), _ref_convT, PW_TOL)
# the Bayesian per-sample weights: one weight set and one bias per batch row, so the weight tensor is indexed by the row as well
case("pw_gemm-per_row_weights", {"x": (40, 64, 64), "w": ((40, 40), lambda g, n, s: torch.randn(n, *s, generator=g) * 40 ** -0.5),
                                 "b": ((40,), lambda g, n, s: 0.3 * torch.randn(n, *s, generator=g))}, none,
     lambda ops, i, p: (ops.pw_gemm(i["x"], ops.pack_pw_weight(i["w"]), 40, bias=i["b"]),),
     lambda i, p: (torch.einsum("bmk,bkhw->bmhw", i["w"], i["x"]) + i["b"][:, :, None, None],), PW_TOL)


def _dw_params(C):
    def params(gen):
        return {"w": torch.randn(C, 1, 3, 3, generator=gen) / 3, "b": 0.2 * torch.randn(C, generator=gen)}
    return params


def _dw64(x, p):
    return F.conv2d(x, p["w"].double(), p["b"].double(), padding=1, groups=x.shape[1])


DW_TOL = (1e-5, 1e-5)
case("dwconv3x3-silu", {"x": (40, 64, 64)}, _dw_params(40), lambda ops, i, p: (ops.dwconv3x3(i["x"], p["w"], p["b"], 1),), lambda i, p: (F.silu(_dw64(i["x"], p)),), DW_TOL)
case("dwconv3x3-gate", {"x": (80, 64, 64)}, _dw_params(80), lambda ops, i, p: (ops.dwconv3x3(i["x"], p["w"], p["b"], 2),),
     lambda i, p: ((lambda h: F.gelu(h[:, :40]) * h[:, 40:])(_dw64(i["x"], p)),), DW_TOL)
# a width that is no multiple of 4: the general kernel
case("dwconv3x3-silu-ragged", {"x": (40, 62, 62)}, _dw_params(40), lambda ops, i, p: (ops.dwconv3x3(i["x"], p["w"], p["b"], 1),), lambda i, p: (F.silu(_dw64(i["x"], p)),), DW_TOL)


# ------------------------------------------------------------------------------------------------ fused tile kernels, up-sampling
def _gd_params(C, H, W):
    def params(gen):
        Hd, t = _gd_case((1, C, H, W), True)
        return {k: v for k, v in t.items() if k not in ("x", "y0", "y1")} | {"Hd": torch.tensor(Hd)}
    return params


def _gd_run(fused):
    def run(ops, i, p):
        Hd = int(p["Hd"])
        perm = ops.gate_interleave(Hd, "cpu")
        Wg, bg = ops.pack_pw_weight(p["wi"][perm.cuda()].contiguous(), x6=True), p["bi"][perm.cuda()].contiguous()
        pre = (i["y"], i.get("y1", i["y"]), p["onw"], p["onb"], 1e-5, ops.pack_vss_back_outproj(p["wop"]), p["bop"]) if fused else None
        return (ops.gdmlp_x6(i["x"], p["lw"], p["lb"], 1e-6, Wg, bg, ops.dw_gate_params10(p["wd"], p["bd"], Hd), ops.pack_pw_weight(p["wo"], x6=True), p["bo"], Hd, pre=pre),)
    return run


def _gd_ref(fused):
    def ref(i, p):
        t = dict(p, **i)
        if fused:
            t["y0"] = t.pop("y")
            t["y1"] = t.pop("y1", t["y0"])
        return (_gd_ref64(int(p["Hd"]), {k: v.float() for k, v in t.items() if k != "Hd"}, fused).double(),)
    return ref


GD_TOL = (1e-4, 4e-5)
case("gdmlp_x6-c40", {"x": (40, 64, 64)}, _gd_params(40, 64, 64), _gd_run(False), _gd_ref(False), GD_TOL)
case("gdmlp_x6-c24", {"x": (24, 64, 72)}, _gd_params(24, 64, 72), _gd_run(False), _gd_ref(False), GD_TOL)
case("gdmlp_x6-c80", {"x": (80, 32, 40)}, _gd_params(80, 32, 40), _gd_run(False), _gd_ref(False), GD_TOL)
# both scan outputs are one tensor here (the kernel adds them): x, y and out at 2^32 elements are 48 GiB, a fourth would pass the 64 GiB of a test
case("gdmlp_x6-pre-c40", {"x": (40, 64, 64), "y": (40, 64, 64)}, _gd_params(40, 64, 64), _gd_run(True), _gd_ref(True), GD_TOL)
# two different scan outputs, at the 2^31 tier: an exchange or a wrong batch base of one of them shows here
case("gdmlp_x6-pre-c40-y0_y1-2^31", {"x": (40, 64, 64), "y": (40, 64, 64), "y1": (40, 64, 64)}, _gd_params(40, 64, 64), _gd_run(True), _gd_ref(True), GD_TOL,
     target=1 << 31)
case("gdmlp_x6-pre-c24", {"x": (24, 64, 72), "y": (24, 64, 72)}, _gd_params(24, 64, 72), _gd_run(True), _gd_ref(True), GD_TOL)


def _front_params(C, Mx):
    def params(gen):
        return {"lw": 1 + 0.2 * torch.randn(C, generator=gen), "lb": 0.1 * torch.randn(C, generator=gen), "wi": torch.randn(C, C, generator=gen) * C ** -0.5,
                "bi": 0.3 * torch.randn(C, generator=gen), "wd": torch.randn(C, 1, 3, 3, generator=gen) / 3, "bd": 0.2 * torch.randn(C, generator=gen),
                "wx": torch.randn(Mx, C, generator=gen) * C ** -0.5}
    return params


def _front_run(ops, i, p):
    Mx = p["wx"].shape[0]
    return ops.ss2d_front(i["x"], p["lw"], p["lb"], 1e-6, ops.pack_pw_weight(p["wi"], x6=True), p["bi"], p["wd"], p["bd"], ops.pack_pw_weight(p["wx"], x6=True), Mx)


def _front_ref(i, p):
    C = i["x"].shape[1]
    tt = F.conv2d(ln64(i["x"], p["lw"], p["lb"], 1e-6), p["wi"].double()[:, :, None, None], p["bi"].double())
    c64 = F.silu(F.conv2d(tt, p["wd"].double(), p["bd"].double(), padding=1, groups=C))
    return c64, F.conv2d(c64, p["wx"].double()[:, :, None, None])


case("ss2d_front-c40", {"x": (40, 64, 64)}, _front_params(40, 20), _front_run, _front_ref, GD_TOL)


def _upfuse_params(gen):
    import copy
    from test_upfuse_gpu import _level
    up, fuse, _ = _level(80, 80321, False)
    return {"cpu": (up, fuse), "gpu": (copy.deepcopy(up).cuda(), copy.deepcopy(fuse).cuda())}


def _upfuse_run(ops, i, p):
    from bem.modules import fold_up_fuse
    return (ops.up_fuse(i["f"], i["skip"], fold_up_fuse(*p["gpu"])),)


def _upfuse_verify(what, got, i, p):
    """the criterion of tests/test_upfuse_gpu.py: no further from the float64 chain than torch's float32 chain, in mean and in max"""
    import stage2_yardstick as Y
    from test_upfuse_gpu import _chain
    r64, r32 = (_chain(i["f"], i["skip"], *p["cpu"], None, dt) for dt in (torch.float64, torch.float32))
    (rm, rM), (hm, hM) = Y.errors(r32, r64), Y.errors(got[0].cpu(), r64)
    print(f"{what}: f32 chain mean {rm:.3e} max {rM:.3e} | up_fuse mean {hm:.3e} max {hM:.3e}")
    assert hm <= rm and hM <= rM, (what, hm, rm, hM, rM)


case("up_fuse-c80", {"f": (80, 20, 24), "skip": (40, 40, 48)}, _upfuse_params, _upfuse_run, None, _upfuse_verify)


# ------------------------------------------------------------------------------------------------ channel attention helpers
case("chan_scale", {"x": ((10, 96, 96), dyadic), "add": ((10, 96, 96), dyadic), "s": ((10,), dyadic), "bc": ((10,), dyadic)}, none,
     lambda ops, i, p: (ops.chan_scale(i["x"], i["s"], add=i["add"], add_bc=i["bc"], add_bc_scale=0.5),),
     lambda i, p: (i["s"][:, :, None, None] * i["x"] + i["add"] + 0.5 * i["bc"][:, :, None, None],), (0, 0), limit=NOLIMIT)


def _sa_verify(what, got, i, p):
    """tests/attn_blocks_ref.py and the per_pixel criterion of tests/test_attn_blocks_gpu.py"""
    import attn_blocks_ref as R
    import test_attn_blocks_gpu as T
    T.per_pixel(got[0], *T.both(R.spatial_attention, i["x"], p["w"], i["g"]), what)


case("spatial_attention", {"x": (10, 96, 96), "g": ((10,), unit)}, lambda gen: {"w": torch.randn(1, 2, 7, 7, generator=gen) / 7},
     lambda ops, i, p: (ops.spatial_attention(i["x"], p["w"], chan_scale=i["g"]),), None, _sa_verify, limit=NOLIMIT, scratch=2 * 96 * 96)


# ------------------------------------------------------------------------------------------------ selection tail
# references and bounds: tests/selection_ref.py and the per_pixel / rounded_once criteria of tests/test_selection_gpu.py
def _sel():
    import selection_ref as R
    import test_selection_gpu as T
    return R, T


def _postproc_verify(what, got, i, p):
    R, T = _sel()
    T.per_pixel(got[0], *T.both(R.cond_postproc, i["pred"], i["tm"], i["noise"], 1, 0.1, zero_sum="zero"), what)


case("cond_postproc", {"pred": ((3, 160, 168), wide_unit), "noise": (3, 160, 168), "tm": ((3,), lambda g, n, s: 0.3 + 0.4 * torch.rand(n, *s, generator=g))}, none,
     lambda ops, i, p: (ops.cond_postproc(i["pred"], i["tm"], i["noise"], 1, 0.1),), None, _postproc_verify, limit=NOLIMIT)


def _finalize_verify(what, got, i, p):
    R, T = _sel()
    (f32, _, _), (f64, _, p64) = T.both(R.candidate_finalize, i["pred"], i["tg"], 1, 260, 250, True, zero_sum="zero")
    T.per_pixel(got[0], f32, f64, what + " final")
    T.rounded_once(got[1], p64, what + " PSNR", R.MARGIN * R.psnr_f32_term(i["pred"], i["tg"], 1, 260, 250, True))
    T.rounded_once(got[1], R.psnr(i["tg"].double(), got[0].cpu().double()), what + " PSNR of the returned final")


# at most 21845 candidates per call: planes of 264 x 252 cross 2^32 below that; crop to 260 x 250 and GT-mean.  The ratio comes from float64
# atomics of several workgroups: rows with equal inputs agree within the final image's own bound of tests/test_ops_gpu.py, not bit for bit
case("candidate_finalize", {"pred": ((3, 264, 252), wide_unit), "tg": ((3, 260, 250), unit)}, none,
     lambda ops, i, p: ops.candidate_finalize(i["pred"], i["tg"], 1, 260, 250, True), None, _finalize_verify, exact=False, ptol=(1e-5, 1e-6), limit=LR.CANDIDATE_LIMIT)


def _plane_mean_verify(what, got, i, p):
    R, T = _sel()
    T.rounded_once(got[0], R.plane_mean(i["x"].double(), 90, 93), what + " 90 x 93 window")
    T.rounded_once(got[1], R.plane_mean(i["x"].double()), what + " whole planes")


case("plane_mean", {"x": (10, 96, 96)}, none, lambda ops, i, p: (ops.plane_mean(i["x"], 90, 93), ops.plane_mean(i["x"])), None, _plane_mean_verify, limit=NOLIMIT)


def _mc_mean_verify(what, got, i, p):
    R, T = _sel()
    T.per_pixel(got[0], *T.both(R.mc_mean, i["raw"].flatten(0, 1), i["tg"], 3, 76, 90, True), what)


# a row is one image with its N = 3 raw outputs; crop 80 x 96 -> 76 x 90 and GT-mean (float64 atomics: as candidate_finalize)
case("mc_mean", {"raw": ((3, 3, 80, 96), wide_unit), "tg": ((3, 76, 90), unit)}, none,
     lambda ops, i, p: (ops.mc_mean(i["raw"].flatten(0, 1), i["tg"], 3, 76, 90, True),), None, _mc_mean_verify, exact=False, ptol=(2e-6, 2e-6))


def _levels(gen, n, shape):
    """images on the levels k / 255, as selection_ref.ssim_inputs makes them: 255 x is never near a half"""
    return torch.randint(0, 256, (n, *shape), generator=gen).float() / 255.0


def _ssim_verify(what, got, i, p):
    R, T = _sel()
    T.rounded_once(got[0], R.ssim(i["fin"].double(), i["tg"].double(), 1), what)


# one float64 atomic per 16 x 16 tile: rows with equal inputs agree within two float32 ulps of a figure below 1
case("ssim", {"fin": ((3, 160, 168), _levels), "tg": ((3, 160, 168), _levels)}, none, lambda ops, i, p: (ops.ssim(i["fin"], i["tg"], 1),), None, _ssim_verify,
     exact=False, ptol=(0.0, 2.0 ** -23))


def _mc_stream_run(spread):
    """mc_accum in two chunks (2 + 1 samples of every image, each chunk a tensor of its own) + mc_finish: the mean of the raw outputs (crop
    96 x 120 -> 92 x 114), or the std of the candidates"""
    def run(ops, i, p):
        st = ops.McState(i["c01"].shape[0], *((96, 120) if spread else (92, 114)), "cuda", mean=not spread, spread=spread)
        for k, n in (("c01", 2), ("c2", 1)):
            ops.mc_accum(st, **{"final" if spread else "raw": i[k].flatten(0, 1)}, samples_per_image=n)
        mc, sd, sm = ops.mc_finish(st, mean=not spread, spread=spread)
        return (sd, sm) if spread else (mc,)
    return run


def _mc_stream_verify(what, got, i, p):
    """the bounds of tests/test_sample_chunk_gpu.py: the mean has the bits of the numpy restatement; the std map is within 4 x the
    restatement's measured distance from float64, and the mean std is the float64 mean of the returned map"""
    import mc_stream_ref as M
    x = torch.cat([i["c01"], i["c2"]], 1).numpy()
    if len(got) == 1:
        s = M.run(x[..., :92, :114], (2, 1), x)
        assert torch.equal(got[0].cpu(), torch.from_numpy(s.mc())), what + ": the mean differs from the float32 restatement"
    else:
        d = float((got[0].cpu().double() - torch.from_numpy(M.std64(x))).abs().max())
        print(f"{what}: std map vs float64 max|d| {d:.3e} (bound {4 * M.REF_STD_DEV:.1e})")
        assert d <= 4 * M.REF_STD_DEV
        close(got[1], got[0].cpu().double().mean(dim=(1, 2, 3)), 1e-12, 0.0, what + " mean std")


case("mc_accum-raw+mc_finish", {"c01": ((2, 3, 96, 120), wide_unit), "c2": ((1, 3, 96, 120), wide_unit)}, none, _mc_stream_run(False), None, _mc_stream_verify, scratch=3 * 92 * 114)
case("mc_accum-final+mc_finish", {"c01": ((2, 3, 96, 120), unit), "c2": ((1, 3, 96, 120), unit)}, none, _mc_stream_run(True), None, _mc_stream_verify, scratch=2 * 3 * 96 * 120)


# ------------------------------------------------------------------------------------------------ the output head of the two-branch archs
def _head_verify(what, got, i, p):
    """the bound of tests/test_twobranch_gpu.py::test_head_forward_vs_float64"""
    from test_twobranch_gpu import _head64
    ref = _head64(torch.cat([i["big"][:, :3], i["big"][:, 6:]], 1), p["w1"], p["b1"], p["w2"], p["b2"])
    err = float((got[0].cpu().double() - ref).abs().max())
    print(f"{what}: max abs err {err:.3e} (ref max {float(ref.abs().max()):.3e})")
    assert err <= 2e-5 * max(1.0, float(ref.abs().max())), err


def _head_params(gen):
    from test_twobranch_gpu import _weights
    return dict(zip(("w1", "b1", "w2", "b2"), _weights(17)))


# the two branch outputs are channel slices of one (B, 9, H, W) tensor: batch stride 9 H W
case("fusion_head", {"big": (9, 96, 96)}, _head_params,
     lambda ops, i, p: (ops.fusion_head(i["big"][:, :3], i["big"][:, 6:], p["w1"], p["b1"], p["w2"], p["b2"]),), None, _head_verify, limit=NOLIMIT)


# ------------------------------------------------------------------------------------------------ scans
# the operating point of tests/test_ops_gpu.py::test_ss2d_scan_long_planes_vs_float64 (dt from 0.05 to ~1, Ds ~ 0.1 N(0,1): the state term is
# as large as D u), its float64 closed form and its bound.  Both orientations read one activation tensor here: x, y0 and y1 at 2^32
# elements and the x_dbl rows are 58 GiB, a second activation tensor would pass the 64 GiB of a test.
def _scan_params(C, R):
    def params(gen):
        return {"dtw": torch.randn(4, C, R, generator=gen) * (0.3 / R ** 0.5), "dtb": torch.log(torch.expm1(0.05 + 0.95 * torch.rand(4, C, generator=gen))),
                "A": -torch.exp(0.5 * torch.randn(4 * C, generator=gen)), "Ds": 0.1 * torch.randn(4 * C, generator=gen)}
    return params


def _silu_normal(gen, n, shape):
    return F.silu(torch.randn(n, *shape, generator=gen))


def _xd(t, rows):
    """rows [1, 1 + 2 rows) of a wider (B, *, L) buffer as the (B, 2, rows, L) x_dbl operand: only the batch stride differs from a contiguous one"""
    return t[:, 1:1 + 2 * rows].unflatten(1, (2, rows))


def _scan_verify(rm):
    def verify(what, got, i, p):
        from test_ops_gpu import _ss2d_fused64
        x = i["x"].double()
        n, C = x.shape[:2]
        R = p["dtw"].shape[2]
        x0 = x.reshape(n, C, -1)
        x1 = x.transpose(2, 3).reshape(n, C, -1) if rm else i.get("x1", i["x"]).double()
        pairs = _ss2d_fused64(x0, x1, _xd(i["w0"], R + 2).double(), _xd(i["w1"], R + 2).double(), *(p[k].double() for k in ("dtw", "dtb", "A", "Ds")))
        for o, (h, (c, u)) in enumerate(zip(got, pairs)):
            h = h.cpu().double()
            if rm and o == 1:
                h = h.transpose(2, 3)                                   # y1 comes back row-major
            e = (h.reshape(n, C, -1) - u - c).abs().max().item()
            ymax, cmax = (c + u).abs().max().item(), c.abs().max().item()
            print(f"{what} orientation {o}: max|y| {ymax:.3f} max|C*h| {cmax:.3f} | max err {e:.2e} = {e / ymax:.1e} max|y| = {e / cmax:.1e} max|C*h|")
            assert e <= 2e-5 * ymax and e <= 2e-5 * cmax, (o, e, ymax, cmax)
    return verify


case("ss2d_scan-strided_xd", {"x": ((40, 4096), _silu_normal), "w0": (13, 4096), "w1": (13, 4096)}, _scan_params(40, 3),
     lambda ops, i, p: ops.ss2d_scan(i["x"], i["x"], _xd(i["w0"], 5), _xd(i["w1"], 5), p["dtw"], p["dtb"], p["A"], p["Ds"]), None, _scan_verify(False),
     limit=NOLIMIT)
# two different activation tensors for the two orientations, at the 2^31 tier
case("ss2d_scan-x0_x1-2^31", {"x": ((40, 4096), _silu_normal), "x1": ((40, 4096), _silu_normal), "w0": (13, 4096), "w1": (13, 4096)}, _scan_params(40, 3),
     lambda ops, i, p: ops.ss2d_scan(i["x"], i["x1"], _xd(i["w0"], 5), _xd(i["w1"], 5), p["dtw"], p["dtb"], p["A"], p["Ds"]), None, _scan_verify(False),
     limit=NOLIMIT, target=1 << 31)
# the row-major form exists for the planes of a 256 x 256 image: 16 x 64 with dt_rank 10 is its level-2 plane
case("ss2d_scan_rm", {"x": ((80, 16, 64), _silu_normal), "w0": (26, 1024), "w1": (26, 1024)}, _scan_params(80, 10),
     lambda ops, i, p: ops.ss2d_scan_rm(i["x"], _xd(i["w0"], 12), _xd(i["w1"], 12), p["dtw"], p["dtb"], p["A"], p["Ds"]), None, _scan_verify(True),
     limit=NOLIMIT)


def _scan_n_params(gen):
    import dstate_ref as D
    _, _, dtw, dtb, A_logs, Ds = D.make_operands(1, 80, 2, 2, 4, seed=1004)
    return {"dtw": dtw, "dtb": dtb, "A_logs": A_logs, "A": -torch.exp(A_logs), "Ds": Ds}


def _scan_n_verify(what, got, i, p):
    """the bound of tests/test_dstate_gpu.py::test_scan_n_kernel_vs_oracle_and_float64: within 2 x the float32 restatement's own error"""
    import dstate_ref as D
    args = (i["x"], i.get("x1", i["x"]), _xd(i["w0"], 13), _xd(i["w1"], 13), p["dtw"], p["dtb"], p["A_logs"], p["Ds"])
    refs, f32s = D.ss2d_scan_n_ref(*args), D.ss2d_scan_n_ref(*args, dtype=torch.float32)
    scale = float(torch.cat(refs).abs().max())
    for o, (h, f32, ref) in enumerate(zip(got, f32s, refs)):
        e_hip, e_f32 = (h.cpu().double() - ref).abs(), (f32.double() - ref).abs()
        print(f"{what} y{o}: HIP max {float(e_hip.max()):.2e} mean {float(e_hip.mean()):.2e} | f32 max {float(e_f32.max()):.2e} mean {float(e_f32.mean()):.2e}")
        assert float(e_hip.max()) <= 2 * float(e_f32.max()) + 1e-6 * scale, (o, float(e_hip.max()), float(e_f32.max()), scale)
        assert float(e_hip.mean()) <= 2 * float(e_f32.mean()) + 1e-7 * scale, (o, float(e_hip.mean()), float(e_f32.mean()))


# d_state 4 at C = 80: dt_rank 5, 13 x_dbl rows per direction
case("ss2d_scan_n-d_state4", {"x": (80, 1024), "w0": (28, 1024), "w1": (28, 1024)}, _scan_n_params,
     lambda ops, i, p: ops.ss2d_scan_n(i["x"], i["x"], _xd(i["w0"], 13), _xd(i["w1"], 13), p["dtw"], p["dtb"], p["A"], p["Ds"]), None, _scan_n_verify, limit=NOLIMIT)


case("ss2d_scan_n-d_state4-x0_x1-2^31", {"x": (80, 1024), "x1": (80, 1024), "w0": (28, 1024), "w1": (28, 1024)}, _scan_n_params,
     lambda ops, i, p: ops.ss2d_scan_n(i["x"], i["x1"], _xd(i["w0"], 13), _xd(i["w1"], 13), p["dtw"], p["dtb"], p["A"], p["Ds"]), None, _scan_n_verify,
     limit=NOLIMIT, target=1 << 31)


# ------------------------------------------------------------------------------------------------ no-reference scorers
# at the 2^32 tier like the rest; inputs and bounds of the random-image part of test_niqe_gpu.py / test_uiqm_gpu.py
# (test_*_bit_reproducible_and_batch_independent).  Their byte workspaces (scratch, in float32 elements per row) are the library's figures.
def _niqe_params(gen):
    import numpy as np
    from bem.scorers import NiqeParams
    from test_niqe_gpu import NPZ
    return {"niqe": NiqeParams.load(NPZ), "g13": np.load(NPZ)}


def _niqe_verify(what, got, i, p):
    import numpy as np
    import niqe_ref as R
    ref = [R.niqe(i["fin"][k].numpy(), p["g13"]) for k in range(i["fin"].shape[0])]
    print(f"{what}: max relative difference {float(np.max(np.abs(got[0].cpu().numpy() / np.array(ref) - 1))):.2e}")
    np.testing.assert_allclose(got[0].cpu().numpy(), ref, rtol=1e-4)


case("niqe", {"fin": ((3, 192, 192), unit)}, _niqe_params, lambda ops, i, p: (ops.niqe(i["fin"], p["niqe"]),), None, _niqe_verify, scratch=130000)


def _uiqm_verify(what, got, i, p):
    import uiqm_ref as R
    for k in range(i["fin"].shape[0]):
        ref = R.scores(i["fin"][k].permute(1, 2, 0).numpy())
        u1, u2 = got[0][k].item(), got[1][k].item()
        assert abs(u1 - ref["uiqm"]) <= 1e-6 * abs(ref["uiqm"]) and abs(u2 - ref["uciqe"]) <= 1e-9 * ref["uciqe"], (what, k, u1, ref["uiqm"], u2, ref["uciqe"])


case("uiqm_uciqe", {"fin": ((3, 150, 220), unit)}, none, lambda ops, i, p: ops.uiqm_uciqe(i["fin"]), None, _uiqm_verify, scratch=120000)


# ------------------------------------------------------------------------------------------------ the runner
def _run_case(ops, monkeypatch, c):
    t0 = time.perf_counter()
    gen = torch.Generator().manual_seed(sum(map(ord, c.name)))
    params = c.params(gen)
    pdev = {k: (dev(v) if torch.is_tensor(v) else v) for k, v in params.items()}
    base = {k: fresh(gen, LR.P, shape) for k, (shape, fresh) in c.ins.items()}
    small = c.run(ops, {k: dev(v) for k, v in base.items()}, pdev)
    rows_of = {k: int(torch.tensor(shape).prod()) for k, (shape, _) in c.ins.items()}
    rows_of.update({f"out{j}": o[0].numel() for j, o in enumerate(small)})
    del small
    cross = c.cross or max(rows_of, key=rows_of.get)
    B = LR.rows_for(rows_of[cross], c.target, c.limit)
    markers = sorted(set().union(*(LR.boundary_rows(R, B) for R in rows_of.values())))
    # Measured on the MI355X (torch.cuda.max_memory_allocated, printed on the LARGE line of every case): the peak is 1.6 to 1.9 GiB under this
    # figure for every case but three -- candidate_finalize 50.4 against 49.3 GiB and mc_mean 28.6 / 27.5 (float64 workspaces and the row
    # gathers of the checks), niqe 32.2 / 36.8 (workspace counted high).  Largest: the scans, 59.6 GiB.
    need = LR.need_bytes(*(B * R for R in rows_of.values()), B * c.scratch)
    LR.require_memory(need)
    torch.cuda.reset_peak_memory_stats()
    big = {k: LR.periodic_fill(torch.empty(B, *shape, device="cuda", dtype=torch.float32), base[k], markers, gen, fresh) for k, (shape, fresh) in c.ins.items()}
    outs = []
    try:
        _check_case(ops, monkeypatch, c, big, outs, pdev, params, markers, B)
        peak = torch.cuda.max_memory_allocated()
    finally:                                   # a failed check keeps this frame alive in its traceback, not what the containers held
        big.clear()
        outs.clear()
        if c.scratch:
            ops._SCRATCH.clear()               # a workspace sized for 2^32 elements is not kept for the tests that follow
        torch.cuda.empty_cache()
    print(f"LARGE {c.name}: B = {B} rows, {cross} = {B * rows_of[cross]} elements, {len(markers)} markers, need_bytes {need / 2**30:.1f} GiB, "
          f"measured peak {peak / 2**30:.1f} GiB, {time.perf_counter() - t0:.2f} s")


def _check_case(ops, monkeypatch, c, big, outs, pdev, params, markers, B):
    with LR.canaries(monkeypatch, outs):
        outs.extend(c.run(ops, big, pdev))
    tol = c.tol if isinstance(c.tol, tuple) else None
    ptol = (0.0, 0.0) if c.exact else (c.ptol or tol)
    for j, o in enumerate(outs):
        assert o.shape[0] == B, (c.name, j, tuple(o.shape))
        refs = LR.check_periodic(o, LR.P, markers, exact=c.exact, rtol=ptol[0], atol=ptol[1])
    rows = sorted(set(refs) | set(markers))
    sub = {k: torch.stack([v[r] for r in rows]) for k, v in big.items()}
    got = [torch.stack([o[r] for r in rows]) for o in outs]
    what = f"{c.name}: {len(rows)} base and marker rows of {B}"
    if tol is None:
        c.tol(what, got, {k: v.cpu() for k, v in sub.items()}, params)
    else:
        for j, (g, r) in enumerate(zip(got, c.ref({k: d64(v) for k, v in sub.items()}, params))):
            close(g, r, *tol, f"{what} vs float64, out{j}")
    if c.alone:
        for n, r in enumerate(rows):
            for j, o in enumerate(c.run(ops, {k: v[n:n + 1] for k, v in sub.items()}, pdev)):
                if c.exact:
                    assert torch.equal(o[0], got[j][n]), f"{c.name} out{j}: row {r} of {B} differs from the op called on that row alone"
                else:
                    assert torch.allclose(o[0], got[j][n], rtol=ptol[0], atol=ptol[1]), f"{c.name} out{j}: row {r} of {B} vs the op called on that row alone"


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_many_rows(ops, monkeypatch, c):
    _run_case(ops, monkeypatch, c)


def test_select_gathers_inside_one_images_candidates(ops, monkeypatch):
    """select_best, select_scores and select_merge with the candidate gather, where cand crosses 2^29 .. 2^32 elements inside the N
    candidates of the second of two images (the keep='all' tensor).  Every candidate is different, so a row from a wrapped address shows; for
    each boundary the scores choose the candidate that contains it, and the row in front of it for the other image."""
    t0 = time.perf_counter()
    chw = 3 * 64 * 80
    N = LR.rows_for(chw, limit=NOLIMIT) // 2 + 1
    LR.require_memory(LR.need_bytes(2 * N * chw))
    cand = torch.empty(2 * N, 3, 64, 80, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(5)
    for s in range(0, 2 * N, 1 << 14):
        cand[s:s + (1 << 14)].normal_(generator=g)
    for row in [T // chw + d for T in LR.BOUNDARIES for d in (-1, 0, 1)]:
        T = row * chw
        want = [(row % N * 7 + 3) % N] * 2
        want[row // N] = row % N
        score = torch.rand(2, N)
        for b in range(2):
            score[b, want[b]] = 2.0
        sd = score.reshape(-1).cuda()
        expect = torch.stack([cand[b * N + want[b]] for b in range(2)])
        for name, call in (("select_best", lambda: ops.select_best(cand, sd, N)), ("select_scores", lambda: ops.select_scores(cand, sd, N, rule="max"))):
            outs = []
            with LR.canaries(monkeypatch, outs):
                res = call()
                outs.extend(t for t in res if t is not None)
            assert res[0].cpu().tolist() == want, (name, T)
            assert torch.equal(res[-1], expect), f"{name}: the gathered image at boundary {T} is not candidate {want}"
        st = ops.BestState(2, (3, 64, 80), "cuda", "max")
        ops.select_merge(st, cand, sd, N)                 # all N samples as one chunk: the tensor that crosses
        assert st.best.cpu().tolist() == want and torch.equal(st.images, expect), ("select_merge", T)
    del cand
    torch.cuda.empty_cache()
    print(f"LARGE select gathers: cand = {2 * N * chw} elements, {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------------------------------------ one huge image
# The tile kernels address one image's planes with 32-bit byte offsets below 2^30 elements (every offset in the upper half of the plane set
# has bit 31 set) and run their *_wide forms with 64-bit offsets from there to 2^31.  C H W = 1 073 740 800 at 4092 x 6560 (exact tiles) is
# the last narrow plane set of C = 40; 4093 x 6559 (ragged last tile row and column) the first wide one.  Other widths: planes of the same
# kind that put C H W on either side of 2^30; C = 80 has no plane of 4093 rows below 2^31 at that width, so it is narrower.
NARROW, WIDE = {40: (4092, 6560), 24: (4092, 10912)}, {40: (4093, 6559), 24: (4093, 10931), 80: (4093, 3281)}
PERIOD = 8                   # two tile rows


def _periodic_image(C, H, W, seed):
    """(1, C, H, W), random in x and in the channels, periodic in y with period 8"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.randn(C, PERIOD, W, device="cuda", generator=g) * 2 + 0.3
    img = torch.empty(1, C, H, W, device="cuda")
    n = H // PERIOD
    img[0, :, :n * PERIOD].view(C, n, PERIOD, W).copy_(base[:, None].expand(C, n, PERIOD, W))
    img[0, :, n * PERIOD:].copy_(base[:, :H - n * PERIOD])
    return img


def _check_interior(out, what):
    """every 8-row block that touches neither border equals rows 8..15, bit for bit: a pixel's value depends on its 3 x 3 neighbourhood
    alone, and its place in the 4 x 32 tile repeats with the period"""
    _, C, H, W = out.shape
    nb = H // PERIOD
    for c in range(C):
        blocks = out[0, c, PERIOD:PERIOD * (nb - 1)].view(nb - 2, PERIOD, W)
        bad = torch.nonzero(~(blocks == blocks[:1]).all(-1).all(-1)).flatten()
        assert bad.numel() == 0, f"{what}: channel {c}, rows {PERIOD * (1 + int(bad[0]))}.. differ from rows 8..15"


def _strips(t):
    """the 24 top and the 24 bottom rows of a (1, C, H, W) image, on the CPU"""
    return t[:, :, :24].cpu(), t[:, :, -24:].cpu()


def _check_strips(out, ref_of_crop, ins, rtol, atol, what):
    """the top 16 and bottom 16 rows against the float64 reference of 24-row crops (the rows used are 8 from the cut)"""
    got = _strips(out)
    for side, sl in ((0, slice(0, 16)), (1, slice(8, 24))):
        ref = ref_of_crop({k: _strips(v)[side] for k, v in ins.items()})
        close(got[side][:, :, sl], ref[:, :, sl], rtol, atol, f"{what} {'top' if side == 0 else 'bottom'} 16 rows")


def _gd_huge(ops, monkeypatch, C, H, W, fused):
    t0 = time.perf_counter()
    Hd, t = _gd_case((1, C, 8, 32), True)
    p = {k: dev(v) for k, v in t.items() if k not in ("x", "y0", "y1")}
    LR.require_memory(LR.need_bytes(*([C * H * W] * (3 if fused else 2))))
    ins = {k: _periodic_image(C, H, W, 11 + j) for j, k in enumerate(("x", "y") if fused else ("x",))}
    outs = []
    with LR.canaries(monkeypatch, outs):
        outs.extend(_gd_run(fused)(ops, ins, dict(p, Hd=torch.tensor(Hd))))
    what = f"gdmlp_x6{' with pre' if fused else ''} C = {C} at {H} x {W} ({C * H * W} elements)"
    _check_interior(outs[0], what)
    _check_strips(outs[0], lambda crop: _gd_ref64(Hd, dict(t, x=crop["x"], y0=crop.get("y"), y1=crop.get("y")), fused), ins, *GD_TOL, what)
    del ins, outs
    torch.cuda.empty_cache()
    print(f"LARGE {what}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("C", [40, 24])
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "pre"])
def test_gdmlp_x6_last_narrow_plane_set(ops, monkeypatch, C, fused):
    _gd_huge(ops, monkeypatch, C, *NARROW[C], fused)


@pytest.mark.parametrize("C", [40, 24, 80])
def test_gdmlp_x6_first_wide_plane_set(ops, monkeypatch, C):
    """gdmlp_x6_wide_kernel<3, 2, 2>, <2, 1, 2> and <5, 3, 1>"""
    assert (1 << 30) <= C * WIDE[C][0] * WIDE[C][1] < (1 << 31)
    _gd_huge(ops, monkeypatch, C, *WIDE[C], False)


@pytest.mark.parametrize("shape", [NARROW[40], WIDE[40]], ids=["narrow", "wide"])
def test_ss2d_front_huge_image(ops, monkeypatch, shape):
    """ss2d_front_x6_kernel<3, 40> with bit 31 set in its offsets, and ss2d_front_x6_wide_kernel<3, 40>"""
    t0 = time.perf_counter()
    H, W = shape
    params = _front_params(40, 20)(torch.Generator().manual_seed(3))
    LR.require_memory(LR.need_bytes(40 * H * W, 40 * H * W, 20 * H * W))
    ins = {"x": _periodic_image(40, H, W, 21)}
    outs = []
    with LR.canaries(monkeypatch, outs):
        outs.extend(_front_run(ops, ins, {k: dev(v) for k, v in params.items()}))
    for j, name in enumerate(("xc", "xd")):
        what = f"ss2d_front {name} at {H} x {W}"
        _check_interior(outs[j], what)
        _check_strips(outs[j], lambda crop: _front_ref({k: v.double() for k, v in crop.items()}, params)[j], ins, *GD_TOL, what)
    del ins, outs
    torch.cuda.empty_cache()
    print(f"LARGE ss2d_front at {H} x {W}: {time.perf_counter() - t0:.2f} s")


def test_vssblock_forward_first_wide_plane_set(ops, monkeypatch):
    """A whole VSSBlock (n_feat 40, d_state 1) on the first wide plane set, 40 x 4093 x 6559: ops.vss_back_supported sends it to the two-kernel
    route -- LayerNorm + in_proj GEMM, depthwise conv, x_proj GEMM, plane transposes, the chunked scan over L = 26 845 987, the out_norm +
    out_proj GEMM with residual, then gdmlp_x6_wide_kernel<3, 2, 2> -- and every kernel of it runs at M L >= 2^30 or on planes of 2^30 elements.

    The scans are not local, so the checks of the tile kernels hold only with a short memory: dt is drawn from 2 .. 4 (a state decays by
    e^-2 per step at least, A = -1), and after 60 steps nothing of it is left in float64.  Then a pixel depends on about thirty rows around
    it, and at a column's end on the other end of the neighbouring column.  Input periodic in y with period 8 as above; the reference is the
    block in float64 (oracle.vssblock_ref with stage2_yardstick.ss2d_core64) on the first 61 rows of the same input: 61 = 4093 mod 8, so its
    top AND its bottom 40 rows have the neighbourhoods of the large image's.  Top 32 and bottom 40 rows against it, every 8-row block between
    against rows 32..39, both at the bound of tests/test_vss_back_gpu.py (1e-4 / 4e-5) -- not bit for bit: the chunked scan carries a
    state whose last bits depend on where in its 2048-step chunks a row falls."""
    from unittest import mock
    import stage2_yardstick as Y
    from oracle import bem_oracle as O
    from bem.modules import VSSBlock
    t0 = time.perf_counter()
    C, (H, W), SMALL, EDGE, BOTTOM = 40, WIDE[40], 61, 32, 40
    assert SMALL % PERIOD == H % PERIOD and C * H * W >= 1 << 30
    torch.manual_seed(3)
    blk = VSSBlock(hidden_dim=C, ssm_d_state=1, ssm_ratio=1, ssm_conv_bias=False, forward_type="v05_noz", mlp_ratio=2, mlp_type="gdmlp").eval()
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for p in (blk.norm.weight, blk.norm.bias, blk.op.out_norm.weight, blk.op.out_norm.bias, blk.norm2.weight, blk.norm2.bias):
            p.add_(0.1 * torch.randn(p.shape, generator=g))
        blk.op.dt_projs_bias.copy_(torch.log(torch.expm1(2 + 2 * torch.rand(blk.op.dt_projs_bias.shape, generator=g))))
        blk.op.dt_projs_weight.mul_(0.05)
        blk.op.Ds.copy_(0.1 * torch.randn(blk.op.Ds.shape, generator=g))
        blk.op.x_proj_weight[:, -2:].mul_(3.0)
    sd = {k: v.detach().double() for k, v in blk.state_dict().items()}
    blk.cuda()
    LR.require_memory(LR.need_bytes(*[C * H * W] * 11))
    x = _periodic_image(C, H, W, 31)
    small = x[:, :, :SMALL].cpu().double()
    lib, calls = ops.lib(), []
    for fn in ("bem_vss_back_x6_f32", "bem_gdmlp_x6_f32"):
        monkeypatch.setattr(lib, fn, lambda *a, fn=fn, real=getattr(lib, fn): calls.append(fn) or real(*a))
    outs = []
    with LR.canaries(monkeypatch, outs), torch.no_grad():
        outs.append(blk(x))
    y = outs[0]
    assert calls == ["bem_gdmlp_x6_f32"], calls
    del x
    what = f"VSSBlock C = {C} at {H} x {W}"
    with mock.patch.object(O, "ss2d_core_ref", Y.ss2d_core64):
        ref = O.vssblock_ref(sd, "", small, None, None)
    assert ref.dtype == torch.float64
    close(y[:, :, :EDGE], ref[:, :, :EDGE], *GD_TOL, what + " top 32 rows vs float64")
    close(y[:, :, -BOTTOM:], ref[:, :, -BOTTOM:], *GD_TOL, what + " bottom 40 rows vs float64")
    nb = -(-(H - EDGE - BOTTOM) // PERIOD)                       # the blocks from row 32 to where the bottom strip begins
    for c in range(C):
        blocks = y[0, c, EDGE:EDGE + nb * PERIOD].view(nb, PERIOD, W)
        bad = torch.nonzero(~torch.isclose(blocks, blocks[:1], rtol=GD_TOL[0], atol=GD_TOL[1]).all(-1).all(-1)).flatten()
        assert bad.numel() == 0, f"{what}: channel {c}, rows {EDGE + PERIOD * int(bad[0])}.. differ from rows 32..39"
    assert H - BOTTOM <= EDGE + nb * PERIOD <= H - 16
    del outs, y
    torch.cuda.empty_cache()
    print(f"LARGE {what}: {time.perf_counter() - t0:.2f} s")


def test_tile_kernel_limits_are_the_wrappers(ops, monkeypatch):
    """The fused SS2D tail has no wide form: from 2^30 elements per image on, vss_back_supported sends a VSSBlock to the two-kernel chain and
    gdmlp_x6(pre=...) is refused by the wrapper.  From 2^31 on gdmlp_x6 and ss2d_front are refused with the library's message.  Neither reaches
    the library: its entry points are replaced by recorders, and the tensors are allocated but never read."""
    from bem import native
    H, W = WIDE[40]
    assert ops.vss_back_supported(40, 160, NARROW[40][0] * NARROW[40][1]) and not ops.vss_back_supported(40, 160, H * W)
    assert ops.vss_back_supported(24, 96, NARROW[24][0] * NARROW[24][1]) and not ops.vss_back_supported(24, 96, WIDE[24][0] * WIDE[24][1])
    calls = []
    for fn in ("bem_vss_back_x6_f32", "bem_gdmlp_x6_f32", "bem_ss2d_front_x6_f32"):
        monkeypatch.setattr(ops.lib(), fn, lambda *a, fn=fn: calls.append(fn) or 1)
    Hd, t = _gd_case((1, 40, 8, 32), True)
    p = {k: dev(v) for k, v in t.items() if k not in ("x", "y0", "y1")}
    LR.require_memory(LR.need_bytes(*[40 * 4200 * 12800] * 2))
    x = torch.empty(1, 40, H, W, device="cuda")
    with pytest.raises(ValueError, match="gdmlp_x6 with pre"):
        _gd_run(True)(ops, {"x": x, "y": x}, dict(p, Hd=torch.tensor(Hd)))
    del x
    x = torch.empty(1, 40, 4200, 12800, device="cuda")                     # 2 150 400 000 elements
    with pytest.raises(native.BemNativeError, match="plane set too large for 32-bit offsets"):
        _gd_run(False)(ops, {"x": x}, dict(p, Hd=torch.tensor(Hd)))
    fp = {k: dev(v) for k, v in _front_params(40, 20)(torch.Generator().manual_seed(3)).items()}
    with pytest.raises(native.BemNativeError, match="plane set too large for 32-bit offsets"):
        _front_run(ops, {"x": x}, fp)
    assert calls == []
    del x
    torch.cuda.empty_cache()


