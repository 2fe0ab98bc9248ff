"""GPU: SS2D's depthwise conv + SiLU, x_proj and four-direction scan as one kernel on small planes (csrc/ss2d_core_small.hip,
ops.ss2d_core_small, the branch of modules.SS2D.forward_fused behind ops.USE_SS2D_CORE).

* (a) the op against a float64 evaluation of conv + SiLU, x_proj and the four scans, held to the distance of the six-launch chain from
  float64 at the same inputs (the pattern of tests/test_upfuse_gpu.py).  The two sum the x_proj products in different orders (the
  chain: bf16-limb products on the matrix cores; the kernel: f32 FMAs in ascending c with a compensated running sum) and neither is
  privileged, so the kernel may be MARGIN times further out than the chain; profiles/ss2d_core_parity.txt holds both errors per shape
  (kernel / chain: mean error 0.98 .. 1.21, max error 0.62 .. 1.65).  The margin is the factor the suite's Stage-II float64 yardstick
  already allows (tests/test_upfuse_gpu.py::_yardstick); a ratio above 4 is a bug, not a tolerance -- an uncompensated FMA chain over c
  reached 4.6 at C = 160 and was replaced;
* (b) two launches on the same inputs give the same bits;
* (c) a deterministic and a Bayesian VSSBlock, switch on and off, both against the float64 oracle within the same bound, and the
  switched-on forward runs none of the chain's middle launches inside SS2D;
* (d) the predicate refuses H W > 256 and d_state > 1, and the block then runs the chain."""
import math
from unittest import mock

import pytest
import torch
import torch.nn.functional as F

import stage2_yardstick as Y
from oracle import bem_oracle as O

pytestmark = pytest.mark.gpu

MARGIN = 2.0
PLANES = [(4, 4), (8, 8), (16, 16), (4, 8), (16, 8)]
WIDTHS = [(8, 1), (40, 3), (80, 5)]                                 # (C, dt_rank)
# every plane at every width, and the level-2 width of Stage I on its 4x4 plane; batch and weight form alternate over the list
CASES = [(C, R, H, W) for (C, R) in WIDTHS for (H, W) in PLANES] + [(160, 10, 4, 4)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bem import ops as _ops
    return _ops


def _inputs(C, R, H, W, B, per_sample, bias):
    """Seeded operands on the CPU: the scan's state term as large as D x (Ds ~ 0.1 N(0,1), dt ~ U[0.05, 1], B / C rows x 3: the draw of
    stage2_yardstick.recurrence_dominated), and channel 1 with dt_projs_bias = 25 in every direction: z > 20, softplus' linear branch."""
    g = torch.Generator().manual_seed(1000 * C + 16 * H + W)
    r = lambda *s: torch.randn(*s, generator=g)
    d = dict(t=r(B, C, H, W), dww=r(*((B,) if per_sample else ()), C, 1, 3, 3) / 3, dwb=(0.2 * r(*((B,) if per_sample else ()), C) if bias else None),
             xw=r(4, R + 2, C) / math.sqrt(C), dtw=(2 * torch.rand(4, C, R, generator=g) - 1) * R ** -0.5,
             A_logs=0.3 * r(4 * C, 1), Ds=Y.DS_SCALE * r(4 * C))
    d["xw"][:, -2:] *= Y.BC_GAIN
    dt = Y.DT_RANGE[0] + (Y.DT_RANGE[1] - Y.DT_RANGE[0]) * torch.rand(4, C, generator=g, dtype=torch.float64)
    d["dtb"] = torch.log(torch.expm1(dt)).float()
    d["dtb"][:, 1] = 25.0
    return d


def _ref64(d):
    """conv + SiLU, x_proj, dt_proj, the four scans and their merge in float64 (stage2_yardstick.scan64; ss2d_core64 without out_norm)."""
    t = d["t"].double()
    B, C, H, W = t.shape
    w = d["dww"].double().expand(B, C, 1, 3, 3).reshape(B * C, 1, 3, 3)
    b = None if d["dwb"] is None else d["dwb"].double().expand(B, C).reshape(B * C)
    xc = F.silu(F.conv2d(t.reshape(1, B * C, H, W), w, b, padding=1, groups=B * C)).reshape(B, C, H, W)
    xs = O.cross_scan_ref(xc)
    R = d["dtw"].shape[2]
    x_dbl = torch.einsum("bkcl,kjc->bkjl", xs, d["xw"].double())
    dts, Bs, Cs = torch.split(x_dbl, [R, 1, 1], dim=2)
    dts = torch.einsum("bkrl,kcr->bkcl", dts, d["dtw"].double())
    ch, du = Y.scan64(xs.reshape(B, 4 * C, H * W), dts.reshape(B, 4 * C, H * W), -torch.exp(d["A_logs"].double()), Bs, Cs, d["Ds"].double(),
                      d["dtb"].double().reshape(-1), blk=4)          # dt = 25 on channel 1: short blocks keep exp(-cl) in range
    return O.cross_merge_ref((ch + du).reshape(B, 4, C, H, W)).reshape(B, C, H, W)


def _dev(d):
    c = {k: (None if v is None else v.cuda().contiguous()) for k, v in d.items()}
    xw = c["xw"]
    c["rows"] = torch.cat([xw[0], xw[2], xw[1], xw[3]], 0).contiguous()            # [dir 0 | dir 2 | dir 1 | dir 3], as SS2D._scan_params
    c["A"] = -torch.exp(c["A_logs"]).reshape(-1).contiguous()
    return c


def _kernel(ops, c):
    return ops.ss2d_core_small(c["t"], c["dww"], c["dwb"], c["rows"], c["dtw"], c["dtb"], c["A"], c["Ds"])


def _chain(ops, c):
    """The six launches of SS2D.forward_fused between in_proj and out_proj (transposed-plane scan), and y0 + y1."""
    B, C, H, W = c["t"].shape
    M, L = c["dtw"].shape[2] + 2, H * W
    xc = ops.dwconv3x3(c["t"], c["dww"], c["dwb"], mode=1)
    xd = ops.pw_gemm(xc, ops.pack_pw_weight(c["rows"]), 4 * M)
    xd1 = ops.transpose_plane_slice(xd, 2 * M, 2 * M)
    y0, y1 = ops.ss2d_scan(xc.view(B, C, L), ops.transpose_planes(xc).view(B, C, L), xd.view(B, 4, M, L)[:, :2], xd1.view(B, 2, M, L),
                           c["dtw"], c["dtb"], c["A"], c["Ds"])
    return y0.view(B, C, H, W) + ops.transpose_planes(y1.view(B, C, W, H))


def _held(got, chain, r64, what):
    """got no further from float64 than MARGIN times the chain is, in mean and in max absolute error."""
    (cm, cM), (km, kM) = Y.errors(chain, r64), Y.errors(got, r64)
    print(f"PARITY {what}: |ref| max {float(r64.abs().max()):.2e} | chain mean {cm:.3e} max {cM:.3e} | kernel mean {km:.3e} max {kM:.3e} "
          f"({km / cm:.2f}x, {kM / cM:.2f}x)")
    assert torch.isfinite(got).all()
    assert km <= MARGIN * cm and kM <= MARGIN * cM, (what, km, cm, kM, cM)


@pytest.mark.parametrize("case", list(enumerate(CASES)), ids=lambda ic: "C{}-R{}-{}x{}".format(*ic[1]))
def test_core_vs_float64_and_chain(ops, case):
    """(a) and (b).  Even cases: B = 3 with per-sample depthwise weights; odd cases: B = 2 with shared ones; the bias alternates with
    the pairs, so every weight form meets a bias and none."""
    i, (C, R, H, W) = case
    per_sample, bias = i % 2 == 0, (i // 2) % 2 == 0
    d = _inputs(C, R, H, W, 3 if per_sample else 2, per_sample, bias)
    assert ops.ss2d_core_small_supported(C, H, W, R)
    c = _dev(d)
    got = _kernel(ops, c)
    assert torch.equal(got, _kernel(ops, c))
    r64 = _ref64(d)
    _held(got.cpu(), _chain(ops, c).cpu(), r64, f"ss2d_core_small C={C} R={R} {H}x{W} B={d['t'].shape[0]} per_sample={per_sample} bias={bias}")


def test_softplus_branch_is_taken(ops):
    """Channel 1 of _inputs sits on softplus' linear branch with the data in: z = dt_proj(x_dbl) + 25 stays above 20 at every position."""
    d = _inputs(40, 3, 8, 8, 2, False, True)
    t = d["t"].double()
    xc = F.silu(F.conv2d(t, d["dww"].double(), d["dwb"].double(), padding=1, groups=40))
    dts = torch.einsum("bkrl,kcr->bkcl", torch.einsum("bkcl,kjc->bkjl", O.cross_scan_ref(xc), d["xw"].double())[:, :, :3], d["dtw"].double())
    z = dts + d["dtb"].double()[None, :, :, None]
    assert float(z[:, :, 1].min()) > 20 and float(z[:, :, 2:].max()) < 20


# ----------------------------------------------------------------------------- the block ---
def _block(C, bayes):
    from basicsr.bayesian import convert2bnn
    from bem.modules import VSSBlock, set_module_paths
    torch.manual_seed(7 + C)
    blk = VSSBlock(hidden_dim=C, ssm_d_state=1, ssm_ratio=1, ssm_conv_bias=False, forward_type="v05_noz", mlp_ratio=4, mlp_type="gdmlp")
    sd = Y.recurrence_dominated(blk.state_dict(), 5)
    with torch.no_grad():
        for k in ("op.out_norm.weight", "op.out_norm.bias", "norm.weight", "norm.bias"):
            sd[k].add_(0.1 * torch.randn(sd[k].shape))
    blk.load_state_dict(sd)
    if bayes:
        convert2bnn(blk, {"sigma_init": 0.05, "decay": 0.998, "pretrain": False})
    set_module_paths(blk)
    return blk.cuda().eval()


def _block_ref64(blk, x, eps):
    """O.vssblock_ref in float64 (stage2_yardstick.ss2d_core64), sample by sample with the injected draws of a Bayesian block."""
    sd = {k: v.detach().cpu().double() for k, v in blk.state_dict().items()}
    out = []
    with mock.patch.object(O, "ss2d_core_ref", Y.ss2d_core64):
        for i in range(x.shape[0]):
            src = None if eps is None else O.EpsSource({k: v[i].double() for k, v in eps.items()})
            out.append(O.vssblock_ref(sd, "", x[i:i + 1].double(), src, None))
    return torch.cat(out, 0)


def _forward(ops, blk, x, eps, on):
    """Eval forward with the switch on / off -> (output, names of the chain's middle launches issued inside SS2D.forward_fused)."""
    from bem.modules import SampleCtx, sampling
    seen, inside = [], []
    real_ff = blk.op.forward_fused

    def ff(*a, **k):
        inside.append(1)
        try:
            return real_ff(*a, **k)
        finally:
            inside.pop()
    patches = [mock.patch.object(ops, "USE_SS2D_CORE", on), mock.patch.object(blk.op, "forward_fused", ff)]
    for name in ("transpose_planes", "transpose_plane_slice", "dwconv3x3", "ss2d_scan", "ss2d_scan_rm", "ss2d_scan_n"):
        def spy(*a, _orig=getattr(ops, name), _name=name, **k):
            if inside:
                seen.append(_name)
            return _orig(*a, **k)
        patches.append(mock.patch.object(ops, name, spy))
    for p in patches:
        p.start()
    try:
        with torch.no_grad(), sampling(None if eps is None else SampleCtx(x.shape[0], {k: v.cuda() for k, v in eps.items()})):
            return blk(x.cuda()).cpu(), seen
    finally:
        for p in reversed(patches):
            p.stop()


@pytest.mark.parametrize("C,H,W,bayes", [(80, 8, 8, False), (40, 16, 16, True), (40, 4, 8, True)], ids=["plain-80-8x8", "bayes-40-16x16", "bayes-40-4x8"])
def test_block_switch_on_and_off_vs_float64(ops, C, H, W, bayes):
    """(c).  C = 80 keeps the deterministic block off the fused SS2D tail (C <= 48), which needs y0 / y1 and stays on the chain."""
    blk = _block(C, bayes)
    B = 3
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(B, C, H, W, generator=g)
    eps = None
    if bayes:
        eps = {}
        for n, m in blk.named_modules():
            if hasattr(m, "mu_weight"):
                eps[n + ".weight"] = torch.randn((B,) + tuple(m.mu_weight.shape), generator=g)
                if getattr(m, "mu_bias", None) is not None:
                    eps[n + ".bias"] = torch.randn((B,) + tuple(m.mu_bias.shape), generator=g)
    on, seen_on = _forward(ops, blk, x, eps, True)
    off, seen_off = _forward(ops, blk, x, eps, False)
    assert seen_on == [], seen_on
    assert sorted(set(seen_off)) == ["dwconv3x3", "ss2d_scan", "transpose_plane_slice", "transpose_planes"], seen_off
    _held(on, off, _block_ref64(blk, x, eps), f"VSSBlock C={C} {H}x{W} bayes={bayes}")


def test_predicate_and_fallback(ops):
    """(d)."""
    assert ops.ss2d_core_small_supported(40, 16, 16, 3) and ops.ss2d_core_small_supported(160, 4, 4, 10)
    assert not ops.ss2d_core_small_supported(40, 16, 17, 3)                # H W > 256
    assert not ops.ss2d_core_small_supported(40, 32, 16, 3)
    assert not ops.ss2d_core_small_supported(40, 16, 16, 3, 2)             # d_state > 1
    assert not ops.ss2d_core_small_supported(160, 16, 16, 10)              # a sample's planes and x_dbl rows beyond one CU's LDS
    assert not ops.ss2d_core_small_supported(40, 10, 10, 3)                # 100 positions: neither whole wavefronts nor below 64
    assert not ops.ss2d_core_small_supported(42, 8, 8, 3)                  # C % 4
    t = torch.zeros(1, 40, 16, 17, device="cuda")
    with pytest.raises(ValueError):
        ops.ss2d_core_small(t, torch.zeros(40, 1, 3, 3, device="cuda"), None, torch.zeros(20, 40, device="cuda"), torch.zeros(4, 40, 3, device="cuda"),
                            torch.zeros(4, 40, device="cuda"), torch.zeros(160, device="cuda"), torch.zeros(160, device="cuda"))
    from bem.modules import VSSBlock
    for kw, shape in ((dict(ssm_d_state=1), (2, 80, 16, 20)), (dict(ssm_d_state=2), (2, 80, 8, 8))):
        torch.manual_seed(1)
        blk = VSSBlock(hidden_dim=80, ssm_ratio=1, ssm_conv_bias=False, forward_type="v05_noz", mlp_ratio=4, mlp_type="gdmlp", **kw).cuda().eval()
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(2))
        on, seen = _forward(ops, blk, x, None, True)
        assert any(s.startswith("ss2d_scan") for s in seen), seen
        assert torch.isfinite(on).all()
