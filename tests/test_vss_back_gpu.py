"""The back half of a VSSBlock as one kernel (bem_vss_back_x6_f32: the SS2D tail x1 = x + out_proj(out_norm(y0 + y1)) + b folded into the
prologue of the fused gdMlp kernel) against the two-kernel chain and against torch in float64; the host row permutation of the out_proj
operand on the CPU and, with an identity weight, on the GPU; the dispatch of VSSBlock.forward."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bem import ops

# (B, C, Hd, H, W): K padded 40 -> 48 and M 40 -> 64 with two ragged tile rows and columns and a batch stride; exactly one tile and one chunk;
# two k-blocks; a plane smaller than a tile.  C > 48 is not shipped (the wide forms spill) and runs the chain.
CASES = [(2, 40, 32, 5, 33), (1, 40, 16, 4, 32), (1, 24, 32, 9, 70), (1, 40, 32, 1, 3)]


def dev(t):
    return t.cuda().contiguous()


def close(a, b, rtol, atol, what=""):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a - b).abs().max().item()
    print(f"{what}: max abs err {err:.3e} (ref max {b.abs().max():.3e})")
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{what}: max abs err {err:.3e} (ref max {b.abs().max():.3e})"


def ln64(v, w, b, eps):
    mu, var = v.mean(1, keepdim=True), v.var(1, unbiased=False, keepdim=True)
    return (v - mu) / (var + eps).sqrt() * w.double()[None, :, None, None] + b.double()[None, :, None, None]


# ------------------------------------------------------------------------------------------ CPU ----
def test_row_permutation_against_the_accumulator_layout():
    """ops.vss_back_rows against a numpy model of the kernel's two layouts: the 32x32 MFMA leaves output row acc_row(r, kh) =
    (r & 3) + 8 (r >> 2) + 4 kh of an M-tile in register r of lane half kh, and load_block keeps channel 16 kb + 8 kh + e of a pixel in
    slot (kb, e) of that half.  Multiplying by the permuted matrix must leave, in register s = 16 mt + r, the value slot (s >> 3, s & 7) holds."""
    for C in (8, 16, 24, 40, 48, 72, 80):
        KB = (C + 15) // 16
        MT = (8 * KB + 15) // 16
        rows = ops.vss_back_rows(C)
        assert len(rows) == 32 * MT
        used = [r for r in rows if r >= 0]
        assert sorted(used) == list(range(C)), "every channel exactly once"
        rng = np.random.default_rng(C)
        W, v = rng.standard_normal((C, C)), rng.standard_normal(C)
        Wz = np.concatenate([W, np.zeros((1, C))], 0)
        acc = Wz[np.array(rows)] @ v                                       # output rows of the MT M-tiles, in packed-row order
        want = W @ v
        for kh in range(2):
            regs = [acc[32 * mt + (r & 3) + 8 * (r >> 2) + 4 * kh] for mt in range(MT) for r in range(16)]      # the lane's registers, s = 16 mt + r
            for kb in range(KB):
                for e in range(8):
                    ch = 16 * kb + 8 * kh + e
                    assert regs[8 * kb + e] == (want[ch] if ch < C else 0.0), (C, kh, kb, e)
            assert all(x == 0.0 for x in regs[8 * KB:])


def test_supported_widths_and_cost():
    L = 256 * 256
    assert ops.vss_back_supported(40, 160, L) and ops.vss_back_supported(24, 32, L) and ops.vss_back_supported(48, 16, L)
    assert not ops.vss_back_supported(80, 320, L) and not ops.vss_back_supported(44, 32, L) and not ops.vss_back_supported(40, 24, L)
    assert ops.vss_back_supported(40, 160, (1 << 30) // 40 - 1) and not ops.vss_back_supported(40, 160, -(-(1 << 30) // 40))     # C L < 2^30
    x = torch.zeros(2, 40, 8, 32)
    nb, nf = ops._gdmlp_x6_cost(x=x, Hd=160, pre=None)
    assert (nb, nf) == (8.0 * x.numel(), 12.0 * 2 * 8 * 32 * (320 * 40 + 160 * 40))         # without pre: as it was
    nb2, nf2 = ops._gdmlp_x6_cost(x=x, Hd=160, pre=(None,) * 7)
    assert nb2 == nb + 8.0 * x.numel() and nf2 == nf + 12.0 * 2 * 8 * 32 * 40 * 40          # + y0, y1 and the C x C GEMM


# ------------------------------------------------------------------------------------------ GPU ----
def _case(cfg, bias, identity=False):
    B, C, Hd, H, W = cfg
    g = torch.Generator().manual_seed(C * Hd + H + 7 * W)
    t = dict(x=torch.randn(B, C, H, W, generator=g) * 2 + 0.3, y0=torch.randn(B, C, H, W, generator=g) + 0.2,
             y1=torch.randn(B, C, H, W, generator=g) * 1.5 - 0.1,
             onw=1 + 0.2 * torch.randn(C, generator=g), onb=0.1 * torch.randn(C, generator=g),
             wop=torch.randn(C, C, generator=g) * C ** -0.5, bop=0.3 * torch.randn(C, generator=g) if bias else None,
             lw=1 + 0.2 * torch.randn(C, generator=g), lb=0.1 * torch.randn(C, generator=g),
             wi=torch.randn(2 * Hd, C, generator=g) * C ** -0.5, bi=0.3 * torch.randn(2 * Hd, generator=g) if bias else None,
             wd=torch.randn(2 * Hd, 1, 3, 3, generator=g) / 3, bd=0.2 * torch.randn(2 * Hd, generator=g) if bias else None,
             wo=torch.randn(C, Hd, generator=g) * Hd ** -0.5, bo=0.3 * torch.randn(C, generator=g) if bias else None)
    if identity:
        t["wop"], t["onw"], t["onb"] = torch.eye(C), torch.ones(C), torch.zeros(C)
    return t


def _run(cfg, t, fused):
    """The fused call, or today's chain (the sum-input LayerNorm GEMM with residual, then the gdMlp kernel); also returns x1 of the chain."""
    B, C, Hd, H, W = cfg
    d = {k: (None if v is None else dev(v)) for k, v in t.items()}
    perm = ops.gate_interleave(Hd, "cpu")
    Wg = ops.pack_pw_weight(dev(t["wi"][perm]), x6=True)
    bg = dev(t["bi"][perm]) if t["bi"] is not None else torch.zeros(2 * Hd, device="cuda")
    w10 = ops.dw_gate_params10(d["wd"], d["bd"], Hd)
    Wo = ops.pack_pw_weight(d["wo"], x6=True)
    if fused:
        pre = (d["y0"], d["y1"], d["onw"], d["onb"], 1e-5, ops.pack_vss_back_outproj(d["wop"]), d["bop"])
        return ops.gdmlp_x6(d["x"], d["lw"], d["lb"], 1e-6, Wg, bg, w10, Wo, d["bo"], Hd, pre=pre), None
    x1 = ops.pw_gemm(d["y0"], ops.pack_pw_weight(d["wop"], x6=True), C, x2=d["y1"], in_mode=1, ln=(d["onw"], d["onb"]), ln_eps=1e-5,
                     bias=d["bop"], res=d["x"])
    return ops.gdmlp_x6(x1, d["lw"], d["lb"], 1e-6, Wg, bg, w10, Wo, d["bo"], Hd), x1


def _ref64(cfg, t):
    B, C, Hd, H, W = cfg
    o = lambda v: None if v is None else v.double()
    x1 = t["x"].double() + F.conv2d(ln64(t["y0"].double() + t["y1"].double(), t["onw"], t["onb"], 1e-5), t["wop"].double()[:, :, None, None], o(t["bop"]))
    tt = F.conv2d(ln64(x1, t["lw"], t["lb"], 1e-6), t["wi"].double()[:, :, None, None], o(t["bi"]))
    hh = F.conv2d(tt, t["wd"].double(), o(t["bd"]), padding=1, groups=2 * Hd)
    return (x1 + F.conv2d(F.gelu(hh[:, :Hd]) * hh[:, Hd:], t["wo"].double()[:, :, None, None], o(t["bo"]))).float(), x1.float()


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("cfg", CASES)
def test_vss_back_vs_chain_and_float64(cfg, bias):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    t = _case(cfg, bias)
    y, _ = _run(cfg, t, True)
    chain, _ = _run(cfg, t, False)
    close(y, chain, 1e-4, 4e-5, f"vss_back vs chain {cfg} bias={bias}")
    close(y, _ref64(cfg, t)[0], 1e-4, 4e-5, f"vss_back vs torch f64 {cfg} bias={bias}")


@pytest.mark.gpu
@pytest.mark.parametrize("C", [40, 24])
def test_identity_out_proj_pins_the_row_permutation(C):
    """out_proj = I, out_norm weight 1 and bias 0: x1 = x + LN(y0 + y1) channel by channel.  With project_out = 0 and no bias the kernel's
    output is x1 itself (the residual it parked in out), so a wrong row order shows as channels swapped."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cfg = (1, C, 16, 5, 33)
    t = _case(cfg, False, identity=True)
    t["wo"] = torch.zeros_like(t["wo"])
    y, _ = _run(cfg, t, True)
    want = (t["x"].double() + ln64(t["y0"].double() + t["y1"].double(), t["onw"], t["onb"], 1e-5)).float()
    close(y, want, 1e-4, 4e-5, f"identity out_proj C={C}")


@pytest.mark.gpu
def test_block_dispatch(monkeypatch):
    """One VSSBlock (n_feat 40, 8 x 40 plane, B = 2): the fused route against the two-kernel route; a grad-mode forward and a block with
    Bayesian leaves never reach the fused entry point (counted at the library call)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from basicsr.bayesian import convert2bnn
    from bem import native
    from bem.modules import VSSBlock
    lib = native.lib()
    real, calls = lib.bem_vss_back_x6_f32, []

    def spy(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(lib, "bem_vss_back_x6_f32", spy)
    torch.manual_seed(3)
    blk = VSSBlock(hidden_dim=40, ssm_d_state=1, ssm_ratio=1, ssm_conv_bias=False, forward_type="v05_noz", mlp_ratio=4, mlp_type="gdmlp").cuda().eval()
    with torch.no_grad():
        for p in (blk.op.out_norm.weight, blk.op.out_norm.bias, blk.norm2.weight, blk.norm2.bias):
            p.add_(0.1 * torch.randn_like(p))
    x = torch.randn(2, 40, 8, 40, device="cuda")
    y = blk(x)
    assert len(calls) == 1
    monkeypatch.setattr(ops, "USE_VSS_BACK", False)
    ref = blk(x)
    assert len(calls) == 1
    monkeypatch.setattr(ops, "USE_VSS_BACK", True)
    close(y, ref, 1e-4, 4e-5, "VSSBlock fused vs chain")
    blk.train()
    out = blk(x.clone().requires_grad_(True))                              # a training forward records the graph: never the fused route
    assert out.requires_grad and len(calls) == 1
    blk.eval()
    convert2bnn(blk, {"sigma_init": 0.05, "decay": 0.998, "pretrain": False})
    assert not blk.op.tail_deferrable(40)
    blk.cuda().eval()
    assert torch.isfinite(blk(x)).all() and len(calls) == 1               # per-sample weight sets stay on the chain
