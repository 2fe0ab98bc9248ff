"""GPU parity: every HIP kernel (through the C ABI / bem.ops) against the CPU oracle on the same
seeded inputs, plus the reference-generated golden vectors.  Tolerances are stated per test."""
import ctypes
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, qd_state_dict
from oracle import bem_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bem import ops as _ops
    return _ops


def dev(t):
    return t.cuda().contiguous()


def close(a, b, rtol=1e-5, atol=1e-6, what=""):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a - b).abs().max().item()
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{what}: max abs err {err:.3e} (ref max {b.abs().max():.3e})"


# ----------------------------------------------------------------------------- selective scan ---
@pytest.mark.parametrize("tag", list("abcde"))
def test_selective_scan_golden(ops, tag):
    """bem_selective_scan_fwd_f32 vs the reference's own output; reference f32 tolerance is
    rtol 6e-4 / atol 2e-3 (test_selective_scan.py:398-405); we hold 1e-4 / 1e-4."""
    g = load_golden(f"g1_scan_{tag}")
    D = dev(g["D"]) if "D" in g else None
    b = dev(g["delta_bias"]) if "delta_bias" in g else None
    y = ops.selective_scan_fwd(dev(g["u"]), dev(g["delta"]), dev(g["A"]), dev(g["B"]), dev(g["C"]), D, b, True)
    close(y, g["y"], 1e-4, 1e-4, f"scan {tag}")


@pytest.mark.parametrize("shape", [(1, 8, 1, 1), (2, 12, 63, 1), (1, 4, 2049, 1), (1, 8, 5000, 2), (3, 8, 1024, 1), (1, 4, 257, 1)])
def test_selective_scan_vs_oracle(ops, shape):
    Bt, KC, L, N = shape
    g = torch.Generator().manual_seed(L)
    u, delta = torch.randn(Bt, KC, L, generator=g), 0.5 * torch.rand(Bt, KC, L, generator=g)
    A = -0.5 * torch.rand(KC, N, generator=g) - 0.01
    Bm, Cm = torch.randn(Bt, 4, N, L, generator=g), torch.randn(Bt, 4, N, L, generator=g)
    D, bias = torch.randn(KC, generator=g), 0.5 * torch.rand(KC, generator=g)
    ref = O.selective_scan_c(u, delta, A, Bm, Cm, D, bias, True)
    y = ops.selective_scan_fwd(dev(u), dev(delta), dev(A), dev(Bm), dev(Cm), dev(D), dev(bias), True)
    close(y, ref, 1e-4, 1e-4, f"scan {shape}")
    ref2 = O.selective_scan_c(u, delta, A, Bm, Cm, None, None, False)
    y2 = ops.selective_scan_fwd(dev(u), dev(delta), dev(A), dev(Bm), dev(Cm), None, None, False)
    close(y2, ref2, 1e-4, 1e-4, f"scan nosoftplus {shape}")


def test_selective_scan_linearity_full_size(ops):
    """Size-independent property at the config-2 level-0 size (L = 16384, 160 rows, batch 2):
    the scan is linear in u for fixed delta/A/B/C -> scan(u1 + 2 u2) = scan(u1) + 2 scan(u2)."""
    g = torch.Generator().manual_seed(0)
    Bt, KC, L = 2, 160, 16384
    u1, u2 = dev(torch.randn(Bt, KC, L, generator=g)), dev(torch.randn(Bt, KC, L, generator=g))
    delta, A = dev(0.5 * torch.rand(Bt, KC, L, generator=g)), dev(-0.5 * torch.rand(KC, 1, generator=g))
    Bm, Cm = dev(torch.randn(Bt, 4, 1, L, generator=g)), dev(torch.randn(Bt, 4, 1, L, generator=g))
    D = dev(torch.randn(KC, generator=g))
    f = lambda u: ops.selective_scan_fwd(u, delta, A, Bm, Cm, D, None, True)
    close(f(u1 + 2 * u2), f(u1) + 2 * f(u2), 1e-3, 1e-3, "linearity")
    # and one row against the C oracle
    ref = O.selective_scan_c(u1[:1, :4].cpu(), delta[:1, :4].cpu(), A[:4].cpu(), Bm[:1, :1].cpu(), Cm[:1, :1].cpu(), D[:4].cpu(), None, True)
    y = ops.selective_scan_fwd(u1[:1, :4].contiguous(), delta[:1, :4].contiguous(), A[:4].contiguous(), Bm[:1, :1].contiguous(),
                               Cm[:1, :1].contiguous(), D[:4].contiguous(), None, True)
    close(y, ref, 1e-4, 1e-4, "row vs oracle")


def test_cross_scan_merge_golden(ops):
    g = load_golden("g2_cross")
    assert torch.equal(ops.cross_scan(dev(g["x"])).cpu(), g["xs"])        # pure data movement: bit exact
    close(ops.cross_merge(dev(g["ys"])), g["y"], 0, 1e-6, "cross_merge")


@pytest.mark.parametrize("hw", [(1, 1), (3, 130), (64, 64)])
def test_cross_scan_merge_shapes(ops, hw):
    H, W = hw
    x = torch.randn(2, 3, H, W)
    assert torch.equal(ops.cross_scan(dev(x)).cpu(), O.cross_scan_ref(x))
    ys = torch.randn(2, 4, 3, H, W)
    close(ops.cross_merge(dev(ys)), O.cross_merge_ref(ys), 0, 1e-6)


# ----------------------------------------------------------------------------- fused ss2d scan --
def _ss2d_case(B, C, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    R = -(-C // 16)
    sd = {"x_proj_weight": torch.randn(4, R + 2, C, generator=g) * C ** -0.5,
          "dt_projs_weight": (torch.rand(4, C, R, generator=g) - 0.5) * 2 * R ** -0.5,
          "dt_projs_bias": torch.randn(4, C, generator=g) - 3.0,
          "A_logs": torch.randn(4 * C, 1, generator=g) * 0.5, "Ds": torch.randn(4 * C, generator=g),
          "out_norm.weight": torch.ones(C), "out_norm.bias": torch.zeros(C)}
    x = F.silu(torch.randn(B, C, H, W, generator=g))
    return sd, x, R


@pytest.mark.parametrize("shape", [(2, 8, 4, 4), (1, 40, 16, 12), (2, 16, 7, 10), (1, 24, 64, 48), (1, 8, 33, 70),
                                   # whole-row forms (L = 256 / 1024 / 4096; dt_rank 3, 5, 10, other) and the mask-free chunked form (L % 2048 == 0)
                                   (2, 40, 16, 16), (1, 80, 32, 32), (1, 160, 16, 16), (1, 8, 64, 64), (1, 40, 64, 96), (1, 8, 128, 128), (1, 80, 32, 128)])
def test_ss2d_scan_vs_oracle(ops, shape):
    """transpose -> x_proj GEMMs -> bem_ss2d_scan -> transpose back, against cross_scan/x_proj/dt_proj/
    selective_scan/cross_merge of the oracle (pre out_norm).  Tolerance 2e-4 rel / 2e-5 abs."""
    B, C, H, W = shape
    sd, x, R = _ss2d_case(B, C, H, W, sum(shape))
    L = H * W
    # oracle, stopping before out_norm
    xs = O.cross_scan_ref(x)
    x_dbl = torch.einsum("bkcl,kjc->bkjl", xs, sd["x_proj_weight"])
    dts, Bs, Cs = torch.split(x_dbl, [R, 1, 1], dim=2)
    dts = torch.einsum("bkrl,kcr->bkcl", dts, sd["dt_projs_weight"])
    ys = O.selective_scan_c(xs.reshape(B, 4 * C, L), dts.reshape(B, 4 * C, L).contiguous(), -torch.exp(sd["A_logs"]),
                            Bs.contiguous(), Cs.contiguous(), sd["Ds"], sd["dt_projs_bias"].reshape(-1), True)
    ref = O.cross_merge_ref(ys.reshape(B, 4, C, H, W)).reshape(B, C, H, W)
    # HIP
    xc = dev(x)
    xw = sd["x_proj_weight"]
    w02 = ops.pack_pw_weight(dev(torch.cat([xw[0], xw[2]], 0)))
    w13 = ops.pack_pw_weight(dev(torch.cat([xw[1], xw[3]], 0)))
    xcT = ops.transpose_planes(xc)
    xd0 = ops.pw_gemm(xc, w02, 2 * (R + 2))
    xd1 = ops.pw_gemm(xcT, w13, 2 * (R + 2))
    close(xd0.view(B, 2, R + 2, L)[:, 0], x_dbl[:, 0], 1e-4, 1e-5, "x_dbl dir0")
    close(xd1.view(B, 2, R + 2, L)[:, 1], x_dbl[:, 3].flip(-1), 1e-4, 1e-5, "x_dbl dir3")
    y0, y1 = ops.ss2d_scan(xc.view(B, C, L), xcT.view(B, C, L), xd0.view(B, 2, R + 2, L), xd1.view(B, 2, R + 2, L),
                           dev(sd["dt_projs_weight"]), dev(sd["dt_projs_bias"]), dev(-torch.exp(sd["A_logs"]).reshape(-1)), dev(sd["Ds"]))
    y = y0.view(B, C, H, W) + ops.transpose_planes(y1.view(B, C, W, H))
    close(y, ref, 2e-4, 2e-5, f"ss2d {shape}")


def _ss2d_fused64(x0, x1, xd0, xd1, dtw, dtb, A, Ds):
    """bem_ss2d_scan restated in float64 (the directions as in tests/test_train_gpu.py::_ss2d_torch, the scan in the blocked closed
    form of tests/stage2_yardstick.py): per orientation, (state term C*h, D*u) of its two directions summed."""
    from stage2_yardstick import scan64
    B, C, L = x0.shape
    R = dtw.shape[2]
    out = []
    for o, (x, xd) in enumerate(((x0, xd0), (x1, xd1))):
        ch = du = 0
        for slot, k in enumerate((o, o + 2)):
            xs, d = (x.flip(-1), xd[:, slot].flip(-1)) if slot else (x, xd[:, slot])
            dts = torch.einsum("cr,brl->bcl", dtw[k], d[:, :R])
            c, u = scan64(xs, dts, A[k * C:(k + 1) * C].view(C, 1), d[:, R].reshape(B, 1, 1, L), d[:, R + 1].reshape(B, 1, 1, L),
                          Ds[k * C:(k + 1) * C], dtb[k])
            ch, du = ch + (c.flip(-1) if slot else c), du + (u.flip(-1) if slot else u)
        out.append((ch, du))
    return out


@pytest.mark.parametrize("shape", [(2, 40, 256, 256, 3),      # sibling level 0 at 256^2: chunked form, 32 chunk carries, batch strides
                                   (1, 40, 224, 320, 3),      # config-5 level 0 (448x640): 35 chunk carries
                                   (1, 80, 112, 160, 5),      # config-5 level 1: L % 2048 != 0, generic chunked kernel
                                   (1, 160, 56, 80, 10),      # config-5 level 2
                                   (1, 80, 128, 128, 5),      # sibling level 1: chunked form with a runtime dt_rank
                                   (1, 18, 32, 32, 10)])      # channel-blocked rows form: grid of 10 (not a multiple of 8), last group 2 of 4 channels
def test_ss2d_scan_long_planes_vs_float64(ops, shape):
    """bem_ss2d_scan on the long planes the shipped nets reach, at a recurrence-dominated operating point (Ds ~ 0.1 N(0,1), dt from
    0.05 to ~1, B and C of unit size: the state term C*h is as large as D*u) against the float64 closed form.  y is held to
    rtol 2e-5 of its largest value and the state term y - D*u on its own to 2e-5 of its largest value, so a carry that is off in one chunk,
    or a state path that is off by 0.01 %, fails (measured on the MI355X: 1.1e-7 .. 1.8e-7 of either).  Forward only (training crops are
    128x128)."""
    B, C, H, W, R = shape
    L = H * W
    g = torch.Generator().manual_seed(L + C)
    x = F.silu(torch.randn(B, C, H, W, generator=g))
    xd0, xd1 = torch.randn(B, 2, R + 2, L, generator=g), torch.randn(B, 2, R + 2, L, generator=g)
    dtw = torch.randn(4, C, R, generator=g) * (0.3 / R ** 0.5)
    dtb = torch.log(torch.expm1(0.05 + 0.95 * torch.rand(4, C, generator=g)))
    A = -torch.exp(0.5 * torch.randn(4 * C, generator=g))
    Ds = 0.1 * torch.randn(4 * C, generator=g)
    xT = x.transpose(2, 3).contiguous()
    d64 = lambda t: t.double()
    (c0, u0), (c1, u1) = _ss2d_fused64(d64(x).view(B, C, L), d64(xT).view(B, C, L), d64(xd0), d64(xd1), d64(dtw), d64(dtb), d64(A), d64(Ds))
    args = [dev(t) for t in (dtw, dtb, A, Ds)]
    y0, y1 = ops.ss2d_scan(dev(x).view(B, C, L), dev(xT).view(B, C, L), dev(xd0), dev(xd1), *args)
    for o, h, c, u in ((0, y0, c0, u0), (1, y1, c1, u1)):
        assert torch.isfinite(h).all()
        e = (h.cpu().double() - u - c).abs().max().item()
        ymax, cmax = (c + u).abs().max().item(), c.abs().max().item()
        print(f"{shape} orientation {o}: max|y| {ymax:.3f} max|C*h| {cmax:.3f} max|D*u| {u.abs().max().item():.3f} | "
              f"max err {e:.2e} = {e / ymax:.1e} max|y| = {e / cmax:.1e} max|C*h|")
        assert e <= 2e-5 * ymax and e <= 2e-5 * cmax, (o, e, ymax, cmax)


# ----------------------------------------------------------------------------- pointwise GEMM ---
@pytest.mark.parametrize("cfg", [(2, 40, 40, 16, 12), (1, 40, 320, 8, 8), (2, 160, 40, 5, 7), (1, 32, 20, 3, 3),
                                 (3, 64, 33, 4, 130), (1, 7, 5, 2, 2), (1, 320, 160, 32, 32)])
def test_pw_gemm_plain_bias_res(ops, cfg):
    """1x1 conv + bias + residual vs F.conv2d.  f32 MFMA = fmaf chain: tolerance 1e-5 * sqrt(K)."""
    B, K, M, H, W = cfg
    g = torch.Generator().manual_seed(K * M)
    x, w = torch.randn(B, K, H, W, generator=g), torch.randn(M, K, generator=g) * K ** -0.5
    b, r = torch.randn(M, generator=g), torch.randn(B, M, H, W, generator=g)
    ref = F.conv2d(x, w[:, :, None, None], b) + r
    y = ops.pw_gemm(dev(x), ops.pack_pw_weight(dev(w)), M, bias=dev(b), res=dev(r))
    close(y, ref, 1e-4, 2e-5, f"pw {cfg}")


def test_pw_gemm_identity_asymmetric(ops):
    """W = I with an asymmetric input catches a transposed C/D mapping (guide section 3)."""
    K = 64
    x = torch.arange(K * 6 * 5, dtype=torch.float32).reshape(1, K, 6, 5)
    y = ops.pw_gemm(dev(x), ops.pack_pw_weight(dev(torch.eye(K))), K)
    assert torch.equal(y.cpu(), x)
    w = torch.zeros(40, 64); w[3, 17] = 2.0; w[39, 0] = -1.0
    y = ops.pw_gemm(dev(x), ops.pack_pw_weight(dev(w)), 40).cpu()
    assert torch.equal(y[0, 3], 2 * x[0, 17]) and torch.equal(y[0, 39], -x[0, 0]) and y[0, 5].abs().max() == 0


@pytest.mark.parametrize("cfg", [(2, 40, 40, 16, 12), (1, 80, 640, 8, 8), (2, 160, 80, 4, 4), (1, 16, 24, 3, 5),
                                 (2, 176, 40, 5, 7), (1, 168, 24, 16, 16), (2, 176, 40, 4, 6, "sum")])
def test_pw_gemm_layernorm(ops, cfg):
    """K <= 160: the register-resident forms.  K > 160 (any net wider than n_feat 40): the streaming form, two sweeps over x for the statistics
    and the parameters in LDS -- first K past the resident form on a ragged odd plane with two M-tiles; a half-filled last k-block with one
    M-tile on the vector path; the sum input."""
    B, K, M, H, W = cfg[:5]
    g = torch.Generator().manual_seed(K + M)
    x = torch.randn(B, K, H, W, generator=g) * 2 + 0.5
    w, lw, lb = torch.randn(M, K, generator=g) * K ** -0.5, torch.randn(K, generator=g), torch.randn(K, generator=g)
    x2 = torch.randn(B, K, H, W, generator=g) if len(cfg) > 5 else None
    ref = F.conv2d(O.layernorm2d_ref(x if x2 is None else x + x2, lw, lb), w[:, :, None, None])
    y = ops.pw_gemm(dev(x), ops.pack_pw_weight(dev(w)), M, x2=None if x2 is None else dev(x2), in_mode=int(x2 is not None), ln=(dev(lw), dev(lb)))
    close(y, ref, 1e-4, 3e-5, f"ln pw {cfg}")


@pytest.mark.parametrize("cfg", [(64, 320, 32, 32, False), (66, 288, 25, 40, False), (3, 1280, 32, 32, False), (2, 512, 7, 9, True), (64, 256, 4, 4, True),
                                 (66, 288, 25, 40, True)])
def test_pw_gemm_layernorm_k160_weights_through_lds(ops, cfg):
    """K = 160 with LayerNorm and >= 8 M-tiles (level-2 project_in, 160 -> 1280): pw_x6_res_lds_kernel -- an M-tile's weights fetched once
    per workgroup by LDS-DMA and shared by its four waves, one barrier per M-tile -- taken when B * L / 32 >= 2048 waves; below that the
    per-wave streaming form with M sliced over grid.y.  Waves past the end of a ragged plane that must keep reaching the barriers, odd plane
    sizes, bias + residual, the sum input, per-sample weights in both forms."""
    B, M, H, W, per_sample = cfg
    K = 160
    g = torch.Generator().manual_seed(M + H)
    x1, x2 = torch.randn(B, K, H, W, generator=g) * 2 + 0.5, torch.randn(B, K, H, W, generator=g)
    lw, lb = torch.randn(K, generator=g), torch.randn(K, generator=g)
    bias, res = torch.randn(M, generator=g), torch.randn(B, M, H, W, generator=g)
    if per_sample:
        w = torch.randn(B, M, K, generator=g) * K ** -0.5
        n = O.layernorm2d_ref(x1, lw, lb)
        ref = torch.stack([F.conv2d(n[i:i + 1], w[i][:, :, None, None])[0] for i in range(B)])
        close(ops.pw_gemm(dev(x1), ops.pack_pw_weight(dev(w)), M, ln=(dev(lw), dev(lb))), ref, 1e-4, 3e-5, f"per-sample weights {cfg}")
        return
    w = torch.randn(M, K, generator=g) * K ** -0.5
    ref = F.conv2d(O.layernorm2d_ref(x1, lw, lb), w[:, :, None, None], bias) + res
    close(ops.pw_gemm(dev(x1), ops.pack_pw_weight(dev(w)), M, ln=(dev(lw), dev(lb)), bias=dev(bias), res=dev(res)), ref, 1e-4, 3e-5, f"ln + bias + res {cfg}")
    ref = F.conv2d(O.layernorm2d_ref(x1 + x2, lw, lb), w[:, :, None, None])
    close(ops.pw_gemm(dev(x1), ops.pack_pw_weight(dev(w)), M, x2=dev(x2), in_mode=1, ln=(dev(lw), dev(lb))), ref, 1e-4, 3e-5, f"sum + ln {cfg}")


def test_pw_gemm_sum_cat_prelu_perbatch(ops):
    g = torch.Generator().manual_seed(5)
    B, C, M, H, W = 3, 24, 40, 6, 10
    x1, x2 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    w, lw, lb = torch.randn(M, C, generator=g) * 0.2, torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.conv2d(O.layernorm2d_ref(x1 + x2, lw, lb), w[:, :, None, None])
    close(ops.pw_gemm(dev(x1), ops.pack_pw_weight(dev(w)), M, x2=dev(x2), in_mode=1, ln=(dev(lw), dev(lb))), ref, 1e-4, 3e-5, "sum+ln")
    w2 = torch.randn(M, 2 * C, generator=g) * 0.2
    a = torch.tensor([0.25])
    ref = F.prelu(F.conv2d(torch.cat([x1, x2], 1), w2[:, :, None, None]), a)
    close(ops.pw_gemm(dev(x1), ops.pack_pw_weight(dev(w2)), M, x2=dev(x2), in_mode=2, prelu=dev(a)), ref, 1e-4, 2e-5, "cat+prelu")
    wb, bb = torch.randn(B, M, C, generator=g) * 0.2, torch.randn(B, M, generator=g)
    ref = torch.stack([F.conv2d(x1[i:i + 1], wb[i][:, :, None, None], bb[i])[0] for i in range(B)])
    close(ops.pw_gemm(dev(x1), ops.pack_pw_weight(dev(wb)), M, bias=dev(bb)), ref, 1e-4, 2e-5, "per-batch weights")


@pytest.mark.parametrize("cfg", [(2, 16, 8, 4, 6), (1, 160, 80, 8, 8), (1, 6, 3, 3, 5)])
def test_conv_transpose_2x2(ops, cfg):
    B, Ci, Co, H, W = cfg
    from bem.modules import ConvT2x2
    torch.manual_seed(Ci)
    m = ConvT2x2(Ci, Co).cuda()
    x = torch.randn(B, Ci, H, W)
    ref = F.conv_transpose2d(x, m.weight.detach().cpu(), m.bias.detach().cpu(), stride=2)
    close(m(dev(x)), ref, 1e-4, 2e-5, f"convT {cfg}")


# ----------------------------------------------------------------------------- convolutions -----
@pytest.mark.parametrize("cfg", [(2, 8, 9, 13), (1, 40, 16, 12), (1, 3, 1, 1), (2, 4, 33, 64),
                                 (2, 8, 16, 64), (1, 6, 8, 8), (2, 4, 32, 128), (1, 4, 4, 4), (1, 2, 8, 256),   # whole-rows-per-wavefront fast form (DPP halo)
                                 (1, 4, 8, 80), (2, 6, 12, 320), (1, 3, 4, 12), (1, 2, 56, 80)])                 # W % 4 == 0, halo columns by clamped loads
def test_dwconv_modes(ops, cfg):
    B, C, H, W = cfg
    g = torch.Generator().manual_seed(C * H)
    x, w, b = torch.randn(B, C, H, W, generator=g), torch.randn(C, 1, 3, 3, generator=g), torch.randn(C, generator=g)
    ref = F.conv2d(x, w, b, padding=1, groups=C)
    close(ops.dwconv3x3(dev(x), dev(w), dev(b), 0), ref, 1e-5, 1e-5, "dw plain")
    close(ops.dwconv3x3(dev(x), dev(w), None, 1), F.silu(F.conv2d(x, w, None, padding=1, groups=C)), 1e-5, 1e-5, "dw silu")
    close(ops.dwconv3x3(dev(x), dev(w), dev(b), 3), x + F.relu(ref), 1e-5, 1e-5, "dw postsmooth")
    if C % 2 == 0:
        a, c = ref.chunk(2, 1)
        close(ops.dwconv3x3(dev(x), dev(w), dev(b), 2), F.gelu(a) * c, 1e-5, 1e-5, "dw gate")
    wb, bb = torch.randn(B, C, 1, 3, 3, generator=g), torch.randn(B, C, generator=g)
    refb = torch.stack([F.conv2d(x[i:i + 1], wb[i], bb[i], padding=1, groups=C)[0] for i in range(B)])
    close(ops.dwconv3x3(dev(x), dev(wb), dev(bb), 0), refb, 1e-5, 1e-5, "dw per-batch")


@pytest.mark.parametrize("cfg", [(2, 32, 32, 16, 20, 3, 1), (1, 11, 40, 9, 33, 3, 1), (1, 40, 16, 8, 8, 3, 1), (2, 40, 80, 16, 12, 4, 2),
                                 (1, 3, 40, 5, 7, 3, 1), (1, 80, 160, 6, 10, 4, 2), (1, 40, 3, 70, 40, 3, 1),
                                 (1, 40, 80, 32, 64, 4, 2), (2, 80, 160, 16, 16, 4, 2), (1, 8, 24, 6, 4, 4, 2), (1, 40, 80, 12, 20, 4, 2)])   # 4x4-s2: row form / f32-MFMA (Wo = 10)
def test_conv2d(ops, cfg, monkeypatch):
    """Dense conv at pad 1 against torch's f32 convolution, whatever form the route gives.  Of the f32-MFMA instantiations these cases reach
    conv2d_mfma_pipe_kernel<3,3,1,2> (11 -> 40 and 3 -> 40) and conv2d_mfma_kernel<4,4,2,3> / <4,4,2,5> (40 -> 80 at 16x12 and 12x20, 80 -> 160 at
    6x10); the other cases run the x6 row and tap forms.  The three-channel slice calls (Cin 3, no bias, no residuals) also pass through
    pipe<3,3,1,1>, pipe<3,3,1,2> and <4,4,2,1|3|5>.  Every instantiation with its epilogue, the other paddings and the direct kernels, against
    float64: tests/test_conv_forms_gpu.py."""
    B, Ci, Co, H, W, k, s = cfg
    g = torch.Generator().manual_seed(Ci * Co)
    x, w, b = torch.randn(B, Ci, H, W, generator=g), torch.randn(Co, Ci, k, k, generator=g) * (Ci * k * k) ** -0.5, torch.randn(Co, generator=g)
    ref = F.conv2d(x, w, b, stride=s, padding=1)
    close(ops.conv2d(dev(x), dev(w), dev(b), stride=s, pad=1), ref, 1e-4, 2e-5, f"conv {cfg}")
    r1 = torch.randn_like(ref)
    close(ops.conv2d(dev(x), dev(w), dev(b), stride=s, pad=1, relu=True, res1=dev(r1), res2=dev(r1)), F.relu(ref) + 2 * r1, 1e-4, 2e-5, "conv relu+res")
    if Ci > 4:
        close(ops.conv2d(dev(x), dev(w[:, 2:5].contiguous()), None, stride=s, pad=1, cin_slice=(2, 3)),
              F.conv2d(x[:, 2:5], w[:, 2:5], None, stride=s, padding=1), 1e-4, 2e-5, "conv channel slice")


@pytest.mark.parametrize("cfg", [(2, 32, 32, 16, 16, True), (1, 40, 16, 9, 14, False), (2, 8, 40, 33, 6, True), (1, 24, 80, 8, 130, False), (1, 32, 32, 128, 128, True)])
def test_conv3x3_x6_taps(ops, cfg):
    """3x3 convolution as nine shifted bf16-limb GEMM taps: borders, half-filled last k-block (Cin % 16 == 8), 1 / 2 / 3 M-tiles, relu +
    two residuals, channel-slice input; against F.conv2d in float64 with the f32 run as the yardstick.  Two of the five cases (W = 16 and
    W = 128, powers of two) are row-form shapes and run that kernel; the other three run the taps."""
    B, Ci, Co, H, W, relu = cfg
    g = torch.Generator().manual_seed(Ci + Co + H)
    x, w, b = torch.randn(B, Ci, H, W, generator=g), torch.randn(Co, Ci, 3, 3, generator=g) * (Ci * 9) ** -0.5, torch.randn(Co, generator=g)
    r1, r2 = torch.randn(B, Co, H, W, generator=g), torch.randn(B, Co, H, W, generator=g)
    def run(dt):
        y = F.conv2d(x.to(dt), w.to(dt), b.to(dt), padding=1)
        return (F.relu(y) if relu else y) + r1.to(dt) + r2.to(dt)
    r64, r32 = run(torch.float64), run(torch.float32)
    xd, wd, r1d, r2d = dev(x), dev(w), dev(r1), dev(r2)
    assert ops.conv2d_route(xd, wd, stride=1, pad=1, res1=r1d, res2=r2d) == ("rows" if W in (16, 128) else "taps")
    y = ops.conv2d(xd, wd, dev(b), stride=1, pad=1, relu=relu, res1=r1d, res2=r2d)
    close(y, r32, 1e-4, 2e-5, f"conv3x3 x6 {cfg}")
    e32 = (r32.double() - r64).abs().mean().item()
    if ops.USE_CONV_X6:        # the limb form's own accuracy claim (the f32-MFMA fallback sits at ~1.3x)
        assert (y.cpu().double() - r64).abs().mean().item() <= 1.2 * e32 + 1e-9
    wide = torch.randn(B, Ci + 6, H, W, generator=g)
    ys = ops.conv2d(dev(wide), dev(w), None, stride=1, pad=1, cin_slice=(4, Ci))
    close(ys, F.conv2d(wide[:, 4:4 + Ci], w, None, padding=1), 1e-4, 2e-5, "conv3x3 x6 channel slice")


# ----------------------------------------------------------------------------- Haar / quaternion -
def test_haar_quaternion_golden(ops):
    g = load_golden("g3_haar")
    close(ops.dwt(dev(g["x"])), g["dwt"], 0, 1e-6, "dwt")
    close(ops.iwt(dev(g["x"])), g["iwt"], 0, 1e-6, "iwt")
    close(ops.hamilton(dev(torch.cat([g["p"], g["q"]], 1))), g["ham"][:, 1:], 0, 1e-6, "hamilton")


def test_quat_dwt_and_iwt_hamilton(ops):
    g = torch.Generator().manual_seed(11)
    x6 = torch.rand(2, 6, 10, 14, generator=g)
    for c0 in (0, 3):
        close(ops.quat_dwt(dev(x6), c0), O.dwt_ref(O.quaternion_stack_ref(x6[:, c0:c0 + 3])), 0, 1e-6, "quat_dwt")
    a, b = torch.randn(2, 16, 5, 7, generator=g), torch.randn(2, 16, 5, 7, generator=g)
    close(ops.iwt_hamilton(dev(a), dev(b)), O.hamilton_ref(O.iwt_ref(a), O.iwt_ref(b))[:, 1:], 1e-6, 1e-6, "iwt_hamilton")
    # round trip at the full config-2 size: IWT(DWT(x)) == x
    x = dev(torch.rand(2, 8, 256, 256, generator=g))
    close(ops.iwt(ops.dwt(x)), x, 0, 1e-6, "haar round trip")


# ----------------------------------------------------------------------------- layout helpers ---
def test_layout_helpers(ops):
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 3, 37, 70, generator=g)
    assert torch.equal(ops.transpose_planes(dev(x)).cpu(), x.transpose(2, 3).contiguous())
    d = torch.zeros(2, 7, 37, 70).cuda()
    ops.copy_channels(dev(x), d, 2, src_c0=1, C=2)
    assert torch.equal(d[:, 2:4].cpu(), x[:, 1:3]) and d[:, :2].abs().max() == 0 and d[:, 4:].abs().max() == 0
    y = torch.randn(2, 4, 6, 8, generator=g)
    s2d = torch.cat([y[:, :, 0::2, 0::2], y[:, :, 1::2, 0::2], y[:, :, 0::2, 1::2], y[:, :, 1::2, 1::2]], 1)
    assert torch.equal(ops.space_to_depth(dev(y)).cpu(), s2d)
    z = torch.randn(2, 8, 5, 3, generator=g)
    assert torch.equal(ops.pixel_shuffle2(dev(z)).cpu(), F.pixel_shuffle(z, 2))
    for s in (2, 16):
        c = torch.rand(2, 3, 4, 5, generator=g)
        close(ops.bilinear_up(dev(c), s), F.interpolate(c, scale_factor=s, mode="bilinear", align_corners=False), 1e-5, 1e-6, f"bilinear x{s}")
    dst = torch.zeros(2, 6, 64, 80).cuda()
    c = torch.rand(2, 3, 4, 5, generator=g)
    ops.bilinear_up(dev(c), 16, dst, 3)
    close(dst[:, 3:], F.interpolate(c, scale_factor=16, mode="bilinear", align_corners=False), 1e-5, 1e-6, "bilinear into slice")
    assert dst[:, :3].abs().max() == 0


# ----------------------------------------------------------------------------- Bayesian / MC ----
def test_bnn_sample(ops):
    g = torch.Generator().manual_seed(13)
    mu, rho, eps = torch.randn(40, 40, generator=g), torch.randn(40, 40, generator=g) - 3, torch.randn(5, 40, 40, generator=g)
    ref = mu + torch.log1p(torch.exp(rho)) * eps
    close(ops.bnn_sample(dev(mu), dev(rho), 5, dev(eps)), ref, 1e-6, 1e-6, "bnn injected eps")
    # Philox path: recover eps, check N(0,1) moments and independence across sets / stream ids
    n = 1 << 16
    z = torch.zeros(n).cuda()
    rho1 = torch.full((n,), float(np.log(np.expm1(1.0)))).cuda()        # softplus(rho) == 1
    e = ops.bnn_sample(z, rho1, 4, None, seed=1234, stream_id=7).cpu()
    assert abs(e.mean()) < 0.01 and abs(e.std() - 1) < 0.01 and abs((e ** 4).mean() - 3) < 0.1
    assert abs(torch.corrcoef(e[:2])[0, 1]) < 0.02
    e2 = ops.bnn_sample(z, rho1, 4, None, seed=1234, stream_id=8).cpu()
    assert not torch.equal(e, e2)
    assert torch.equal(e, ops.bnn_sample(z, rho1, 4, None, seed=1234, stream_id=7).cpu())   # reproducible


def test_mc_postproc_and_finalize(ops):
    g = torch.Generator().manual_seed(14)
    N, h, w = 3, 4, 5
    pred = torch.randn(2 * N, 3, h, w, generator=g) * 0.5 + 0.4
    tmean = torch.rand(2, 3, generator=g)
    noise = torch.randn(2 * N, 3, h, w, generator=g)
    c = pred.clamp(0, 1)
    ratio = tmean.repeat_interleave(N, 0)[:, :, None, None] / c.mean(dim=(2, 3), keepdim=True)
    ref = (c * ratio).clamp(0, 1) + noise * 0.1
    close(ops.cond_postproc(dev(pred), dev(tmean), dev(noise), N, 0.1), ref, 1e-5, 1e-6, "cond postproc")
    close(ops.cond_postproc(dev(pred), None, None, N, 0.1), c, 0, 0, "cond postproc clamp only")
    Hp, Wp, hh, ww = 16, 24, 13, 21
    P = torch.randn(2 * N, 3, Hp, Wp, generator=g) * 0.4 + 0.5
    T = torch.rand(2, 3, hh, ww, generator=g)
    close(ops.plane_mean(dev(P), hh, ww), P[:, :, :hh, :ww].mean(dim=(2, 3)), 1e-5, 1e-6, "plane mean")
    close(ops.plane_mean(dev(P)), P.mean(dim=(2, 3)), 1e-5, 1e-6, "plane mean, whole aligned planes (16-byte loads)")
    close(ops.plane_mean(dev(P[:, :, :, :21].contiguous())), P[:, :, :, :21].mean(dim=(2, 3)), 1e-5, 1e-6, "plane mean, whole planes of odd width")
    fin, ps = ops.candidate_finalize(dev(P), dev(T), N, hh, ww, True)
    for i in range(2 * N):
        q = P[i, :, :hh, :ww].clamp(0, 1).permute(1, 2, 0).numpy()
        t = T[i // N].permute(1, 2, 0).numpy()
        q = np.clip(q * (t.mean(axis=(0, 1), keepdims=True) / q.mean(axis=(0, 1), keepdims=True)), 0, 1)
        close(fin[i].permute(1, 2, 0), q, 1e-5, 1e-6, "final")
        assert abs(ps[i].item() - O.psnr_ref(t, q)) < 1e-3
    fin2, _ = ops.candidate_finalize(dev(P), None, N, hh, ww, False)
    close(fin2, P[:, :, :hh, :ww].clamp(0, 1), 0, 0, "finalize no target")


# ----------------------------------------------------------------------------- error behaviour --
def test_rejects_bad_arguments(ops):
    from bem.native import BemNativeError
    x = torch.randn(1, 4, 4, 4)
    with pytest.raises(BemNativeError):
        ops.dwt(x)                       # CPU tensor: no CPU path
    with pytest.raises(ValueError):
        ops.dwt(dev(torch.randn(1, 4, 5, 4)))
    with pytest.raises(ValueError):
        ops.pw_gemm(dev(x), ops.pack_pw_weight(dev(torch.randn(8, 5))), 8)
    with pytest.raises(BemNativeError):
        ops.conv2d(dev(x), dev(torch.randn(4, 4, 5, 5)), None, stride=1, pad=2)


# ----------------------------------------------------------------------------- fused gdMlp ------
# ----------------------------------------------------------------------------- scan backward ----
@pytest.mark.parametrize("tag", list("abcde"))
def test_selective_scan_bwd_golden(ops, tag):
    """bem_selective_scan_bwd_f32 vs the autograd gradients of the reference's selective_scan_torch (g1 fixtures).
    The reference's own f32 gradient tolerances are rtol 6e-4..6e-3 / atol 2e-3..2e-2 (test_selective_scan.py:398-405,
    490-503); held here at 2e-3 rel / 2e-3 abs of the gradient scale."""
    g = load_golden(f"g1_scan_{tag}")
    D = dev(g["D"]) if "D" in g else None
    b = dev(g["delta_bias"]) if "delta_bias" in g else None
    du, dd, dA, dB, dC, dD, db = ops.selective_scan_bwd(dev(g["u"]), dev(g["delta"]), dev(g["A"]), dev(g["B"]), dev(g["C"]), D, b, dev(g["dout"]), True)
    for name, got in (("du", du), ("ddelta", dd), ("dA", dA), ("dB", dB), ("dC", dC), ("dD", dD), ("dbias", db)):
        if name in g:
            ref = g[name]
            scale = float(ref.abs().max())
            close(got, ref, 2e-3, 2e-3 * max(scale, 1.0) * 0.5, f"{name} [{tag}]")


def test_selective_scan_fn_autograd(ops):
    """The operator seam is differentiable end to end (SelectiveScanHip mirrors SelectiveScanCuda, csms6s.py:75-113)."""
    from basicsr.vmamba.models.csms6s import selective_scan_fn
    g = load_golden("g1_scan_a")
    ins = [dev(g[k]).requires_grad_() for k in ("u", "delta", "A", "B", "C", "D", "delta_bias")]
    y = selective_scan_fn(*ins, True, True)
    close(y, g["y"], 1e-4, 1e-4, "fwd")
    grads = torch.autograd.grad(y, ins, dev(g["dout"]))
    for name, got in zip(("du", "ddelta", "dA", "dB", "dC", "dD", "dbias"), grads):
        close(got, g[name], 2e-3, 2e-3 * max(float(g[name].abs().max()), 1.0) * 0.5, name)


def test_cross_scan_merge_autograd(ops):
    """cross_scan_fn / cross_merge_fn backward against autograd through the oracle restatement."""
    from basicsr.vmamba.models.csm_triton import cross_merge_fn, cross_scan_fn
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 3, 5, 7, generator=g)
    gy = torch.randn(2, 4, 3, 35, generator=g)
    xr = x.clone().requires_grad_()
    ref, = torch.autograd.grad(O.cross_scan_ref(xr), xr, gy)
    xd = dev(x).requires_grad_()
    got, = torch.autograd.grad(cross_scan_fn(xd), xd, dev(gy))
    close(got, ref, 0, 1e-6, "cross_scan backward")
    ys = torch.randn(2, 4, 3, 5, 7, generator=g)
    gm = torch.randn(2, 3, 35, generator=g)
    yr = ys.clone().requires_grad_()
    ref, = torch.autograd.grad(O.cross_merge_ref(yr), yr, gm)
    yd = dev(ys).requires_grad_()
    got, = torch.autograd.grad(cross_merge_fn(yd), yd, dev(gm))
    close(got, ref, 0, 1e-6, "cross_merge backward")


def test_image_prep_kernels(ops):
    """bem_pad_reflect / bem_resize_down / bem_randn / bem_add_channels vs the oracle's numpy / torch forms."""
    g = torch.Generator().manual_seed(31)
    x = torch.rand(2, 3, 60, 52, generator=g)
    pad = ops.pad_reflect(dev(x), 64, 64)
    ref = np.stack([O.pad_reflect_ref(x[i].permute(1, 2, 0).numpy(), 64) for i in range(2)])
    assert np.array_equal(pad.cpu().permute(0, 2, 3, 1).numpy(), ref)
    x_d = dev(x)
    assert ops.pad_reflect(x_d, 60, 52) is x_d                                           # already that size: the input itself, no launch
    close(ops.resize_down(pad, 16), O.cv2_resize_down(pad.cpu(), 16), 0, 1e-7, "resize_down")
    z = ops.randn((1 << 16,), "cuda", seed=7, stream_id=3).cpu()
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02
    assert torch.equal(z, ops.randn((1 << 16,), "cuda", seed=7, stream_id=3).cpu())
    d = dev(torch.ones(2, 4, 5, 6)); sc = torch.rand(2, 6, 5, 6, generator=g)
    ops.add_channels(dev(sc), d, 0, src_c0=3, C=3)
    close(d[:, :3], 1 + sc[:, 3:6], 0, 1e-7, "add_channels"); assert (d[:, 3] == 1).all()


def test_select_best_first_max(ops):
    """ops.select_best (bem_select_scores_f32, rule 3) vs BEMPipeline.select (eval.py:284-285): ties -> first index, negative PSNRs divide by a negative max."""
    from bem.pipeline import BEMPipeline
    rows = [[20.0, 25.5, 25.5, 3.0], [7.0, 7.0, 7.0, 7.0], [-3.0, -1.0, -2.0, -1.0], [100.0, 99.0, 100.0, 1.0], [1.5, 2.5, 3.5, 4.5]]
    ps = dev(torch.tensor(rows).reshape(-1))
    g = torch.Generator().manual_seed(5)
    fin = dev(torch.rand(len(rows) * 4, 3, 6, 5, generator=g))
    best, bp, img = ops.select_best(fin, ps, 4)
    exp = [BEMPipeline.select(r) for r in rows]
    assert best.cpu().tolist() == exp
    assert bp.cpu().tolist() == [pytest.approx(r[e]) for r, e in zip(rows, exp)]
    assert torch.equal(img.cpu(), torch.stack([fin[i * 4 + e].cpu() for i, e in enumerate(exp)]))
    fin2 = dev(torch.rand(4, 3, 3, 3, generator=g))                      # chw not a multiple of 4 -> scalar gather
    b2, _, img2 = ops.select_best(fin2, dev(torch.tensor([1.0, 5.0, 2.0, 9.0])), 2)
    assert b2.cpu().tolist() == [1, 1] and torch.equal(img2.cpu(), fin2[[1, 3]].cpu())


@pytest.mark.parametrize("cfg", [(40, 320, 64, 64, True), (160, 40, 64, 64, False), (80, 640, 32, 32, True), (160, 1280, 16, 16, True),
                                 (640, 160, 16, 16, False), (320, 40, 16, 16, True)])
def test_pw_gemm_x6_accuracy(ops, cfg):
    """The bf16-limb GEMM against a float64 reference: its mean error must not exceed that of torch's own f32 evaluation
    on the CPU (what the reference runs), and it must carry no bias (limb products in two accumulators, pw_gemm_x6.hip)."""
    K, M, H, W, ln = cfg
    g = torch.Generator().manual_seed(K + M)
    x = torch.randn(2, K, H, W, generator=g) * 1.7 + 0.3
    w = torch.randn(M, K, generator=g) * K ** -0.5
    lnp = (torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.1) if ln else None
    b, r = torch.randn(M, generator=g), torch.randn(2, M, H, W, generator=g)

    def run(dt):
        xx = x.to(dt)
        if ln:
            xx = F.layer_norm(xx.permute(0, 2, 3, 1), (K,), lnp[0].to(dt), lnp[1].to(dt), 1e-5).permute(0, 3, 1, 2)
        return F.conv2d(xx, w.to(dt)[:, :, None, None], b.to(dt)) + r.to(dt)
    r64, r32 = run(torch.float64), run(torch.float32)
    y = ops.pw_gemm(dev(x), ops.pack_pw_weight(dev(w), x6=True), M, ln=None if lnp is None else (dev(lnp[0]), dev(lnp[1])), bias=dev(b), res=dev(r))
    d = y.cpu().double() - r64
    e32 = (r32.double() - r64).abs().mean().item()
    assert d.abs().mean().item() <= e32, (d.abs().mean().item(), e32)
    assert abs(d.mean().item()) < 0.1 * e32, ("bias", d.mean().item(), e32)


def test_transpose_plane_slice_and_strided_scan_inputs(ops, monkeypatch):
    """transpose of a channel slice (batch-strided source) and bem_ss2d_scan_strided: x_dbl given as channel slices of a
    wider buffer must give the same result as contiguous copies."""
    g = torch.Generator().manual_seed(77)
    x = torch.randn(3, 7, 5, 9, generator=g)
    t = ops.transpose_plane_slice(dev(x), 2, 4)
    assert torch.equal(t.cpu(), x[:, 2:6].transpose(2, 3).contiguous())
    # transpose_planes_into: the planes land in channels [2, 5) of a wider destination, whose other channels stay as they were
    xs, before = torch.randn(2, 3, 5, 7, generator=g), torch.randn(2, 6, 7, 5, generator=g)
    dst = dev(before)
    assert ops.transpose_planes_into(dev(xs), dst, 2) is dst
    assert torch.equal(dst[:, 2:5].cpu(), xs.transpose(2, 3)) and torch.equal(dst[:, :2].cpu(), before[:, :2]) and torch.equal(dst[:, 5:].cpu(), before[:, 5:])
    launched = []
    with monkeypatch.context() as m:                     # a rejected call launches nothing
        m.setattr(ops.lib(), "bem_transpose_planes_f32", lambda *a: launched.append(a) or 1)
        for bad_dst, c0 in ((dst, 4), (dst, -1), (dev(torch.zeros(2, 6, 5, 7)), 2), (dev(torch.zeros(1, 6, 7, 5)), 2)):
            with pytest.raises(ValueError):              # 4 + 3 > 6 channels; a negative offset; planes not transposed; another batch
                ops.transpose_planes_into(dev(xs), bad_dst, c0)
        with pytest.raises(ValueError):
            ops.transpose_plane_slice(dev(x), 5, 3)      # channels [5, 8) of 7
    assert launched == [] and torch.equal(dst[:, :2].cpu(), before[:, :2]) and torch.equal(dst[:, 5:].cpu(), before[:, 5:])
    B, C, H, W, R = 2, 8, 16, 16, 3
    L = H * W
    x0, x1 = torch.randn(B, C, L, generator=g), torch.randn(B, C, L, generator=g)
    wide = torch.randn(B, 4, R + 2, L, generator=g)
    dtw, dtb = torch.randn(4, C, R, generator=g) * 0.3, torch.randn(4, C, generator=g) - 2
    A, Ds = -torch.rand(4 * C, generator=g), torch.randn(4 * C, generator=g)
    wd = dev(wide)
    a = ops.ss2d_scan(dev(x0), dev(x1), wd[:, :2], wd[:, 2:], dev(dtw), dev(dtb), dev(A), dev(Ds))
    b = ops.ss2d_scan(dev(x0), dev(x1), wd[:, :2].contiguous(), wd[:, 2:].contiguous(), dev(dtw), dev(dtb), dev(A), dev(Ds))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_bnn_sample_packed_equals_sample_then_pack(ops):
    """bem_bnn_sample_pack_x6 = bem_bnn_sample_f32 followed by bem_pack_pw_weight_x6, bit for bit (Philox and injected eps)."""
    g = torch.Generator().manual_seed(3)
    M, K, ns = 40, 23, 3
    mu, rho = torch.randn(M, K, generator=g), torch.randn(M, K, generator=g) - 3
    eps = torch.randn(ns, M, K, generator=g)
    for e in (None, dev(eps)):
        a = ops.bnn_sample_packed(dev(mu), dev(rho), ns, M, K, e, seed=11, stream_id=5)
        b = ops.pack_pw_weight(ops.bnn_sample(dev(mu), dev(rho), ns, e, seed=11, stream_id=5), x6=True)
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
        sigma = ops.bnn_sample(dev(torch.zeros_like(mu)), dev(rho), 1, dev(torch.ones_like(mu)))[0]     # log1p(exp(rho)) by the sampler itself
        c = ops.bnn_sample_packed(dev(mu), sigma, ns, M, K, e, seed=11, stream_id=5, sigma_given=True)
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))


@pytest.mark.parametrize("cfg", [(40, 320, False), (40, 40, True), (160, 40, True)])
def test_pw_gemm_x6_no_sporadic_corruption_at_load(ops, cfg):
    """A full-size launch (config-5 level-0 plane, 224x320 = 71680 pixels) with bias (+ residual): every output within 1e-3 of
    the f32 reference.  An earlier epilogue that read the bias back from LDS as float4 corrupted a few 16-pixel groups per
    10^7 outputs, only at this load; element-wise comparison of the whole tensor catches that class."""
    K, M, use_res = cfg
    g = torch.Generator().manual_seed(K * M)
    x = dev(torch.randn(1, K, 224, 320, generator=g)); w = dev(torch.randn(M, K, generator=g) * K ** -0.5)
    b = dev(torch.randn(M, generator=g)); r = dev(torch.randn(1, M, 224, 320, generator=g)) if use_res else None
    ref = torch.einsum("mk,bkhw->bmhw", w, x) + b[None, :, None, None] + (r if use_res else 0)
    for _ in range(3):
        y = ops.pw_gemm(x, ops.pack_pw_weight(w, x6=True), M, bias=b, res=r)
        assert int(((y - ref).abs() > 1e-3).sum()) == 0


def test_pw_gemm_x6_generic_epilogue_full_size(ops):
    """The generic x6 epilogue (bias through LDS scalars): ConvTranspose2d scatter mode with bias at the config-5 decoder plane
    (80 -> 40 channels, 112x160 -> 224x320) and an M < 8 launch, every output against torch f32 (no test covered
    out_mode 1 / M < 8 element-wise at full size)."""
    g = torch.Generator().manual_seed(123)
    x = torch.randn(2, 80, 112, 160, generator=g)
    w = torch.randn(80, 40, 2, 2, generator=g) * 80 ** -0.5
    b = torch.randn(40, generator=g)
    ref = F.conv_transpose2d(x, w, b, stride=2)
    w4 = w.permute(2, 3, 1, 0).reshape(160, 80).contiguous()
    for _ in range(3):
        y = ops.pw_gemm(dev(x), ops.pack_pw_weight(dev(w4), x6=True), 160, bias=dev(b.repeat(4).contiguous()), convT_Win=160)
        assert y.shape == ref.shape and int(((y.cpu() - ref).abs() > 1e-3).sum()) == 0
    x = torch.randn(1, 40, 224, 320, generator=g)
    w = torch.randn(5, 40, generator=g) * 40 ** -0.5
    b = torch.randn(5, generator=g)
    ref = torch.einsum("mk,bkhw->bmhw", w, x) + b[None, :, None, None]
    y = ops.pw_gemm(dev(x), ops.pack_pw_weight(dev(w), x6=True), 5, bias=dev(b))
    assert int(((y.cpu() - ref).abs() > 1e-3).sum()) == 0


@pytest.mark.parametrize("cfg", [(2, 40, 160, 16, 64, True), (4, 40, 160, 128, 128, True), (2, 24, 32, 13, 45, True), (1, 7, 16, 8, 32, False),
                                 (3, 48, 96, 5, 3, True), (1, 16, 64, 33, 70, True), (2, 80, 320, 64, 64, True), (1, 64, 48, 9, 37, False),
                                 (2, 72, 16, 4, 32, True), (1, 33, 16, 2, 31, True), (1, 40, 160, 5, 33, True)])
def test_gdmlp_x6_vs_chain_and_float64(ops, cfg):
    """bem_gdmlp_x6_f32 (the whole gdMlp branch: LayerNorm + project_in + depthwise 3x3 + GELU gate + project_out + residual, the
    2Hd- and Hd-channel tensors only in LDS) against the three-kernel chain and against torch in float64 (vmamba.py:116-133,1330-1333):
    image borders inside and across the 4 x 32 tiles, ragged planes (5 x 33: a one-pixel tile column under a partial tile row), C not a
    multiple of 16 / 32, no biases, both bench shapes."""
    B, C, Hd, H, W, bias = cfg
    g = torch.Generator().manual_seed(C * Hd + H)
    x = torch.randn(B, C, H, W, generator=g) * 2 + 0.3
    lw, lb = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    wi = torch.randn(2 * Hd, C, generator=g) * C ** -0.5
    bi = 0.3 * torch.randn(2 * Hd, generator=g) if bias else None
    wd = torch.randn(2 * Hd, 1, 3, 3, generator=g) / 3
    bd = 0.2 * torch.randn(2 * Hd, generator=g) if bias else None
    wo = torch.randn(C, Hd, generator=g) * Hd ** -0.5
    bo = 0.3 * torch.randn(C, generator=g) if bias else None
    perm = ops.gate_interleave(Hd, "cpu")
    Wg = ops.pack_pw_weight(dev(wi[perm].contiguous()), x6=True)
    bg = dev(bi[perm].contiguous()) if bias else torch.zeros(2 * Hd, device="cuda")
    w10 = ops.dw_gate_params10(dev(wd), None if bd is None else dev(bd), Hd)
    Wo = ops.pack_pw_weight(dev(wo), x6=True)
    xg = dev(x)
    y = ops.gdmlp_x6(xg, dev(lw), dev(lb), 1e-6, Wg, bg, w10, Wo, None if bo is None else dev(bo), Hd)
    t = ops.pw_gemm(xg, ops.pack_pw_weight(dev(wi), x6=True), 2 * Hd, ln=(dev(lw), dev(lb)), ln_eps=1e-6, bias=None if bi is None else dev(bi))
    chain = ops.pw_gemm(ops.dwconv3x3(t, dev(wd), None if bd is None else dev(bd), 2), Wo, C, bias=None if bo is None else dev(bo), res=xg)
    close(y, chain, 1e-4, 4e-5, f"gdmlp_x6 vs chain {cfg}")
    xd = x.double()
    mu, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
    n = (xd - mu) / (var + 1e-6).sqrt() * lw.double()[None, :, None, None] + lb.double()[None, :, None, None]
    tt = F.conv2d(n, wi.double()[:, :, None, None], None if bi is None else bi.double())
    hh = F.conv2d(tt, wd.double(), None if bd is None else bd.double(), padding=1, groups=2 * Hd)
    ref = (xd + F.conv2d(F.gelu(hh[:, :Hd]) * hh[:, Hd:], wo.double()[:, :, None, None], None if bo is None else bo.double())).float()
    close(y, ref, 1e-4, 4e-5, f"gdmlp_x6 vs torch f64 {cfg}")


@pytest.mark.parametrize("shape", [(2, 40, 128, 128, 3), (1, 80, 64, 64, 5), (2, 160, 32, 32, 10), (1, 6, 16, 64, 10), (1, 5, 256, 16, 5),
                                   (1, 18, 32, 32, 10)])      # grid of 10 workgroups (not a multiple of 8), last group 2 of 4 channels
def test_ss2d_scan_row_major_form(ops, shape):
    """bem_ss2d_scan_rm (orientation 1 staged through LDS, y1 row-major) against the transposed-tensor form: identical
    arithmetic, so the results must agree to the last bit; non-square planes and a partial channel group included."""
    B, C, H, W, R = shape
    g = torch.Generator().manual_seed(H + C)
    L = H * W
    x = dev(torch.randn(B, C, H, W, generator=g))
    xd0, xd1 = dev(torch.randn(B, 2, R + 2, L, generator=g)), dev(torch.randn(B, 2, R + 2, L, generator=g))
    dtw, dtb = dev(torch.randn(4, C, R, generator=g) * 0.3), dev(torch.randn(4, C, generator=g) - 2)
    A, Ds = dev(-torch.rand(4 * C, generator=g)), dev(torch.randn(4 * C, generator=g))
    assert ops.ss2d_scan_rm_supported(H, W, R)
    y0, y1 = ops.ss2d_scan_rm(x, xd0, xd1, dtw, dtb, A, Ds)
    xT = ops.transpose_planes(x)
    r0, r1 = ops.ss2d_scan(x.view(B, C, L), xT.view(B, C, L), xd0, xd1, dtw, dtb, A, Ds)
    assert torch.equal(y0.view(B, C, L), r0)
    assert torch.equal(y1, ops.transpose_planes(r1.view(B, C, W, H)))


# ------------------------------------------------------------------------------------------------------------------
# native seam: the module the reference's csms6s.py imports
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "d", "e"])
def test_selective_scan_cuda_oflex_module(tag):
    """``selective_scan_cuda_oflex.fwd`` / ``.bwd`` called with the reference's own argument lists (csms6s.py:85,101) against the
    outputs and the seven gradients recorded from the reference (g1_scan_*.npz); tolerances of test_selective_scan.py:398-405."""
    import selective_scan_cuda_oflex as ext
    g = load_golden(f"g1_scan_{tag}")
    u, delta, A, B, C = (dev(g[k]) for k in ("u", "delta", "A", "B", "C"))
    D = dev(g["D"]) if "D" in g else None
    bias = dev(g["delta_bias"]) if "delta_bias" in g else None
    out, x, *rest = ext.fwd(u, delta, A, B, C, D, bias, True, 1, True)
    assert out.dtype == torch.float32 and x.shape == (u.shape[0], u.shape[1], (u.shape[2] + 2047) // 2048, 2 * A.shape[1]) and not rest
    close(out, g["y"], 6e-4, 2e-3, "fwd")
    du, dd, dA, dB, dC, dD, db, *rest = ext.bwd(u, delta, A, B, C, D, bias, dev(g["dout"]), x, True, 1)
    for name, got in (("du", du), ("ddelta", dd), ("dA", dA), ("dB", dB), ("dC", dC), ("dD", dD), ("dbias", db)):
        if name in g:
            close(got, g[name], 6e-3, 2e-2, name)
        else:
            assert got is None
    # half-precision inputs: computed in f32, du / ddelta come back in the input dtype, out_float=False returns the input dtype
    o16, _ = ext.fwd(u.half(), delta.half(), A, B.half(), C.half(), D, bias, True, 1, False)
    assert o16.dtype == torch.float16
    with pytest.raises(RuntimeError):
        ext.fwd(u.cpu(), delta.cpu(), A.cpu(), B.cpu(), C.cpu(), None, None, True, 1, True)
    with pytest.raises(RuntimeError):
        ext.fwd(u, delta, A.double(), B, C, D, bias, True, 1, True)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("L", [7, 200, 1000, 4096, 4099])
def test_selective_scan_cuda_oflex_16bit_inputs(dtype, L):
    """float16 / bfloat16 u, delta, B, C at the seam (selective_scan_oflex.cpp:166-216): the forward kernel reads the 16-bit tensors itself and
    must equal, bit for bit, the float32 kernel on the exactly-representable upcast values (every tile shape: 64 / 128 / 256 threads, vector and
    ragged rows); the backward's casts are the library's own kernels and must equal torch's .to() (round to nearest even, NaN kept)."""
    import selective_scan_cuda_oflex as ext
    g = torch.Generator().manual_seed(L)
    Bn, Dm, N, G = 2, 6, 3, 2
    u, delta = dev(torch.randn(Bn, Dm, L, generator=g)).to(dtype), dev(torch.randn(Bn, Dm, L, generator=g) * 0.5).to(dtype)
    A, D, bias = dev(-torch.rand(Dm, N, generator=g) - 0.1), dev(torch.randn(Dm, generator=g)), dev(torch.randn(Dm, generator=g) * 0.1)
    Bm, Cm = dev(torch.randn(Bn, G, N, L, generator=g)).to(dtype), dev(torch.randn(Bn, G, N, L, generator=g)).to(dtype)
    o16, _ = ext.fwd(u, delta, A, Bm, Cm, D, bias, True, 1, True)
    o32, x = ext.fwd(u.float(), delta.float(), A, Bm.float(), Cm.float(), D, bias, True, 1, True)
    assert o16.dtype == torch.float32 and torch.equal(o16, o32)
    olow, _ = ext.fwd(u, delta, A, Bm, Cm, D, bias, True, 1, False)
    assert olow.dtype == dtype and torch.equal(olow, o32.to(dtype))
    dout = dev(torch.randn(Bn, Dm, L, generator=g))
    got = ext.bwd(u, delta, A, Bm, Cm, D, bias, dout.to(dtype), x, True, 1)
    ref = ext.bwd(u.float(), delta.float(), A, Bm.float(), Cm.float(), D, bias, dout.to(dtype).float(), x, True, 1)
    assert got[0].dtype == dtype and got[1].dtype == dtype and got[3].dtype == torch.float32
    assert torch.equal(got[0], ref[0].to(dtype)) and torch.equal(got[1], ref[1].to(dtype))
    for name, a, b in zip(("dA", "dB", "dC", "dD", "dbias"), got[2:], ref[2:]):      # float atomics over the dims of a group / the batch: sum order varies
        close(a, b.cpu().numpy(), 1e-5, 1e-5, name)
    # the casts themselves on awkward values
    v = dev(torch.tensor([0.0, -0.0, 1.0, 65504.0, 7e4, 1e-8, 3.3895314e38, float("inf"), float("nan"), 1.00390625, 1.005859375, 0.1], dtype=torch.float32))
    low = ext._to16(v, dtype)
    want = v.to(dtype)
    assert torch.equal(torch.isnan(low), torch.isnan(want)) and torch.equal(low[~torch.isnan(low)], want[~torch.isnan(want)])
    assert torch.equal(ext._f32(want[~torch.isnan(want)]), want[~torch.isnan(want)].float())


@pytest.mark.parametrize("H,W", [(64, 64), (37, 29), (128, 128), (5, 3)])
def test_attn_stats_f64(H, W):
    """bem_attn_stats_f64 (the Gram matrix and channel sums the folded cross attention of QD/model4.py:99-139 is built from): f64 sums of
    f32 inputs against torch.float64, over chunk boundaries (2048 pixels), ragged tails and unaligned row lengths."""
    from bem import native
    g = torch.Generator().manual_seed(H * 131 + W)
    f1, f2 = dev(torch.randn(3, 32, H, W, generator=g)), dev(torch.randn(3, 32, H, W, generator=g) * 0.5 + 0.1)
    stats = torch.empty(3, 32 * 32 + 64, device=f1.device, dtype=torch.float64)
    native.check(native.lib().bem_attn_stats_f64(ctypes.c_void_p(f1.data_ptr()), ctypes.c_void_p(f2.data_ptr()), ctypes.c_void_p(stats.data_ptr()), 3, H * W,
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "attn_stats")
    a, b = f1.double().reshape(3, 32, -1).cpu(), f2.double().reshape(3, 32, -1).cpu()
    want = torch.cat([torch.einsum("bip,bjp->bij", a, b).reshape(3, -1), a.sum(-1), b.sum(-1)], 1)
    assert torch.allclose(stats.cpu(), want, rtol=1e-12, atol=1e-10), float((stats.cpu() - want).abs().max())


def test_hamilton_product_reference_name():
    from basicsr.QD.quaternion import hamilton_product
    g = load_golden("g3_haar")
    close(hamilton_product(dev(g["p"]), dev(g["q"])), g["ham"], 1e-6, 1e-6, "hamilton_product")


# ------------------------------------------------------------------------------------------------------------------
# selection metrics and rules (eval.py:224-225,268-297,308-314; Enhancement/utils.py:12-57)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,h,w", [(2, 3, 37, 45), (1, 2, 64, 64), (1, 1, 11 + 16, 11 + 1)])
def test_ssim_matches_utils_formula(ops, B, N, h, w):
    """bem_ssim_f32 against the oracle's restatement of calculate_ssim(img_as_ubyte(target), img_as_ubyte(pred)) (float64, 11x11
    Gaussian, valid region).  Tolerance 1e-6: the kernel is float64 too, only the summation order differs."""
    g = torch.Generator().manual_seed(h * w)
    tg = torch.rand(B, 3, h, w, generator=g)
    fin = (tg[:, None] + 0.1 * torch.randn(B, N, 3, h, w, generator=g)).clamp(0, 1).reshape(B * N, 3, h, w)
    got = ops.ssim(dev(fin), dev(tg), N).cpu()
    for bn in range(B * N):
        ref = O.ssim_ref(O.img_as_ubyte_ref(tg[bn // N].permute(1, 2, 0).numpy()), O.img_as_ubyte_ref(fin[bn].permute(1, 2, 0).numpy()))
        assert abs(float(got[bn]) - ref) < 1e-6, (bn, float(got[bn]), ref)


def test_select_scores_rules(ops):
    """Weighted PSNR/SSIM rule, index(max), index(min) -- first index on ties, negative maxima, against eval.py's list arithmetic."""
    g = torch.Generator().manual_seed(5)
    B, N = 6, 5
    ps = torch.rand(B, N, generator=g) * 10 + 15
    ss = torch.rand(B, N, generator=g) * 0.3 + 0.6
    ps[1, 3] = ps[1, 1] = ps[1].max() + 1.0            # tie: the first of the two wins
    ss[1, 3] = ss[1, 1]
    ps[2] = -ps[2]                                      # negative PSNRs: dividing by a negative maximum flips the order, as in the reference
    fin = torch.rand(B * N, 3, 4, 4, generator=g)
    for wgt in (1.0, 0.5, 0.0):
        best, b1, b2, img = ops.select_scores(dev(fin), dev(ps.reshape(-1)), N, dev(ss.reshape(-1)), wgt, "weighted")
        ref = [O.select_ref(ps[b].double().tolist(), ss[b].double().tolist(), wgt) for b in range(B)]
        assert best.cpu().tolist() == ref, (wgt, best.cpu().tolist(), ref)
        assert torch.equal(img.cpu(), torch.stack([fin[b * N + ref[b]] for b in range(B)]))
        assert torch.equal(b1.cpu(), torch.stack([ps[b, ref[b]] for b in range(B)])) and torch.equal(b2.cpu(), torch.stack([ss[b, ref[b]] for b in range(B)]))
    for rule, nr in (("max", "clip"), ("min", "niqe")):
        best = ops.select_scores(None, dev(ps.reshape(-1)), N, rule=rule)[0]
        assert best.cpu().tolist() == [O.select_ref(no_ref_list=ps[b].tolist(), no_ref=nr) for b in range(B)]


def test_mc_mean(ops):
    g = torch.Generator().manual_seed(6)
    B, N, Hp, Wp, h, w = 2, 4, 24, 32, 21, 27
    raw = torch.rand(B * N, 3, Hp, Wp, generator=g) * 1.4 - 0.2
    tg = torch.rand(B, 3, h, w, generator=g)
    for gm in (False, True):
        got = ops.mc_mean(dev(raw), dev(tg), N, h, w, gm).cpu()
        for b in range(B):
            pr = raw[b * N:(b + 1) * N, :, :h, :w].permute(0, 2, 3, 1).numpy()
            ref = O.mc_mean_ref(pr, tg[b].permute(1, 2, 0).numpy(), gm)
            close(got[b].permute(1, 2, 0), torch.from_numpy(ref), 2e-6, 2e-6, f"mc mean gt_mean={gm}")


@pytest.mark.parametrize("cfg", [(2, 40, 80, 128, 128, False), (1, 80, 160, 64, 64, False), (2, 8, 7, 4, 4, False), (1, 24, 33, 6, 16, True),
                                 (3, 16, 40, 2, 128, False), (1, 40, 96, 10, 32, True), (1, 48, 64, 34, 8, False)])
def test_conv4x4s2_coalesced_rows(ops, cfg):
    """The 4x4 stride-2 pad-1 down-sampling conv on the coalesced-row x6 kernel (conv_x6.hip; DecompDualBranchDDWavelet_arch.py:40-41):
    both bench shapes (40 -> 80 at 128x128, 80 -> 160 at 64x64), one / two / three row blocks of output channels incl. an odd count,
    half-filled last k-block (Cin % 16 == 8), output rows of 2 .. 64 pixels (1 .. 32 lanes per row: every DPP neighbour / padding case),
    odd output heights, a partly empty last wave, relu, a channel-slice input; against F.conv2d in float64 with the f32 run as yardstick."""
    B, Ci, Co, H, W, relu = cfg
    g = torch.Generator().manual_seed(Ci + Co + H + W)
    x, w, b = torch.randn(B, Ci, H, W, generator=g), torch.randn(Co, Ci, 4, 4, generator=g) * (Ci * 16) ** -0.5, torch.randn(Co, generator=g)

    def run(dt):
        y = F.conv2d(x.to(dt), w.to(dt), b.to(dt), stride=2, padding=1)
        return F.relu(y) if relu else y
    r64, r32 = run(torch.float64), run(torch.float32)
    xd, wd = dev(x), dev(w)
    assert ops.conv2d_route(xd, wd, stride=2, pad=1) == "rows"
    y = ops.conv2d(xd, wd, dev(b), stride=2, pad=1, relu=relu)
    close(y, r32, 1e-4, 2e-5, f"conv4x4s2 {cfg}")
    e32 = (r32.double() - r64).abs().mean().item()
    e = (y.cpu().double() - r64).abs().mean().item()
    assert e <= 1.5 * e32 + 1e-9, (e, e32)                   # the limb form's accuracy claim: not worse than torch's f32 convolution
    if Ci >= 16:                                             # channels [8, 16) of the wider tensor
        y2 = ops.conv2d(dev(x), dev(w[:, 8:16].contiguous()), None, stride=2, pad=1, cin_slice=(8, 8))
        close(y2, F.conv2d(x[:, 8:16], w[:, 8:16], None, stride=2, padding=1), 1e-4, 2e-5, "conv4x4s2 channel slice")


@pytest.mark.parametrize("cfg", [(2, 32, 32, 128, 128, True), (1, 32, 40, 128, 128, False), (2, 40, 16, 64, 64, True), (1, 8, 7, 5, 4, True),
                                 (3, 24, 33, 3, 8, False), (1, 16, 80, 9, 32, True), (1, 48, 32, 1, 16, False), (1, 32, 32, 37, 128, True)])
def test_conv3x3_row_form(ops, cfg):
    """3x3 stride-1 pad-1 convs on the row-form x6 kernel (conv_x6.hip; QD/model4.py:181-200, DecompDualBranchDDWavelet_arch.py:190):
    the decomposition net's 32 -> 32 at 128x128, first_conv 32 -> 40 and proj 40 -> 16, rows of 4 .. 128 pixels (1 .. 32 lanes per row),
    heights that leave the last wave partly empty, one / two / three row blocks of output channels, half-filled last k-block, relu and
    both residual inputs, a channel-slice input; against F.conv2d in float64 with the f32 run as yardstick."""
    B, Ci, Co, H, W, relu = cfg
    g = torch.Generator().manual_seed(Ci + Co + H + W)
    x, w, b = torch.randn(B, Ci, H, W, generator=g), torch.randn(Co, Ci, 3, 3, generator=g) * (Ci * 9) ** -0.5, torch.randn(Co, generator=g)
    r1, r2 = torch.randn(B, Co, H, W, generator=g), torch.randn(B, Co, H, W, generator=g)

    def run(dt):
        y = F.conv2d(x.to(dt), w.to(dt), b.to(dt), padding=1)
        return (F.relu(y) if relu else y) + r1.to(dt) + r2.to(dt)
    r64, r32 = run(torch.float64), run(torch.float32)
    xd, wd, r1d, r2d = dev(x), dev(w), dev(r1), dev(r2)
    assert ops.conv2d_route(xd, wd, stride=1, pad=1, res1=r1d, res2=r2d) == "rows"
    y = ops.conv2d(xd, wd, dev(b), stride=1, pad=1, relu=relu, res1=r1d, res2=r2d)
    close(y, r32, 1e-4, 2e-5, f"conv3x3 rows {cfg}")
    e32 = (r32.double() - r64).abs().mean().item()
    e = (y.cpu().double() - r64).abs().mean().item()
    assert e <= 1.5 * e32 + 1e-9, (e, e32)
    y0 = ops.conv2d(dev(x), dev(w), None, stride=1, pad=1)                                  # no bias, no residuals
    close(y0, F.conv2d(x, w, None, padding=1), 1e-4, 2e-5, "conv3x3 rows plain")
    if Ci >= 16:
        y2 = ops.conv2d(dev(x), dev(w[:, 8:16].contiguous()), None, stride=1, pad=1, cin_slice=(8, 8))
        close(y2, F.conv2d(x[:, 8:16], w[:, 8:16], None, padding=1), 1e-4, 2e-5, "conv3x3 rows channel slice")


@pytest.mark.parametrize("cfg", [(2, 40, 3, 16, 64, True), (4, 40, 3, 128, 128, False), (2, 24, 2, 13, 45, True), (1, 8, 1, 8, 32, False),
                                 (3, 48, 3, 5, 3, True), (1, 16, 6, 33, 70, True), (1, 32, 2, 4, 32, False), (1, 40, 3, 5, 33, True)])
def test_ss2d_front_x6_vs_chain_and_float64(ops, cfg):
    """bem_ss2d_front_x6_f32 (LayerNorm + in_proj + depthwise 3x3 + SiLU + x_proj in one kernel, the in_proj output only in LDS) against the
    three-kernel chain and against torch in float64 (vmamba.py:700-716,1326): image borders inside and across the 4 x 32 tiles, ragged planes
    (5 x 33: a one-pixel tile column under a partial tile row), C not a multiple of 16, with / without biases, the bench's level-0 shape."""
    B, C, R, H, W, bias = cfg
    Mx = 4 * (R + 2)
    g = torch.Generator().manual_seed(C * Mx + H)
    x = torch.randn(B, C, H, W, generator=g) * 2 + 0.3
    lw, lb = 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    wi = torch.randn(C, C, generator=g) * C ** -0.5
    bi = 0.3 * torch.randn(C, generator=g) if bias else None
    wd = torch.randn(C, 1, 3, 3, generator=g) / 3
    bd = 0.2 * torch.randn(C, generator=g) if bias else None
    wx = torch.randn(Mx, C, generator=g) * C ** -0.5
    Wpi, Wpx = ops.pack_pw_weight(dev(wi), x6=True), ops.pack_pw_weight(dev(wx), x6=True)
    xg = dev(x)
    xc, xd = ops.ss2d_front(xg, dev(lw), dev(lb), 1e-6, Wpi, None if bi is None else dev(bi), dev(wd), None if bd is None else dev(bd), Wpx, Mx)
    t = ops.pw_gemm(xg, Wpi, C, ln=(dev(lw), dev(lb)), ln_eps=1e-6, bias=None if bi is None else dev(bi))
    xc_ref = ops.dwconv3x3(t, dev(wd), None if bd is None else dev(bd), 1)
    xd_ref = ops.pw_gemm(xc_ref, Wpx, Mx)
    close(xc, xc_ref, 1e-4, 4e-5, f"ss2d_front xc vs chain {cfg}")
    close(xd, xd_ref, 1e-4, 4e-5, f"ss2d_front xd vs chain {cfg}")
    xd64 = x.double()
    mu, var = xd64.mean(1, keepdim=True), xd64.var(1, unbiased=False, keepdim=True)
    n = (xd64 - mu) / (var + 1e-6).sqrt() * lw.double()[None, :, None, None] + lb.double()[None, :, None, None]
    tt = F.conv2d(n, wi.double()[:, :, None, None], None if bi is None else bi.double())
    c64 = F.silu(F.conv2d(tt, wd.double(), None if bd is None else bd.double(), padding=1, groups=C))
    close(xc, c64.float(), 1e-4, 4e-5, f"ss2d_front xc vs torch f64 {cfg}")
    close(xd, F.conv2d(c64, wx.double()[:, :, None, None]).float(), 1e-4, 4e-5, f"ss2d_front xd vs torch f64 {cfg}")


@pytest.mark.parametrize("cfg", [(71680, 32, 32, 32, 2), (131072, 32, 64, 0, 0), (71680, 96, 40, 40, 2)])
def test_x6_gemm_bias_epilogue_under_load(ops, cfg):
    """Regression for the round-3 corruption: the decomposition's attention-fuse GEMM (M = 32, K = 32 + 32, cat input) at the config-5 plane
    size launches 280 workgroups, i.e. two on some CUs, and a few times per run 16 outputs of one row (lanes 48..63 of a wave) came out
    WITHOUT their bias: a packed add took the high register of the freshly global-loaded bias pair for its low result and read the
    pair's pre-load content (fixed by a VALU copy, guarded by scripts/isa_audit.py check 2).  Six launches each,
    every output against float64."""
    L, M, K1, K2, mode = cfg
    g = torch.Generator().manual_seed(L + M)
    x1 = dev(torch.randn(1, K1, L, generator=g))
    x2 = dev(torch.randn(1, K2, L, generator=g)) if K2 else None
    W = torch.randn(M, K1 + K2, generator=g) * 0.1
    bias = torch.randn(M, generator=g)
    Wp = ops.pack_pw_weight(dev(W), x6=True)
    xin = torch.cat([x1, x2], 1)[0] if K2 else x1[0]
    ref = (dev(W).double() @ xin.double() + dev(bias).double()[:, None])
    for rep in range(6):
        out = ops.pw_gemm(x1, Wp, M, x2=x2, in_mode=mode, bias=dev(bias))
        bad = int(((out[0].double() - ref).abs() > 1e-4).sum())
        assert bad == 0, f"{cfg} launch {rep}: {bad} outputs off by more than 1e-4"


def test_scratch_buffers_are_kept_per_stream(ops, monkeypatch):
    """The two scratch buffers that outlive a call.  The x6 weight gradient (smallest shape: one 32-pixel chunk, one ragged tile) on the
    current stream and on a second one: both against float64 at test_train_gpu.py::test_pw_wgrad's tolerance, from two scratch tensors.
    NIQE twice on one stream: one workspace, bit-identical scores."""
    import os
    from conftest import GOLDEN
    from bem.scorers import NiqeParams
    monkeypatch.setattr(ops, "_SCRATCH", {})
    monkeypatch.setattr(ops, "WGRAD_X6_MIN_PIXELS", 0)
    B, M, K, L = 1, 8, 8, 32
    g = torch.Generator().manual_seed(11)
    dy, x = torch.randn(B, M, L, generator=g), torch.randn(B, K, L, generator=g)
    ref = torch.einsum("bml,bkl->mk", dy.double(), x.double())
    atol = 3e-6 * float(ref.abs().max()) * max(1.0, (B * L) ** 0.5 / 8)
    dyd, xd = dev(dy), dev(x)
    dw1 = ops.pw_wgrad_(dyd, xd, torch.zeros(M, K, device="cuda"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dw2 = ops.pw_wgrad_(dyd, xd, torch.zeros(M, K, device="cuda"))
    side.synchronize()
    close(dw1, ref, 0.0, atol, "dw on the current stream")
    close(dw2, ref, 0.0, atol, "dw on the side stream")
    bufs = {k: v for k, v in ops._SCRATCH.items() if k[0] == "wgrad_x6"}
    assert {k[2] for k in bufs} == {torch.cuda.current_stream().cuda_stream, side.cuda_stream} and len(bufs) == 2
    assert len({v.data_ptr() for v in bufs.values()}) == 2 and all(v.numel() == 1 << 20 for v in bufs.values())
    params = NiqeParams.load(os.path.join(GOLDEN, "g13_niqe.npz"))
    final = dev(torch.rand(2, 3, 96, 96, generator=g))
    s1 = ops.niqe(final, params)
    (key, ws), = [(k, v) for k, v in ops._SCRATCH.items() if k[0] == "niqe"]
    s2 = ops.niqe(final, params)
    assert [k for k in ops._SCRATCH if k[0] == "niqe"] == [key] and ops._SCRATCH[key] is ws
    assert ops._scratch("niqe", final.device, ws.numel(), torch.uint8).data_ptr() == ws.data_ptr()
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64))         # bit for bit (one 96 x 96 block scores NaN: see ops.niqe)
