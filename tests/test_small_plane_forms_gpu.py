"""GPU: the small-plane forms of the pointwise x6 GEMM (K split over the waves of a workgroup, pw_x6_small_kernel) and of the depthwise 3x3
(several channels per workgroup) against float64 / F.conv2d, at the smallest shapes that reach every branch: planes on either side of
the L <= 32 / 64 / 128 dispatch edges, odd planes (scalar pixel path), ragged last waves, empty and half-filled k-slices, one and several
M-tiles, LayerNorm inside and outside the one-chunk limit, every input / output mode, shared and per-sample weights."""
import pytest
import torch
import torch.nn.functional as F

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


def ln64(x, lw, lb, eps=1e-5):
    """LayerNorm over channels of (B, K, H, W), float64."""
    x = x.double()
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * lw.double()[None, :, None, None] + lb.double()[None, :, None, None]


def gemm64(x, w, bias=None):
    """x (B, K, H, W) float64, w (M, K) or (B, M, K), bias (M) or (B, M) -> (B, M, H, W) float64."""
    w = w.double()
    y = torch.einsum("mk,bkhw->bmhw", w, x.double()) if w.dim() == 2 else torch.einsum("bmk,bkhw->bmhw", w, x.double())
    if bias is not None:
        bias = bias.double()
        y = y + (bias[None, :, None, None] if bias.dim() == 1 else bias[:, :, None, None])
    return y


# 4x4: one 32-pixel wave, 4-way K split; 8x8: one 64-pixel wave, 4-way; 5x5: odd L, scalar pixel path; 7x10: two pixel-waves, 2-way split,
# ragged second wave; 12x16: three pixel-waves and 16x16 (the 256-pixel boundary): the forms for larger planes
PLANES = [(4, 4), (8, 8), (5, 5), (7, 10), (12, 16), (16, 16)]
# 40: 3 k-blocks (K <= 48 keeps the resident form); 80: 5 k-blocks, q = 2, the fourth slice is empty; 160: 10 k-blocks; 168: 11 k-blocks (not
# divisible by 4, half-filled last block; with LayerNorm and a 2-way split outside the one-chunk limit); 320 / 640: several chunks per slice
KS_ = [40, 80, 160, 168, 320, 640]
MS = [28, 40, 160, 320]      # one ragged M-tile, two M-tiles with a ragged last, 5 and 10 M-tiles


@pytest.mark.parametrize("K", KS_)
@pytest.mark.parametrize("plane", PLANES)
def test_small_plane_gemm_vs_float64(ops, plane, K):
    """Per-sample weights and bias (B = 3) with a residual, LayerNorm for K <= 168; shared weights and bias (B = 2) without LayerNorm.
    Bounds of test_pw_gemm_layernorm / test_pw_gemm_sum_cat_prelu_perbatch: rtol 1e-4, atol 3e-5 with LayerNorm, 2e-5 without."""
    H, W = plane
    g = torch.Generator().manual_seed(1000 * K + 10 * H + W)
    ln = K <= 168
    x3 = torch.randn(3, K, H, W, generator=g) * 2 + 0.5
    lw, lb = torch.randn(K, generator=g), torch.randn(K, generator=g)
    x3n = ln64(x3, lw, lb) if ln else x3.double()
    x3d = dev(x3)
    for M in MS:
        w3, b3 = torch.randn(3, M, K, generator=g) * K ** -0.5, torch.randn(3, M, generator=g)
        res = torch.randn(3, M, H, W, generator=g)
        y = ops.pw_gemm(x3d, ops.pack_pw_weight(dev(w3)), M, ln=(dev(lw), dev(lb)) if ln else None, bias=dev(b3), res=dev(res))
        close(y, gemm64(x3n, w3, b3) + res.double(), 1e-4, 3e-5 if ln else 2e-5, f"per-sample {plane} K={K} M={M} ln={ln}")
        w2, b2 = torch.randn(M, K, generator=g) * K ** -0.5, torch.randn(M, generator=g)
        y = ops.pw_gemm(x3d[:2].contiguous(), ops.pack_pw_weight(dev(w2)), M, bias=dev(b2))
        close(y, gemm64(x3[:2], w2, b2), 1e-4, 2e-5, f"shared {plane} K={K} M={M}")


@pytest.mark.parametrize("plane", [(4, 4), (8, 8), (5, 5), (7, 10), (12, 16)])
def test_small_plane_gemm_input_modes(ops, plane):
    """The sum input (with and without LayerNorm: with it, 64-pixel waves stay on the resident forms), the cat input + PReLU with the channel
    seam inside a k-block and inside a wave's slice, per-sample weights."""
    H, W = plane
    g = torch.Generator().manual_seed(7 + H * W)
    B = 3
    for C, M in ((80, 40), (160, 28), (320, 160)):
        x1, x2 = torch.randn(B, C, H, W, generator=g) * 2 + 0.5, torch.randn(B, C, H, W, generator=g)
        w = torch.randn(B, M, C, generator=g) * C ** -0.5
        close(ops.pw_gemm(dev(x1), ops.pack_pw_weight(dev(w)), M, x2=dev(x2), in_mode=1), gemm64(x1.double() + x2.double(), w), 1e-4, 2e-5, f"sum {plane} C={C}")
        if C <= 160:
            lw, lb = torch.randn(C, generator=g), torch.randn(C, generator=g)
            close(ops.pw_gemm(dev(x1), ops.pack_pw_weight(dev(w)), M, x2=dev(x2), in_mode=1, ln=(dev(lw), dev(lb))),
                  gemm64(ln64(x1.double() + x2.double(), lw, lb), w), 1e-4, 3e-5, f"sum + ln {plane} C={C}")
    a = torch.tensor([0.25])
    for C1, C2, M in ((40, 40, 40), (56, 24, 28), (160, 160, 160)):
        x1, x2 = torch.randn(B, C1, H, W, generator=g), torch.randn(B, C2, H, W, generator=g)
        w, b = torch.randn(B, M, C1 + C2, generator=g) * (C1 + C2) ** -0.5, torch.randn(M, generator=g)
        ref = gemm64(torch.cat([x1, x2], 1), w, b)
        ref = torch.where(ref >= 0, ref, 0.25 * ref)
        close(ops.pw_gemm(dev(x1), ops.pack_pw_weight(dev(w)), M, x2=dev(x2), in_mode=2, bias=dev(b), prelu=dev(a)), ref, 1e-4, 2e-5, f"cat + prelu {plane} {C1}+{C2}")


@pytest.mark.parametrize("plane", [(4, 4), (8, 8), (5, 5), (7, 10)])
def test_small_plane_gemm_conv_transpose_output(ops, plane):
    """out_mode 1 (the 2x2 transposed-convolution scatter of the up-sampling GEMMs, K 160 -> 4 x 80 and K 80 -> 4 x 40) through the small form."""
    H, W = plane
    g = torch.Generator().manual_seed(11 + H * W)
    for K, Co in ((160, 80), (80, 40)):
        M = 4 * Co
        x, w, b = torch.randn(3, K, H, W, generator=g), torch.randn(M, K, generator=g) * K ** -0.5, torch.randn(M, generator=g)
        y = gemm64(x, w, b).reshape(3, 2, 2, Co, H, W)                     # row = (2 qy + qx) * Co + co  ->  out[co][2 y + qy][2 x + qx]
        ref = y.permute(0, 3, 4, 1, 5, 2).reshape(3, Co, 2 * H, 2 * W)
        close(ops.pw_gemm(dev(x), ops.pack_pw_weight(dev(w)), M, bias=dev(b), convT_Win=W), ref, 1e-4, 2e-5, f"convT {plane} K={K}")


def test_small_plane_gemm_accuracy_k640(ops):
    """test_pw_gemm_x6_accuracy's criterion at K 640, L 64, where the summation tree changes most (four slices of 10 k-blocks, joined through
    LDS): mean |error| against float64 no larger than that of torch's own f32 evaluation on the CPU, |mean error| below a tenth of it."""
    K, M, H, W = 640, 160, 8, 8
    g = torch.Generator().manual_seed(K + M)
    x = torch.randn(2, K, H, W, generator=g) * 1.7 + 0.3
    w = torch.randn(M, K, generator=g) * K ** -0.5
    b, r = torch.randn(M, generator=g), torch.randn(2, M, H, W, generator=g)

    def run(dt):
        return F.conv2d(x.to(dt), w.to(dt)[:, :, None, None], b.to(dt)) + r.to(dt)
    r64, r32 = run(torch.float64), run(torch.float32)
    y = ops.pw_gemm(dev(x), ops.pack_pw_weight(dev(w), x6=True), M, bias=dev(b), res=dev(r))
    d = y.cpu().double() - r64
    e32 = (r32.double() - r64).abs().mean().item()
    print(f"mean |err| {d.abs().mean().item():.3e} (torch f32 on the CPU {e32:.3e}), mean err {d.mean().item():.3e}")
    assert d.abs().mean().item() <= e32, (d.abs().mean().item(), e32)
    assert abs(d.mean().item()) < 0.1 * e32, ("bias", d.mean().item(), e32)


@pytest.mark.parametrize("cfg", [(640, 160, 8, 8, False), (160, 320, 4, 4, True), (320, 40, 7, 10, False)])
def test_small_plane_gemm_bit_reproducible(ops, cfg):
    """The slices are joined in the fixed order 1, 2, 3 (LayerNorm: the statistics in slice order): the same call twice gives the same bits."""
    K, M, H, W, ln = cfg
    g = torch.Generator().manual_seed(K)
    x, w = dev(torch.randn(64, K, H, W, generator=g)), ops.pack_pw_weight(dev(torch.randn(64, M, K, generator=g) * K ** -0.5))
    lnp = (dev(torch.randn(K, generator=g)), dev(torch.randn(K, generator=g))) if ln else None
    y1 = ops.pw_gemm(x, w, M, ln=lnp)
    y2 = ops.pw_gemm(x, w, M, ln=lnp)
    assert torch.equal(y1, y2)


@pytest.mark.parametrize("C", [6, 70])
@pytest.mark.parametrize("plane", [(4, 4), (8, 8), (16, 16)])
def test_small_plane_dwconv_vs_conv2d(ops, plane, C):
    """256, 64 and 16 channels per workgroup; C = 6 (one partly filled group) and C = 70 (a ragged last group where there are several); mode 2
    pairs channel c with c + C of 2 C input channels.  Modes 0-3, shared and per-sample (B = 3) weights and bias; bounds of test_dwconv_modes."""
    H, W = plane
    B = 3
    g = torch.Generator().manual_seed(C * H)
    x, w, b = torch.randn(B, C, H, W, generator=g), torch.randn(C, 1, 3, 3, generator=g), torch.randn(C, generator=g)
    wb, bb = torch.randn(B, C, 1, 3, 3, generator=g), torch.randn(B, C, generator=g)
    ref = F.conv2d(x, w, b, padding=1, groups=C)
    refb = torch.stack([F.conv2d(x[i:i + 1], wb[i], bb[i], padding=1, groups=C)[0] for i in range(B)])
    close(ops.dwconv3x3(dev(x), dev(w), dev(b), 0), ref, 1e-5, 1e-5, "dw plain")
    close(ops.dwconv3x3(dev(x), dev(wb), dev(bb), 0), refb, 1e-5, 1e-5, "dw plain per-sample")
    close(ops.dwconv3x3(dev(x), dev(w), None, 1), F.silu(F.conv2d(x, w, None, padding=1, groups=C)), 1e-5, 1e-5, "dw silu")
    close(ops.dwconv3x3(dev(x), dev(wb), dev(bb), 1), F.silu(refb), 1e-5, 1e-5, "dw silu per-sample")
    close(ops.dwconv3x3(dev(x), dev(w), dev(b), 3), x + F.relu(ref), 1e-5, 1e-5, "dw postsmooth")
    close(ops.dwconv3x3(dev(x), dev(wb), dev(bb), 3), x + F.relu(refb), 1e-5, 1e-5, "dw postsmooth per-sample")
    # gate: C output channels from 2 C input channels
    x2, w2, b2 = torch.randn(B, 2 * C, H, W, generator=g), torch.randn(2 * C, 1, 3, 3, generator=g), torch.randn(2 * C, generator=g)
    wb2, bb2 = torch.randn(B, 2 * C, 1, 3, 3, generator=g), torch.randn(B, 2 * C, generator=g)
    a, c = F.conv2d(x2, w2, b2, padding=1, groups=2 * C).chunk(2, 1)
    close(ops.dwconv3x3(dev(x2), dev(w2), dev(b2), 2), F.gelu(a) * c, 1e-5, 1e-5, "dw gate")
    a, c = torch.stack([F.conv2d(x2[i:i + 1], wb2[i], bb2[i], padding=1, groups=2 * C)[0] for i in range(B)]).chunk(2, 1)
    close(ops.dwconv3x3(dev(x2), dev(wb2), dev(bb2), 2), F.gelu(a) * c, 1e-5, 1e-5, "dw gate per-sample")
