"""CPU: the algebra behind the folded decoder level (bem.modules.compose_up_fuse / fold_up_fuse).

fuse(cat(up(pre(f)), skip)) with up = ConvTranspose2d(C, C/2, 2, stride 2), fuse and pre bias-free 1x1 convs is, per output phase (a, b),
    out[:, 2i+a, 2j+b] = Wc[2a+b] f[:, i, j] + Wf2 skip[:, 2i+a, 2j+b] + bc.
Checked in float64 against torch's conv_transpose2d -> cat -> conv2d to 1e-12."""
import pytest
import torch
import torch.nn.functional as F

from bem.modules import ConvT2x2, PwConv2d, compose_up_fuse, fold_up_fuse


def _layers(c, seed, pre):
    g = torch.Generator().manual_seed(seed)
    co = c // 2
    up_w, up_b = torch.randn(c, co, 2, 2, generator=g, dtype=torch.float64), torch.randn(co, generator=g, dtype=torch.float64)
    fuse_w = torch.randn(co, c, 1, 1, generator=g, dtype=torch.float64)
    pre_w = torch.randn(c, c, 1, 1, generator=g, dtype=torch.float64) if pre else None
    return up_w, up_b, fuse_w, pre_w


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("c,h,w", [(14, 3, 5), (80, 4, 6)])
def test_fold_algebra_float64(c, h, w, pre):
    up_w, up_b, fuse_w, pre_w = _layers(c, 100 * c + h, pre)
    g = torch.Generator().manual_seed(7)
    f = torch.randn(2, c, h, w, generator=g, dtype=torch.float64)
    skip = torch.randn(2, c // 2, 2 * h, 2 * w, generator=g, dtype=torch.float64)
    x = F.conv2d(f, pre_w) if pre else f
    want = F.conv2d(torch.cat([F.conv_transpose2d(x, up_w, up_b, stride=2), skip], 1), fuse_w)
    wc, bc, wf2 = compose_up_fuse(up_w, up_b, fuse_w, pre_w)
    assert wc.shape == (4, c // 2, c) and bc.shape == (c // 2,) and wf2.shape == (c // 2, c // 2) and wc.dtype == torch.float64
    got = torch.empty_like(want)
    for a in range(2):
        for b in range(2):
            got[:, :, a::2, b::2] = (torch.einsum("mk,nkij->nmij", wc[2 * a + b], f) + torch.einsum("mc,ncij->nmij", wf2, skip[:, :, a::2, b::2])
                                     + bc[None, :, None, None])
    err = float((got - want).abs().max())
    assert err <= 1e-12 * max(1.0, float(want.abs().max())), err


def test_compose_takes_f32_weights_in_float64():
    """The helper composes from the f32 parameters without rounding in between: the result is the float64 product of the f32 values."""
    up_w, up_b, fuse_w, pre_w = (t.float() for t in _layers(16, 3, True))
    wc, bc, wf2 = compose_up_fuse(up_w, up_b, fuse_w, pre_w)
    wc2, bc2, wf22 = compose_up_fuse(up_w.double(), up_b.double(), fuse_w.double(), pre_w.double())
    assert wc.dtype == torch.float64 and torch.equal(wc, wc2) and torch.equal(bc, bc2) and torch.equal(wf2, wf22)


def test_fold_refuses_a_biased_fuse_or_pre():
    up = ConvT2x2(8, 4)
    with pytest.raises(ValueError):
        fold_up_fuse(up, PwConv2d(8, 4, bias=True), None)
    with pytest.raises(ValueError):
        fold_up_fuse(up, PwConv2d(8, 4, bias=False), PwConv2d(8, 8, bias=True))


def test_fold_refuses_other_widths():
    with pytest.raises(ValueError):
        fold_up_fuse(ConvT2x2(8, 4), PwConv2d(12, 4, bias=False), None)          # a skip that is not C/2 wide
    with pytest.raises(ValueError):
        fold_up_fuse(ConvT2x2(8, 4), PwConv2d(8, 4, bias=False), PwConv2d(6, 8, bias=False))
