"""GPU parity of the training step: every backward kernel through the C ABI against torch-CPU
autograd of the oracle's restatement of the same op, the VSSBlock / Stage-II gradients against the fixtures generated from the
reference's own autograd (tests/golden/g4_vssblock.npz, g6_ddw.npz), and clip + AdamW against torch.optim.AdamW.

Tolerances: f32 chains; gradients are compared per tensor as max|err| <= rtol * max|ref| + atol with the rtol written in each test
(the reference's own kernel tests allow rtol 6e-4 .. 6e-3 / atol 2e-3 .. 2e-2 for f32 gradients, test_selective_scan.py:398-405,490-503)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import PKG, load_golden, qd_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bem import native
    native.lib()
    return torch.device("cuda", 0)


def close(a, b, rtol, atol=0.0, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max())
    ref = float(b.abs().max())
    assert err <= rtol * ref + atol, f"{what}: max|err| {err:.3e} vs max|ref| {ref:.3e} (rtol {rtol}, atol {atol})"
    return err


def G(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------- small kernels
def test_l1_loss_and_grad(dev):
    from bem import ops
    g = G(0)
    for shape in ((2, 3, 17, 13), (1, 3, 64, 64)):
        p, t = torch.rand(shape, generator=g), torch.rand(shape, generator=g)
        p[0, 0, 0, 0] = t[0, 0, 0, 0]                       # sign(0) = 0
        pr = p.clone().requires_grad_()
        ref = 0.7 * (pr - t).abs().mean()
        ref.backward(torch.tensor(2.5))
        loss = ops.l1_loss(p.to(dev), t.to(dev), 0.7)
        dp = ops.l1_loss_bwd(p.to(dev), t.to(dev), 0.7, torch.tensor([2.5], device=dev))
        assert abs(float(loss) - float(ref)) <= 1e-6 * abs(float(ref))
        close(dp, pr.grad, 1e-6, what="dpred")


def test_iwt_hamilton_bwd(dev):
    from bem import ops
    from oracle import bem_oracle as O
    g = G(1)
    for (B, h, w) in ((2, 6, 5), (1, 16, 24)):
        a = torch.randn(B, 16, h, w, generator=g, requires_grad=True)
        b = torch.randn(B, 16, h, w, generator=g, requires_grad=True)
        out = O.hamilton_ref(O.iwt_ref(a), O.iwt_ref(b))[:, 1:]
        do = torch.randn(out.shape, generator=g)
        out.backward(do)
        fwd = ops.iwt_hamilton(a.detach().to(dev), b.detach().to(dev))
        close(fwd, out, 1e-6, what="fwd")
        d1, d2 = ops.iwt_hamilton_bwd(a.detach().to(dev), b.detach().to(dev), do.to(dev))
        close(d1, a.grad, 2e-6, what="dq1w")
        close(d2, b.grad, 2e-6, what="dq2w")


def test_pixel_unshuffle_and_sums(dev):
    from bem import ops
    g = G(2)
    x = torch.randn(2, 5, 6, 8, generator=g)
    assert torch.equal(ops.pixel_unshuffle2(x.to(dev)).cpu(), F.pixel_unshuffle(x, 2))
    assert torch.equal(ops.pixel_shuffle2(ops.pixel_unshuffle2(x.to(dev))).cpu(), x)
    acc = torch.full((5,), 0.5, device=dev)
    ops.channel_sum_(x.to(dev), acc)
    close(acc, 0.5 + x.sum(dim=(0, 2, 3)), 1e-5, 1e-5, "channel_sum")
    y = torch.randn(2, 5, 6, 8, generator=g)
    close(ops.add(x.to(dev), y.to(dev), 0.25), x + 0.25 * y, 1e-7, what="add")


@pytest.mark.parametrize("shape", [(2, 40, 16, 12), (1, 7, 9, 5), (2, 160, 8, 8), (1, 80, 33, 20),
                                   (3, 640, 2, 2), (2, 320, 4, 4), (2, 200, 1, 3), (2, 320, 5, 4)])     # C > 160: one workgroup per pixel on planes <= 16 pixels, pixel-per-thread above
@pytest.mark.parametrize("two", [False, True])
def test_ln_bwd(dev, shape, two):
    from bem import ops
    g = G(3)
    B, C, H, W = shape
    x1 = torch.randn(shape, generator=g) * 2 + 0.5
    x2 = torch.randn(shape, generator=g) if two else None
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dn, dres = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    xs = (x1 + x2 if two else x1).clone().requires_grad_()
    gr, br = gam.clone().requires_grad_(), bet.clone().requires_grad_()
    n = F.layer_norm(xs.permute(0, 2, 3, 1), (C,), gr, br, 1e-5).permute(0, 3, 1, 2)
    n.backward(dn)
    dgam, dbet = torch.full((C,), 1.0, device=dev), torch.zeros(C, device=dev)
    dx, nn_ = ops.ln_bwd(x1.to(dev), dn.to(dev), gam.to(dev), bet.to(dev), 1e-5, dgam, dbet, x2=None if x2 is None else x2.to(dev), dres=dres.to(dev))
    close(nn_, n, 2e-6, 2e-6, "LN(x)")
    close(dx, xs.grad + dres, 1e-5, 1e-6, "dx")
    close(dgam, 1.0 + gr.grad, 2e-5, 1e-5, "dgamma (accumulated onto 1)")
    close(dbet, br.grad, 2e-5, 1e-5, "dbeta")
    close(ops.ln_fwd(x1.to(dev), gam.to(dev), bet.to(dev), 1e-5, x2=None if x2 is None else x2.to(dev)), n, 2e-6, 2e-6, "ln_fwd")


@pytest.mark.parametrize("shape", [(2, 8, 16, 12), (1, 6, 9, 7), (2, 4, 32, 32), (1, 2, 5, 3)])
@pytest.mark.parametrize("mode,bias", [(1, False), (1, True), (2, True), (0, True)])
def test_dwact_bwd(dev, shape, mode, bias):
    """dpre, the depthwise weight / bias gradients, and the input gradient = dwconv(dpre, flipped kernel)."""
    from bem import ops
    g = G(4)
    B, Cw, H, W = shape
    Cout = Cw // 2 if mode == 2 else Cw
    t = torch.randn(shape, generator=g, requires_grad=True)
    w = (torch.randn(Cw, 1, 3, 3, generator=g) * 0.4).requires_grad_()
    b = (torch.randn(Cw, generator=g) * 0.3).requires_grad_() if bias else None
    pre = F.conv2d(t, w, b, padding=1, groups=Cw)
    pre.retain_grad()
    if mode == 1:
        out = F.silu(pre)
    elif mode == 2:
        a, c = pre.chunk(2, 1)
        out = F.gelu(a) * c
    else:
        out = pre
    do = torch.randn(B, Cout, H, W, generator=g)
    out.backward(do)
    close(ops.dwconv3x3(t.detach().to(dev), w.detach().to(dev), None if b is None else b.detach().to(dev), mode=mode), out, 5e-6, 1e-6, "forward")
    dw = torch.zeros(Cw, 1, 3, 3, device=dev)
    db = torch.zeros(Cw, device=dev) if bias else None
    dpre = ops.dwact_bwd(t.detach().to(dev), w.detach().to(dev), None if b is None else b.detach().to(dev), do.to(dev), dw, db, mode)
    close(dpre, pre.grad, 2e-5, 1e-6, "dpre")
    close(dw, w.grad, 5e-5, 1e-5, "dw")
    if bias:
        close(db, b.grad, 5e-5, 1e-5, "dbias")
    dt = ops.dwconv3x3(dpre, w.detach().flip(2, 3).contiguous().to(dev), None, mode=0)
    close(dt, t.grad, 3e-5, 1e-6, "dt")


@pytest.mark.parametrize("B,M,C1,C2,L", [(2, 40, 40, 0, 192), (1, 320, 40, 0, 1024), (2, 20, 40, 0, 77), (3, 80, 80, 80, 130), (1, 640, 160, 0, 64),
                                         (2, 33, 7, 0, 31), (1, 160, 320, 0, 100), (2, 16, 64, 0, 256), (3, 80, 80, 80, 144), (4, 320, 40, 0, 4096),
                                         (2, 40, 160, 0, 1024), (5, 7, 33, 0, 16)])
@pytest.mark.parametrize("form", ["x6", "f32"])
def test_pw_wgrad(dev, B, M, C1, C2, L, form, monkeypatch):
    """Both weight-gradient forms on every shape: bem_pw_wgrad_x6_f32 (L % 32 == 0; operands straight into the bf16 matrix cores, normally
    chosen for launches of >= 16384 pixels) and bem_pw_wgrad_f32."""
    from bem import ops
    if form == "x6" and L % 32:
        pytest.skip("the x6 form needs L % 32 == 0")
    monkeypatch.setattr(ops, "WGRAD_X6_MIN_PIXELS", 0 if form == "x6" else 1 << 62)
    g = G(5)
    dy = torch.randn(B, M, L, generator=g)
    x1 = torch.randn(B, C1, L, generator=g)
    x2 = torch.randn(B, C2, L, generator=g) if C2 else None
    xx = torch.cat([x1, x2], 1) if C2 else x1
    ref = torch.einsum("bml,bkl->mk", dy.double(), xx.double())
    dw = torch.full((M, C1 + C2), 0.25, device=dev)
    db = torch.zeros(M, device=dev)
    ops.pw_wgrad_(dy.to(dev), x1.to(dev), dw, x2=None if x2 is None else x2.to(dev), dbias=db)
    scale = float(ref.abs().max())
    close(dw, 0.25 + ref, 0.0, 3e-6 * scale * max(1.0, (B * L) ** 0.5 / 8), "dw (accumulated onto 0.25)")
    close(db, dy.double().sum(dim=(0, 2)), 0.0, 1e-5 * float(dy.abs().sum(dim=(0, 2)).max()), "dbias")


@pytest.mark.parametrize("form", ["x6", "f32"])
def test_pw_wgrad_row_blocks_and_strided_dy(dev, form, monkeypatch):
    """The stacked x_proj form: dy is a channel slice of a wider tensor and the row blocks of dw are permuted ([0,2,1,3])."""
    from bem import ops
    monkeypatch.setattr(ops, "WGRAD_X6_MIN_PIXELS", 0 if form == "x6" else 1 << 62)
    g = G(6)
    B, R2, C, L = 2, 5, 40, 192
    wide = torch.randn(B, 4 * R2 + 3, L, generator=g)
    x = torch.randn(B, C, L, generator=g)
    ref = torch.einsum("bml,bkl->mk", wide[:, :4 * R2].double(), x.double()).view(4, R2, C)[[0, 2, 1, 3]]
    dw = torch.zeros(4, R2, C, device=dev)
    wd = wide.to(dev)
    ops.pw_wgrad_(wd, x.to(dev), dw, blk_rows=R2, perm=(0, 2, 1, 3), dy_bstride=wd.stride(0), M=4 * R2)
    close(dw, ref, 0.0, 1e-5 * float(ref.abs().max()), "permuted row blocks")


@pytest.mark.parametrize("B,Cin,H,W,Cout,k,s,p", [(2, 8, 12, 10, 16, 3, 1, 1), (1, 32, 16, 16, 40, 3, 1, 1), (2, 16, 16, 12, 32, 4, 2, 1),
                                                   (1, 40, 32, 32, 80, 4, 2, 1), (1, 3, 9, 7, 5, 3, 1, 1)])
def test_conv_wgrad_and_input_grad(dev, B, Cin, H, W, Cout, k, s, p):
    from bem import autograd as ag, ops
    g = G(7)
    x = torch.randn(B, Cin, H, W, generator=g, requires_grad=True)
    w = (torch.randn(Cout, Cin, k, k, generator=g) * 0.2).requires_grad_()
    b = torch.randn(Cout, generator=g, requires_grad=True)
    out = F.conv2d(x, w, b, stride=s, padding=p)
    do = torch.randn(out.shape, generator=g)
    out.backward(do)
    dw, db = torch.zeros(Cout, Cin, k, k, device=dev), torch.zeros(Cout, device=dev)
    ops.conv_wgrad_(do.to(dev), x.detach().to(dev), dw, db, stride=s, pad=p)
    close(dw, w.grad, 0.0, 2e-5 * float(w.grad.abs().max()), "dw")
    close(db, b.grad, 0.0, 2e-5 * float(b.grad.abs().max()), "dbias")
    wd = w.detach().to(dev)
    if k == 3:
        dx = ops.conv2d(do.to(dev), ops.ConvWeight(wd).input_grad(), None, stride=1, pad=1)
    else:
        dx = ops.pixel_shuffle2(ops.conv2d(do.to(dev), ag._wT4(wd), None, stride=1, pad=1))
    close(dx, x.grad, 0.0, 3e-5 * float(x.grad.abs().max()), "dx")


# ---------------------------------------------------------------------------------------------- fused SS2D backward
def _scan_blocked(u, delta, A, Bm, Cm, D, delta_bias, blk=256):
    """The selective-scan recurrence h_t = a_t h_{t-1} + dt_t B_t u_t, y_t = C_t h_t + D u_t (d_state 1) in float64 and closed form per block
    of 256 steps (h_t = sum_{s <= t} exp(cl_t - cl_s) b_s + exp(cl_t) h_in, cl = running sum of log a inside the block): the same function
    as the oracle's per-step loop, differentiable, and minutes faster at L = 16384.  Checked against that loop below."""
    Bn, C, L = u.shape
    dt = F.softplus(delta.double() + delta_bias.double()[None, :, None])
    la, bu = dt * A.double().view(1, C, 1), dt * Bm.double().view(Bn, 1, L) * u.double()
    h, ys = torch.zeros(Bn, C, dtype=torch.float64), []
    tri = torch.tril(torch.ones(blk, blk, dtype=torch.bool))
    for s0 in range(0, L, blk):
        e0 = min(L, s0 + blk)
        cl = torch.cumsum(la[:, :, s0:e0], -1)
        n = e0 - s0
        M = torch.exp((cl[:, :, :, None] - cl[:, :, None, :]).masked_fill(~tri[:n, :n], -float("inf")))
        hb = torch.einsum("bcts,bcs->bct", M, bu[:, :, s0:e0]) + torch.exp(cl) * h[:, :, None]
        ys.append(hb)
        h = hb[:, :, -1]
    return (torch.cat(ys, -1) * Cm.double().view(Bn, 1, L) + D.double()[None, :, None] * u.double()).float()


def _ss2d_torch(x0, x1, xd0, xd1, dtw, dtb, A, Ds, blocked=False):
    """The fused op restated with the oracle's scan (autograd-capable): returns y0 (row-major order), y1 (transposed order)."""
    from oracle import bem_oracle as O
    B, C, L = x0.shape
    R = dtw.shape[2]
    ys = []
    for o, (x, xd) in enumerate(((x0, xd0), (x1, xd1))):
        y = 0
        for slot, k in enumerate((o, o + 2)):
            rev = slot == 1
            xs, d = (x.flip(-1), xd[:, slot].flip(-1)) if rev else (x, xd[:, slot])
            dts = torch.einsum("cr,brl->bcl", dtw[k], d[:, :R])
            if blocked:
                yk = _scan_blocked(xs, dts, A[k * C:(k + 1) * C], d[:, R], d[:, R + 1], Ds[k * C:(k + 1) * C], dtb[k])
            else:
                yk = O.selective_scan_ref(xs, dts, A[k * C:(k + 1) * C].view(C, 1), d[:, R].reshape(B, 1, 1, L), d[:, R + 1].reshape(B, 1, 1, L),
                                          Ds[k * C:(k + 1) * C], dtb[k], True)
            y = y + (yk.flip(-1) if rev else yk)
        ys.append(y)
    return ys


_SCAN_BWD = [(2, 8, 192, 3), (1, 5, 77, 2), (1, 4, 1030, 1), (1, 3, 4100, 3), (1, 2, 9000, 2),
             (3, 7, 64, 5), (2, 6, 16, 10), (2, 3, 4, 10), (1, 4, 256, 3), (1, 4, 300, 3),       # Stage-I planes: one wavefront per row
             # whole-row channel-blocked forms (full and partial channel groups)
             (2, 5, 1024, 2), (1, 6, 1024, 1), (1, 5, 4096, 3), (1, 9, 1024, 5), (1, 3, 256, 10), (1, 5, 16384, 3)]
# the two whole-row forms without a case above: (L = 4096, R = 5) and (L = 1024, R = 10)
_SCAN_BWD_ROWS = [(1, 5, 4096, 5), (1, 3, 1024, 10)]
# x_dbl as the training path hands it over (bem/autograd.py: xd.view(B,4,M,L)[:, :2], twice the contiguous batch stride), B = 2: the
# workgroup-per-channel kernel (L = 16), the wavefront-per-row one (64), the 256- and 1024-thread tiled ones (300, 4100), a whole-row form
_SCAN_BWD_STRIDED = [(2, 6, 16, 10), (2, 7, 64, 5), (2, 4, 300, 3), (2, 3, 4100, 3), (2, 5, 1024, 2)]


@pytest.mark.parametrize("B,C,L,R,strided", [c + (False,) for c in _SCAN_BWD + _SCAN_BWD_ROWS] + [c + (True,) for c in _SCAN_BWD_STRIDED],
                         ids=["-".join(map(str, c)) for c in _SCAN_BWD + _SCAN_BWD_ROWS] + ["-".join(map(str, c)) + "-strided" for c in _SCAN_BWD_STRIDED])
def test_ss2d_scan_bwd(dev, B, C, L, R, strided):
    from bem import ops
    added = strided or (B, C, L, R) in _SCAN_BWD_ROWS       # the later cases take the blocked reference throughout: seconds, not minutes
    g = G(8)
    x0 = torch.randn(B, C, L, generator=g, requires_grad=True)
    x1 = torch.randn(B, C, L, generator=g, requires_grad=True)
    xd0 = (torch.randn(B, 2, R + 2, L, generator=g) * 0.7).requires_grad_()
    xd1 = (torch.randn(B, 2, R + 2, L, generator=g) * 0.7).requires_grad_()
    dtw = (torch.randn(4, C, R, generator=g) * 0.5).requires_grad_()
    dtb = (torch.randn(4, C, generator=g) * 0.5 - 1.0).requires_grad_()
    Alog = (torch.rand(4 * C, 1, generator=g) - 1.5).requires_grad_()        # A = -exp(A_logs) in (-0.6, -0.2)
    Ds = torch.randn(4 * C, generator=g, requires_grad=True)
    A = -torch.exp(Alog).view(-1)
    # L >= 8192: the per-step loop of the oracle takes minutes under autograd; the blocked closed form of the same recurrence stands in for it
    # (L = 300 runs both and compares them)
    y0, y1 = _ss2d_torch(x0, x1, xd0, xd1, dtw, dtb, A, Ds, blocked=L >= 8192 or added)
    if L == 300 and not added:
        with torch.no_grad():
            z0, z1 = _ss2d_torch(x0, x1, xd0, xd1, dtw, dtb, A, Ds, blocked=True)
        close(z0, y0, 1e-5, 1e-6, "blocked reference vs loop"); close(z1, y1, 1e-5, 1e-6, "blocked reference vs loop")
    dy0, dy1 = torch.randn(B, C, L, generator=g), torch.randn(B, C, L, generator=g)
    (y0 * dy0).sum().add((y1 * dy1).sum()).backward()
    d = lambda t: t.detach().to(dev).contiguous()
    if strided:
        wide = [torch.full((B, 4, R + 2, L), 3.5, device=dev) for _ in range(2)]
        for w_, t in zip(wide, (xd0, xd1)):
            w_[:, :2].copy_(t.detach())
        xdv = {id(xd0): wide[0][:, :2], id(xd1): wide[1][:, :2]}
        assert xdv[id(xd0)].stride(0) == 2 * xd0.stride(0) and not xdv[id(xd0)].is_contiguous()
        dc, d = d, lambda t: xdv[id(t)] if id(t) in xdv else dc(t)
    f0, f1 = ops.ss2d_scan(d(x0), d(x1), d(xd0), d(xd1), d(dtw), d(dtb), d(A), d(Ds))
    close(f0, y0, 2e-4, 1e-5, "fwd y0"); close(f1, y1, 2e-4, 1e-5, "fwd y1")
    dAl, dDs = torch.zeros(4 * C, device=dev), torch.zeros(4 * C, device=dev)
    ddtw, ddtb = torch.zeros(4, C, R, device=dev), torch.zeros(4, C, device=dev)
    dx0, dx1, dxd0, dxd1 = ops.ss2d_scan_bwd(d(x0), d(x1), d(xd0), d(xd1), d(dy0), d(dy1), d(dtw), d(dtb), d(A), d(Ds), dAl, dDs, ddtw, ddtb)
    rt = 1e-3     # reference tolerance for f32 gradients: rtol 6e-4 .. 6e-3 (test_selective_scan.py:398-405)
    close(dx0, x0.grad, rt, 1e-5, "dx0"); close(dx1, x1.grad, rt, 1e-5, "dx1")
    close(dxd0, xd0.grad, rt, 1e-5, "dxd0"); close(dxd1, xd1.grad, rt, 1e-5, "dxd1")
    close(dAl, Alog.grad.view(-1), rt, 1e-4, "dA_logs"); close(dDs, Ds.grad, rt, 1e-4, "dDs")
    close(ddtw, dtw.grad, rt, 1e-4, "ddt_projs_weight"); close(ddtb, dtb.grad, rt, 1e-4, "ddt_projs_bias")


# ---------------------------------------------------------------------------------------------- blocks and nets
def test_vssblock_backward_golden(dev):
    """VSSBlock C = 40 on 16x12: dx and the parameter gradients recorded from the REFERENCE's autograd (g4_vssblock.npz)."""
    from bem.modules import VSSBlock
    g = load_golden("g4_vssblock")
    blk = VSSBlock(hidden_dim=40, ssm_d_state=1, ssm_ratio=1, ssm_conv_bias=False, forward_type="v05_noz", mlp_ratio=4, mlp_type="gdmlp",
                   channel_first=True).to(dev)
    blk.load_state_dict(g["sd"], strict=True)
    blk.train()
    x = g["x"].to(dev).requires_grad_()
    y = blk(x)
    close(y, g["y"], 2e-5, 1e-5, "forward")
    y.backward(g["dout"].to(dev))
    close(x.grad, g["dx"], 1e-3, 1e-5, "dx")
    params = dict(blk.named_parameters())
    for k, ref in g["grads"].items():
        close(params[k].grad, ref, 2e-3, 1e-5 * float(ref.abs().max()) + 1e-7, k)


@pytest.mark.parametrize("wgrad_form", ["default", "x6"])
def test_vssblock_backward_all_grads_vs_oracle(dev, wgrad_form, monkeypatch):
    """Every parameter gradient of the block against autograd through the oracle (pinned to the reference by the test above
    and by tests/test_oracle_golden.py), on a plane with odd sizes (general kernels) and on 32x32 (row-major scan form).  'x6' forces
    the bf16-matrix-core weight-gradient kernel wherever L % 32 == 0 (by default it takes launches of >= 16384 pixels only): all its
    call forms inside the block -- LayerNorm-ed input, strided dy with permuted row blocks (x_proj), bias sums."""
    from bem import ops
    from bem.modules import VSSBlock
    from oracle import bem_oracle as O
    if wgrad_form == "x6":
        monkeypatch.setattr(ops, "WGRAD_X6_MIN_PIXELS", 0)
    sd0 = load_golden("g4_vssblock")["sd"]
    for (H, W), seed in (((9, 7), 11), ((32, 32), 12)):
        g = G(seed)
        blk = VSSBlock(hidden_dim=40, ssm_d_state=1, ssm_ratio=1, ssm_conv_bias=False, forward_type="v05_noz", mlp_ratio=4, mlp_type="gdmlp",
                       channel_first=True).to(dev)
        blk.load_state_dict(sd0, strict=True)
        blk.train()
        x = torch.randn(2, 40, H, W, generator=g)
        do = torch.randn(2, 40, H, W, generator=g)
        sd = {k: v.clone().requires_grad_() for k, v in sd0.items()}
        xr = x.clone().requires_grad_()
        O.vssblock_ref(sd, "", xr).backward(do)
        xd = x.to(dev).requires_grad_()
        blk(xd).backward(do.to(dev))
        close(xd.grad, xr.grad, 1e-3, 1e-5, "dx")
        for k, p in blk.named_parameters():
            ref = sd[k].grad
            close(p.grad, ref, 3e-3, 2e-5 * float(ref.abs().max()) + 1e-7, f"{H}x{W} {k}")


def _load_stage2(name, g, dev, n_feat=16, num_blocks=(2, 1, 1), decomp="model4"):
    from basicsr.archs import build_network
    net = build_network(dict(type=name, in_channels=6, out_channels=3, n_feat=n_feat, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp",
                             use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=list(num_blocks), decomp_model=decomp))
    missing, unexpected = net.load_state_dict(g["sd"], strict=False)
    assert not unexpected and all(k.startswith("decomp.") for k in missing), (missing, unexpected)
    return net.to(dev)


def test_stage2_training_gradients_golden(dev):
    """DecompDualBranchDDWavelet (reduced width) 1x6x64x64, L1 loss: loss, total gradient norm and the recorded gradients of the
    REFERENCE's training step (g6_ddw.npz), then every gradient against the oracle's autograd."""
    from bem import autograd as ag
    from oracle import bem_oracle as O
    g = load_golden("g6_ddw")
    net = _load_stage2("DecompDualBranchDDWavelet", g, dev)
    net.train()
    x, gt = g["x"].to(dev), g["gt"].to(dev)
    out = net(x)[-1]
    close(out, g["out"], 2e-4, 2e-5, "forward (train mode)")
    loss = ag.l1_loss(out, gt)
    assert abs(float(loss) - float(g["loss"])) < 2e-6
    loss.backward()
    named = {k: p for k, p in net.named_parameters() if p.requires_grad}
    assert all(p.grad is not None for p in named.values())
    gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in named.values())))
    assert abs(gn - float(g["grad_norm"])) < 2e-4 * float(g["grad_norm"]), (gn, float(g["grad_norm"]))
    sd = {**{k: v.clone().requires_grad_() for k, v in g["sd"].items()}, **qd_state_dict("model4")}
    (O.ddwavelet_ref(sd, g["x"]) - g["gt"]).abs().mean().backward()
    gmax = max(float(sd[k].grad.abs().max()) for k in named)
    worst = 0.0
    for k, p in named.items():
        ref = sd[k].grad
        # per tensor: 0.5 % of its own largest entry, floored at 1e-5 of the largest gradient entry of the net
        worst = max(worst, close(p.grad, ref, 5e-3, 1e-5 * gmax, k) / (float(ref.abs().max()) + 1e-5 * gmax))
    for k, ref in g["grads"].items():
        close(named[k].grad, ref, 5e-3, 1e-5 * gmax, "reference fixture " + k)
    print(f"stage-II gradients: worst per-tensor relative error {worst:.2e}, grad norm {gn:.6f} (reference {float(g['grad_norm']):.6f})")


def test_adamw_and_clip_match_torch(dev):
    from bem.train import BemAdamW
    g = G(20)
    shapes = [(7, 5), (33,), (4, 3, 3, 3), (1,), (128, 40)]
    ps_ref = [torch.randn(s, generator=g).requires_grad_() for s in shapes]
    ps = [torch.nn.Parameter(p.detach().clone().to(dev)) for p in ps_ref]
    ref = torch.optim.AdamW(ps_ref, lr=2e-3, betas=(0.9, 0.999), weight_decay=1e-2)
    opt = BemAdamW(ps, lr=2e-3, betas=(0.9, 0.999), weight_decay=1e-2)
    for step in range(4):
        ref.zero_grad(); opt.zero_grad()
        for pr, pd in zip(ps_ref, ps):
            gr = torch.randn(pr.shape, generator=g) * (3.0 if step % 2 == 0 else 0.01)     # clipping active / inactive
            pr.grad = gr.clone()
            pd.grad.copy_(gr.to(dev))
        n_ref = torch.nn.utils.clip_grad_norm_(ps_ref, 1.0)
        n_dev = opt.clip_grad_norm_(1.0)
        ref.step(); opt.step()
        assert abs(float(n_dev) - float(n_ref)) <= 1e-5 * float(n_ref)
        for pr, pd in zip(ps_ref, ps):
            close(pd, pr, 2e-6, 1e-7, f"step {step} parameter")
            close(pd.grad, pr.grad, 2e-6, 1e-8, f"step {step} clipped gradient")


def test_image_enhancer_train_step_matches_oracle(dev):
    """ImageEnhancer.optimize_parameters (registry seam, option-file driven) for two steps against the oracle's restatement of
    image_enhancer_model.py:165-216 on the same weights, inputs and conditions: loss, gradient norm, parameters after the steps."""
    from basicsr.models import build_model
    from oracle import bem_oracle as O
    g = load_golden("g6_ddw")
    opt = dict(model_type="ImageEnhancer", is_train=True, num_gpu=1, dist=False, condition=dict(type="mean", scale_down=16, noise_level=0.0),
               network_g=dict(type="DecompDualBranchDDWavelet", in_channels=6, out_channels=3, n_feat=16, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                              mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[2, 1, 1], decomp_model="model4"),
               path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None),
               train=dict(total_iter=10, warmup_iter=-1, max_grad_norm=1, use_amp=False,
                          scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=[6, 4], restart_weights=[1, 1], eta_mins=[0.0002, 0.000001]),
                          optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]),
                          pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean")))
    lq, gt = g["x"][:, :3], g["gt"]
    gen = G(33)
    gt_down = F.interpolate(gt, scale_factor=1 / 16, mode="bilinear") + 0.1 * torch.randn(1, 3, 4, 4, generator=gen)
    sd = {**g["sd"], **qd_state_dict("model4")}
    ref = O.train_step_ref(sd, lq, gt, gt_down, steps=2, lr=2e-4, weight_decay=1e-4, max_grad_norm=1.0)
    model = build_model(opt)                 # is_train: the flat parameter / gradient buffers exist from here on
    model.net_g.load_state_dict(g["sd"], strict=False)      # copies into the flat buffer's views
    for it in range(2):
        model.feed_train_data(dict(lq=lq, gt=gt, gt_down=gt_down))
        tn = model.optimize_parameters(it + 1)
        assert abs(float(model.log_dict["l_pix"]) - ref["loss"][it]) < 3e-6, (it, float(model.log_dict["l_pix"]), ref["loss"][it])
        assert abs(float(tn) - ref["grad_norm"][it]) < 5e-4 * ref["grad_norm"][it], (it, float(tn), ref["grad_norm"][it])
    named = dict(model.net_g.named_parameters())
    # Adam's first steps are sign-like (update = lr * g / (|g| + eps)): an element whose gradient is at rounding level may move the
    # other way.  Hold the UPDATE (not just the weight) to 5 % on all but a small fraction of the elements, and every weight to
    # the size of one full update.
    bad = tot = 0
    for k, v in ref["params"].items():
        u_ref, u_dev = (v - sd[k]).double(), (named[k].detach().cpu() - sd[k]).double()
        assert float((u_dev - u_ref).abs().max()) <= 2 * 2 * 2e-4 * 1.05, k
        bad += int(((u_dev - u_ref).abs() > 0.05 * u_ref.abs() + 2e-6).sum())
        tot += v.numel()
    assert bad <= 0.01 * tot, f"{bad} of {tot} parameter updates differ from the oracle's"


def test_dualbranch_blocks_backward_vs_torch_autograd(dev):
    """The training forms of DecompDualBranch's bottleneck blocks (DecompModel_arch.py:57-99) and of the full-resolution Hamilton product
    (:351-352): outputs and every gradient (inputs, 1x1 transform, gate, SE weights, 7x7 / 3x3 attention kernel) against torch's autograd
    through the oracle's restatements on the CPU."""
    import bem.archs as A
    from bem import autograd as ag
    from oracle import bem_oracle as O
    gen = G(41)
    B, C, H, W = 3, 32, 9, 7

    def leaf(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).requires_grad_()

    def run(mod_out, ref_out, dout, pairs, what):
        close(mod_out, ref_out, 2e-5, 2e-6, what + " forward")
        mod_out.backward(dout.to(dev))
        ref_out.backward(dout)
        for name, got, want in pairs():
            close(got, want, 2e-4, 2e-6, f"{what} d{name}")

    # cross-fusion: x_tgt + gate * (W x_src + b)
    cf = A.CrossFusionBlock(C).to(dev).train()
    with torch.no_grad():
        cf.gate.add_(0.3 * torch.randn(1, C, 1, 1, generator=gen).to(dev)); cf.transform.bias.add_(0.1 * torch.randn(C, generator=gen).to(dev))
    sd = {"cf.transform.weight": cf.transform.weight.detach().cpu().clone().requires_grad_(), "cf.transform.bias": cf.transform.bias.detach().cpu().clone().requires_grad_(),
          "cf.gate": cf.gate.detach().cpu().clone().requires_grad_()}
    xs, xt = leaf(B, C, H, W), leaf(B, C, H, W)
    xs_d, xt_d = xs.detach().to(dev).requires_grad_(), xt.detach().to(dev).requires_grad_()
    for p_ in cf.parameters():
        p_.grad = None
    run(cf(xs_d, xt_d), O.cross_fusion_ref(sd, "cf.", xs, xt), torch.randn(B, C, H, W, generator=gen),
        lambda: [("x_src", xs_d.grad, xs.grad), ("x_tgt", xt_d.grad, xt.grad), ("W", cf.transform.weight.grad, sd["cf.transform.weight"].grad),
                 ("b", cf.transform.bias.grad, sd["cf.transform.bias"].grad), ("gate", cf.gate.grad, sd["cf.gate"].grad)], "cross-fusion")
    # SE block
    se = A.SEBlock(C, reduction=8).to(dev).train()
    with torch.no_grad():
        for p_ in se.parameters():
            p_.add_(0.8 * torch.randn(p_.shape, generator=gen).to(dev))
    sd = {"se.fc.0.weight": se.fc[0].weight.detach().cpu().clone().requires_grad_(), "se.fc.2.weight": se.fc[2].weight.detach().cpu().clone().requires_grad_()}
    x = leaf(B, C, H, W)
    x_d = x.detach().to(dev).requires_grad_()
    run(se(x_d), O.se_block_ref(sd, "se.", x), torch.randn(B, C, H, W, generator=gen),
        lambda: [("x", x_d.grad, x.grad), ("W1", se.fc[0].weight.grad, sd["se.fc.0.weight"].grad), ("W2", se.fc[2].weight.grad, sd["se.fc.2.weight"].grad)], "SE")
    # spatial attention, both kernel sizes
    for k in (7, 3):
        sa = A.SpatialAttention(k).to(dev).train()
        with torch.no_grad():
            sa.conv.weight.add_(0.5 * torch.randn(sa.conv.weight.shape, generator=gen).to(dev))
        sd = {"sa.conv.weight": sa.conv.weight.detach().cpu().clone().requires_grad_()}
        x = leaf(B, C, H, W)
        x_d = x.detach().to(dev).requires_grad_()
        run(sa(x_d), O.spatial_attention_ref(sd, "sa.", x), torch.randn(B, C, H, W, generator=gen),
            lambda: [("x", x_d.grad, x.grad), ("w", sa.conv.weight.grad, sd["sa.conv.weight"].grad)], f"attention {k}x{k}")
    # Hamilton product of two 4-channel maps, imaginary parts
    p4, q4 = leaf(B, 4, H, W), leaf(B, 4, H, W)
    p_d, q_d = p4.detach().to(dev).requires_grad_(), q4.detach().to(dev).requires_grad_()
    run(ag.HamiltonFn.apply(p_d, q_d), O.hamilton_ref(p4, q4)[:, 1:], torch.randn(B, 3, H, W, generator=gen),
        lambda: [("p", p_d.grad, p4.grad), ("q", q_d.grad, q4.grad)], "Hamilton")


def test_dualbranch_train_step_matches_oracle(dev):
    """ImageEnhancer.optimize_parameters with DecompDualBranch as the net (Options/DecompDualBranch_*.yml) for two steps against the oracle's
    restatement of the training step (image_enhancer_model.py:165-216) around dualbranch_ref on the fixture's weights: loss, gradient norm,
    parameter updates."""
    from basicsr.models import build_model
    from oracle import bem_oracle as O
    g = load_golden("g12_dualbranch")
    opt = dict(model_type="ImageEnhancer", is_train=True, num_gpu=1, dist=False, condition=dict(type="mean", scale_down=16, noise_level=0.0),
               network_g=dict(type="DecompDualBranch", in_channels=6, out_channels=3, n_feat=16, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                              mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[1, 1, 1], decomp_model="model4"),
               path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None),
               train=dict(total_iter=10, warmup_iter=-1, max_grad_norm=1, use_amp=False,
                          scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=[6, 4], restart_weights=[1, 1], eta_mins=[0.0002, 0.000001]),
                          optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]),
                          pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean")))
    x = torch.as_tensor(g["x"])
    lq = x[:, :3].contiguous()
    gen = G(34)
    gt = (3.5 * lq + 0.05 * torch.randn(lq.shape, generator=gen)).clamp(0, 1)
    gt_down = F.interpolate(gt, scale_factor=1 / 16, mode="bilinear") + 0.1 * torch.randn(1, 3, 2, 2, generator=gen)
    sd0 = {k: torch.as_tensor(v) for k, v in g["sd"].items()}
    sd = {**sd0, **qd_state_dict("model4")}
    ref = O.train_step_ref(sd, lq, gt, gt_down, steps=2, lr=2e-4, weight_decay=1e-4, max_grad_norm=1.0, stage2=O.dualbranch_ref)
    model = build_model(opt)
    model.net_g.load_state_dict(sd0, strict=False)
    for it in range(2):
        model.feed_train_data(dict(lq=lq, gt=gt, gt_down=gt_down))
        tn = model.optimize_parameters(it + 1)
        assert abs(float(model.log_dict["l_pix"]) - ref["loss"][it]) < 3e-6, (it, float(model.log_dict["l_pix"]), ref["loss"][it])
        assert abs(float(tn) - ref["grad_norm"][it]) < 5e-4 * ref["grad_norm"][it], (it, float(tn), ref["grad_norm"][it])
    named = dict(model.net_g.named_parameters())
    assert set(ref["params"]) == {k for k in named if not k.startswith("decomp.")}
    bad = tot = 0
    for k, v in ref["params"].items():
        u_ref, u_dev = (v - sd[k]).double(), (named[k].detach().cpu() - sd[k]).double()
        assert float((u_dev - u_ref).abs().max()) <= 2 * 2 * 2e-4 * 1.05, k
        bad += int(((u_dev - u_ref).abs() > 0.05 * u_ref.abs() + 2e-6).sum())
        tot += v.numel()
    assert bad <= 0.01 * tot, f"{bad} of {tot} parameter updates differ from the oracle's"


@pytest.mark.parametrize("tag,arch,dm,ref", [("g9_dualdd", "DecompDualBranch2DD", "model4", "dualbranch2dd_ref"), ("g9_dual2", "DecompDualBranch2", "model1", "dualbranch2_ref"),
                                             ("g9_singledd", "DecompSingleBranchDD", "model1", "singlebranchdd_ref"), ("g6_single", "DecompSingleBranch", "model1", "singlebranch_ref")])
def test_sibling_archs_train_step_matches_oracle(dev, tag, arch, dm, ref):
    """The other Stage-II archs of the 14 Decomp*.yml in training: two ImageEnhancer.optimize_parameters steps
    (full-resolution U-Nets, Hamilton product as an autograd node) against the oracle's training step around that arch's restatement, on the
    weights of the arch's fixture."""
    from basicsr.models import build_model
    from oracle import bem_oracle as O
    g = load_golden(tag)
    sd0 = {k: torch.as_tensor(v) for k, v in g["sd"].items()}
    n_feat, nb = (16, [2, 1, 1]) if tag == "g6_single" else (8, [1, 1, 1])             # the widths the fixtures were recorded at (tests/golden/make_golden.py)
    opt = dict(model_type="ImageEnhancer", is_train=True, num_gpu=1, dist=False, condition=dict(type="mean", scale_down=16, noise_level=0.0),
               network_g=dict(type=arch, in_channels=6, out_channels=3, n_feat=n_feat, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                              mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=nb, decomp_model=dm),
               path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None),
               train=dict(total_iter=10, warmup_iter=-1, max_grad_norm=1, use_amp=False,
                          scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=[6, 4], restart_weights=[1, 1], eta_mins=[0.0002, 0.000001]),
                          optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]),
                          pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean")))
    lq = torch.as_tensor(g["x"])[:, :3, :32, :32].contiguous()                       # 32x32 crops: the oracle's per-step scan loop under autograd is the cost
    h, w = lq.shape[-2:]
    gen = G(35)
    gt = (3.5 * lq + 0.05 * torch.randn(lq.shape, generator=gen)).clamp(0, 1)
    gt_down = F.interpolate(gt, scale_factor=1 / 16, mode="bilinear") + 0.1 * torch.randn(1, 3, h // 16, w // 16, generator=gen)
    sd = {**sd0, **qd_state_dict(dm)}
    r = O.train_step_ref(sd, lq, gt, gt_down, steps=2, lr=2e-4, weight_decay=1e-4, max_grad_norm=1.0, stage2=getattr(O, ref))
    model = build_model(opt)
    model.net_g.load_state_dict(sd0, strict=False)
    for it in range(2):
        model.feed_train_data(dict(lq=lq, gt=gt, gt_down=gt_down))
        tn = model.optimize_parameters(it + 1)
        assert abs(float(model.log_dict["l_pix"]) - r["loss"][it]) < 3e-6, (it, float(model.log_dict["l_pix"]), r["loss"][it])
        assert abs(float(tn) - r["grad_norm"][it]) < 5e-4 * r["grad_norm"][it], (it, float(tn), r["grad_norm"][it])
    named = dict(model.net_g.named_parameters())
    bad = tot = 0
    for k, v in r["params"].items():
        u_ref, u_dev = (v - sd[k]).double(), (named[k].detach().cpu() - sd[k]).double()
        assert float((u_dev - u_ref).abs().max()) <= 2 * 2 * 2e-4 * 1.05, k
        bad += int(((u_dev - u_ref).abs() > 0.05 * u_ref.abs() + 2e-6).sum())
        tot += v.numel()
    assert bad <= 0.01 * tot, f"{bad} of {tot} parameter updates differ from the oracle's"


def test_checkpoint_resume_continues_the_run(dev, tmp_path):
    """save (net_g_<iter>.pth + <iter>.state) after two steps, build a fresh ImageEnhancer through the resume path (load_resume_state
    -> check_resume -> pretrain path, resume_training) and take two more steps: same learning rates and, to the noise of the
    atomically reduced gradients, the same parameters as the run that never stopped (base_model.py:236-394, train.py:74-94,132-137).
    The saved optimizer state also loads into torch.optim.AdamW."""
    import copy
    from basicsr.models import build_model
    from basicsr.utils import load_resume_state
    g = load_golden("g6_ddw")
    root = tmp_path / "experiments" / "resume_run"
    opt = dict(name="resume_run", model_type="ImageEnhancer", is_train=True, num_gpu=1, dist=False, rank=0,
               condition=dict(type="mean", scale_down=16, noise_level=0.0),
               network_g=dict(type="DecompDualBranchDDWavelet", in_channels=6, out_channels=3, n_feat=16, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                              mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[2, 1, 1], decomp_model="model4"),
               path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None, models=str(root / "models"),
                         training_states=str(root / "training_states"), experiments_root=str(root)),
               train=dict(total_iter=10, warmup_iter=-1, max_grad_norm=1, use_amp=False,
                          scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=[3, 7], restart_weights=[1, 1], eta_mins=[0.0001, 0.000001]),
                          optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]),
                          pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean")))
    lq, gt = g["x"][:, :3], g["gt"]
    gt_down = F.interpolate(gt, scale_factor=1 / 16, mode="bilinear")
    batch = dict(lq=lq, gt=gt, gt_down=gt_down)

    def steps(model, first, n):
        lrs = []
        for it in range(first, first + n):
            model.update_learning_rate(it, warmup_iter=-1)
            model.feed_train_data(batch)
            model.optimize_parameters(it)
            lrs.append(model.get_current_learning_rate()[0])
        return lrs

    a = build_model(copy.deepcopy(opt))
    a.net_g.load_state_dict(g["sd"], strict=False)
    steps(a, 1, 2)
    a.save(0, 2, best_metric={"psnr": 20.0, "iter": 2})
    assert a.save_best({"psnr": 20.0, "iter": 2}).endswith("best_psnr_20.00_2.pth")
    lr_a = steps(a, 3, 2)

    opt_b = copy.deepcopy(opt)
    opt_b["auto_resume"] = True
    state = load_resume_state(opt_b, experiments_root=str(tmp_path / "experiments"))
    assert state["iter"] == 2 and opt_b["path"]["pretrain_network_g"].endswith("net_g_2.pth")
    b = build_model(opt_b)                                   # loads net_g_2.pth through pretrain_network_g
    b.resume_training(state)
    assert b.optimizer_g._steps == 2
    lr_b = steps(b, state["iter"] + 1, 2)
    assert lr_a == lr_b, (lr_a, lr_b)
    pa, pb = dict(a.net_g.named_parameters()), dict(b.net_g.named_parameters())
    worst = max(float((pa[k].detach() - pb[k].detach()).abs().max()) for k in pa)
    assert worst <= 2e-5, worst                              # an un-resumed optimizer (moments at zero) differs by ~ lr = 2e-4 per step
    # cross-load into torch's optimizer: same state layout
    ref_opt = torch.optim.AdamW([{"params": gp["params"]} for gp in b.optimizer_g.param_groups], lr=1e-3)
    ref_opt.load_state_dict(b.optimizer_g.state_dict())
    st = ref_opt.state_dict()["state"]
    assert all(float(v["step"]) == 4 for v in st.values()) and len(st) == sum(len(gp["params"]) for gp in b.optimizer_g.param_groups)


# ------------------------------------------------------------------------------------------------------------------
# Stage-I training
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["prelu", "bilinear", "depth_to_space", "mask_token", "kl", "reparam"])
def test_stage1_training_kernels(dev, case):
    """The small Stage-I training kernels against torch autograd of the reference formulas (UNet_arch.py:74-78,97-127,463-466;
    base_layer.py:26-40; conv.py:100-104)."""
    from bem import ops
    g = G(5)
    d = lambda t: t.to(dev)
    if case == "prelu":
        x = torch.randn(2, 5, 7, 9, generator=g, requires_grad=True); a = torch.tensor([0.25], requires_grad=True)
        dy = torch.randn(2, 5, 7, 9, generator=g)
        y = F.prelu(x, a); y.backward(dy)
        assert torch.equal(ops.prelu(d(x.detach()), d(a.detach())).cpu(), y.detach())
        da = torch.zeros(1, device=dev)
        dx = ops.prelu_bwd(d(x.detach()), d(a.detach()), d(dy), da)
        close(dx, x.grad, 1e-6, 1e-7, "prelu dx"); close(da, a.grad, 1e-5, 1e-6, "prelu dslope")
    elif case == "bilinear":
        for s_ in (2, 16):
            x = torch.randn(2, 3, 4, 5, generator=g, requires_grad=True)
            dy = torch.randn(2, 3, 4 * s_, 5 * s_, generator=g)
            F.interpolate(x, scale_factor=s_, mode="bilinear", align_corners=False).backward(dy)
            close(ops.bilinear_up_bwd(d(dy), s_), x.grad, 1e-5, 1e-5, f"bilinear x{s_} adjoint")
    elif case == "depth_to_space":
        x = torch.randn(2, 3, 6, 8, generator=g)
        assert torch.equal(ops.depth_to_space(ops.space_to_depth(d(x))).cpu(), x)
    elif case == "mask_token":
        fea = torch.randn(2, 6, 4, 5, generator=g, requires_grad=True); tok = torch.randn(1, 6, 1, 1, generator=g, requires_grad=True)
        m = (torch.rand(2, 4, 5, generator=g) < 0.5).float(); dy = torch.randn(2, 6, 4, 5, generator=g)
        w = m.unsqueeze(1)
        y = fea * (1.0 - w) + tok.expand(2, -1, 4, 5) * w; y.backward(dy)
        close(ops.mask_token(d(fea.detach()), d(m), d(tok.detach().reshape(-1))), y.detach(), 1e-6, 1e-7, "mask_token")
        dt = torch.zeros(6, device=dev)
        close(ops.mask_token_bwd(d(dy), d(m), dt), fea.grad, 1e-6, 1e-7, "mask_token dfea")
        close(dt, tok.grad.reshape(-1), 1e-5, 1e-6, "mask_token dtoken")
    elif case == "kl":
        from oracle import bem_oracle as O
        mu = torch.randn(700, generator=g, requires_grad=True); rho = (torch.randn(700, generator=g) - 3).requires_grad_(True)
        pmu, prho = mu.detach() + 0.1 * torch.randn(700, generator=g), rho.detach() + 0.2 * torch.randn(700, generator=g)
        kl = O.kl_div_ref(mu, torch.log1p(torch.exp(rho)), pmu, torch.log1p(torch.exp(prho)))
        (0.37 * kl).backward()
        out = torch.zeros(1, device=dev)
        ops.bnn_kl_(d(mu.detach()), d(rho.detach()), d(pmu), d(prho), out)
        close(out, kl.detach().reshape(1), 2e-5, 1e-6, "kl value")
        dmu, drho = torch.zeros(700, device=dev), torch.zeros(700, device=dev)
        ops.bnn_kl_bwd_(d(mu.detach()), d(rho.detach()), d(pmu), d(prho), torch.tensor([0.37], device=dev), dmu, drho)
        close(dmu, mu.grad, 1e-4, 1e-7, "kl dmu"); close(drho, rho.grad, 1e-4, 1e-7, "kl drho")
        pm, pr = d(pmu).clone(), d(prho).clone()
        ops.bnn_prior_ema_(pm, pr, d(mu.detach()), d(rho.detach()), 0.1)
        close(pm, 0.1 * pmu + 0.9 * mu.detach(), 1e-6, 1e-7, "prior ema mu"); close(pr, 0.1 * prho + 0.9 * rho.detach(), 1e-6, 1e-7, "prior ema rho")
    else:
        mu = torch.randn(300, generator=g, requires_grad=True); rho = (torch.randn(300, generator=g) - 3).requires_grad_(True)
        e, gw = torch.randn(300, generator=g), torch.randn(300, generator=g)
        (mu + torch.log1p(torch.exp(rho)) * e).backward(gw)
        dmu, drho = torch.zeros(300, device=dev), torch.zeros(300, device=dev)
        ops.bnn_reparam_bwd_(d(gw), d(e), d(rho.detach()), dmu, drho)
        close(dmu, mu.grad, 1e-6, 1e-7, "reparam dmu"); close(drho, rho.grad, 1e-5, 1e-7, "reparam drho")


def _cg_opt(n_feat=16, num_blocks=(2, 1, 1), mini_batch=8, periods=(1, 9)):
    return dict(name="cg", model_type="ConditionGenerator", is_train=True, num_gpu=1, dist=False, rank=0, sigma_init=0.05, selective=True,
                condition=dict(type="mean", scale_down=16, noise_level=0.1),
                datasets=dict(train=dict(mini_batch_sizes=[mini_batch])),
                network_g=dict(type="Network", in_channels=3, out_channels=3, n_feat=n_feat, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                               mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=list(num_blocks)),
                path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None),
                train=dict(total_iter=10, warmup_iter=-1, max_grad_norm=1, use_amp=False, mixing_augs=dict(mixup=False),
                           scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=list(periods), restart_weights=[1, 1], eta_mins=[0.0002, 0.000001]),
                           optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]),
                           pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean")))


def test_condition_generator_train_step_golden(dev):
    """ConditionGenerator.optimize_parameters (registry seam) for two iterations against the REFERENCE's own Stage-I training step
    (tests/golden/g11_stage1_train.npz: its Network + Bayesian leaves in train() mode, get_kl_loss, AdamW) with the recorded eps injected:
    KL and pixel losses, gradient norm, every gradient of iteration 1 (mu, rho, LayerNorm, PReLU, mask token, ...), parameters and
    EMA priors after iteration 2.  Iteration 1 uses the MIM mask, iteration 2 runs past the first scheduler period (mask dropped,
    mask_token skipped by the optimizer)."""
    from basicsr.models import build_model
    from bem.modules import SampleCtx, sampling
    g = load_golden("g11_stage1_train")
    model = build_model(_cg_opt(mini_batch=int(g["mini_batch"])))
    net = model.net_g
    missing, unexpected = net.load_state_dict(g["sd"], strict=True)
    for k, v in g["prior0"].items():                       # the reference's priors sit at ITS random initial values: install them
        mod, name = k.rsplit(".", 1)
        getattr(net.get_submodule(mod), name).copy_(v.to(dev))
    for it in range(2):
        model.feed_train_data(dict(lq_down=g["lq"], gt=g["gt"], gt_down=g["gt"], mask=g["mask"]))
        with sampling(SampleCtx(1, {k: v.to(dev) for k, v in g[f"eps{it}"].items()})):
            tn = model.optimize_parameters(it + 1)
        assert abs(float(model.log_dict["l_kl"]) - float(g["l_kl"][it])) <= 1e-4 * max(1.0, abs(float(g["l_kl"][it]))), (it, float(model.log_dict["l_kl"]), g["l_kl"])
        assert abs(float(model.log_dict["l_pix"]) - float(g["l_pix"][it])) <= 1e-5, (it, float(model.log_dict["l_pix"]), g["l_pix"])
        assert abs(float(tn) - float(g["grad_norm"][it])) <= 1e-3 * float(g["grad_norm"][it]), (it, float(tn), g["grad_norm"])
    named = dict(net.named_parameters())
    bad = tot = 0
    for k, v in g["params"].items():
        dlt = (named[k].detach().cpu() - v).abs()
        assert float(dlt.max()) <= 2 * 2 * 2e-4 * 1.05, k
        bad += int((dlt > 2e-6).sum()); tot += v.numel()
    assert bad <= 0.01 * tot, (bad, tot)
    for k, v in g["prior2"].items():
        mod, name = k.rsplit(".", 1)
        got = getattr(net.get_submodule(mod), name).cpu()
        assert torch.allclose(got, v, rtol=0, atol=2e-4) and float(((got - v).abs() > 2e-6).float().mean()) <= 0.02, k


def test_stage1_training_gradients_golden(dev):
    """Every parameter gradient of one Stage-I training iteration (loss = 0.01 * KL / mini_batch + L1, MIM mask on) against the
    reference's (g11 'grads'): read from .grad after backward, before any optimizer step."""
    from basicsr.bayesian import convert2bnn_selective, get_kl_loss
    from basicsr.archs import build_network
    from bem import autograd as ag
    from bem.modules import SampleCtx, sampling
    g = load_golden("g11_stage1_train")
    opt = _cg_opt()
    net = build_network(opt["network_g"])
    convert2bnn_selective(net, {"sigma_init": 0.05, "decay": 0.998, "pretrain": False})
    net = net.to(dev)
    net.load_state_dict(g["sd"], strict=True)
    for k, v in g["prior0"].items():
        mod, name = k.rsplit(".", 1)
        getattr(net.get_submodule(mod), name).copy_(v.to(dev))
    net.train()
    with sampling(SampleCtx(1, {k: v.to(dev) for k, v in g["eps0"].items()})):
        _, pred = net(g["lq"].to(dev), mask=g["mask"].to(dev))
    kl = get_kl_loss(net)
    pix = ag.l1_loss(pred, g["gt"].to(dev))
    ag.ScaledSumFn.apply(pix, kl, 0.01 / int(g["mini_batch"])).backward()
    assert abs(float(kl.detach()) - float(g["l_kl"][0])) <= 1e-4 * max(1.0, float(g["l_kl"][0]))
    for k, p in net.named_parameters():
        ref = g["grads"][k]
        assert p.grad is not None, k
        scale = float(ref.abs().max())
        err = float((p.grad.cpu() - ref).abs().max())
        assert err <= 2e-3 * scale + 1e-7, (k, err, scale)
    # a second backward through the same graph is refused by autograd; a second FORWARD draws a new sample and a new EMA step
    assert all(m.sample is None for m in net.modules() if hasattr(m, "kl_terms"))


# ------------------------------------------------------------------------------------------------------------------
# the training driver: basicsr/train.py's loop over the tensor dataset shim
# ------------------------------------------------------------------------------------------------------------------
def _run_driver(root, yml, extra, total, auto_resume=False):
    from basicsr.train import train_pipeline
    argv = ["--opt", os.path.join(PKG, "Options", yml), "--synthetic", "4",
            "--force_yml", "network_g:n_feat=16", "network_g:num_blocks=[1,1,1]", f"train:total_iter={total}", "logger:save_checkpoint_freq=3",
            "logger:print_freq=1", "datasets:train:batch_size_per_gpu=2", "datasets:train:gt_size=64", "train:scheduler:periods=[4,4,4]"] + extra
    if auto_resume:
        argv.append("--auto_resume")
    torch.manual_seed(100)
    model, info = train_pipeline(str(root), argv=argv)
    return model, info


@pytest.mark.parametrize("yml,first,total", [("DecompDualBranch2DDWavelet_4.yml", 3, 6), ("CG_UNet_LOLv1.yml", 6, 8), ("DecompDualBranch_4.yml", 3, 6)])
def test_training_driver_save_resume_reproduces_the_run(dev, tmp_path, yml, first, total):
    """basicsr/train.py:97-262 over the tensor dataset shim: run A trains `total` iterations without a break; run B stops after `first`
    (checkpoints every 3 iterations), is started again with --auto_resume (train.py:74-94: newest .state, resume_training, the loader
    skipping the batches already consumed) and finishes.  Both end with the same learning rate and -- to the noise of the atomically
    reduced gradients -- the same parameters.  Stage I: the scheduler's first period ends at iteration 4, so the state saved at 6 holds a
    mask token whose optimizer step lags the other parameters (a grad-None parameter in the reference's AdamW): it must resume."""
    a, ia = _run_driver(tmp_path / "A", yml, [], total)
    b0, ib0 = _run_driver(tmp_path / "B", yml, [], first)
    name = yml[:-4]
    st = tmp_path / "B" / "experiments" / name / "training_states"
    assert (st / f"{first}.state").is_file() and (tmp_path / "B" / "experiments" / name / "models" / f"net_g_{first}.pth").is_file()
    assert (tmp_path / "B" / "experiments" / name / "models" / "net_g_latest.pth").is_file()
    del b0
    b, ib = _run_driver(tmp_path / "B", yml, [], total, auto_resume=True)
    assert ia["iter"] == ib["iter"] == total
    assert a.get_current_learning_rate() == b.get_current_learning_rate()
    pa, pb = dict(a.net_g.named_parameters()), dict(b.net_g.named_parameters())
    worst = max(float((pa[k].detach() - pb[k].detach()).abs().max()) for k in pa)
    assert worst <= 4e-5, worst                              # a run resumed with zeroed moments or a shifted batch order differs by ~ lr = 2e-4 per step
    # the run moved: parameters differ from the initial seed-100 net by many learning rates
    assert (st / f"{(total // 3) * 3}.state").is_file()


def test_stage1_bayes_bank_equals_the_per_leaf_steps(dev, tmp_path, monkeypatch):
    """The Bayesian bookkeeping of a Stage-I training iteration for all 90 Bayesian tensors of the net in one launch each (BayesBank over
    bem_bnn_bank_*: prior EMA + eps draw + weight sample, KL, KL backward, reparameterisation backward; conv.py:84-112, tools.py:76-84)
    against the same 6 iterations done tensor by tensor (BEM_BAYES_BANK=0), both launched kernel by kernel.  The bank draws every tensor
    from the Philox stream the per-leaf forward uses for it, so the two runs see the same weight samples: parameters, EMA priors and
    losses agree to the noise of the atomically reduced gradients."""
    from bem.modules import BayesBank
    monkeypatch.setenv("BEM_STAGE1_GRAPH", "0")
    monkeypatch.setenv("BEM_BAYES_BANK", "0")
    a, ia = _run_driver(tmp_path / "A", "CG_UNet_LOLv1.yml", [], 6)
    assert BayesBank.of(a.net_g) is None
    monkeypatch.setenv("BEM_BAYES_BANK", "1")
    b, ib = _run_driver(tmp_path / "B", "CG_UNet_LOLv1.yml", [], 6)
    bank = BayesBank.of(b.net_g)
    assert bank is not None and bank.ready() and len(bank.views) == sum(2 if m.bias else 1 for m in bank.leaves) >= 30
    pa, pb = dict(a.net_g.named_parameters()), dict(b.net_g.named_parameters())
    worst = max(float((pa[k].detach() - pb[k].detach()).abs().max()) for k in pa)
    assert worst <= 4e-5, worst
    for (ka, ma), (kb, mb) in zip(a.net_g.named_modules(), b.net_g.named_modules()):
        if hasattr(ma, "kl_terms"):
            assert ma.step == mb.step == 6
            for ta, tb in zip(ma.kl_terms(), mb.kl_terms()):
                assert float((ta[2] - tb[2]).abs().max()) <= 4e-5 and float((ta[3] - tb[3]).abs().max()) <= 4e-5, ka
    assert abs(float(a.log_dict["l_kl"]) - float(b.log_dict["l_kl"])) <= 1e-4 * max(1.0, abs(float(a.log_dict["l_kl"])))
    assert abs(float(a.log_dict["l_pix"]) - float(b.log_dict["l_pix"])) <= 1e-4


def test_stage1_captured_step_equals_the_launched_one(dev, tmp_path, monkeypatch):
    """the Stage-I training step replayed from a HIP graph (condition_generator_model.py:176-218 -- zero_grad,
    forward with the MIM mask, KL + L1, backward, clip, AdamW) against the same 8 iterations launched kernel by kernel
    (BEM_STAGE1_GRAPH=0).  Everything that changes between iterations is read from device memory in the captured form: the Philox epoch
    of the weight draws, the learning rate of the warm-up / cosine schedule, Adam's bias corrections, each leaf's EMA decay
    (1 + step) / (10 + step) -- a stale value of any of them moves the parameters by about one learning rate (2e-4) per iteration.  The
    scheduler period ends at iteration 4: the mask-less geometry is a second graph and the mask token drops out of the optimizer."""
    monkeypatch.setenv("BEM_STAGE1_GRAPH", "0")
    a, ia = _run_driver(tmp_path / "A", "CG_UNet_LOLv1.yml", [], 8)
    assert not getattr(a, "_graphs", None)
    monkeypatch.setenv("BEM_STAGE1_GRAPH", "1")
    b, ib = _run_driver(tmp_path / "B", "CG_UNet_LOLv1.yml", [], 8)
    captured = [g for g in b._graphs.values() if isinstance(g, dict)]
    assert len(captured) == 2 and all(isinstance(g["graph"], torch.cuda.CUDAGraph) for g in captured)      # with and without the mask
    assert a.get_current_learning_rate() == b.get_current_learning_rate()
    pa, pb = dict(a.net_g.named_parameters()), dict(b.net_g.named_parameters())
    worst = max(float((pa[k].detach() - pb[k].detach()).abs().max()) for k in pa)
    assert worst <= 4e-5, worst
    for (ka, ma), (kb, mb) in zip(a.net_g.named_modules(), b.net_g.named_modules()):
        if hasattr(ma, "kl_terms"):
            assert ma.step == mb.step == 8, (ka, ma.step, mb.step)
            for ta, tb in zip(ma.kl_terms(), mb.kl_terms()):
                assert float((ta[2] - tb[2]).abs().max()) <= 4e-5 and float((ta[3] - tb[3]).abs().max()) <= 4e-5, ka     # EMA priors
    sa, sb = a.optimizer_g.state_dict()["state"], b.optimizer_g.state_dict()["state"]
    assert [float(v["step"]) for v in sa.values()] == [float(v["step"]) for v in sb.values()]
    assert abs(float(a.log_dict["l_kl"]) - float(b.log_dict["l_kl"])) <= 1e-4 * max(1.0, abs(float(a.log_dict["l_kl"])))
    assert abs(float(a.log_dict["l_pix"]) - float(b.log_dict["l_pix"])) <= 1e-4


# ------------------------------------------------------------------------------------------------------------------
# BASELINE config 4 at its real size (B 16, 256x256, n_feat 40): the dispatch the bench runs
# ------------------------------------------------------------------------------------------------------------------
def _cfg4():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cfg4_grads", os.path.join(os.path.dirname(PKG), "scripts", "cfg4_grads.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_config4_full_size_default_dispatch_vs_generic_kernels(dev, tmp_path):
    """One ImageEnhancer forward / backward at B 16, 256x256, full width, in the DEFAULT dispatch (x6 weight gradients on every launch of
    >= 16384 pixels, the L = 16384 / 4096 / 1024 row-form scan backward, the atomics-reduced parameter gradients) against the same step in
    a process started with BEM_WGRAD_X6=0 BEM_SCAN_BWD_ROWS=0 (f32-MFMA weight gradients through LDS, generic scan backward): same loss,
    and every parameter gradient within 1e-5 of the net's largest gradient element (the two forms differ by summation order only)."""
    import subprocess
    import sys
    m = _cfg4()
    loss, grads = m.compute(16, 256, 1)
    out = tmp_path / "generic.pt"
    env = dict(os.environ, BEM_WGRAD_X6="0", BEM_SCAN_BWD_ROWS="0")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(PKG), "scripts", "cfg4_grads.py"), str(out), "16", "256", "1"], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ref = torch.load(out, weights_only=True)
    assert abs(loss - ref["loss"]) <= 2e-6 * abs(ref["loss"]), (loss, ref["loss"])
    assert set(grads) == set(ref["grads"]) and len(grads) > 300
    gmax = max(float(g.abs().max()) for g in ref["grads"].values())
    worst = max((float((grads[k] - ref["grads"][k]).abs().max()), k) for k in grads)
    assert worst[0] <= 1e-5 * gmax, (worst, gmax)
    na = sum(float((g.double() ** 2).sum()) for g in grads.values()) ** 0.5
    nb = sum(float((g.double() ** 2).sum()) for g in ref["grads"].values()) ** 0.5
    assert abs(na - nb) <= 1e-5 * nb, (na, nb)


def test_config4_full_width_batch_additivity_and_oracle_crop(dev):
    """Size-independent checks of the full-width training step: (i) the L1-mean gradient of a 2-image batch at 256x256 equals the mean of
    the two single-image gradients (every reduction over the batch -- weight gradients, scan parameter gradients, LayerNorm -- is linear in
    the batch); (ii) one 64x64 pair through the SAME full-width net against oracle.train_step_ref (torch-CPU autograd of the restated net,
    itself pinned by the reference fixture g10_train): loss, gradient norm and every gradient."""
    from oracle import bem_oracle as O
    m = _cfg4()
    l2, g2 = m.compute(2, 256, 3)
    la, ga = m.compute(2, 256, 3, images=slice(0, 1))
    lb, gb = m.compute(2, 256, 3, images=slice(1, 2))
    assert abs(l2 - 0.5 * (la + lb)) <= 2e-6 * l2
    gmax = max(float(g.abs().max()) for g in g2.values())
    worst = max((float((g2[k] - 0.5 * (ga[k] + gb[k])).abs().max()), k) for k in g2)
    assert worst[0] <= 2e-5 * gmax, (worst, gmax)
    # (ii) the oracle on one 64x64 pair of the same seeded full-width net
    from basicsr.models import build_model
    from basicsr.utils.options import parse
    from bem import ops
    from bem.pipeline import synthetic_pair
    l1, g1 = m.compute(1, 64, 5)
    opt = parse(os.path.join(PKG, "Options", "DecompDualBranch2DDWavelet_4.yml"), is_train=True)
    opt["dist"] = False
    torch.manual_seed(100)
    sd = {k: v.detach().cpu() for k, v in build_model(opt).net_g.state_dict().items()}
    lq, gt = synthetic_pair((1, 3, 64, 64), seed=5)
    gd = ops.resize_down(gt.cuda(), 16).cpu()
    ref = O.train_step_ref(sd, lq, gt, gd, steps=1, scan=O.selective_scan_ref)
    assert abs(l1 - ref["loss"][0]) < 5e-6, (l1, ref["loss"][0])
    n1 = sum(float((g.double() ** 2).sum()) for g in g1.values()) ** 0.5
    assert abs(n1 - ref["grad_norm"][0]) <= 2e-3 * ref["grad_norm"][0], (n1, ref["grad_norm"][0])
    rmax = max(float(g.abs().max()) for g in ref["grads"].values())
    for k, g in ref["grads"].items():
        assert float((g1[k] - g).abs().max()) <= 2e-3 * float(g.abs().max()) + 2e-5 * rmax, k
