"""CPU checks of tests/backward_ref.py: every float64 restatement against an independent formula on a tiny case (the oracle's per-step
scan loop, tests/dstate_ref.py, closed-form derivatives, central differences, torch.optim.AdamW), and the two error rules against
outputs that are right, slightly off and missing a tile."""
import pytest
import torch
import torch.nn.functional as F

import backward_ref as R
import dstate_ref as D

F64 = torch.float64


def G(seed):
    return torch.Generator().manual_seed(seed)


def rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=F64) * scale


def near(a, b, tol, what=""):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, ref = float((a - b).abs().max()), float(b.abs().max())
    assert err <= tol * max(ref, 1e-300), (what, err, ref)


def fd(f, x, h=1e-6):
    """Central differences of the scalar f at the float64 tensor x."""
    g = torch.zeros_like(x)
    flat, gf = x.reshape(-1), g.reshape(-1)
    for i in range(flat.numel()):
        keep = float(flat[i])
        flat[i] = keep + h
        up = float(f(x))
        flat[i] = keep - h
        gf[i] = (up - float(f(x))) / (2 * h)
        flat[i] = keep
    return g


def sums_ok(o, fill=0.0):
    """A reduced output lies within the sum of the absolute values of its terms."""
    assert o.reduced and o.n >= 1
    assert bool(((o.value.double() - fill).abs() <= o.S * (1 + 1e-12) + 1e-300).all())


# ---------------------------------------------------------------------------------------------------------------- scans
def _seam_operands(g, Bt, KC, L, N, K):
    u, delta = rnd(g, Bt, KC, L), rnd(g, Bt, KC, L, scale=0.5)
    A = -torch.exp(rnd(g, KC, N, scale=0.3))
    Bm, Cm = rnd(g, Bt, K, N, L), rnd(g, Bt, K, N, L)
    return u, delta, A, Bm, Cm, rnd(g, KC), rnd(g, KC, scale=0.5) - 1.0, rnd(g, Bt, KC, L)


def test_scan_blocked_equals_the_step_loop():
    """Blocks of 16 over L = 37 (two full blocks and a ragged one, the state carried across both joints), N = 3."""
    g = G(0)
    u, dt = rnd(g, 2, 3, 37), torch.rand(2, 3, 37, generator=g, dtype=F64)
    A, Bm, Cm, Dv = -torch.rand(2, 3, 3, 37, generator=g, dtype=F64), rnd(g, 2, 3, 3, 37), rnd(g, 2, 3, 3, 37), rnd(g, 2, 3, 37)
    near(R.scan_blocked(u, dt, A, Bm, Cm, Dv, blk=16), R.scan_steps(u, dt, A, Bm, Cm, Dv), 1e-12, "blocked vs steps")
    near(R.scan_blocked(u, dt, A, Bm, Cm, Dv, blk=128), R.scan_steps(u, dt, A, Bm, Cm, Dv), 1e-12, "one ragged block")


@pytest.mark.parametrize("softplus,with_D,with_bias", [(True, True, True), (False, True, False), (True, False, True), (True, False, False)])
def test_selective_scan_bwd_ref_vs_the_oracle_loop(softplus, with_D, with_bias):
    """Forward and every gradient against autograd through the oracle's per-step loop (float32 inside: compared at its precision), and
    against the step loop of this module in float64."""
    from oracle import bem_oracle as O
    Bt, KC, L, N, K = 2, 6, 41, 3, 2
    u, delta, A, Bm, Cm, Dv, bias, dout = _seam_operands(G(1), Bt, KC, L, N, K)
    if not softplus:
        delta = delta.abs() + 0.05
    Dv, bias = (Dv if with_D else None), (bias if with_bias else None)
    got = R.selective_scan_bwd_ref(u, delta, A, Bm, Cm, Dv, bias, dout, softplus, F64)
    steps = R.selective_scan_bwd_ref(u, delta, A, Bm, Cm, Dv, bias, dout, softplus, F64, scan=R.scan_steps)
    leaves = [t.float().requires_grad_() for t in (u, delta, A, Bm, Cm)] + [None if t is None else t.float().requires_grad_() for t in (Dv, bias)]
    y = O.selective_scan_ref(*leaves, softplus)
    gr = torch.autograd.grad(y, [t for t in leaves if t is not None], dout.float())
    names = ["du", "ddelta", "dA", "dB", "dC"] + (["dD"] if with_D else []) + (["ddelta_bias"] if with_bias else [])
    assert sorted(got) == sorted(names)
    for nm, ref in zip(names, gr):
        near(got[nm].value, ref, 2e-5, nm + " vs oracle")
        near(got[nm].value, steps[nm].value, 1e-11, nm + " vs step loop")
        if got[nm].reduced:
            sums_ok(got[nm])
    assert got["dA"].n == Bt * L and got["dB"].n == KC // K and not got["du"].reduced


@pytest.mark.parametrize("N,L", [(1, 21), (3, 37)])
def test_ss2d_bwd_ref_vs_dstate_ref(N, L):
    """The fused layout (both orientations, reversed directions, x_dbl rows, dt projection) against autograd through the per-step
    restatement of tests/dstate_ref.py; the fill is added to the four accumulated outputs only."""
    g = G(2)
    B, C, Rk = 2, 3, 2
    x0, x1 = rnd(g, B, C, L), rnd(g, B, C, L)
    xd0, xd1 = rnd(g, B, 2, Rk + 2 * N, L, scale=0.7), rnd(g, B, 2, Rk + 2 * N, L, scale=0.7)
    dtw, dtb, A_logs, Ds = rnd(g, 4, C, Rk, scale=0.5), rnd(g, 4, C, scale=0.5) - 1, rnd(g, 4 * C, N, scale=0.3), rnd(g, 4 * C)
    dy0, dy1 = rnd(g, B, C, L), rnd(g, B, C, L)
    leaves = [t.clone().requires_grad_() for t in (x0, x1, xd0, xd1, dtw, dtb, A_logs, Ds)]
    r0, r1 = D.ss2d_scan_n_ref(*leaves)
    gr = torch.autograd.grad([r0, r1], leaves, [dy0, dy1])
    got = R.ss2d_bwd_ref(x0, x1, xd0, xd1, dtw, dtb, -torch.exp(A_logs), Ds, dy0, dy1, F64, fill=0.5)
    for nm, ref, fill in zip(("dx0", "dx1", "dxd0", "dxd1", "ddtw", "ddtb", "dA_logs", "dDs"), gr, (0, 0, 0, 0, 0.5, 0.5, 0.5, 0.5)):
        near(got[nm].value, ref + fill, 1e-11, nm)
        assert got[nm].reduced == (nm not in ("dx0", "dx1"))
        if got[nm].reduced:
            sums_ok(got[nm], fill)
    assert got["dxd0"].n == C and got["ddtw"].n == B * L + 1
    f32 = R.ss2d_bwd_ref(x0, x1, xd0, xd1, dtw, dtb, -torch.exp(A_logs), Ds, dy0, dy1, torch.float32, fill=0.5)
    assert f32["dx0"].value.dtype == torch.float32 and 0 < float((f32["dx0"].value.double() - got["dx0"].value).abs().max()) < 1e-4


# ---------------------------------------------------------------------------------------------------------------- GEMMs, LN, depthwise
def test_pw_wgrad_ref_vs_loops():
    g = G(3)
    dy, x = rnd(g, 2, 3, 5), rnd(g, 2, 4, 5)
    dy[:, :, 3] = 0                                              # a dead pixel is no term
    o = R.pw_wgrad_ref(dy, x, F64, fill=0.25)
    dw = torch.full((3, 4), 0.25, dtype=F64)
    for b in range(2):
        for l in range(5):
            dw += dy[b, :, l, None] * x[b, None, :, l]
    near(o["dw"].value, dw, 1e-13); near(o["dbias"].value, 0.25 + dy.sum((0, 2)), 1e-13)
    assert o["dw"].n == 2 * 4 + 1
    sums_ok(o["dw"], 0.25); sums_ok(o["dbias"], 0.25)


@pytest.mark.parametrize("k,s,p", [(3, 1, 1), (4, 2, 1)])
def test_conv_wgrad_ref_vs_unfold(k, s, p):
    g = G(4)
    x = rnd(g, 2, 3, 6, 8)
    Ho, Wo = (6 + 2 * p - k) // s + 1, (8 + 2 * p - k) // s + 1
    dy = rnd(g, 2, 5, Ho, Wo)
    o = R.conv_wgrad_ref(dy, x, (5, 3, k, k), s, p, F64)
    cols = F.unfold(x, k, padding=p, stride=s)                   # (B, Cin k k, Ho Wo)
    near(o["dw"].value, torch.einsum("bml,bnl->mn", dy.reshape(2, 5, -1), cols).view(5, 3, k, k), 1e-13)
    near(o["dw"].S, torch.einsum("bml,bnl->mn", dy.reshape(2, 5, -1).abs(), cols.abs()).view(5, 3, k, k), 1e-13)
    assert o["dw"].n == 2 * Ho * Wo
    near(o["dbias"].value, dy.sum((0, 2, 3)), 1e-13)


@pytest.mark.parametrize("two,res", [(False, False), (True, True)])
def test_ln_ref_vs_closed_form(two, res):
    g = G(5)
    x1, x2 = rnd(g, 2, 5, 3, 4) * 2 + 0.5, (rnd(g, 2, 5, 3, 4) if two else None)
    gam, bet, dn, dres = rnd(g, 5), rnd(g, 5), rnd(g, 2, 5, 3, 4), (rnd(g, 2, 5, 3, 4) if res else None)
    o = R.ln_ref(x1, x2, gam, bet, 1e-5, dn, dres, F64, fill=1.0)
    x = x1 + x2 if two else x1
    mu = x.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + 1e-5)
    xh = (x - mu) * rstd
    gg = dn * gam.view(1, 5, 1, 1)
    dx = rstd * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    near(o["n"].value, xh * gam.view(1, 5, 1, 1) + bet.view(1, 5, 1, 1), 1e-12)
    near(o["dx"].value, dx + dres if res else dx, 1e-11)
    near(o["dgamma"].value, 1.0 + (dn * xh).sum((0, 2, 3)), 1e-12); near(o["dbeta"].value, 1.0 + dn.sum((0, 2, 3)), 1e-12)
    assert o["dgamma"].n == 2 * 12 + 1
    sums_ok(o["dgamma"], 1.0)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_dwact_ref_vs_closed_form(mode):
    import math
    g = G(6)
    Cw, Cout = 4, (2 if mode == 2 else 4)
    t, w, b, do = rnd(g, 2, Cw, 5, 6), rnd(g, Cw, 1, 3, 3, scale=0.4), rnd(g, Cw, scale=0.3), rnd(g, 2, Cout, 5, 6)
    o = R.dwact_ref(t, w, b, do, mode, F64)
    pre = F.conv2d(t, w, b, padding=1, groups=Cw)
    if mode == 0:
        dpre = do
    elif mode == 1:
        sg = torch.sigmoid(pre)
        dpre = do * sg * (1 + pre * (1 - sg))
    else:
        h1, h2 = pre[:, :2], pre[:, 2:]
        cdf, pdf = 0.5 * (1 + torch.erf(h1 / math.sqrt(2))), torch.exp(-0.5 * h1 * h1) / math.sqrt(2 * math.pi)
        dpre = torch.cat([do * h2 * (cdf + h1 * pdf), do * h1 * cdf], 1)
    near(o["dpre"].value, dpre, 1e-12)
    tp = F.pad(t, (1, 1, 1, 1))
    dw = torch.stack([(dpre * tp[:, :, ky:ky + 5, kx:kx + 6]).sum((0, 2, 3)) for ky in range(3) for kx in range(3)], 1).view(Cw, 1, 3, 3)
    near(o["dw"].value, dw, 1e-12); near(o["dbias"].value, dpre.sum((0, 2, 3)), 1e-12)
    sums_ok(o["dw"]); assert o["dw"].n == 2 * 30


# ---------------------------------------------------------------------------------------------------------------- small kernels
def test_hamilton_ref_vs_oracle_and_differences():
    from oracle import bem_oracle as O
    g = G(7)
    q8, do = rnd(g, 1, 8, 2, 2), rnd(g, 1, 3, 2, 2)
    near(R.hamilton_imag(q8[:, :4], q8[:, 4:]), O.hamilton_ref(q8[:, :4], q8[:, 4:])[:, 1:], 1e-14)
    near(R.hamilton_bwd_ref(q8, do, F64)["dq8"].value, fd(lambda q: (R.hamilton_imag(q[:, :4], q[:, 4:]) * do).sum(), q8.clone()), 1e-8)


def test_l1_channel_sum_prelu_mask_token_refs():
    g = G(8)
    p, t = rnd(g, 2, 3, 4), rnd(g, 2, 3, 4)
    p[0, 0, 0] = t[0, 0, 0]
    o = R.l1_ref(p, t, 0.7, 2.5, F64)
    near(o["loss"].value, [0.7 * float((p - t).abs().sum()) / 24], 1e-14)
    near(o["dpred"].value, 2.5 * 0.7 * torch.sign(p - t) / 24, 1e-14)
    assert o["loss"].n == 2
    x = rnd(g, 2, 3, 1, 5)
    o = R.channel_sum_ref(x, F64, fill=0.5)
    near(o["sum"].value, [0.5 + sum(float(x[b, c, 0, i]) for b in range(2) for i in range(5)) for c in range(3)], 1e-13)
    assert o["sum"].n == 11
    xx, a, do = rnd(g, 3, 7), torch.tensor([0.25], dtype=F64), rnd(g, 3, 7)
    o = R.prelu_bwd_ref(xx, a, do, F64)
    near(o["dx"].value, torch.where(xx >= 0, do, 0.25 * do), 1e-14)
    near(o["dslope"].value, [float((do * xx)[xx < 0].sum())], 1e-13)
    assert o["dslope"].n == int((xx < 0).sum())
    dout, m = rnd(g, 2, 3, 2, 2), (torch.rand(2, 2, 2, generator=g) < 0.5).double()
    o = R.mask_token_bwd_ref(dout, m, F64)
    fea, tok = rnd(g, 2, 3, 2, 2).requires_grad_(), rnd(g, 1, 3, 1, 1).requires_grad_()
    (fea * (1 - m[:, None]) + tok * m[:, None]).backward(dout)
    near(o["dfea"].value, fea.grad, 1e-14); near(o["dtoken"].value, tok.grad.reshape(-1), 1e-13)


def test_kl_ref_vs_oracle_and_differences():
    from oracle import bem_oracle as O
    g = G(9)
    mu, rho = rnd(g, 6), rnd(g, 6) - 3
    pmu, prho = mu + 0.1 * rnd(g, 6), rho + 0.2 * rnd(g, 6)
    o = R.kl_ref(mu, rho, pmu, prho, 0.37, F64, fill=0.5)
    kl = lambda m, r: O.kl_div_ref(m, torch.log1p(torch.exp(r)), pmu, torch.log1p(torch.exp(prho)))
    near(o["kl"].value, [0.5 + float(kl(mu, rho))], 1e-13)
    assert o["kl"].n == 7 and o["dmu"].reduced and o["dmu"].n == 2
    same = R.kl_ref(torch.cat([mu, pmu]), torch.cat([rho, prho]), torch.cat([pmu, pmu]), torch.cat([prho, prho]), 0.37, F64)
    assert same["kl"].n == 6                                     # equal posterior and prior: a term of exactly 0 is no term
    near(o["dmu"].value, 0.5 + 0.37 * fd(lambda m: kl(m, rho), mu.clone()), 1e-7)
    near(o["drho"].value, 0.5 + 0.37 * fd(lambda r: kl(mu, r), rho.clone()), 1e-7)


def test_adamw_ref_vs_torch():
    g = G(10)
    p0, g0 = rnd(g, 50), rnd(g, 50)
    p = p0.clone().requires_grad_()
    opt = torch.optim.AdamW([p], lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    m, v = torch.zeros(50, dtype=F64), torch.zeros(50, dtype=F64)
    cur = p0
    for step in (1, 2, 3):
        gs = g0 * step
        p.grad = gs.clone()
        tn = float(torch.nn.utils.clip_grad_norm_([p], 1.0))
        opt.step()
        o = R.adamw_ref(cur, gs, m, v, 2e-3, (0.9, 0.999), 1e-8, 1e-2, step, min(1.0, 1.0 / (tn + 1e-6)), F64)
        cur, m, v = o["p"].value, o["m"].value, o["v"].value
        near(cur, p.detach(), 1e-12, f"step {step}"); near(o["g"].value, p.grad, 1e-12)
    near(R.sumsq_ref(g0, F64), float((g0 ** 2).sum()), 1e-14)


# ---------------------------------------------------------------------------------------------------------------- the rules
def test_rules_accept_f32_and_refuse_a_wrong_or_missing_term():
    g = G(11)
    r64 = rnd(g, 4, 300)
    r32 = r64.float()
    R.check_elementwise(r32, r64, r32, "exact f32")
    bad = r32.clone(); bad[2, 7] += 1e-4
    with pytest.raises(AssertionError):
        R.check_elementwise(bad, r64, r32, "one element off")
    dy, x = rnd(g, 2, 3, 96), rnd(g, 2, 4, 96)
    o64, o32 = R.pw_wgrad_ref(dy, x, F64), R.pw_wgrad_ref(dy, x, torch.float32)
    R.check_reduced(o32["dw"].value, o64["dw"], o32["dw"], "f32 sum")
    R.check_reduced(torch.einsum("bml,bkl->mk", dy.float().flip(-1), x.float().flip(-1)), o64["dw"], o32["dw"], "another order")
    probe = dy.clone(); probe[:, :, :64] = 0; probe[0] = 0                       # only the last 32-pixel tile of image 1 is live
    p64, p32 = R.pw_wgrad_ref(probe, x, F64), R.pw_wgrad_ref(probe, x, torch.float32)
    assert p64["dw"].n == 32
    R.check_reduced(p32["dw"].value, p64["dw"], p32["dw"], "probe")
    with pytest.raises(AssertionError):
        R.check_reduced(torch.zeros(3, 4), p64["dw"], p32["dw"], "the live tile dropped")
    with pytest.raises(AssertionError):
        R.check_reduced(2 * p32["dw"].value, p64["dw"], p32["dw"], "the live tile added twice")
    with pytest.raises(AssertionError):
        R.check_reduced(torch.full((3, 4), float("nan")), p64["dw"], p32["dw"], "nan")
    assert any(l.startswith("PARITY") and "rule 2" in l for l in R.LINES)
