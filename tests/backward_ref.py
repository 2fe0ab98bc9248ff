"""Float64 references and the two error rules of tests/test_backward_edges_gpu.py.

Every backward op of the training step is restated here in plain torch on the CPU with the number format as a parameter: float64 is the
truth, float32 the yardstick (what a correct f32 evaluation of the same formulas loses).  Gradients come from torch.autograd.  Every
function returns {name: Out}; an Out carries the value and, for a REDUCED output (a sum over pixels, batch or channels), the sum S of
the absolute values of its terms and their number n -- taken from the same autograd run by handing the op one copy of the shared operand
per term (a broadcast parameter becomes a leaf of the broadcast shape: its gradient IS the list of terms).

Rule 1, element-wise outputs:   max|got - f64| <= 2 max|f32 - f64| + 1e-6 max|f64|                    (tests/test_dstate_gpu.py)
Rule 2, reduced outputs:        |got - f64| <= n 2^-24 S + 2 max|f32 - f64|   per element
    n 2^-24 S is the worst case of an f32 sum of n terms in any order; the second part absorbs the roundings inside a term.
There is no other tolerance.  tests/test_backward_ref_cpu.py checks each restatement against an independent formula."""
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24


class Out:
    """value: the output; S / n: sum of |terms| per element and number of terms (reduced outputs only)."""

    def __init__(self, value, S=None, n=None):
        self.value, self.S, self.n = value, S, n

    @property
    def reduced(self):
        return self.S is not None


def _cv(t, dtype):
    return None if t is None else t.detach().cpu().to(dtype)


# ---------------------------------------------------------------------------------------------------------------- the rules
LINES = []          # one line per checked output: what profiles/backward_edges_parity.txt is made of


def _line(case, what, rule, err, e32, bound, tight=None):
    ratio = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
    s = f"PARITY {case} | {what} | rule {rule} | err {err:.3e} | f32 {e32:.3e} | err/f32 {ratio:.3g} | err/bound {err / bound if bound > 0 else 0.0:.3g}"
    if tight is not None:
        s += f" | err/(n 2^-24 S) {tight:.3g}"
    LINES.append(s)
    print(s)


def check_elementwise(got, r64, r32, what, case=""):
    """Rule 1.  got: the kernel's output (any device), r64 / r32: the two restatements."""
    got, r64, r32 = got.detach().cpu().double(), r64.detach().double(), r32.detach().double()
    assert got.shape == r64.shape == r32.shape, (case, what, got.shape, r64.shape, r32.shape)
    assert bool(torch.isfinite(got).all()), (case, what, "non-finite output")
    err, e32, scale = float((got - r64).abs().max()), float((r32 - r64).abs().max()), float(r64.abs().max())
    bound = 2 * e32 + 1e-6 * scale
    _line(case, what, 1, err, e32, bound)
    assert err <= bound, f"{case} {what}: max|err| {err:.3e} > 2 x {e32:.3e} (f32 restatement) + 1e-6 x {scale:.3e}"


def check_reduced(got, o64, o32, what, case="", extra=0.0):
    """Rule 2.  o64 / o32: Out of the two restatements; S and n are taken from the float64 one.  extra: a documented approximation of the
    kernel propagated through the formula by the caller (per element or scalar), 0 everywhere but where a docstring says otherwise."""
    got, r64, r32 = got.detach().cpu().double(), o64.value.detach().double(), o32.value.detach().double()
    assert got.shape == r64.shape == r32.shape, (case, what, got.shape, r64.shape, r32.shape)
    assert bool(torch.isfinite(got).all()), (case, what, "non-finite output")
    err, e32 = (got - r64).abs(), float((r32 - r64).abs().max())
    first = o64.n * U24 * o64.S.double()
    bound = first + 2 * e32 + extra
    worst = int(torch.argmax(err - bound))
    e_w, b_w, f_w = float(err.reshape(-1)[worst]), float(bound.reshape(-1)[worst]), float(first.reshape(-1)[worst])
    _line(case, what, 2, e_w, e32, b_w, e_w / f_w if f_w > 0 else float("inf") if e_w > 0 else 0.0)
    assert bool((err <= bound).all()), (f"{case} {what}: |err| {e_w:.3e} > n 2^-24 S = {f_w:.3e} (n = {o64.n}) + 2 x {e32:.3e} (f32 restatement)"
                                        f" at flat index {worst}")


def check(got, o64, o32, what, case="", extra=0.0):
    if o64.reduced:
        check_reduced(got, o64, o32, what, case, extra)
    else:
        check_elementwise(got, o64.value, o32.value, what, case)


# ---------------------------------------------------------------------------------------------------------------- (a) weight gradients
def pw_wgrad_ref(dy, x, dtype, fill=0.0):
    """dw (M,K) = fill + sum_{b,l} dy[b,m,l] x[b,k,l], dbias (M) = fill + sum_{b,l} dy: n = the pixels with a non-zero dy, plus the fill."""
    dy, x = _cv(dy, dtype), _cv(x, dtype)
    live = int((dy != 0).any(1).sum())
    n = live + (1 if fill else 0)
    dw = torch.einsum("bml,bkl->mk", dy, x) + fill
    S = torch.einsum("bml,bkl->mk", dy.abs().double(), x.abs().double()) + abs(fill)
    return {"dw": Out(dw, S, n), "dbias": Out(dy.sum(dim=(0, 2)) + fill, dy.abs().double().sum(dim=(0, 2)) + abs(fill), n)}


def conv_wgrad_ref(dy, x, wshape, stride, pad, dtype, fill=0.0):
    """Weight / bias gradient of conv2d(x, w, stride, pad) by autograd through F.conv2d; S from the same contraction of |dy| and |x|."""
    dy, x = _cv(dy, dtype), _cv(x, dtype)
    w = torch.zeros(wshape, dtype=dtype, requires_grad=True)
    dw, = torch.autograd.grad(F.conv2d(x, w, None, stride=stride, padding=pad), w, dy)
    wa = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    S, = torch.autograd.grad(F.conv2d(x.abs().double(), wa, None, stride=stride, padding=pad), wa, dy.abs().double())
    live = int((dy != 0).any(1).sum())
    n = live + (1 if fill else 0)
    return {"dw": Out(dw + fill, S + abs(fill), n),
            "dbias": Out(dy.sum(dim=(0, 2, 3)) + fill, dy.abs().double().sum(dim=(0, 2, 3)) + abs(fill), n)}


# ---------------------------------------------------------------------------------------------------------------- (b) LayerNorm2d
def ln_ref(x1, x2, gamma, beta, eps, dn, dres, dtype, fill=0.0):
    """LayerNorm over the channels of x = x1 (+ x2): n, dx (+ dres), dgamma = fill + sum dn xhat, dbeta = fill + sum dn."""
    x1, x2, gamma, beta, dn, dres = (_cv(t, dtype) for t in (x1, x2, gamma, beta, dn, dres))
    C = x1.shape[1]
    x = (x1 if x2 is None else x1 + x2).requires_grad_()
    n = F.layer_norm(x.permute(0, 2, 3, 1), (C,), gamma, beta, eps).permute(0, 3, 1, 2)
    dx, = torch.autograd.grad(n, x, dn)
    xd = x.detach()
    mu = xd.mean(1, keepdim=True)
    xhat = (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(1, keepdim=True) + eps)
    terms = int((dn != 0).any(1).sum()) + (1 if fill else 0)
    return {"n": Out(n.detach()), "dx": Out(dx if dres is None else dx + dres),
            "dgamma": Out((dn * xhat).sum(dim=(0, 2, 3)) + fill, (dn * xhat).abs().double().sum(dim=(0, 2, 3)) + abs(fill), terms),
            "dbeta": Out(dn.sum(dim=(0, 2, 3)) + fill, dn.abs().double().sum(dim=(0, 2, 3)) + abs(fill), terms)}


# ---------------------------------------------------------------------------------------------------------------- (c) depthwise 3x3 + activation
def dwact_ref(t, w, bias, dout, mode, dtype, fill=0.0):
    """pre = dwconv3x3(t) + bias; out = pre (mode 0), SiLU(pre) (1), GELU(pre[:Hd]) pre[Hd:] (2).  dpre = dL/dpre; dw[c,ky,kx] = fill +
    sum dpre t(shifted), dbias = fill + sum dpre."""
    t, w, bias, dout = (_cv(a, dtype) for a in (t, w, bias, dout))
    Cw = t.shape[1]
    w = w.view(Cw, 1, 3, 3)
    pre = F.conv2d(t, w, bias, padding=1, groups=Cw).requires_grad_()
    if mode == 1:
        out = F.silu(pre)
    elif mode == 2:
        a, c = pre.chunk(2, 1)
        out = F.gelu(a) * c
    else:
        out = pre * 1.0
    dpre, = torch.autograd.grad(out, pre, dout)
    wl = w.clone().requires_grad_()
    dw, = torch.autograd.grad(F.conv2d(t, wl, None, padding=1, groups=Cw), wl, dpre)
    wa = torch.zeros(Cw, 1, 3, 3, dtype=torch.float64, requires_grad=True)
    S, = torch.autograd.grad(F.conv2d(t.abs().double(), wa, None, padding=1, groups=Cw), wa, dpre.abs().double())
    n = int((dpre != 0).any(1).sum()) + (1 if fill else 0)
    return {"dpre": Out(dpre), "dw": Out(dw + fill, S + abs(fill), n),
            "dbias": Out(dpre.sum(dim=(0, 2, 3)) + fill, dpre.abs().double().sum(dim=(0, 2, 3)) + abs(fill), n)}


# ---------------------------------------------------------------------------------------------------------------- scans
def scan_blocked(u, dt, A, Bm, Cm, D, blk=128):
    """h_t = exp(dt_t A_t) h_{t-1} + dt_t B_t u_t, y_t = sum_n C_t h_t + D_t u_t with EVERY operand given per (batch, channel, position):
    u, dt, D (Bt,C,L); A, Bm, Cm (Bt,C,N,L).  Closed form per block of blk steps (h_t = sum_{s<=t} exp(cl_t - cl_s) b_s + exp(cl_t) h_in,
    cl the running sum of dt A inside the block): tests/test_train_gpu.py::_scan_blocked for N states, differentiable, in the dtype of
    its operands."""
    Bt, C, L = u.shape
    la = dt[:, :, None, :] * A
    bu = (dt * u)[:, :, None, :] * Bm
    h = torch.zeros(Bt, C, la.shape[2], dtype=u.dtype)
    tri = torch.tril(torch.ones(blk, blk, dtype=torch.bool))
    ys = []
    for s0 in range(0, L, blk):
        e0 = min(L, s0 + blk)
        n = e0 - s0
        cl = torch.cumsum(la[..., s0:e0], -1)
        M = torch.exp((cl[..., :, None] - cl[..., None, :]).masked_fill(~tri[:n, :n], -float("inf")))
        hb = torch.einsum("bcnts,bcns->bcnt", M, bu[..., s0:e0]) + torch.exp(cl) * h[..., None]
        ys.append((hb * Cm[..., s0:e0]).sum(2))
        h = hb[..., -1]
    return torch.cat(ys, -1) + D * u


def scan_steps(u, dt, A, Bm, Cm, D):
    """The same recurrence step by step (the form of the oracle's loop), for the CPU check of scan_blocked."""
    h = torch.zeros(u.shape[0], u.shape[1], A.shape[2], dtype=u.dtype)
    ys = []
    for t in range(u.shape[-1]):
        h = torch.exp(dt[:, :, None, t] * A[..., t]) * h + (dt * u)[:, :, None, t] * Bm[..., t]
        ys.append((h * Cm[..., t]).sum(-1))
    return torch.stack(ys, -1) + D * u


def _leaf(t):
    return t.detach().clone().requires_grad_()


def _one_scan(u, z, A, Bs, Cs, D, dy, softplus, scan=scan_blocked):
    """One direction: u, z (Bt,C,L) (z = the pre-softplus step size), A (C,N), Bs, Cs (Bt,C,N,L) or (Bt,1,N,L) shared by the channels,
    D (C) or None, dy (Bt,C,L).  Returns the gradients w.r.t. per-term copies: du, dz (Bt,C,L); gA, gB, gC (Bt,C,N,L); gD (Bt,C,L)."""
    Bt, C, L = u.shape
    N = A.shape[1]
    ul, zl = _leaf(u), _leaf(z)
    Ae = _leaf(A[None, :, :, None].expand(Bt, C, N, L))
    Be, Ce = _leaf(Bs.expand(Bt, C, N, L)), _leaf(Cs.expand(Bt, C, N, L))
    De = _leaf((torch.zeros(C, dtype=u.dtype) if D is None else D)[None, :, None].expand(Bt, C, L))
    y = scan(ul, F.softplus(zl) if softplus else zl, Ae, Be, Ce, De)
    return torch.autograd.grad(y, [ul, zl, Ae, Be, Ce, De], dy)


def selective_scan_bwd_ref(u, delta, A, B, C, D, delta_bias, dout, delta_softplus, dtype, scan=scan_blocked):
    """Gradients of oracle.selective_scan_ref (u, delta (Bt,KC,L); A (KC,N); B, C (Bt,K,N,L); D, delta_bias (KC) | None) in ``dtype``."""
    u, delta, A, B, C, D, delta_bias, dout = (_cv(t, dtype) for t in (u, delta, A, B, C, D, delta_bias, dout))
    Bt, KC, L = u.shape
    K, N = B.shape[1], B.shape[2]
    Cd = KC // K
    z = delta if delta_bias is None else delta + delta_bias[None, :, None]
    du, dz, gA, gB, gC, gD = _one_scan(u, z, A, B.repeat_interleave(Cd, 1), C.repeat_interleave(Cd, 1), D, dout, delta_softplus, scan)
    red = lambda g, dims, n: Out(g.sum(dim=dims), g.abs().double().sum(dim=dims), n)
    out = {"du": Out(du), "ddelta": Out(dz), "dA": red(gA, (0, 3), Bt * L),
           "dB": red(gB.view(Bt, K, Cd, N, L), 2, Cd), "dC": red(gC.view(Bt, K, Cd, N, L), 2, Cd)}
    if D is not None:
        out["dD"] = red(gD, (0, 2), Bt * L)
    if delta_bias is not None:
        out["ddelta_bias"] = red(dz, (0, 2), Bt * L)
    return out


def ss2d_bwd_ref(x0, x1, xd0, xd1, dtw, dtb, A, Ds, dy0, dy1, dtype, fill=0.0, scan=scan_blocked):
    """Gradients of the fused SS2D scan in the operand layout of bem_ss2d_scan(_n)_f32 (tests/dstate_ref.py): x0, x1, dy0, dy1 (B,C,L);
    xd0, xd1 (B,2,R+2N,L) rows [dt | B | C] of directions {0,2} / {1,3}; dtw (4,C,R), dtb (4,C), A (4C,N) = -exp(A_logs), Ds (4C).
    dx0 / dx1 are element-wise (the two directions of an orientation added); dxd0 / dxd1 sum over the C channels; dA_logs (= dA A),
    dDs, ddtw, ddtb sum over batch and positions and sit on ``fill``."""
    x0, x1, xd0, xd1, dtw, dtb, A, Ds, dy0, dy1 = (_cv(t, dtype) for t in (x0, x1, xd0, xd1, dtw, dtb, A, Ds, dy0, dy1))
    B, C, L = x0.shape
    R = dtw.shape[2]
    A = A.reshape(4 * C, -1)
    N = A.shape[1]
    nf = 1 if fill else 0
    dA, SA = torch.zeros(4 * C, N, dtype=dtype), torch.zeros(4 * C, N, dtype=torch.float64)
    dD, SD = torch.zeros(4 * C, dtype=dtype), torch.zeros(4 * C, dtype=torch.float64)
    dW, SW = torch.zeros(4, C, R, dtype=dtype), torch.zeros(4, C, R, dtype=torch.float64)
    db, Sb = torch.zeros(4, C, dtype=dtype), torch.zeros(4, C, dtype=torch.float64)
    res = {}
    for o, (x, xd, dy) in enumerate(((x0, xd0, dy0), (x1, xd1, dy1))):
        dx = 0
        dxd, Sxd = torch.zeros_like(xd), torch.zeros(xd.shape, dtype=torch.float64)
        for slot, k in enumerate((o, o + 2)):
            fl = (lambda t: t.flip(-1)) if slot == 1 else (lambda t: t)
            rows = fl(xd[:, slot])
            dts, Bs, Cs = rows[:, :R], rows[:, R:R + N], rows[:, R + N:]
            ck = slice(k * C, (k + 1) * C)
            z = torch.einsum("cr,brl->bcl", dtw[k], dts) + dtb[k][None, :, None]
            du, dz, gA, gB, gC, gD = _one_scan(fl(x), z, A[ck], Bs[:, None], Cs[:, None], Ds[ck], fl(dy), True, scan)
            dx = dx + fl(du)
            dA[ck], SA[ck] = gA.sum(dim=(0, 3)) * A[ck], gA.abs().double().sum(dim=(0, 3)) * A[ck].abs().double()
            dD[ck], SD[ck] = gD.sum(dim=(0, 2)), gD.abs().double().sum(dim=(0, 2))
            db[k], Sb[k] = dz.sum(dim=(0, 2)), dz.abs().double().sum(dim=(0, 2))
            dW[k], SW[k] = torch.einsum("bcl,brl->cr", dz, dts), torch.einsum("bcl,brl->cr", dz.abs().double(), dts.abs().double())
            dxd[:, slot, :R] = fl(torch.einsum("bcl,cr->brl", dz, dtw[k]))
            Sxd[:, slot, :R] = fl(torch.einsum("bcl,cr->brl", dz.abs().double(), dtw[k].abs().double()))
            dxd[:, slot, R:R + N], Sxd[:, slot, R:R + N] = fl(gB.sum(1)), fl(gB.abs().double().sum(1))
            dxd[:, slot, R + N:], Sxd[:, slot, R + N:] = fl(gC.sum(1)), fl(gC.abs().double().sum(1))
        res[f"dx{o}"] = Out(dx)
        res[f"dxd{o}"] = Out(dxd, Sxd, C)
    n = B * L + nf
    res.update(dA_logs=Out(dA + fill, SA + abs(fill), n), dDs=Out(dD + fill, SD + abs(fill), n),
               ddtw=Out(dW + fill, SW + abs(fill), n), ddtb=Out(db + fill, Sb + abs(fill), n))
    return res


# ---------------------------------------------------------------------------------------------------------------- (g) small kernels
def hamilton_imag(p, q):
    """i, j, k parts of the quaternion product p x q, (B,4,H,W) each (QD/quaternion.py)."""
    r1, i1, j1, k1 = p.unbind(1)
    r2, i2, j2, k2 = q.unbind(1)
    return torch.stack([r1 * i2 + i1 * r2 + j1 * k2 - k1 * j2, r1 * j2 - i1 * k2 + j1 * r2 + k1 * i2, r1 * k2 + i1 * j2 - j1 * i2 + k1 * r2], 1)


def hamilton_bwd_ref(q8, dout, dtype, product=hamilton_imag):
    q8, dout = _cv(q8, dtype).requires_grad_(), _cv(dout, dtype)
    dq, = torch.autograd.grad(product(q8[:, :4], q8[:, 4:]), q8, dout)
    return {"dq8": Out(dq)}


def l1_ref(pred, gt, weight, gmul, dtype):
    """loss = weight mean|pred - gt|, dpred = gmul weight sign(pred - gt) / numel.  The kernel sums the terms in float64, so of rule 2's n
    roundings per term two remain: the float32 difference pred - gt inside each term (at worst 2^-24 S when all go one way) and the
    float32 rounding of the result: n = 2."""
    pred, gt = _cv(pred, dtype).requires_grad_(), _cv(gt, dtype)
    loss = weight * (pred - gt).abs().mean()
    dp, = torch.autograd.grad(loss, pred, torch.tensor(1.0 if gmul is None else gmul, dtype=dtype))
    return {"loss": Out(loss.detach().reshape(1), loss.detach().abs().double().reshape(1), 2), "dpred": Out(dp)}


def channel_sum_ref(x, dtype, fill=0.0):
    """out[c] = fill + sum_{b,p} x[b,c,p]; n = the positions that are non-zero in some channel, plus the fill."""
    x = _cv(x, dtype)
    dims = (0,) + tuple(range(2, x.dim()))
    return {"sum": Out(x.sum(dim=dims) + fill, x.abs().double().sum(dim=dims) + abs(fill), int((x != 0).any(1).sum()) + (1 if fill else 0))}


def prelu_bwd_ref(x, slope, dout, dtype, fill=0.0):
    x, slope, dout = _cv(x, dtype), _cv(slope, dtype).requires_grad_(), _cv(dout, dtype)
    xl = x.clone().requires_grad_()
    dx, da = torch.autograd.grad(F.prelu(xl, slope), [xl, slope], dout)
    terms = (dout * x)[(x < 0) & (dout != 0)]
    return {"dx": Out(dx), "dslope": Out(da + fill, terms.abs().double().sum().reshape(1) + abs(fill), terms.numel() + (1 if fill else 0))}


def _kl_terms(mu, rho, pmu, prho):
    sq, sp = torch.log1p(torch.exp(rho)), torch.log1p(torch.exp(prho))
    return torch.log(sp) - torch.log(sq) + (sq ** 2 + (mu - pmu) ** 2) / (2 * sp ** 2) - 0.5


def kl_ref(mu, rho, pmu, prho, g, dtype, fill=0.0):
    """kl = fill + mean of the KL terms (base_layer.py:38-39), n = the non-zero terms (a term is exactly 0 where mu = prior_mu and
    rho = prior_rho) plus the fill; dmu, drho = fill + g d(kl)/d(mu, rho): `+=` outputs of one term on top of the fill, n = 2."""
    mu, rho, pmu, prho = (_cv(t, dtype) for t in (mu, rho, pmu, prho))
    ml, rl = _leaf(mu), _leaf(rho)
    terms = _kl_terms(ml, rl, pmu, prho)
    n = mu.numel()
    dmu, drho = torch.autograd.grad(terms.mean(), [ml, rl], torch.tensor(g, dtype=dtype))
    live = int((terms.detach() != 0).sum())
    return {"kl": Out((terms.detach().mean() + fill).reshape(1), (terms.detach().abs().double().sum() / n + abs(fill)).reshape(1), live + (1 if fill else 0)),
            "dmu": Out(dmu + fill, dmu.abs().double() + abs(fill), 2), "drho": Out(drho + fill, drho.abs().double() + abs(fill), 2)}


def mask_token_bwd_ref(dout, mask, dtype, fill=0.0):
    """y = fea (1 - w) + token w, w = mask (B,H,W) over the channels: dfea = dout (1 - w), dtoken[c] = fill + sum_{b,p} dout w."""
    dout, mask = _cv(dout, dtype), _cv(mask, dtype)
    w = mask[:, None]
    t = dout * w
    return {"dfea": Out(dout * (1 - w)), "dtoken": Out(t.sum(dim=(0, 2, 3)) + fill, t.abs().double().sum(dim=(0, 2, 3)) + abs(fill),
                                                      int(((mask != 0) & (dout != 0).any(1)).sum()) + (1 if fill else 0))}


def sumsq_ref(g, dtype):
    g = _cv(g, dtype)
    return (g * g).sum()


def adamw_ref(p, g, m, v, lr, betas, eps, wd, step, coef, dtype):
    """torch.optim.AdamW's documented update on flat buffers, after the gradient has been scaled by the clip coefficient ``coef``:
    g <- coef g; p <- p (1 - lr wd); m <- b1 m + (1 - b1) g; v <- b2 v + (1 - b2) g^2; p <- p - lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps)."""
    p, g, m, v = (_cv(t, dtype) for t in (p, g, m, v))
    b1, b2 = betas
    g = g * coef
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - (lr / (1 - b1 ** step)) * (m / (v.sqrt() / (1 - b2 ** step) ** 0.5 + eps))
    return {"p": Out(p), "g": Out(g), "m": Out(m), "v": Out(v)}
