"""GPU: the train block -- ``optim_g.type: Adam`` (bem_adam_step_f32, bem.train.BemAdam), ``pixel_opt.type: MSELoss / CharbonnierLoss``
(bem_mse_loss_f32, bem_charbonnier_loss_f32) and the reference's schedulers inside the two training steps and the driver.

Yardstick: torch on the CPU in float64 (torch.optim.Adam; F.mse_loss / the Charbonnier formula under autograd).  Bounds: the two rules of
tests/backward_ref.py and nothing else -- rule 1 for element-wise outputs (2 x the error of the same computation in float32 on the CPU
+ 1e-6 of the scale), rule 2 for the reduced ones (n 2^-24 S + 2 x that error), n counted where the reference is defined.  The scalars the
C ABI takes as float (lr, betas, Adam's and Charbonnier's eps, weight decay) are rounded to float32 BEFORE the references run: the
formula is evaluated at the values the kernel gets (tests/test_backward_edges_gpu.py::test_adamw_step_direct does the same)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import backward_ref as R
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bem import native
    native.lib()
    return torch.device("cuda", 0)


def G(seed):
    return torch.Generator().manual_seed(seed)


def f32(x):
    return float(np.float32(x))


def both(fn, *a, **k):
    return fn(*a, dtype=F64, **k), fn(*a, dtype=F32, **k)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


PAD, FILL = 32, -7.5
EPS = float(np.float32(1e-12))          # CharbonnierLoss's default eps as bem_charbonnier_loss_f32 receives it


class Guarded:
    """n floats inside a buffer with PAD sentinel floats on either side (the view stays 16-byte aligned)."""

    def __init__(self, host, dev):
        self.buf = torch.full((host.numel() + 2 * PAD,), FILL, device=dev, dtype=F32)
        self.t = self.buf[PAD:PAD + host.numel()]
        self.t.copy_(host.to(dev))

    def guards(self):
        assert bool((self.buf[:PAD] == FILL).all()) and bool((self.buf[-PAD:] == FILL).all()), "a write outside the buffer"


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
def adam_ref(p, g, m, v, lr, betas, eps, wd, step, coef, dtype):
    """torch.optim.Adam's documented update (amsgrad=False, maximize=False) on flat buffers after the clip: g <- coef g; g' = g + wd p;
    m <- b1 m + (1 - b1) g'; v <- b2 v + (1 - b2) g'^2; p <- p - lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps)."""
    p, g, m, v = (t.detach().cpu().to(dtype) for t in (p, g, m, v))
    b1, b2 = betas
    g = g * coef
    gd = g + wd * p
    m = b1 * m + (1 - b1) * gd
    v = b2 * v + (1 - b2) * gd * gd
    p = p - (lr / (1 - b1 ** step)) * (m / (v.sqrt() / (1 - b2 ** step) ** 0.5 + eps))
    return {"p": R.Out(p), "g": R.Out(g), "m": R.Out(m), "v": R.Out(v)}


def test_adam_ref_is_torch_optim_adam():
    """The restated formula against torch.optim.Adam itself, in float64 (runs without touching the device)."""
    lr, betas, eps, wd = 2e-3, (0.9, 0.999), 1e-8, 0.01
    g = G(1)
    p0, g1, g2 = (torch.randn(50, generator=g, dtype=F64) for _ in range(3))
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([q], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    o = {"p": R.Out(p0), "m": R.Out(torch.zeros(50, dtype=F64)), "v": R.Out(torch.zeros(50, dtype=F64))}
    for t, gr in enumerate((g1, g2), 1):
        q.grad = gr.clone()
        opt.step()
        o = adam_ref(o["p"].value, gr, o["m"].value, o["v"].value, lr, betas, eps, wd, t, 1.0, F64)
        assert float((o["p"].value - q.detach()).abs().max()) <= 1e-15
        assert float((o["v"].value - opt.state[q]["exp_avg_sq"]).abs().max()) <= 1e-15


def _buffers(dev, n, seed, gscale=3.0):
    g = G(seed)
    host = dict(p=torch.randn(n, generator=g), g=torch.randn(n, generator=g) * gscale, m=torch.randn(n, generator=g) * 0.1,
                v=torch.rand(n, generator=g) * 0.01)
    return host, {k: Guarded(h, dev) for k, h in host.items()}


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_step_direct(dev, wd, step):
    """bem_adam_step_f32 at n = 1000 (three full blocks and a partial one): (1) the update without the clip; (2) lr and the bias
    corrections read from device memory under a wrong host lr give the same bits; (3) with weight_decay > 0 the result is NOT the AdamW
    kernel's on the same inputs, with weight_decay = 0 both are Adam's formula (the one flag of the shared body); (4) max_norm = 1 with a
    gradient norm above it (clipped, norm written out) and (5) below it (coefficient 1: g keeps its bits)."""
    from bem import ops
    n = 1000
    lr, b1, b2, eps, wd = (f32(h) for h in (2e-3, 0.9, 0.999, 1e-8, wd))
    betas = (b1, b2)
    tag = f"adam n=1000 wd={wd:g} step={step}"
    # (1)
    host, acc = _buffers(dev, n, 860)
    ops.adam_step_(acc["p"].t, acc["g"].t, acc["m"].t, acc["v"].t, lr, betas, eps, wd, step, max_norm=0.0)
    assert torch.equal(bits(acc["g"].t), bits(host["g"])), "max_norm = 0 changed the gradient"
    o64, o32 = both(adam_ref, host["p"], host["g"], host["m"], host["v"], lr, betas, eps, wd, step, 1.0)
    for k in ("p", "m", "v"):
        R.check(acc[k].t, o64[k], o32[k], k, tag + " no clip")
    for a in acc.values():
        a.guards()
    plain = {k: a.t.clone() for k, a in acc.items()}
    # (2)
    _, acc2 = _buffers(dev, n, 860)
    hyper = torch.tensor([np.float32(lr), np.float32(1.0 - b1 ** step), np.float32(math.sqrt(1.0 - b2 ** step))], dtype=F32, device=dev)
    ops.adam_step_(acc2["p"].t, acc2["g"].t, acc2["m"].t, acc2["v"].t, 123.0, betas, eps, wd, 0, max_norm=0.0, hyper=hyper)
    for k in plain:
        assert torch.equal(bits(acc2[k].t), bits(plain[k])), f"hyper: {k} differs from the host-value call"
    # (3)
    _, accw = _buffers(dev, n, 860)
    ops.adamw_step_(accw["p"].t, accw["g"].t, accw["m"].t, accw["v"].t, lr, betas, eps, wd, step, max_norm=0.0)
    if wd > 0:
        # g' = g + wd p moves m by (1 - b1) wd p ~ 1e-3 |p|, four orders above its float32 rounding; AdamW's m never sees p
        dm = float((accw["m"].t - plain["m"]).abs().max())
        assert dm > 1e-4 and not torch.equal(bits(accw["p"].t), bits(plain["p"])), dm
        w64, _ = both(R.adamw_ref, host["p"], host["g"], host["m"], host["v"], lr, betas, eps, wd, step, 1.0)
        assert float((plain["p"].cpu().double() - w64["p"].value).abs().max()) > 1e-6            # and it is not AdamW's update either
    else:                              # the two formulas coincide (not bit for bit: the compiler fuses p (1 - lr wd) - ... its own way)
        for k in ("p", "m", "v"):
            R.check(accw[k].t, o64[k], o32[k], k, tag + " AdamW kernel against Adam's formula")
    # (4)
    host3, acc3 = _buffers(dev, n, 861)
    ss = torch.zeros(1, device=dev, dtype=F64)
    ops.grad_sumsq(acc3["g"].t, ss)
    norm = Guarded(torch.zeros(1), dev)
    ops.adam_step_(acc3["p"].t, acc3["g"].t, acc3["m"].t, acc3["v"].t, lr, betas, eps, wd, step, max_norm=1.0, sumsq=ss, norm_out=norm.t)
    tn = float(host3["g"].double().pow(2).sum().sqrt())
    assert tn > 1.0 and abs(float(norm.t) - tn) <= 2.0 ** -23 * tn, (float(norm.t), tn)
    o64, o32 = both(adam_ref, host3["p"], host3["g"], host3["m"], host3["v"], lr, betas, eps, wd, step, min(1.0, 1.0 / (tn + 1e-6)))
    for k in ("g", "p", "m", "v"):
        R.check(acc3[k].t, o64[k], o32[k], k, tag + " clip 1.0, norm above")
    norm.guards()
    for a in acc3.values():
        a.guards()
    # (5)
    host4, acc4 = _buffers(dev, n, 862, gscale=0.01)
    ops.grad_sumsq(acc4["g"].t, ss)
    ops.adam_step_(acc4["p"].t, acc4["g"].t, acc4["m"].t, acc4["v"].t, lr, betas, eps, wd, step, max_norm=1.0, sumsq=ss, norm_out=norm.t)
    tn = float(host4["g"].double().pow(2).sum().sqrt())
    assert tn < 1.0 and abs(float(norm.t) - tn) <= 2.0 ** -23 * tn, (float(norm.t), tn)
    assert torch.equal(bits(acc4["g"].t), bits(host4["g"])), "a norm below max_norm changed the gradient"
    o64, o32 = both(adam_ref, host4["p"], host4["g"], host4["m"], host4["v"], lr, betas, eps, wd, step, 1.0)
    for k in ("p", "m", "v"):
        R.check(acc4[k].t, o64[k], o32[k], k, tag + " clip 1.0, norm below")
    for a in acc4.values():
        a.guards()


# ---------------------------------------------------------------------------------------------------------------- 2. the optimizer
def _flat(ts):
    return torch.cat([t.detach().reshape(-1).cpu().double() for t in ts])


def test_bem_adam_five_steps_vs_torch_adam(dev):
    """BemAdam over five steps against torch.optim.Adam (float64, CPU) on the same gradient sequence: parameters of 7 and 1025 elements
    (the _align4 padding between them); the small one takes no part in step 3 (skip= here, .grad None there) and is updated again in
    steps 4 and 5 with its own step count (_lag); after step 2 the state_dict goes into a torch.optim.Adam and from there back into
    a NEW BemAdam over new parameters, which finishes the run."""
    from bem.train import BemAdam
    lr, b1, b2, eps, wd = (f32(h) for h in (1e-2, 0.9, 0.999, 1e-8, 0.01))
    kw = dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    g = G(870)
    shapes = [(7,), (25, 41)]
    init = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) for s in shapes] for _ in range(5)]

    def torch_run(dtype):
        ps = [torch.nn.Parameter(t.to(dtype).clone()) for t in init]          # .to(float32) alone would hand the step ``init`` itself
        opt = torch.optim.Adam(ps, **kw)
        for it, gs in enumerate(grads, 1):
            for i, (p, gr) in enumerate(zip(ps, gs)):
                p.grad = None if (it == 3 and i == 0) else gr.to(dtype)
            opt.step()
        return ps, opt
    (p64, o64), (p32, o32) = torch_run(F64), torch_run(F32)

    def make():
        ps = [torch.nn.Parameter(t.to(dev)) for t in init]
        return ps, BemAdam([{"params": ps}], **kw)
    ps, opt = make()
    assert opt._flat[0]["p"].numel() == 8 + 1028 and opt.defaults["weight_decay"] == wd
    for it, gs in enumerate(grads, 1):
        if it == 3:                                            # mid-run: through torch.optim.Adam and back, into fresh buffers
            sd = opt.state_dict()
            cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
            tor = torch.optim.Adam(cpu, lr=1.0)
            tor.load_state_dict(sd)
            assert tor.param_groups[0]["lr"] == lr and tor.param_groups[0]["weight_decay"] == wd
            assert [float(tor.state[q]["step"]) for q in cpu] == [2.0, 2.0]
            assert all(torch.equal(tor.state[q]["exp_avg"], opt.state[p]["exp_avg"].cpu()) for q, p in zip(cpu, ps))
            sd2, vals = tor.state_dict(), [p.detach().clone() for p in ps]
            ps, opt = make()
            with torch.no_grad():
                for p, v in zip(ps, vals):
                    p.copy_(v)
            opt.load_state_dict(sd2)
            assert opt._steps == 2 and not opt._lag
        opt.zero_grad()
        for p, gr in zip(ps, gs):
            p.grad.copy_(gr.to(dev))
        opt.step(skip=[ps[0]] if it == 3 else [])
        if it == 3:
            assert opt._lag[ps[0]] == 1 and not opt.graph_safe([])
    assert [float(opt.state[p]["step"]) for p in ps] == [4.0, 5.0] == [float(o64.state[p]["step"]) for p in p64]
    for what, pick in (("p", lambda o, q: q), ("exp_avg", lambda o, q: o.state[q]["exp_avg"]), ("exp_avg_sq", lambda o, q: o.state[q]["exp_avg_sq"])):
        got, r64, r32 = (_flat([pick(o, q) for q in qs]) for o, qs in ((opt, ps), (o64, p64), (o32, p32)))
        R.check_elementwise(got, r64, r32, what, "BemAdam 5 steps, 7 + 1025 elements")
    f = opt._flat[0]
    assert all(float(f[k][7]) == 0.0 and float(f[k][8 + 1025:].abs().max()) == 0.0 for k in ("p", "m", "v"))      # the padding words stay 0


# ---------------------------------------------------------------------------------------------------------------- 3. the losses
def pixel_loss_ref(kind, pred, gt, weight, eps, gmul, dtype, reduction="mean"):
    """weight * mean (or sum) of sqrt((pred - gt)^2 + eps) / of (pred - gt)^2, and d/dpred under an upstream gradient gmul.  Rule 2's n for
    the loss -- every term is >= 0, so S = |loss| -- counts the float32 roundings that reach it, each at most 2^-24 S when all go one way
    (the kernels add the terms in float64):
      Charbonnier  d = pred - gt (its relative error passes to the term at most once), d^2 (halved by the root), + eps (halved), the root,
                   the float32 result: 1 + 1/2 + 1/2 + 1 + 1 = 4;
      MSE          d (doubled by the square, which is exact in float64) and the float32 result: 2 + 1 = 3;
      'sum'        one more: the weight the kernel gets is float32(weight * numel)."""
    x, y = pred.detach().cpu().to(dtype).requires_grad_(), gt.detach().cpu().to(dtype)
    terms = torch.sqrt((x - y) ** 2 + eps) if kind == "charbonnier" else F.mse_loss(x, y, reduction="none")
    loss = weight * (terms.mean() if reduction == "mean" else terms.sum())
    dp, = torch.autograd.grad(loss, x, torch.tensor(gmul, dtype=dtype))
    n = (4 if kind == "charbonnier" else 3) + (reduction == "sum")
    return {"loss": R.Out(loss.detach().reshape(1), loss.detach().abs().double().reshape(1), n), "dpred": R.Out(dp)}


def _pair(n, seed):
    """pred, gt in [0,1) (|d| up to ~1) with, where there is room, d = 0 exactly (twice), |d| = 1e-7 of either sign (below sqrt(eps) =
    1e-6: the term is ~1.005e-6 and the gradient ~0.0995 weight / n, not 1e-7 and weight / n) and d = +-1."""
    g = G(seed)
    pred, gt = torch.rand(n, generator=g), torch.rand(n, generator=g)
    special = [(0.25, 0.25), (1e-7, 0.0), (0.0, 1e-7), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0)]
    at = [0, n // 3, n // 2, n - 2, n - 1, n // 5] if n >= 6 else []
    for i, (a, b) in zip(at, special):
        pred[i], gt[i] = a, b
    return pred, gt, at


def _on_device(pred, gt, dev, unaligned):
    """Contiguous device copies; ``unaligned``: views that start at element 1 of their buffers (4 bytes past a 16-byte boundary)."""
    if not unaligned:
        return pred.to(dev), gt.to(dev)
    a, b = torch.zeros(pred.numel() + 1, device=dev), torch.zeros(pred.numel() + 1, device=dev)
    a[1:].copy_(pred); b[1:].copy_(gt)
    assert a[1:].data_ptr() % 16 == 4 and a[1:].is_contiguous()
    return a[1:], b[1:]


SIZES = [1, 1000, 3 * 37 * 53]


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["charbonnier", "mse"])
def test_pixel_losses_vs_float64(dev, kind, n, unaligned):
    """ops.charbonnier_loss(_bwd) / ops.mse_loss(_bwd): n = 1 (for d = 0, |d| = 1e-7 and |d| ~ 1 in turn), 1000 and 3*37*53 = 5883 (odd:
    three floats behind the last float4; 23 workgroups), 16-byte aligned and from element 1 of a buffer (the single-float form).  Loss by
    rule 2, dpred by rule 1, with and without an upstream gmul = 3; the gradient at d = 0 is exactly 0; two calls give the same bits."""
    from bem import ops
    w, eps = 0.75, EPS
    fwd = (lambda p, g: ops.charbonnier_loss(p, g, w, eps)) if kind == "charbonnier" else (lambda p, g: ops.mse_loss(p, g, w))
    bwd = (lambda p, g, m: ops.charbonnier_loss_bwd(p, g, w, eps, m)) if kind == "charbonnier" else (lambda p, g, m: ops.mse_loss_bwd(p, g, w, m))
    if n == 1:
        cases = [(torch.tensor([a]), torch.tensor([b]), []) for a, b in ((0.5, 0.5), (1e-7, 0.0), (0.0, 1e-7), (0.9, 0.1))]
    else:
        cases = [_pair(n, 880 + n)]
    for ci, (pred, gt, at) in enumerate(cases):
        tag = f"{kind} n={n}{' unaligned' if unaligned else ''}{f' case {ci}' if n == 1 else ''}"
        p, g = _on_device(pred, gt, dev, unaligned)
        loss, dp = fwd(p, g), bwd(p, g, None)
        gm = torch.full((1,), 3.0, device=dev)
        dp3 = bwd(p, g, gm)
        o64, o32 = both(pixel_loss_ref, kind, pred, gt, w, eps, 1.0)
        R.check(loss, o64["loss"], o32["loss"], "loss", tag)
        R.check(dp, o64["dpred"], o32["dpred"], "dpred", tag)
        o64, o32 = both(pixel_loss_ref, kind, pred, gt, w, eps, 3.0)
        R.check(dp3, o64["dpred"], o32["dpred"], "dpred gmul=3", tag)
        zero = (pred == gt).nonzero().flatten().tolist()
        assert (n > 1 and len(zero) >= 2) or n == 1
        assert all(float(dp[i]) == 0.0 and float(dp3[i]) == 0.0 for i in zero), "the gradient at d = 0 is not exactly 0"
        if kind == "charbonnier" and n > 1:
            small = [i for i in at if abs(float(pred[i]) - float(gt[i])) == f32(1e-7)]
            assert len(small) == 2
            for i in small:                         # eps decides the value here: without it the gradient would be +-w / n
                assert abs(abs(float(dp[i])) - w / n * 1e-7 / math.sqrt(1e-14 + 1e-12)) <= 1e-3 * w / n, (i, float(dp[i]))
        assert torch.equal(bits(fwd(p, g)), bits(loss)) and torch.equal(bits(bwd(p, g, None)), bits(dp)), "two calls differ"
        assert torch.equal(p.cpu(), pred) and torch.equal(g.cpu(), gt)                            # the operands are read only


@pytest.mark.parametrize("name", ["CharbonnierLoss", "MSELoss"])
def test_loss_modules_mean_and_sum_under_autograd(dev, name):
    """build_loss(...)(pred, target) through bem.autograd: 'sum' against the float64 sum and against numel x the 'mean' module's value,
    backward under an upstream gradient of 3 (gmul stays on the device), the target takes no gradient."""
    from basicsr.losses import build_loss
    kind = "charbonnier" if name == "CharbonnierLoss" else "mse"
    shape, w = (2, 3, 37, 53), 0.5
    pred, gt, _ = _pair(2 * 3 * 37 * 53, 890)
    pred, gt = pred.view(shape), gt.view(shape)
    vals = {}
    for red in ("mean", "sum"):
        crit = build_loss({"type": name, "loss_weight": w, "reduction": red}).to(dev)
        x, y = pred.to(dev).requires_grad_(), gt.to(dev).requires_grad_()
        l = crit(x, y)
        assert l.shape == () and l.requires_grad
        l.backward(torch.tensor(3.0, device=dev))
        assert y.grad is None
        o64, o32 = both(pixel_loss_ref, kind, pred, gt, w, EPS, 3.0, reduction=red)
        R.check(l.detach().reshape(1), o64["loss"], o32["loss"], "loss", f"{name} {red}")
        R.check(x.grad, o64["dpred"], o32["dpred"], "dpred gmul=3", f"{name} {red}")
        vals[red] = float(l.detach())
    n = pred.numel()
    assert abs(vals["sum"] - n * vals["mean"]) <= 2 * 2.0 ** -23 * vals["sum"]          # one float32 rounding each


# ---------------------------------------------------------------------------------------------------------------- 4. the Stage-II step
def _enhancer_opt(pixel_opt):
    train = dict(total_iter=10, warmup_iter=-1, use_amp=False,                   # no max_grad_norm: the gradients are read unclipped
                 scheduler=dict(type="MultiStepLR", milestones=[1], gamma=0.5),
                 optim_g=dict(type="Adam", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]), pixel_opt=dict(pixel_opt))
    return dict(name="trainblock", model_type="ImageEnhancer", is_train=True, num_gpu=1, dist=False, rank=0, manual_seed=100,
                condition=dict(type="mean", scale_down=16, noise_level=0.0),
                network_g=dict(type="DecompDualBranchDDWavelet", in_channels=6, out_channels=3, n_feat=16, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                               mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[1, 1, 1], decomp_model="model4"),
                path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None), train=train)


@pytest.mark.parametrize("pixel_opt", [dict(type="CharbonnierLoss", loss_weight=0.5, reduction="mean"),
                                       dict(type="MSELoss", loss_weight=0.5, reduction="sum")], ids=["charbonnier-mean", "mse-sum"])
def test_image_enhancer_step_with_adam_and_the_pixel_loss(dev, pixel_opt):
    """Two iterations of ImageEnhancer (n_feat 16, blocks [1,1,1], batch 2, 32x32) under Adam + the pixel loss + MultiStepLR with a
    milestone at 1 (the second iteration runs at half the learning rate).  Per iteration: the logged l_pix is the float64 formula on the
    net's own prediction (rule 2; loss_weight 0.5 divides out exactly); the flat parameter / moment buffers after the step are
    torch.optim.Adam's -- one float64 and one float32 CPU optimizer fed the gradients read from the flat buffer before each step, at the
    scheduler's learning rate (rule 1)."""
    from basicsr.models import build_model
    from bem.pipeline import synthetic_pair
    from bem.train import BemAdam
    torch.manual_seed(100)
    m = build_model(_enhancer_opt(pixel_opt))
    opt = m.optimizer_g
    assert type(opt) is BemAdam and type(m.cri_pix).__name__ == pixel_opt["type"]
    flats = [(f, gr) for f, gr in zip(opt._flat, opt.param_groups) if f is not None]
    assert len(flats) == 1
    f, group = flats[0]
    b1, b2 = (f32(b) for b in group["betas"])
    eps, wd = f32(group["eps"]), f32(group["weight_decay"])
    assert wd == f32(1e-4)
    cpu = {}
    for dt in (F64, F32):
        q = torch.nn.Parameter(f["p"].detach().cpu().to(dt))
        cpu[dt] = (q, torch.optim.Adam([q], lr=1.0, betas=(b1, b2), eps=eps, weight_decay=wd))
    seen, before = [], []
    hook = m.net_g.register_forward_hook(lambda mod, a, out: seen.append(out[1].detach().clone()))
    real_step = opt.step

    def step(*a, **k):
        before.append(f["g"].detach().cpu().clone())
        return real_step(*a, **k)
    opt.step = step
    kind = "charbonnier" if pixel_opt["type"] == "CharbonnierLoss" else "mse"
    try:
        for it in (1, 2):
            lq, gt = synthetic_pair((2, 3, 32, 32), seed=20 + it)
            m.update_learning_rate(it, warmup_iter=-1)
            lr = m.get_current_learning_rate()[0]
            assert lr == 2e-4 * (1.0 if it == 1 else 0.5)
            m.feed_train_data(dict(lq=lq, gt=gt, gt_down=F.interpolate(gt, scale_factor=1 / 16, mode="bilinear")))
            m.optimize_parameters(it)
            tag = f"ImageEnhancer Adam + {pixel_opt['type']} {pixel_opt['reduction']} it {it}"
            assert len(seen) == it and len(before) == it and seen[-1].shape == gt.shape
            o64, o32 = both(pixel_loss_ref, kind, seen[-1], gt, 1.0, EPS, 1.0, reduction=pixel_opt["reduction"])
            R.check(torch.tensor([float(m.log_dict["l_pix"])], dtype=F64), o64["loss"], o32["loss"], "l_pix", tag)
            assert float(before[-1].abs().max()) > 0
            for dt, (q, o) in cpu.items():
                o.param_groups[0]["lr"] = f32(lr)
                q.grad = before[-1].to(dt)
                o.step()
            (q64, a64), (q32, a32) = cpu[F64], cpu[F32]
            R.check_elementwise(f["p"], q64.detach(), q32.detach(), "p", tag)
            R.check_elementwise(f["m"], a64.state[q64]["exp_avg"], a32.state[q32]["exp_avg"], "exp_avg", tag)
            R.check_elementwise(f["v"], a64.state[q64]["exp_avg_sq"], a32.state[q32]["exp_avg_sq"], "exp_avg_sq", tag)
    finally:
        hook.remove()
        opt.step = real_step


# ---------------------------------------------------------------------------------------------------------------- 5. Stage I and the driver
def _option_file(tmp_path, yml, edit):
    """A copy of a shipped option file under its own name (the run's directory names follow it) with its train block edited."""
    import yaml
    with open(os.path.join(PKG, "Options", yml)) as fh:
        opt = yaml.safe_load(fh)
    edit(opt["train"])
    os.makedirs(tmp_path / "options", exist_ok=True)
    path = str(tmp_path / "options" / yml)
    with open(path, "w") as fh:
        yaml.safe_dump(opt, fh)
    return path


def _argv(opt_path, total):
    return ["--opt", opt_path, "--synthetic", "4", "--force_yml", "network_g:n_feat=16", "network_g:num_blocks=[1,1,1]",
            f"train:total_iter={total}", "logger:save_checkpoint_freq=3", "logger:print_freq=1", "datasets:train:batch_size_per_gpu=2",
            "datasets:train:gt_size=64"]


def _run_driver(root, opt_path, total, auto_resume=False):
    from basicsr.train import train_pipeline
    torch.manual_seed(100)
    return train_pipeline(str(root), argv=_argv(opt_path, total) + (["--auto_resume"] if auto_resume else []))


LAUNCHED = """
import sys
root, pkg, run_root, opt_path, out = sys.argv[1:6]
sys.path[:0] = [root, pkg]
import torch
from basicsr.train import train_pipeline
torch.manual_seed(100)
model, info = train_pipeline(run_root, argv=eval(sys.argv[6]))
assert not getattr(model, "_graphs", None), "BEM_STAGE1_GRAPH=0 still captured"
torch.save({"iter": info["iter"], "lr": model.get_current_learning_rate(), "optimizer": type(model.optimizer_g).__name__,
            "params": {k: v.detach().cpu() for k, v in model.net_g.named_parameters()},
            "steps": [float(v["step"]) for v in model.optimizer_g.state_dict()["state"].values()],
            "l_kl": float(model.log_dict["l_kl"]), "l_pix": float(model.log_dict["l_pix"])}, out)
"""


def test_stage1_adam_mse_captured_step_equals_the_launched_one(dev, tmp_path, monkeypatch):
    """ConditionGenerator under Adam + MSELoss: eight iterations replayed from the HIP graph here against the same eight launched kernel by
    kernel in a second process (BEM_STAGE1_GRAPH=0), with the protocol and the bounds of
    tests/test_train_gpu.py::test_stage1_captured_step_equals_the_launched_one (the scheduler period ends at iteration 4: a second
    geometry without the mask, and a mask token that lags).  The first run really replayed: both geometries hold a recorded graph."""
    from bem.train import BemAdam

    def edit(train):
        train["optim_g"]["type"] = "Adam"
        train["pixel_opt"]["type"] = "MSELoss"
        train["scheduler"]["periods"] = [4, 4, 4]
    opt_path = _option_file(tmp_path, "CG_UNet_LOLv1.yml", edit)
    monkeypatch.setenv("BEM_STAGE1_GRAPH", "1")
    b, ib = _run_driver(tmp_path / "B", opt_path, 8)
    assert type(b.optimizer_g) is BemAdam and type(b.cri_pix).__name__ == "MSELoss"
    captured = [g for g in b._graphs.values() if isinstance(g, dict)]
    assert len(captured) == 2 and all(isinstance(g["graph"], torch.cuda.CUDAGraph) for g in captured)      # with and without the mask
    out = tmp_path / "launched.pt"
    env = dict(os.environ, BEM_STAGE1_GRAPH="0")
    r = subprocess.run([sys.executable, "-c", LAUNCHED, ROOT, PKG, str(tmp_path / "A"), opt_path, str(out), repr(_argv(opt_path, 8))], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    a = torch.load(out, weights_only=True)
    assert a["iter"] == ib["iter"] == 8 and a["optimizer"] == "BemAdam"
    assert a["lr"] == b.get_current_learning_rate()
    pb = dict(b.net_g.named_parameters())
    worst = max(float((a["params"][k] - pb[k].detach().cpu()).abs().max()) for k in pb)
    assert set(a["params"]) == set(pb) and worst <= 4e-5, worst
    assert a["steps"] == [float(v["step"]) for v in b.optimizer_g.state_dict()["state"].values()] and min(a["steps"]) == 4.0 < max(a["steps"]) == 8.0
    assert abs(a["l_kl"] - float(b.log_dict["l_kl"])) <= 1e-4 * max(1.0, abs(a["l_kl"]))
    assert abs(a["l_pix"] - float(b.log_dict["l_pix"])) <= 1e-4


def test_training_driver_resumes_under_cosine_annealing_restart_lr(dev, tmp_path):
    """basicsr/train.py with ``scheduler.type: CosineAnnealingRestartLR`` (periods [2, 4], the second cycle at half weight, eta_min 1e-6):
    six iterations without a break against three, a stop and --auto_resume for the rest -- the protocol and the bound of
    tests/test_train_gpu.py::test_training_driver_save_resume_reproduces_the_run.  Both end on the learning rate of the formula in the
    second cycle, which a scheduler restarted from zero (or the shipped cyclic one) would not give."""
    yml = "DecompDualBranch2DDWavelet_4.yml"
    eta = 1e-6

    def edit(train):
        train["scheduler"] = dict(type="CosineAnnealingRestartLR", periods=[2, 4], restart_weights=[1, 0.5], eta_min=eta)
    opt_path = _option_file(tmp_path, yml, edit)
    a, ia = _run_driver(tmp_path / "A", opt_path, 6)
    b0, _ = _run_driver(tmp_path / "B", opt_path, 3)
    assert type(a.schedulers[0]).__name__ == "CosineAnnealingRestartLR"
    st = tmp_path / "B" / "experiments" / yml[:-4] / "training_states"
    assert (st / "3.state").is_file()
    del b0
    b, ib = _run_driver(tmp_path / "B", opt_path, 6, auto_resume=True)
    assert ia["iter"] == ib["iter"] == 6
    assert a.get_current_learning_rate() == b.get_current_learning_rate()
    want = eta + 0.5 * 0.5 * (2e-4 - eta) * (1 + math.cos(math.pi * (3 / 4)))          # iteration 6 = scheduler epoch 5 = position 3 of the 4-long cycle
    assert abs(a.get_current_learning_rate()[0] - want) <= np.spacing(want)
    pa, pb = dict(a.net_g.named_parameters()), dict(b.net_g.named_parameters())
    worst = max(float((pa[k].detach() - pb[k].detach()).abs().max()) for k in pa)
    assert worst <= 4e-5, worst
    assert (st / "6.state").is_file()
