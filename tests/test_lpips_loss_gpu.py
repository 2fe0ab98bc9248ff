"""The LPIPS loss term (train.lpips_opt) on the GPU against the float64 torch-CPU restatement tests/lpips_loss_ref.py on seeded weights:
each backward kernel of csrc/lpips.hip alone, the whole node, the training step and the driver.

Bounds.  Head backward: 1e-6 of the float64 tensor's maximum, the forward head's bound (f64 arithmetic on f32 features; what is left is
the f32 rounding of the result).  Pool and input-stage backward: bit-equal.  Whole node: loss 1e-5 relative, gradient 1e-5 of the float64
gradient's maximum over the whole tensor -- the bounds of the VGG19 feature pass and of the metric; the f32 torch
evaluation of the same restatement is printed beside every figure and stays at or below 2.4e-6 on these cases."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_loss_ref as L
import lpips_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

WEIGHT = 0.5


@pytest.fixture(scope="module")
def sds():
    return R.seeded_state_dicts(0)


@pytest.fixture(scope="module")
def wdir(tmp_path_factory, sds):
    d = tmp_path_factory.mktemp("lpips_weights")
    torch.save(sds[0], d / R.ALEXNET_FILE)
    torch.save(sds[1], d / R.LIN_FILE)
    return str(d)


@pytest.fixture(scope="module")
def crit(wdir):
    from basicsr.losses import build_loss
    return build_loss(dict(type="LPIPSLoss", loss_weight=WEIGHT, weights_dir=wdir)).cuda()


# ------------------------------------------------------------------------------ 1. head backward
def _head_case(C, h, w, with_gin):
    """feat (6,C,h,w): rows 0..2 ref, 3..5 pred; pair 0 has a pixel all-zero in pred only, pair 1 in ref only, pair 2 in both."""
    g = torch.Generator().manual_seed(C * 100 + h * 10 + w + int(with_gin))
    f = torch.relu(torch.randn(6, C, h, w, generator=g))
    f[3, :, 0, 0] = 0
    f[1, :, h - 1, w - 1] = 0
    f[2, :, h - 1, w - 1] = 0
    f[5, :, h - 1, w - 1] = 0
    lin = torch.rand(C, generator=g) * 2 / C
    gin = torch.randn(3, C, h, w, generator=g) * 1e-3 if with_gin else None
    return f, lin, gin


@pytest.mark.parametrize("with_gin", [False, True])
@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (5, 13)])
@pytest.mark.parametrize("C", [64, 192, 384, 256])
def test_head_backward(C, h, w, with_gin):
    from bem import ops
    f, lin, gin = _head_case(C, h, w, with_gin)
    scale, up = 0.7 / 3, 1.5                                   # loss_weight / B and the upstream gradient
    want = L.head_bwd(f.double(), lin.double(), None if gin is None else gin.double(), scale * up)
    gmul = torch.tensor([up], device="cuda")
    gd = None if gin is None else gin.cuda()
    got = ops.lpips_layer_bwd(f.cuda(), lin.cuda(), gd, gmul, scale)
    assert got.shape == (3, C, h, w) and got.dtype == torch.float32
    err, top = float((got.cpu().double() - want).abs().max()), float(want.abs().max())
    print(f"head bwd C={C} {h}x{w} gin={with_gin}: max err {err:.3e}, max {top:.3e}, ratio {err / top:.2e}")
    assert top > 0 and bool(torch.isfinite(got).all()) and err <= 1e-6 * top
    assert not got[0, :, 0, 0].any() and not got[2, :, h - 1, w - 1].any()           # all-zero pred pixels: 0, not NaN
    assert torch.equal(ops.lpips_layer_bwd(f.cuda(), lin.cuda(), gd, gmul, scale), got)
    # without gmul the factor is 1
    one = ops.lpips_layer_bwd(f.cuda(), lin.cuda(), gd, None, scale * up)
    assert float((one.cpu().double() - want).abs().max()) <= 1e-6 * top
    # from a crop of a wider tensor, and into a larger output whose border comes back exactly zero
    big = torch.randn(6, C, h + 2, w + 3)
    big[:, :, 1:1 + h, 2:2 + w] = f
    assert torch.equal(ops.lpips_layer_bwd(big.cuda()[:, :, 1:1 + h, 2:2 + w], lin.cuda(), gd, gmul, scale), got)
    out = torch.full((3, C, h + 2, w + 5), float("nan"), device="cuda")
    ret = ops.lpips_layer_bwd(f.cuda(), lin.cuda(), gd, gmul, scale, out=out, origin=(1, 2))
    assert ret is out and torch.equal(out[:, :, 1:1 + h, 2:2 + w], got)
    out[:, :, 1:1 + h, 2:2 + w] = 0
    assert not out.any() and not torch.isnan(out).any()
    # the same into a view of a wider tensor: nothing outside the view is touched
    wide = torch.full((3, C, h + 1, w + 4), 7.0, device="cuda")
    ops.lpips_layer_bwd(f.cuda(), lin.cuda(), gd, gmul, scale, out=wide[:, :, :, 1:1 + w + 1], origin=(1, 0))
    assert torch.equal(wide[:, :, 1:, 1:1 + w], got) and not wide[:, :, 0, 1:2 + w].any() and not wide[:, :, :, 1 + w].any()
    assert bool((wide[:, :, :, 0] == 7).all()) and bool((wide[:, :, :, 2 + w:] == 7).all())
    if not with_gin:
        same = torch.cat([f[3:], f[3:]]).cuda()
        assert not ops.lpips_layer_bwd(same, lin.cuda(), None, gmul, scale).any()      # pred == ref: exactly zero


# ------------------------------------------------------------------------------ 2. pool backward
@pytest.mark.parametrize("H,W", L.POOL_SIZES + [(49, 74)])
def test_pool_backward(H, W):
    from bem import ops
    y, dpool = L.tied_pool_case(H, W)
    yg = y.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(F.max_pool2d(yg, 3, 2), yg, dpool)
    got = ops.relu_pool3s2_bwd(y.cuda(), dpool.cuda())
    assert got.is_contiguous() and torch.equal(got.cpu(), want)
    assert torch.equal(got.cpu(), L.pool_bwd(y, dpool))
    big = torch.full((2, 3, H + 3, W + 5), 9.0)                                       # larger than anything in y: it must not be read
    big[:, :, 1:1 + H, 2:2 + W] = y
    assert torch.equal(ops.relu_pool3s2_bwd(big.cuda()[:, :, 1:1 + H, 2:2 + W], dpool.cuda()).cpu(), want)


# ------------------------------------------------------------------------------ 3. input-stage backward
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("H,W", [(31, 31), (37, 53)])
def test_prep_backward(H, W, normalize):
    from bem import native, ops
    Hb, Wb = L.block_hw(H, W)
    gxs = torch.randn(2, 48, Hb, Wb, generator=torch.Generator().manual_seed(H + W))
    g = L.unblock_grad(gxs, H, W).numpy()
    want = (np.float32(2 if normalize else 1) * g) / np.float32(R.SCALE).reshape(1, 3, 1, 1)
    assert want.dtype == np.float32
    got = ops.lpips_prep_bwd(gxs.cuda(), H, W, normalize=normalize).cpu().numpy()
    assert got.shape == (2, 3, H, W) and np.array_equal(got, want)
    with pytest.raises(native.BemNativeError, match="mode 1"):
        ops.lpips_prep_bwd(gxs.cuda(), H, W, quantise=True)


def test_entries_refuse_bad_arguments_by_name():
    from bem import native
    lib = native.lib()
    t = torch.zeros(4096, device="cuda")
    p = t.data_ptr()
    calls = [
        (lambda: lib.bem_lpips_layer_bwd_f32(None, 35, 35, 7, p, None, None, 1.0, p, 35, 35, 7, 1, 1, 5, 7, 5, 7, 0, 0, None), b"null"),
        (lambda: lib.bem_lpips_layer_bwd_f32(p, 35, 35, 7, p, None, None, 1.0, p, 35, 35, 7, 0, 1, 5, 7, 5, 7, 0, 0, None), b"bad shape"),
        (lambda: lib.bem_lpips_layer_bwd_f32(p, 35, 35, 7, p, None, None, 1.0, p, 35, 35, 7, 1, 1, 5, 0, 5, 7, 0, 0, None), b"bad shape"),
        (lambda: lib.bem_lpips_layer_bwd_f32(p, 35, 35, 7, p, None, None, 1.0, p, 35, 35, 7, 1, 1, 5, 7, 5, 7, 1, 0, None), b"does not lie"),
        (lambda: lib.bem_lpips_layer_bwd_f32(p, 35, 35, 6, p, None, None, 1.0, p, 35, 35, 7, 1, 1, 5, 7, 5, 7, 0, 0, None), b"feature strides"),
        (lambda: lib.bem_lpips_layer_bwd_f32(p, 35, 35, 7, p, None, None, 1.0, p, 35, 34, 7, 1, 1, 5, 7, 5, 7, 0, 0, None), b"output strides"),
        (lambda: lib.bem_relu_pool3s2_bwd_f32(p, 35, 7, None, p, 1, 5, 7, None), b"null"),
        (lambda: lib.bem_relu_pool3s2_bwd_f32(p, 35, 7, p, p, 0, 5, 7, None), b"3 x 3"),
        (lambda: lib.bem_relu_pool3s2_bwd_f32(p, 35, 7, p, p, 1, 2, 7, None), b"3 x 3"),
        (lambda: lib.bem_relu_pool3s2_bwd_f32(p, 30, 7, p, p, 1, 5, 7, None), b"strides"),
        (lambda: lib.bem_lpips_prep_bwd_f32(p, None, 1, 31, 31, 0, None), b"null"),
        (lambda: lib.bem_lpips_prep_bwd_f32(p, p, 0, 31, 31, 0, None), b"batch size"),
        (lambda: lib.bem_lpips_prep_bwd_f32(p, p, 1, 30, 31, 0, None), b"31 x 31"),
        (lambda: lib.bem_lpips_prep_bwd_f32(p, p, 1, 31, 30, 2, None), b"31 x 31"),
        (lambda: lib.bem_lpips_prep_bwd_f32(p, p, 1, 31, 31, 1, None), b"mode 1"),
        (lambda: lib.bem_lpips_prep_bwd_f32(p, p, 1, 31, 31, 3, None), b"mode 3"),
        (lambda: lib.bem_lpips_mean_f32(None, p, 1, 1.0, None), b"null"),
        (lambda: lib.bem_lpips_mean_f32(p, p, 0, 1.0, None), b"batch size"),
    ]
    for call, word in calls:
        assert call() != 0 and word in lib.bem_last_error(), (word, lib.bem_last_error())
    torch.cuda.synchronize()
    assert not t.any()                                                                  # a refused call launches nothing


# ------------------------------------------------------------------------------ 4. the whole node against float64
SHAPES = [(31, 31), (37, 53), (64, 64), (100, 152)]
KINDS = ("independent", "near", "same")


def _pairs(H, W):
    """{kind: (pred, gt)} in [0,1] (``near`` leaves it slightly: nothing is clipped)."""
    g = torch.Generator().manual_seed(H * 1000 + W)
    gt = torch.rand(2, 3, H, W, generator=g)
    ind = torch.rand(2, 3, H, W, generator=g)
    noise = torch.randn(2, 3, H, W, generator=g)
    return {"independent": (ind, gt), "near": (gt + 0.1 * noise, gt), "same": (gt.clone(), gt)}


@pytest.fixture(scope="module")
def refs(sds):
    """(float64 loss and gradient, f32 torch-CPU loss and gradient) of every case, computed once."""
    out = {}
    for H, W in SHAPES:
        for kind, (pred, gt) in _pairs(H, W).items():
            out[(H, W, kind)] = (L.loss_and_grad(sds[0], sds[1], pred, gt, WEIGHT, torch.float64),
                                 L.loss_and_grad(sds[0], sds[1], pred, gt, WEIGHT, torch.float32))
    return out


def _hip(crit, pred, gt):
    p = pred.cuda().requires_grad_(True)
    loss = crit(p, gt.cuda())
    loss.backward()
    return loss.detach(), p.grad


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_loss_and_gradient_against_float64(crit, refs, H, W, kind):
    pred, gt = _pairs(H, W)[kind]
    (l64, g64), (l32, g32) = refs[(H, W, kind)]
    loss, grad = _hip(crit, pred, gt)
    assert loss.shape == () and loss.dtype == torch.float32 and grad.shape == pred.shape and grad.dtype == torch.float32
    if kind == "same":
        assert float(l64) == 0.0 and not g64.any()
        assert float(loss) == 0.0 and not grad.any()
        return
    lerr, lerr32 = abs(float(loss) - float(l64)) / float(l64), abs(float(l32) - float(l64)) / float(l64)
    top = float(g64.abs().max())
    gerr, gerr32 = float((grad.cpu().double() - g64).abs().max()) / top, float((g32.double() - g64).abs().max()) / top
    print(f"lpips loss {H}x{W} {kind}: f64 loss {float(l64):.6e}, rel err HIP {lerr:.2e} / CPU f32 {lerr32:.2e}; "
          f"gradient max {top:.3e}, err / max HIP {gerr:.2e} / CPU f32 {gerr32:.2e}")
    assert bool(torch.isfinite(g64).all()) and float(l64) > 0 and top > 0
    assert lerr <= 1e-5
    assert gerr <= 1e-5


# ------------------------------------------------------------------------------ 5. the node's behaviour
def test_node_behaviour(crit, sds):
    from bem import autograd as ag
    pred, gt = _pairs(37, 53)["independent"]
    net = crit.lpips
    before_fw = net(gt.cuda() * 2 - 1, pred.cuda() * 2 - 1).clone()
    before_01 = net.distance01(gt.cuda(), pred.cuda()).clone()
    # no gradient wanted: nothing saved, and gt never takes one
    saved = []
    real = ag.LPIPSFn.forward

    def spy(ctx, *a):
        out = real(ctx, *a)
        saved.append(len(ctx.to_save) if getattr(ctx, "to_save", None) else 0)
        return out
    ag.LPIPSFn.forward = staticmethod(spy)
    try:
        plain = crit(pred.cuda(), gt.cuda())
        with_gt = crit(pred.cuda(), gt.cuda().requires_grad_(True))
        p = pred.cuda().requires_grad_(True)
        loss = crit(p, gt.cuda())
    finally:
        ag.LPIPSFn.forward = staticmethod(real)
    assert saved == [0, 0, 5]
    assert not plain.requires_grad and not with_gt.requires_grad and loss.requires_grad
    assert torch.equal(plain, loss.detach()) and torch.equal(with_gt, plain)
    # the forward value is the metric's: weight * mean of forward(normalize=True)
    d = net(gt.cuda(), pred.cuda(), normalize=True).view(-1).double()
    assert abs(float(loss.detach()) - WEIGHT * float(d.mean())) <= 1e-6 * float(loss.detach())
    # two backward passes are bit-identical; an upstream factor scales the gradient
    (g1,) = torch.autograd.grad(loss, p, retain_graph=True)
    (g2,) = torch.autograd.grad(loss, p, retain_graph=True)
    assert torch.equal(g1, g2) and bool(g1.any())
    (g3,) = torch.autograd.grad(3 * loss, p)
    top = float(g1.abs().max())
    assert float((g3.double() - 3 * g1.double()).abs().max()) <= 1e-6 * 3 * top
    # normalize=False on inputs already in [-1,1]: the same loss, half the gradient (d(2x - 1) = 2 dx)
    from basicsr.losses import LPIPSLoss
    raw = LPIPSLoss.__new__(LPIPSLoss)
    torch.nn.Module.__init__(raw)
    raw.loss_weight, raw.normalize, raw.lpips = WEIGHT, False, net
    q = (pred.cuda() * 2 - 1).requires_grad_(True)
    lraw = raw(q, gt.cuda() * 2 - 1)
    (graw,) = torch.autograd.grad(lraw, q)
    assert abs(float(lraw.detach()) - float(loss.detach())) <= 2e-6 * float(loss.detach())
    assert float((2 * graw.double() - g1.double()).abs().max()) <= 1e-5 * top
    # the metric itself is untouched by the loss having used its module
    assert torch.equal(net(gt.cuda() * 2 - 1, pred.cuda() * 2 - 1), before_fw) and torch.equal(net.distance01(gt.cuda(), pred.cuda()), before_01)
    with pytest.raises(ValueError, match="31 x 31"):
        crit(torch.rand(1, 3, 30, 40, device="cuda"), torch.rand(1, 3, 30, 40, device="cuda"))


# ------------------------------------------------------------------------------ 6. the training step
LPIPS_OPT = dict(type="LPIPSLoss", loss_weight=WEIGHT)


def _opt(pixel=True, lpips=True):
    train = dict(total_iter=10, warmup_iter=-1, max_grad_norm=1, use_amp=False,
                 scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=[6, 4], restart_weights=[1, 1], eta_mins=[0.0002, 0.000001]),
                 optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]))
    if pixel:
        train["pixel_opt"] = dict(type="L1Loss", loss_weight=1, reduction="mean")
    if lpips:
        train["lpips_opt"] = dict(LPIPS_OPT)
    return dict(model_type="ImageEnhancer", is_train=True, num_gpu=1, dist=False, manual_seed=100, condition=dict(type="mean", scale_down=16, noise_level=0.0),
                network_g=dict(type="DecompDualBranchDDWavelet", in_channels=6, out_channels=3, n_feat=16, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                               mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[1, 1, 1], decomp_model="model4"),
                path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None), train=train)


def _batch():
    from bem.pipeline import synthetic_pair
    lq, gt = synthetic_pair((2, 3, 64, 64), seed=9)
    return dict(lq=lq, gt=gt, gt_down=F.interpolate(gt, scale_factor=1 / 16, mode="bilinear"))


def _model(opt, sd0=None):
    from basicsr.models import build_model
    torch.manual_seed(100)
    m = build_model(opt)
    if sd0 is not None:
        m.net_g.load_state_dict(sd0, strict=True)
    return m


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.net_g.named_parameters() if p.requires_grad and p.grad is not None}


@pytest.fixture()
def weights_env(wdir, monkeypatch):
    from bem.lpips import WEIGHTS_ENV
    monkeypatch.setenv(WEIGHTS_ENV, wdir)


def test_training_step_with_the_lpips_term(weights_env, tmp_path):
    """Parameter gradients of L1 + LPIPS = those of the two single-term steps on the same weights and data (the two gradients of ``preds``
    meet in ag.fork_n); the log carries both terms, l_lpips without its weight; two steps run; nothing of LPIPS reaches a checkpoint."""
    from bem import ops
    data = _batch()
    both = _model(_opt(True, True))
    sd0 = {k: v.detach().clone() for k, v in both.net_g.state_dict().items()}
    runs = {}
    for tag, m in (("both", both), ("pix", _model(_opt(True, False), sd0)), ("lp", _model(_opt(False, True), sd0))):
        m.feed_train_data(data)
        m.optimize_parameters(1)
        runs[tag] = (_grads(m), dict(m.log_dict))
    gb, gp, gq = runs["both"][0], runs["pix"][0], runs["lp"][0]
    assert set(gb) == set(gp) == set(gq) and len(gb) > 50
    worst = 0.0
    for k in gb:
        s = gp[k] + gq[k]
        err, scale = float((gb[k] - s).abs().max()), float(s.abs().max())
        worst = max(worst, err / max(scale, 1e-30))
        assert err <= 1e-5 * scale, (k, err, scale)
    print(f"gradient additivity: worst err / max {worst:.2e}")
    assert any(float(gq[k].abs().max()) > 1e-3 * float(gp[k].abs().max()) for k in gb), "the LPIPS term must reach the parameters"
    log = runs["both"][1]
    assert list(log) == ["l_pix", "l_lpips"] and list(runs["lp"][1]) == ["l_lpips"] and list(runs["pix"][1]) == ["l_pix"]
    assert abs(float(log["l_pix"]) - float(runs["pix"][1]["l_pix"])) <= 1e-6 * float(log["l_pix"])
    # l_lpips is the module's value without its weight
    both2 = _model(_opt(True, True), sd0)
    both2.feed_train_data(data)
    x = torch.empty(2, 6, 64, 64, device="cuda")
    ops.copy_channels(both2.lq.contiguous(), x, 0)
    ops.bilinear_up(both2.conds, 16, dst=x, dst_c0=3)
    with torch.no_grad():
        value = both2.cri_lpips(both2.net_g(x, mask=None)[1], both2.gt)
    assert float(value) > 0 and abs(float(log["l_lpips"]) * WEIGHT - float(value)) <= 1e-5 * float(value), (float(log["l_lpips"]), float(value))
    before = {k: p.detach().clone() for k, p in both.net_g.named_parameters() if p.requires_grad}
    both.feed_train_data(data)
    both.optimize_parameters(2)
    moved = sum(int(not torch.equal(p.detach(), before[k])) for k, p in both.net_g.named_parameters() if k in before)
    assert moved >= 0.9 * len(before) and all(torch.isfinite(p).all() for p in both.net_g.parameters())
    # frozen buffers only: neither the criterion's nor the net's state dict nor a checkpoint file holds an LPIPS key
    assert not both.cri_lpips.state_dict() and not any("lpips" in k.lower() for k in both.net_g.state_dict())
    both.opt["path"]["models"] = str(tmp_path / "models")
    ck = torch.load(both.save_network(both.net_g, "net_g", 2), weights_only=True)
    assert set(ck) == {"params"} and set(ck["params"]) == set(sd0)


class _LaunchLog:
    """Stands in for the library handle of bem.ops and notes the name of every ``bem_*`` call."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("bem_"):
            return f

        def call(*a):
            self._log.append(name)
            return f(*a)
        return call


def test_without_lpips_opt_nothing_is_built_or_launched(weights_env, monkeypatch):
    from bem import autograd as ag
    from bem import native, ops

    def refuse(*a, **k):
        raise AssertionError("no LPIPS node without lpips_opt")
    log, lib = [], native.lib()
    m = _model(_opt(True, False))
    with monkeypatch.context() as mp:
        mp.setattr(ag.LPIPSFn, "forward", staticmethod(refuse))
        mp.setattr(ops, "lib", lambda: _LaunchLog(lib, log))
        m.feed_train_data(_batch())
        m.optimize_parameters(1)
    assert m.cri_lpips is None and list(m.log_dict) == ["l_pix"]
    assert len(log) > 100 and not [n for n in log if "lpips" in n or "pool3s2" in n], sorted(set(log))
    assert not any("lpips" in k.lower() for k in m.net_g.state_dict()) and not any("lpips" in n.lower() for n, _ in m.net_g.named_buffers())
    # and with the block the step does make them
    log2 = []
    m2 = _model(_opt(True, True))
    with monkeypatch.context() as mp:
        mp.setattr(ops, "lib", lambda: _LaunchLog(lib, log2))
        m2.feed_train_data(_batch())
        m2.optimize_parameters(1)
    names = [n for n in log2 if "lpips" in n or "pool3s2" in n]
    assert names == (["bem_lpips_prep_f32", "bem_maxpool3s2_f32", "bem_maxpool3s2_f32"] + ["bem_lpips_layer_ws_elems", "bem_lpips_layer_f32"] * 5
                     + ["bem_lpips_mean_f32"] + ["bem_lpips_layer_bwd_f32"] * 3 + ["bem_relu_pool3s2_bwd_f32", "bem_lpips_layer_bwd_f32"] * 2
                     + ["bem_lpips_prep_bwd_f32"]), names
    with pytest.raises(ValueError, match="all None"):
        _model(_opt(False, False))


# ------------------------------------------------------------------------------ 7. the driver
def _driver_args(tmp_path, wdir):
    import yaml
    with open(os.path.join(PKG, "Options", "DecompDualBranch2DDWavelet_4.yml")) as f:
        opt = yaml.safe_load(f)
    opt["train"]["lpips_opt"] = dict(LPIPS_OPT)
    yml = tmp_path / "DecompDualBranch2DDWavelet_4_lpips.yml"
    with open(yml, "w") as f:
        yaml.safe_dump(opt, f)
    return ["--opt", str(yml), "--synthetic", "8", "--lpips_weights", wdir,
            "--force_yml", "network_g:n_feat=16", "network_g:num_blocks=[1,1,1]", "train:total_iter=2", "logger:save_checkpoint_freq=100",
            "logger:print_freq=1", "datasets:train:batch_size_per_gpu=2", "datasets:train:gt_size=64", "train:scheduler:periods=[4,4,4]"]


def test_training_driver_reports_l_lpips(tmp_path, wdir, capsys, monkeypatch):
    """basicsr/train.py with an option file that carries ``lpips_opt`` and --lpips_weights: two iterations, ``l_lpips`` in the log line;
    with the files missing the run stops with the FileNotFoundError of bem.lpips before a model is built."""
    import basicsr.train as drv
    from bem.lpips import WEIGHTS_ENV
    monkeypatch.setenv(WEIGHTS_ENV, "unset-by-the-driver")                       # parse_options overwrites it; monkeypatch restores it
    torch.manual_seed(100)
    model, info = drv.train_pipeline(str(tmp_path), argv=_driver_args(tmp_path, wdir))
    assert info["iter"] == 2
    log = model.get_current_log()
    assert "l_pix" in log and float(log["l_lpips"]) > 0 and np.isfinite(float(log["l_lpips"]))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "l_lpips:" in ln]
    assert len(lines) == 2 and all("l_pix:" in ln for ln in lines), lines
    empty = tmp_path / "no_weights"
    empty.mkdir()

    def refuse(*a, **k):
        raise AssertionError("the model must not be built when the weight files are missing")
    monkeypatch.setattr(drv, "build_model", refuse)
    with pytest.raises(FileNotFoundError, match="LPIPS weights not found"):
        drv.train_pipeline(str(tmp_path), argv=_driver_args(tmp_path, str(empty)))
