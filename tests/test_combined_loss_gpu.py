"""GPU: the CombinedLoss term (csrc/pixstat_loss.hip, bem.ops.pixstat_loss / pixstat_loss_bwd / mse_loss, bem.autograd.PixStatLossFn,
PerceptualLoss with criterion l2, basicsr.losses.CombinedLoss, ``train.combined_opt`` of ImageEnhancer) against the float64 restatement
of tests/pixstat_loss_ref.py.

Tolerance of every comparison with an f32 chain in it (that of tests/test_ssim_loss_gpu.py): the test evaluates the same restatement in
f32 on the CPU, prints that error next to the HIP error and allows 4 x the f32 restatement's error, with one f32 ulp of the largest
reference magnitude as the floor (``_allowed``).  The histogram counts are compared exactly.  The l2 perceptual term has the bound of
tests/test_perceptual_gpu.py: loss within 1e-5 relative, every gradient element within 1e-5 of the tensor's largest magnitude."""
import math

import pytest
import torch
import torch.nn.functional as F

import pixstat_loss_ref as R
import vgg_ref

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bem import native
    native.lib()
    return torch.device("cuda", 0)


def _allowed(err32, ref_max):
    return max(4.0 * err32, ULP * ref_max)


def _within_1ulp(a, b):
    inf = torch.full_like(b, float("inf"))
    return bool(((a == b) | (a == torch.nextafter(b, inf)) | (a == torch.nextafter(b, -inf))).all())


def _shapes():
    """One element; 663 elements per sample (the second sample starts 12 bytes past a 16-byte boundary); C = 1 with an odd batch; the
    edges of the whole-sample form (samples of up to K / 4 elements go to a workgroup whole, a wave each): K / 4 and K / 4 + 1; the chunk
    edges K, K + 1 (a 1-element tail chunk) and 2 K + 3; more samples than one grid dimension holds, each far below a chunk."""
    from bem import ops
    K = ops.pixstat_loss_chunk()
    return [(1, 1, 1, 1), (2, 3, 13, 17), (5, 1, 24, 40), (3, 1, 1, K // 4), (3, 1, 1, K // 4 + 1), (3, 1, 1, K), (2, 1, 1, K + 1),
            (2, 1, 1, 2 * K + 3), (65537, 1, 1, 3)]


_REF = {}


def _ref(shape):
    """(pred, gt, values64, grad64, values32, grad32, counts of pred, counts of gt) of one shape, computed once."""
    if shape not in _REF:
        pred, gt = R.pair(shape, seed=sum(shape))
        _REF[shape] = (pred, gt) + R.loss_and_grad(pred, gt, R.ALPHAS, torch.float64) + R.loss_and_grad(pred, gt, R.ALPHAS, torch.float32) \
            + (R.counts(pred), R.counts(gt))
    return _REF[shape]


def _err(a, b):
    """|a - b| of two scalars; 0 where both are the same infinity or both NaN."""
    a, b = float(a), float(b)
    return 0.0 if a == b or (math.isnan(a) and math.isnan(b)) else abs(a - b)


# ---------------------------------------------------------------------------------------------- 1. values, gradient, counts
@pytest.mark.parametrize("case", range(9))
def test_values_gradient_and_counts_vs_float64(dev, case):
    from bem import autograd as ag
    from bem import ops
    shape = _shapes()[case]
    if case == 5:
        assert shape == (3, 1, 1, 4096)
    pred, gt, v64, g64, v32, g32, hp, hg = _ref(shape)
    x, y = pred.to(dev).requires_grad_(True), gt.to(dev)
    loss, vals = ag.pixstat_loss(x, y, R.ALPHAS)
    assert loss.shape == () and loss.dtype == torch.float32 and vals.shape == (6,) and not vals.requires_grad
    loss.backward()
    assert float(loss.detach()) == float(vals[0])
    got = vals.cpu().double()
    # floor of a value: one f32 ulp of the largest magnitude its reference handles -- 40 for psnr (40 - 20 log10 ...), the largest |d|,
    # d^2 and sample mean for the means, 1 for the histogram shares -- and for the loss the sum of its terms' floors
    dmax = float((pred.double() - gt.double()).abs().max())
    mag = dict(smooth_l1=max(dmax, 1e-30), mse=max(dmax * dmax, 1e-30), psnr=40.0, color=1.0, hist=1.0)
    mag["loss"] = sum(a * mag[k] for a, k in zip(R.ALPHAS, ("smooth_l1", "hist", "psnr", "color")))
    for i, k in enumerate(R.VALUES):
        e, c = _err(got[i], v64[i]), _err(v32[i].double(), v64[i])
        print(f"{shape} {k}: {float(v64[i]):.8g} HIP err {e:.2e} (torch CPU f32 {c:.2e}, floor {ULP * mag[k]:.2e})")
        assert e <= _allowed(c, mag[k]), (k, e, c)
    eg, cg, gmax = float((x.grad.cpu().double() - g64).abs().max()), float((g32.double() - g64).abs().max()), float(g64.abs().max())
    print(f"{shape} max |grad| {gmax:.2e} HIP err {eg:.2e} (torch CPU f32 {cg:.2e}, ratio {eg / max(cg, 1e-30):.2f})")
    assert gmax > 0 and bool(torch.isfinite(x.grad).all()) and eg <= _allowed(cg, gmax), (eg, cg)
    _, hist = ops.pixstat_loss(x.detach(), y, R.ALPHAS, return_hist=True)
    assert hist.shape == (2, 256) and hist.dtype == torch.int64
    assert torch.equal(hist[0].cpu(), hp) and torch.equal(hist[1].cpu(), hg)
    assert int(hp.sum()) < pred.numel() or pred.numel() < 76                       # the planted out-of-range values are not counted


def test_forward_alone_writes_no_record_and_gives_the_same_values(dev):
    from bem import ops
    for shape in ((5, 1, 24, 40), _shapes()[7]):
        pred, gt = (t.to(dev) for t in _ref(shape)[:2])
        v0 = ops.pixstat_loss(pred, gt, R.ALPHAS)
        v1, rec = ops.pixstat_loss(pred, gt, R.ALPHAS, want_grad=True)
        assert torch.equal(v0, v1) and rec.shape == (2 + shape[0],) and rec.dtype == torch.float64 and bool(torch.isfinite(rec).all())


# ---------------------------------------------------------------------------------------------- 2. reproducible, gmul, gt, strides
@pytest.mark.parametrize("case", [2, 7])
def test_two_calls_are_bit_identical(dev, case):
    from bem import autograd as ag
    pred, gt = (t.to(dev) for t in _ref(_shapes()[case])[:2])
    out = []
    for _ in range(2):
        x = pred.clone().requires_grad_(True)
        l, vals = ag.pixstat_loss(x, gt, R.ALPHAS)
        l.backward()
        out.append((vals.clone(), x.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_the_record_holds_one_colour_coefficient_per_sample(dev):
    """-alpha6 sign(mean gt_b - mean pred_b) / n, from that sample's sums alone: the signs of the first two samples are the same with three
    more samples behind them, and they are those of the float64 means."""
    from bem import ops
    pred, gt = _ref((5, 1, 24, 40))[:2]
    want = -torch.sign(gt.double().mean(dim=(1, 2, 3)) - pred.double().mean(dim=(1, 2, 3)))
    pred, gt = pred.to(dev), gt.to(dev)
    _, r5 = ops.pixstat_loss(pred, gt, (0.0, 0.0, 0.0, 1.0), want_grad=True)
    _, r2 = ops.pixstat_loss(pred[:2].contiguous(), gt[:2].contiguous(), (0.0, 0.0, 0.0, 1.0), want_grad=True)
    assert torch.equal(r5[2:].cpu(), want / 4800.0) and torch.equal(r2[2:].cpu(), want[:2] / 1920.0) and not r5[:2].any()


def test_gmul_scales_the_gradient_and_gt_gets_none(dev):
    from bem import autograd as ag
    pred, gt = _ref((5, 1, 24, 40))[:2]
    x, y = pred.to(dev).requires_grad_(True), gt.to(dev).requires_grad_(True)
    ag.pixstat_loss(x, y, R.ALPHAS)[0].backward()
    g1 = x.grad.clone()
    assert y.grad is None
    x.grad = None
    (3 * ag.pixstat_loss(x, y, R.ALPHAS)[0]).backward()
    assert _within_1ulp(x.grad, 3 * g1) and float(g1.abs().max()) > 0


def test_non_contiguous_pred_equals_its_contiguous_copy(dev):
    from bem import autograd as ag
    gen = torch.Generator().manual_seed(7)
    big, gt = torch.rand(2, 5, 24, 40, generator=gen).to(dev), torch.rand(2, 3, 24, 40, generator=gen).to(dev)
    xs = big[:, 1:4].detach().requires_grad_(True)
    xc = big[:, 1:4].contiguous().requires_grad_(True)
    assert not xs.is_contiguous()
    (ls, vs), (lc, vc) = ag.pixstat_loss(xs, gt, R.ALPHAS), ag.pixstat_loss(xc, gt, R.ALPHAS)
    ls.backward(); lc.backward()
    assert torch.equal(vs, vc) and torch.equal(xs.grad, xc.grad)


def test_unaligned_views_take_the_scalar_path(dev):
    """Tensors that start 4 bytes into a buffer: no float4 access is possible.  The values and the gradient are those of aligned copies up
    to the order of the f64 sums (another element-to-thread assignment): one f32 ulp, 1e-12 relative in the f64 record."""
    from bem import ops
    pred, gt = (t.to(dev) for t in _ref((2, 3, 13, 17))[:2])
    n = pred.numel()
    bp, bg = torch.zeros(n + 1, device=dev), torch.zeros(n + 1, device=dev)
    bp[1:], bg[1:] = pred.flatten(), gt.flatten()
    up, ug = bp[1:].view(pred.shape), bg[1:].view(gt.shape)
    assert up.data_ptr() % 16 == 4 and up.is_contiguous()
    v0, r0 = ops.pixstat_loss(pred, gt, R.ALPHAS, want_grad=True)
    v1, r1 = ops.pixstat_loss(up, ug, R.ALPHAS, want_grad=True)
    assert _within_1ulp(v1, v0) and torch.allclose(r1, r0, rtol=1e-12, atol=0.0)
    assert _within_1ulp(ops.pixstat_loss_bwd(up, ug, r1), ops.pixstat_loss_bwd(pred, gt, r0))
    assert torch.equal(ops.pixstat_loss_bwd(up, ug, r0), ops.pixstat_loss_bwd(pred, gt, r0))            # one record: element for element


# ---------------------------------------------------------------------------------------------- 3. identical pairs, equal means, alpha3 alone
@pytest.mark.parametrize("shape", [(5, 1, 24, 40), (2, 1, 1, 4097)])
def test_identical_pair(dev, shape):
    from bem import autograd as ag
    gt = _ref((5, 1, 24, 40))[1] if shape[0] == 5 else torch.rand(shape, generator=torch.Generator().manual_seed(3))
    x = gt.clone().to(dev).requires_grad_(True)
    loss, vals = ag.pixstat_loss(x, gt.to(dev), (1.0, 0.05, 0.0, 0.25))           # alpha5 = 0: the -inf of psnr stays out of the sum
    loss.backward()
    v = dict(zip(R.VALUES, vals.tolist()))
    assert v["smooth_l1"] == 0.0 and v["mse"] == 0.0 and v["color"] == 0.0 and v["hist"] == 0.0 and v["psnr"] == float("-inf") and v["loss"] == 0.0
    assert bool(torch.isfinite(x.grad).all()) and not x.grad.any()
    x.grad = None
    loss, vals = ag.pixstat_loss(x, gt.to(dev), R.ALPHAS)                          # with the psnr term: -inf as torch gives, gradient 0 (torch: NaN)
    loss.backward()
    assert float(loss.detach()) == float("-inf") and bool(torch.isfinite(x.grad).all()) and not x.grad.any()


def test_equal_sample_means_give_no_colour_gradient_in_that_sample(dev):
    from bem import ops
    pred, gt = (t.clone() for t in _ref((5, 1, 24, 40))[:2])
    pred[0] = gt[0]
    pred, gt = pred.to(dev), gt.to(dev)
    _, rec = ops.pixstat_loss(pred, gt, (0.0, 0.0, 0.0, 1.0), want_grad=True)
    g = ops.pixstat_loss_bwd(pred, gt, rec)
    assert float(rec[2]) == 0.0 and not g[0].any() and bool((g[1:].abs() == 1.0 / pred.numel()).all())
    assert all(bool((g[b] == g[b].flatten()[0]).all()) for b in range(1, 5))


class _LaunchLog:
    """The library with every call's name recorded."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self._log.append(name)
            return fn(*a)
        return call


def test_alpha3_alone_gives_a_zero_gradient_and_launches_no_backward(dev, monkeypatch):
    from bem import autograd as ag
    from bem import native, ops
    pred, gt = _ref((5, 1, 24, 40))[:2]
    x = pred.to(dev).requires_grad_(True)
    log, lib = [], native.lib()
    monkeypatch.setattr(ops, "lib", lambda: _LaunchLog(lib, log))
    loss, vals = ag.pixstat_loss(x, gt.to(dev), (0.0, 1.0, 0.0, 0.0))
    loss.backward()
    assert log == ["bem_pixstat_loss_ws_bytes", "bem_pixstat_loss_f32"], log
    assert float(loss.detach()) == float(vals[5]) > 0 and x.grad.shape == x.shape and not x.grad.any()


# ---------------------------------------------------------------------------------------------- 4. refusals
def test_refusals(dev):
    from bem import native, ops
    z = torch.zeros(1, 3, 8, 8, device=dev)
    with pytest.raises(ValueError, match="B,C,H,W"):
        ops.pixstat_loss(z, torch.zeros(1, 3, 8, 9, device=dev), R.ALPHAS)
    with pytest.raises(ValueError, match="B,C,H,W"):
        ops.pixstat_loss(z[0], z[0], R.ALPHAS)
    with pytest.raises(TypeError):
        ops.pixstat_loss(z.double(), z.double(), R.ALPHAS)
    with pytest.raises(ValueError, match="contiguous"):
        ops.pixstat_loss(z.transpose(2, 3), z.transpose(2, 3), R.ALPHAS)
    with pytest.raises(ValueError, match="alphas"):
        ops.pixstat_loss(z, z, (1.0, -0.05, 0.0, 0.0))
    with pytest.raises(ValueError, match="record"):
        ops.pixstat_loss_bwd(z, z, torch.zeros(2, device=dev, dtype=torch.float64))
    L = native.lib()
    t = torch.zeros(4096, device=dev)
    p = t.data_ptr()
    assert L.bem_pixstat_loss_f32(p, None, p, None, p, 1, 16, 1.0, 0.0, 0.0, 0.0, None) != 0 and b"null" in L.bem_last_error()
    assert L.bem_pixstat_loss_f32(p, p, p, None, p, 1 << 20, 1 << 12, 1.0, 0.0, 0.0, 0.0, None) != 0 and b"32-bit histogram counters" in L.bem_last_error()
    assert L.bem_pixstat_loss_bwd_f32(p, p, p, p, 1 << 31, 2, None, None) != 0 and b"32-bit histogram counters" in L.bem_last_error()
    assert L.bem_pixstat_loss_f32(p, p, p, None, p, 0, 16, 1.0, 0.0, 0.0, 0.0, None) != 0 and b"empty" in L.bem_last_error()
    assert L.bem_pixstat_loss_f32(p, p, p, None, p, 1, 16, 1.0, -1.0, 0.0, 0.0, None) != 0 and b"negative alpha" in L.bem_last_error()
    assert L.bem_pixstat_loss_ws_bytes(1 << 20, 1 << 12) == 0 and L.bem_pixstat_loss_ws_bytes(1, 16) == 2048 + 16 * 2
    torch.cuda.synchronize()
    assert not t.any()


# ---------------------------------------------------------------------------------------------- 5. the MSE loss, PerceptualLoss l2
@pytest.mark.parametrize("shape", [(2, 3, 13, 17), (1, 1, 1, 1)])
def test_mse_loss_and_its_backward_vs_float64(dev, shape):
    from bem import ops
    pred, gt = R.pair(shape, seed=5 + sum(shape))
    w = 0.06
    res = {}
    for dt in (torch.float64, torch.float32):
        x = pred.to(dt).clone().requires_grad_(True)
        l = w * F.mse_loss(x, gt.to(dt))
        res[dt] = (l.detach(), torch.autograd.grad(l, x)[0])
    (l64, g64), (l32, g32) = res[torch.float64], res[torch.float32]
    l = ops.mse_loss(pred.to(dev), gt.to(dev), w)
    g = ops.mse_loss_bwd(pred.to(dev), gt.to(dev), w)
    g3 = ops.mse_loss_bwd(pred.to(dev), gt.to(dev), w, gmul=torch.full((1,), 3.0, device=dev))
    el, cl = abs(float(l) - float(l64)), abs(float(l32) - float(l64))
    eg, cg, gmax = float((g.cpu().double() - g64).abs().max()), float((g32.double() - g64).abs().max()), float(g64.abs().max())
    dmax = float((pred.double() - gt.double()).abs().max())
    print(f"{shape}: mse loss {float(l64):.6g} HIP err {el:.2e} (torch CPU f32 {cl:.2e}); max |grad| {gmax:.2e} HIP err {eg:.2e} (f32 {cg:.2e})")
    assert l.shape == (1,) and el <= _allowed(cl, w * dmax * dmax) and eg <= _allowed(cg, gmax)
    assert bool(((g3 - 3 * g).abs() <= 4 * ULP * (3 * g).abs()).all())             # gmul folds into the kernel's scale: a few roundings apart


def test_perceptual_l2_vs_float64(dev):
    from bem import autograd as ag
    from bem.percep import PerceptualLoss
    sd = vgg_ref.seeded_state_dict("conv3_3", seed=11)
    lw, pw = {"relu3_3": 1}, 0.06
    g = torch.Generator().manual_seed(12)
    pred, gt = torch.rand(2, 3, 32, 32, generator=g), torch.rand(2, 3, 32, 32, generator=g)
    l64, g64 = R.perceptual_l2_loss_and_grad(sd, pred, gt, lw, pw, torch.float64, use_input_norm=False)
    l32, g32 = R.perceptual_l2_loss_and_grad(sd, pred, gt, lw, pw, torch.float32, use_input_norm=False)
    crit = PerceptualLoss(lw, use_input_norm=False, range_norm=False, criterion="l2", perceptual_weight=pw, state_dict=sd).to(dev)
    x = pred.to(dev).requires_grad_(True)
    loss, style = crit(x, gt.to(dev))
    loss.backward()
    el, cl = abs(float(loss.detach()) - float(l64)) / float(l64), abs(float(l32) - float(l64)) / float(l64)
    gmax = float(g64.abs().max())
    eg, cg = float((x.grad.cpu().double() - g64).abs().max()) / gmax, float((g32.double() - g64).abs().max()) / gmax
    print(f"l2 perceptual loss {float(l64):.6g}: HIP rel err {el:.2e} (torch CPU f32 {cl:.2e}); gradient err / max {eg:.2e} (f32 {cg:.2e})")
    assert style is None and float(l64) > 0 and gmax > 0 and el <= 1e-5 and eg <= 1e-5
    # criterion l1 is untouched: the same module built with l1 calls the L1 entry, never the MSE one
    crit1 = PerceptualLoss(lw, use_input_norm=False, criterion="l1", perceptual_weight=pw, state_dict=sd).to(dev)
    l1 = crit1(pred.to(dev), gt.to(dev))[0]
    assert abs(float(l1) - float(vgg_ref.perceptual_loss(sd, pred, gt, lw, pw, use_input_norm=False))) <= 1e-5 * float(l1)


# ---------------------------------------------------------------------------------------------- 6. the training step
def _opt(pixel=False, combined=None):
    train = dict(total_iter=10, warmup_iter=-1, use_amp=False,                   # no max_grad_norm: the gradients are read unclipped
                 scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=[6, 4], restart_weights=[1, 1], eta_mins=[0.0002, 0.000001]),
                 optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]))
    if pixel:
        train["pixel_opt"] = dict(type="L1Loss", loss_weight=1, reduction="mean")
    if combined:
        train["combined_opt"] = dict(combined)
    return dict(name="comb", model_type="ImageEnhancer", is_train=True, num_gpu=1, dist=False, rank=0, manual_seed=100,
                condition=dict(type="mean", scale_down=16, noise_level=0.0),
                network_g=dict(type="DecompDualBranchDDWavelet", in_channels=6, out_channels=3, n_feat=8, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                               mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[1, 1, 1], decomp_model="model4"),
                path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None), train=train)


def _batch(n=2, seed=9):
    from bem.pipeline import synthetic_pair
    lq, gt = synthetic_pair((n, 3, 64, 64), seed=seed)
    return dict(lq=lq, gt=gt, gt_down=F.interpolate(gt, scale_factor=1 / 16, mode="bilinear"))


def _model(opt):
    from basicsr.models import build_model
    torch.manual_seed(100)
    return build_model(opt)


LOG_KEYS = ["l_comb", "l_comb_smooth_l1", "l_comb_percep", "l_comb_hist", "l_comb_psnr", "l_comb_color", "l_comb_ssim"]


@pytest.fixture(scope="module")
def step(dev):
    """One training step with the whole recipe at loss_weight 2 (seeded VGG weights): the model, its log, the step's preds and the
    gradient that reached them."""
    comb = dict(type="CombinedLoss", loss_weight=2.0, state_dict=vgg_ref.seeded_state_dict("conv3_3", seed=5))
    m = _model(_opt(False, comb))
    data = _batch()
    seen = []

    def hook(mod, a, out):
        seen.append(out[1].detach().clone())
        out[1].register_hook(lambda g: seen.append(g.detach().clone()))
    h = m.net_g.register_forward_hook(hook)
    try:
        m.feed_train_data(data)
        m.optimize_parameters(1)
    finally:
        h.remove()
    return dict(model=m, log=dict(m.log_dict), preds=seen[0], dpreds=seen[1], data=data)


def test_step_logs_exactly_the_terms_parts(step):
    log = step["log"]
    assert list(log) == LOG_KEYS and all(math.isfinite(float(v)) for v in log.values())
    assert all(bool(torch.isfinite(p).all()) for p in step["model"].net_g.parameters())
    a = dict(zip(LOG_KEYS[1:], (1.00, 0.06, 0.05, 0.0083, 0.25, 0.5)))
    want = sum(a[k] * float(log[k]) for k in a)
    # l_comb is the f32 sum of three f32 terms, divided by loss_weight: a few roundings of the largest term's magnitude
    big = max(abs(a[k] * float(log[k])) for k in a)
    print(f"l_comb {float(log['l_comb']):.7f} vs the sum of its weighted parts {want:.7f}")
    assert abs(float(log["l_comb"]) - want) <= 8 * ULP * max(big, abs(want))
    v64 = R.values(step["preds"].cpu(), step["data"]["gt"], R.ALPHAS)
    for k in ("smooth_l1", "hist", "psnr", "color"):               # f64 results rounded once to f32; psnr is a difference from 40
        assert abs(float(log["l_comb_" + k]) - float(v64[k])) <= ULP * (40.0 if k == "psnr" else abs(float(v64[k]))), k


def test_step_gradient_at_preds_is_the_sum_of_the_three_parts(step, dev):
    """The gradient that reached preds against the three parts' own nodes run on the same preds one by one, added in the order the fork
    chain adds them (g_pix + (g_percep + g_ssim)): the same kernels on the same operands.  Allowed: one f32 ulp of the largest gradient
    magnitude (a sum that a kernel forms in another order from launch to launch); the difference is printed."""
    from bem import autograd as ag
    crit, gt = step["model"].cri_combined, step["data"]["gt"].to(dev)
    gs = []
    for part in ("pix", "percep", "ssim"):
        x = step["preds"].clone().requires_grad_(True)
        if part == "pix":
            l = ag.pixstat_loss(x, gt, crit.pix_alphas)[0]
        elif part == "percep":
            l = crit.percep(x, gt)[0]
        else:
            l = crit.ssim(x, gt)
        l.backward()
        assert float(x.grad.abs().max()) > 0
        gs.append(x.grad)
    want = gs[0] + (gs[1] + gs[2])
    err = float((step["dpreds"] - want).abs().max())
    print(f"d preds: max |joint - sum of parts| {err:.2e}, max |grad| {float(want.abs().max()):.2e}")
    assert err <= ULP * float(want.abs().max())


def test_with_alpha2_and_alpha4_off_only_the_pixstat_entries_run(dev, monkeypatch):
    from bem import native, ops
    loss_side = ("loss", "vgg", "lpips", "ssim", "pixstat")                         # what the loss terms' entries are called
    log, lib = [], native.lib()
    m = _model(_opt(True, dict(type="CombinedLoss", alpha2=0, alpha4=0)))          # no VGG file, no SSIM window
    assert m.cri_combined.percep is None and m.cri_combined.ssim is None
    with monkeypatch.context() as mp:
        mp.setattr(ops, "lib", lambda: _LaunchLog(lib, log))
        m.feed_train_data(_batch())
        m.optimize_parameters(1)
    names = [n for n in log if any(w in n for w in loss_side)]
    # forward in the order of the terms, then the two backward launches in the order the autograd engine takes them
    assert names[:3] == ["bem_l1_loss_f32", "bem_pixstat_loss_ws_bytes", "bem_pixstat_loss_f32"], names
    assert sorted(names[3:]) == ["bem_l1_loss_f32", "bem_pixstat_loss_bwd_f32"], names
    assert list(m.log_dict) == ["l_pix", "l_comb", "l_comb_smooth_l1", "l_comb_hist", "l_comb_psnr", "l_comb_color"]
    # the two loss values meet in one bem_add_f32, the two gradients of preds in another
    assert log.index("bem_add_f32") > log.index("bem_pixstat_loss_f32") and log.count("bem_add_f32") >= 2


def test_without_combined_opt_nothing_is_built_or_launched(dev, monkeypatch):
    from bem import native, ops
    log, lib = [], native.lib()
    m = _model(_opt(True))
    assert not hasattr(m, "cri_combined")
    with monkeypatch.context() as mp:
        mp.setattr(ops, "lib", lambda: _LaunchLog(lib, log))
        m.feed_train_data(_batch())
        m.optimize_parameters(1)
    assert list(m.log_dict) == ["l_pix"] and not [n for n in log if "pixstat" in n or "mse_loss" in n]
    with pytest.raises(ValueError, match="all None"):
        _model(_opt(False))


def test_images_below_the_ssim_window_need_alpha4_off(dev):
    from basicsr.losses import build_loss
    g = torch.Generator().manual_seed(4)
    pred, gt = torch.rand(2, 3, 8, 8, generator=g).to(dev).requires_grad_(True), torch.rand(2, 3, 8, 8, generator=g).to(dev)
    crit = build_loss(dict(type="CombinedLoss", alpha2=0, alpha4=0))
    crit(pred, gt).backward()
    assert list(crit.parts) == ["smooth_l1", "hist", "psnr", "color"] and bool(torch.isfinite(pred.grad).all())
    with pytest.raises(ValueError, match="11x11"):
        build_loss(dict(type="CombinedLoss", alpha2=0))(pred, gt)
