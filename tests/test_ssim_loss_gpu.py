"""GPU: the SSIM loss term (csrc/ssim_loss.hip, bem.ops.ssim_loss / ssim_loss_bwd, bem.autograd.SSIMLossFn, basicsr.losses.SSIMLoss,
``train.ssim_opt`` of ImageEnhancer) against the float64 restatement of tests/ssim_loss_ref.py, and validation SSIM.

Tolerance of every comparison with an f32 chain in it: the test evaluates the same restatement in f32 on the CPU, prints that error
next to the HIP error and allows 4 x the f32 restatement's worst error, with one f32 ulp of the largest reference magnitude as the floor
(``_allowed``).  DESIGN.md section 4.11 holds the measured ratios."""
import math

import pytest
import torch
import torch.nn.functional as F

import ssim_loss_ref as R

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
    """One valid position; a valid region below one tile; the valid region one more than a whole number of tiles in each direction
    (2 x 3 tiles: 43 x 75 with the kernel's 32 x 32 tile); C != 3 with an odd batch; more planes than one grid dimension holds (the
    planes go through grid.y and grid.z, 32768 per z step)."""
    from bem import ops
    T = ops.ssim_loss_tile()
    return [(2, 3, 11, 11), (2, 3, 13, 17), (1, 3, T + 11, 2 * T + 11), (5, 1, 24, 40), (32768 + 5, 1, 11, 11)]


_REF = {}


def _ref(shape, weight=0.5):
    """(pred, gt, loss64, grad64, loss32, grad32) of one shape, computed once."""
    if shape not in _REF:
        pred, gt = R.pair(shape, seed=sum(shape))
        _REF[shape] = (pred, gt) + R.loss_and_grad(pred, gt, weight, torch.float64) + R.loss_and_grad(pred, gt, weight, torch.float32)
    return _REF[shape]


# ---------------------------------------------------------------------------------------------- 1. loss and gradient
@pytest.mark.parametrize("case", range(5))
def test_loss_and_gradient_vs_float64(dev, case):
    from bem import autograd as ag
    shape = _shapes()[case]
    if case == 2:
        assert shape == (1, 3, 43, 75)
    pred, gt, l64, g64, l32, g32 = _ref(shape)
    x = pred.to(dev).requires_grad_(True)
    loss = ag.ssim_loss(x, gt.to(dev), 0.5)
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    el, eg = abs(float(loss.detach()) - float(l64)), float((x.grad.cpu().double() - g64).abs().max())
    cl, cg = abs(float(l32) - float(l64)), float((g32.double() - g64).abs().max())
    # Floors: one f32 ulp of the largest reference magnitude.  For the gradient that is its largest element.  The loss is weight * (1 - the
    # mean of the S map), so the magnitudes its reference handles are the S values it averages, not the small difference left at the end:
    # the floor is one f32 ulp of weight * max |S| (about 6e-8 here).  Its f32 yardstick is this shape's own draw (2.9e-9 at (2,3,13,17)).
    gmax, smax = float(g64.abs().max()), 0.5 * float(R.ssim_map(pred, gt).abs().max())
    print(f"{shape}: loss {float(l64):.6f} HIP err {el:.2e} (torch CPU f32 {cl:.2e}, ratio {el / max(cl, 1e-30):.2f}, floor {ULP * smax:.2e}); "
          f"max |grad| {gmax:.2e} HIP err {eg:.2e} (f32 {cg:.2e}, ratio {eg / max(cg, 1e-30):.2f})")
    assert el <= _allowed(cl, smax), (el, cl, smax)
    assert eg <= _allowed(cg, gmax), (eg, cg)


def test_forward_alone_writes_no_maps_and_gives_the_same_loss(dev):
    from bem import ops
    pred, gt = (t.to(dev) for t in _ref((5, 1, 24, 40))[:2])
    l0 = ops.ssim_loss(pred, gt, 0.5)
    l1, coef = ops.ssim_loss(pred, gt, 0.5, want_grad=True)
    assert torch.equal(l0, l1) and coef.shape == (3, 5, 1, 14, 30) and bool(torch.isfinite(coef).all())


# ---------------------------------------------------------------------------------------------- 2. gmul, gt, non-contiguous pred
def test_gmul_scales_the_gradient_and_gt_gets_none(dev):
    from bem import autograd as ag
    pred, gt = _ref((5, 1, 24, 40))[:2]
    x, y = pred.to(dev).requires_grad_(True), gt.to(dev).requires_grad_(True)
    ag.ssim_loss(x, y, 0.5).backward()
    g1 = x.grad.clone()
    assert y.grad is None
    x.grad = None
    (3 * ag.ssim_loss(x, y, 0.5)).backward()
    assert _within_1ulp(x.grad, 3 * g1) and float(g1.abs().max()) > 0


def test_non_contiguous_pred_equals_its_contiguous_copy(dev):
    from bem import autograd as ag
    gen = torch.Generator().manual_seed(7)
    big, gt = torch.rand(2, 5, 24, 40, generator=gen).to(dev), torch.rand(2, 3, 24, 40, generator=gen).to(dev)
    xs = big[:, 1:4].detach().requires_grad_(True)
    xc = big[:, 1:4].contiguous().requires_grad_(True)
    assert not xs.is_contiguous()
    ls, lc = ag.ssim_loss(xs, gt, 1.0), ag.ssim_loss(xc, gt, 1.0)
    ls.backward(); lc.backward()
    assert torch.equal(ls, lc) and torch.equal(xs.grad, xc.grad)


# ---------------------------------------------------------------------------------------------- 3. reproducible
def test_two_calls_are_bit_identical(dev):
    from bem import autograd as ag
    pred, gt = (t.to(dev) for t in _ref(_shapes()[2])[:2])
    out = []
    for _ in range(2):
        x = pred.clone().requires_grad_(True)
        l = ag.ssim_loss(x, gt, 0.5)
        l.backward()
        out.append((l.detach().clone(), x.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ---------------------------------------------------------------------------------------------- 4. all-zero and identical pairs
@pytest.mark.parametrize("kind", ["zero", "identical"])
def test_zero_and_identical_pairs(dev, kind):
    from bem import autograd as ag
    gt = torch.zeros(2, 3, 24, 40) if kind == "zero" else _ref((5, 1, 24, 40))[1]
    x = gt.clone().to(dev).requires_grad_(True)
    loss = ag.ssim_loss(x, gt.to(dev), 1.0)
    loss.backward()
    assert abs(float(loss.detach())) <= ULP and bool(torch.isfinite(x.grad).all())
    assert float(loss.detach()) == 0.0           # more than is asked: S is one division of two equal products and the mean a division by Npos
    if kind == "zero":
        assert not x.grad.any()


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals(dev):
    from bem import native, ops
    z = torch.zeros(1, 3, 10, 16, device=dev)
    for a, b in ((z, z), (z.transpose(2, 3).contiguous(), z.transpose(2, 3).contiguous())):
        with pytest.raises(ValueError, match="11x11"):
            ops.ssim_loss(a, b)
    with pytest.raises(ValueError, match="11x11"):
        ops.ssim_loss_bwd(z, z, torch.zeros(3, 1, 3, 1, 6, device=dev))
    with pytest.raises(ValueError):
        ops.ssim_loss(torch.zeros(1, 3, 16, 16, device=dev), torch.zeros(1, 3, 16, 17, device=dev))
    with pytest.raises(ValueError):
        ops.ssim_loss_bwd(torch.zeros(1, 3, 16, 16, device=dev), torch.zeros(1, 3, 16, 16, device=dev), torch.zeros(3, 1, 3, 6, 5, device=dev))
    L = native.lib()
    t = torch.zeros(512, device=dev)
    p = t.data_ptr()
    assert L.bem_ssim_loss_f32(p, p, p, None, p, 1, 10, 16, 1.0, None) != 0 and b"11x11" in L.bem_last_error()
    assert L.bem_ssim_loss_bwd_f32(p, p, p, p, 1, 16, 10, 1.0, None, None) != 0 and b"11x11" in L.bem_last_error()
    assert L.bem_ssim_loss_f32(p, None, p, None, p, 1, 16, 16, 1.0, None) != 0 and b"null" in L.bem_last_error()
    assert L.bem_ssim_loss_f32(p, p, p, None, p, 32768 * 65535 + 1, 11, 11, 1.0, None) != 0 and b"planes" in L.bem_last_error()
    torch.cuda.synchronize()
    assert not t.any()


# ---------------------------------------------------------------------------------------------- 6. the training step
SSIM_OPT = dict(type="SSIMLoss", loss_weight=0.5)
PERCEP_OPT = dict(type="PerceptualLoss", layer_weights={"conv5_4": 1}, vgg_type="vgg19", use_input_norm=True, range_norm=False,
                  perceptual_weight=0.01, style_weight=0, criterion="l1")


def _opt(pixel=True, ssim=None, percep=False, metrics=None):
    train = dict(total_iter=10, warmup_iter=-1, use_amp=False,                   # no max_grad_norm: the gradients are read unclipped
                 scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=[6, 4], restart_weights=[1, 1], eta_mins=[0.0002, 0.000001]),
                 optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]))
    if pixel:
        train["pixel_opt"] = dict(type="L1Loss", loss_weight=1, reduction="mean")
    if ssim:
        train["ssim_opt"] = dict(ssim)
    if percep:
        train["perceptual_opt"] = dict(PERCEP_OPT)
    opt = dict(name="ssim", model_type="ImageEnhancer", is_train=True, num_gpu=1, dist=False, rank=0, manual_seed=100,
               condition=dict(type="mean", scale_down=16, noise_level=0.0),
               network_g=dict(type="DecompDualBranchDDWavelet", in_channels=6, out_channels=3, n_feat=8, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                              mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[1, 1, 1], decomp_model="model4"),
               path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None), train=train)
    if metrics is not None:
        opt["val"] = dict(window_size=16, save_img=False, metrics=metrics)
    return opt


def _batch(n=2, seed=9):
    from bem.pipeline import synthetic_pair
    lq, gt = synthetic_pair((n, 3, 32, 32), seed=seed)
    return dict(lq=lq, gt=gt, gt_down=F.interpolate(gt, scale_factor=1 / 16, mode="bilinear"))


def _model(opt, sd0=None):
    from basicsr.models import build_model
    torch.manual_seed(100)
    m = build_model(opt)
    if sd0 is not None:
        m.net_g.load_state_dict(sd0, strict=True)
    return m


def _step(m, data):
    """One training step -> (parameter gradients, log, that step's preds)."""
    seen = []
    h = m.net_g.register_forward_hook(lambda mod, a, out: seen.append(out[1].detach().clone()))
    try:
        m.feed_train_data(data)
        m.optimize_parameters(1)
    finally:
        h.remove()
    grads = {k: p.grad.detach().clone() for k, p in m.net_g.named_parameters() if p.requires_grad and p.grad is not None}
    return grads, dict(m.log_dict), seen[0]


def _rel(a, b):
    """Worst over the tensors of max |a - b| / max |b|."""
    return max(float((a[k] - b[k]).abs().max()) / max(float(b[k].abs().max()), 1e-30) for k in b)


@pytest.fixture(scope="module")
def steps(dev):
    """One step each of L1 + SSIM, L1 alone, SSIM alone and SSIM alone at three times the weight, from the same weights and batch."""
    data = _batch()
    both = _model(_opt(True, SSIM_OPT))
    sd0 = {k: v.detach().clone() for k, v in both.net_g.state_dict().items()}
    runs = {"both": _step(both, data)}
    for tag, opt in (("pix", _opt(True)), ("ssim", _opt(False, SSIM_OPT)), ("ssim3", _opt(False, dict(SSIM_OPT, loss_weight=1.5)))):
        m = _model(opt, sd0)
        runs[tag] = _step(m, data)
        if tag == "pix":
            assert m.cri_ssim is None
    return dict(runs=runs, data=data, model=both)


def test_step_logs_the_unweighted_term(steps):
    _, log, preds = steps["runs"]["both"]
    assert list(log) == ["l_pix", "l_ssim"] and list(steps["runs"]["ssim"][1]) == ["l_ssim"]
    gt = steps["data"]["gt"]
    l64, l32 = float(R.loss(preds.cpu(), gt, 1.0, torch.float64)), float(R.loss(preds.cpu(), gt, 1.0, torch.float32))
    err, err32 = abs(float(log["l_ssim"]) - l64), abs(l32 - l64)
    print(f"l_ssim {float(log['l_ssim']):.6f} vs float64 {l64:.6f}: err {err:.2e}, torch CPU f32 {err32:.2e}")
    assert 0 < l64 < 2 and err <= _allowed(err32, l64)                # 1 - SSIM lies in [0, 2]; an untrained net sits near 1


def test_step_gradients_are_the_sum_of_the_single_loss_steps(steps):
    """L1 + SSIM against L1-only + SSIM-only.  Both sides are f32 evaluations of one real quantity through the same backward chain with
    the roundings placed differently (the joint step rounds the sum at preds and carries it through the chain once).  There is no f32
    CPU restatement of the whole net to take the yardstick of item 1 from, so the f32 figure is the chain evaluated a second time with its
    roundings displaced: the SSIM-only step at three times the weight, divided by 3, against the SSIM-only step (the float-atomic order
    noise of the parameter gradients is in both figures; the rule of test_perceptual_gpu.py's path-against-itself check).  Both figures
    are errors divided by the tensor's largest magnitude, so the floor, one f32 ulp of that magnitude, is 2^-23 of 1.  The yardstick is
    one draw per run: two runs on an MI355X gave the figures quoted in DESIGN.md section 4.11; its spread beyond those is not measured."""
    r = steps["runs"]
    gb, gp, gq, gq3 = (r[t][0] for t in ("both", "pix", "ssim", "ssim3"))
    assert set(gb) == set(gp) == set(gq) == set(gq3) and len(gb) > 50
    err = _rel(gb, {k: gp[k] + gq[k] for k in gb})
    err32 = _rel({k: v / 3 for k, v in gq3.items()}, gq)
    print(f"gradient additivity: worst err / max {err:.2e}; the chain against itself at 3 x the weight {err32:.2e}, ratio {err / max(err32, 1e-30):.2f}")
    assert any(float(gq[k].abs().max()) > 1e-3 * float(gp[k].abs().max()) for k in gb), "the SSIM term must reach the parameters"
    assert err <= _allowed(err32, 1.0), (err, err32)


def test_without_ssim_opt_nothing_is_built(steps, monkeypatch):
    from bem import ops

    def refuse(*a, **k):
        raise AssertionError("no SSIM launch without ssim_opt")
    m = _model(_opt(True))
    monkeypatch.setattr(ops, "ssim_loss", refuse)
    monkeypatch.setattr(ops, "ssim_loss_bwd", refuse)
    _, log, _ = _step(m, steps["data"])
    assert m.cri_ssim is None and list(log) == ["l_pix"]
    with pytest.raises(ValueError, match="all None"):
        _model(_opt(False))


def test_three_terms_in_one_step(dev, tmp_path, monkeypatch):
    import vgg_ref
    path = tmp_path / "vgg19_seeded.pth"
    torch.save(vgg_ref.seeded_state_dict("conv5_4", seed=5), path)
    monkeypatch.setenv("BEM_VGG19_WEIGHTS", str(path))
    m = _model(_opt(True, SSIM_OPT, percep=True))
    _, log, _ = _step(m, _batch())
    assert list(log) == ["l_pix", "l_percep", "l_ssim"] and all(math.isfinite(float(v)) and float(v) > 0 for v in log.values())
    assert all(bool(torch.isfinite(p).all()) for p in m.net_g.parameters())


# ---------------------------------------------------------------------------------------------- 7. validation SSIM
METRICS = dict(psnr=dict(type="calculate_psnr", crop_border=0, test_y_channel=False),
               ssim=dict(type="calculate_ssim", crop_border=0, test_y_channel=False))


class _Loader(list):
    dataset = None


def _val_loader():
    a, b = _batch(1, seed=5), _batch(1, seed=6)
    b["crop_hw"] = (30, 27)
    return _Loader([a, b])


def test_validation_reports_ssim_and_leaves_psnr_alone(dev, capsys):
    from bem import ops
    m = _model(_opt(True, metrics=METRICS))
    sd0 = {k: v.detach().clone() for k, v in m.net_g.state_dict().items()}
    seen = []
    h = m.net_g.register_forward_hook(lambda mod, a, out: seen.append(out[-1].detach().clone()))
    try:
        ret = m.validation(_val_loader(), 1)
    finally:
        h.remove()
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Validation")]
    want = []
    for data, pred in zip(_val_loader(), seen):
        hh, ww = data.get("crop_hw", (32, 32))
        want.append(float(ops.ssim(pred[..., :hh, :ww].contiguous(), data["gt"].to(dev)[..., :hh, :ww].contiguous(), 1)))
    assert len(want) == 2 and m.metric_results["ssim"] == sum(want) / 2 and 0 < m.metric_results["ssim"] < 1
    assert len(line) == 1 and "# psnr:" in line[0] and line[0].endswith(f"\t # ssim: {m.metric_results['ssim']:.4f}")
    opt = _opt(True, metrics={"psnr": METRICS["psnr"]})
    m0 = _model(opt, sd0)
    ret0 = m0.validation(_val_loader(), 1)
    assert ret == ret0 == m.metric_results["psnr"] == m0.metric_results["psnr"] and list(m0.metric_results) == ["psnr"]
    assert "ssim" not in capsys.readouterr().out


def test_validation_refuses_crop_border_and_y_channel_by_name(dev):
    for bad in (dict(crop_border=4), dict(test_y_channel=True)):
        metrics = dict(METRICS, ssim=dict(METRICS["ssim"], **bad))
        with pytest.raises(NotImplementedError, match=list(bad)[0]):
            _model(_opt(True, metrics=metrics))
    m = _model(_opt(True, metrics=METRICS))
    m.opt["val"]["metrics"]["ssim"] = dict(METRICS["ssim"], crop_border=4)
    with pytest.raises(NotImplementedError, match="crop_border"):
        m.validation(_val_loader(), 1)


def test_validation_of_images_below_the_window_gives_nan(dev, capsys):
    m = _model(_opt(True, metrics=METRICS))
    a, b = _batch(1, seed=5), _batch(1, seed=6)
    a["crop_hw"] = b["crop_hw"] = (8, 8)
    ret = m.validation(_Loader([a, b]), 1)
    out = capsys.readouterr().out
    assert math.isnan(m.metric_results["ssim"]) and math.isfinite(ret) and ret == m.metric_results["psnr"]
    assert out.count("Warning") == 1 and "# ssim: nan" in out
