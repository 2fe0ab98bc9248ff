"""The VGG19 perceptual loss on the GPU: the kernels of percep.hip bit for bit against torch on the CPU, PerceptualLoss against the
reference's recorded run (tests/golden/g17_perceptual.npz) and against the float64 restatement (tests/vgg_ref.py) at full depth, the
training step of ImageEnhancer with ``perceptual_opt``, and the training driver.

Bound of the f32 chains (the project's own, test_config4_full_size_default_dispatch_vs_generic_kernels): loss within 1e-5 relative,
every gradient element within 1e-5 of the tensor's largest magnitude.  A wrong tap, mask or route is orders above that.  Each such test
prints the error of the f32 torch-CPU restatement against float64 next to the HIP error (DESIGN.md section 4.6 holds the measured ratios)."""
import os

import pytest
import torch
import torch.nn.functional as F

import vgg_ref as R
from conftest import PKG, load_golden

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (3, 2), (7, 9), (8, 8), (64, 66)]            # the planes are those of B = 2, C = 3
MORE_SHAPES = [(5, 8), (6, 16), (9, 12)]                       # wide paths with a dropped odd row, and several wide units per row


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bem import native
    native.lib()
    return torch.device("cuda", 0)


def G(seed):
    return torch.Generator().manual_seed(seed)


def _planes(hw, seed, kind="randn"):
    x = torch.randn(2, 3, *hw, generator=G(seed))
    if kind == "quarter":                  # multiples of 1/4: equal positive values meet in most windows
        x = (x * 2).round() / 4
    if kind == "zero_plane":
        x[1, 1] = 0
    return x


def _within_1ulp(a, b):
    inf = torch.full_like(b, float("inf"))
    return bool(((a == b) | (a == torch.nextafter(b, inf)) | (a == torch.nextafter(b, -inf))).all())


# ---------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("hw", SHAPES + MORE_SHAPES)
@pytest.mark.parametrize("kind", ["randn", "quarter", "zero_plane"])
def test_maxpool_and_its_fused_backward_bit_exact(dev, hw, kind):
    from bem import ops
    H, W = hw
    x = _planes(hw, 10 + H * W, kind).requires_grad_(True)
    y = torch.relu(x)
    p = F.max_pool2d(y, 2, 2)
    dpool = torch.randn(p.shape, generator=G(11))
    p.backward(dpool)
    yd = y.detach().to(dev)
    assert torch.equal(ops.maxpool2(yd).cpu(), p.detach())
    assert torch.equal(ops.maxpool2(x.detach().to(dev)).cpu(), F.max_pool2d(x.detach(), 2, 2))       # negative inputs too
    dy = ops.relu_pool_bwd(yd, dpool.to(dev)).cpu()
    assert torch.equal(dy, x.grad)
    if H % 2:
        assert not dy[:, :, H - 1].any()
    if W % 2:
        assert not dy[:, :, :, W - 1].any()
    if kind == "quarter" and H * W >= 16:
        win = y.detach()[:, :, :H // 2 * 2, :W // 2 * 2].unfold(2, 2, 2).unfold(3, 2, 2).reshape(2, 3, H // 2, W // 2, 4)
        m = win.max(-1, keepdim=True).values
        assert int((((win == m) & (m > 0)).sum(-1) > 1).sum()) > 0, "the case is meant to hold positive ties"


def test_pool_refuses_planes_below_2x2(dev):
    from bem import ops
    for shp in ((2, 3, 1, 8), (2, 3, 8, 1)):
        with pytest.raises(ValueError, match="2 x 2"):
            ops.maxpool2(torch.zeros(shp, device=dev))
        with pytest.raises(ValueError, match="2 x 2"):
            ops.relu_pool_bwd(torch.zeros(shp, device=dev), torch.zeros(2, 3, 1, 1, device=dev))
    from bem import native
    L = native.lib()
    t = torch.zeros(8, device=dev)
    assert L.bem_maxpool2_f32(t.data_ptr(), t.data_ptr(), 1, 1, 8, None) != 0 and b"2 x 2" in L.bem_last_error()


@pytest.mark.parametrize("hw", SHAPES)
def test_relu_and_relu_bwd_bit_exact(dev, hw):
    from bem import ops
    x = _planes(hw, 20, "zero_plane")
    dy = torch.randn(x.shape, generator=G(21))
    y = torch.relu(x)
    assert torch.equal(ops.relu(x.to(dev)).cpu(), y)
    ref = dy * (y > 0)
    assert torch.equal(ops.relu_bwd(y.to(dev), dy.to(dev)).cpu(), ref)
    d = dy.to(dev)
    assert ops.relu_bwd(y.to(dev), d, inplace=True) is d and torch.equal(d.cpu(), ref)
    # a view that starts 4 bytes into the buffer: the single-float path
    xs, ds = x.flatten().to(dev)[1:], dy.flatten().to(dev)[1:]
    assert xs.data_ptr() % 16 == 4
    assert torch.equal(ops.relu(xs).cpu(), y.flatten()[1:]) and torch.equal(ops.relu_bwd(xs, ds).cpu(), (dy * (x > 0)).flatten()[1:])


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("range_norm", [False, True])
def test_vgg_prep_and_its_adjoint_within_1ulp(dev, hw, range_norm):
    from bem import ops
    H, W = hw
    pred, gt = torch.rand(2, 3, H, W, generator=G(30)), torch.rand(2, 3, H, W, generator=G(31))
    if range_norm:
        pred, gt = pred * 2 - 1, gt * 2 - 1
    mean, std = torch.Tensor(R.MEAN).view(1, 3, 1, 1), torch.Tensor(R.STD).view(1, 3, 1, 1)

    def ref(x):
        return ((((x + 1) / 2) if range_norm else x) - mean) / std
    xn = ops.vgg_prep(pred.to(dev), gt.to(dev), True, range_norm).cpu()
    assert xn.shape == (4, 8, H, W) and not xn[:, 3:].any()
    assert _within_1ulp(xn[:2, :3], ref(pred)) and _within_1ulp(xn[2:, :3], ref(gt))
    assert torch.equal(ops.vgg_prep(pred.to(dev), gt.to(dev), False, False).cpu()[:2, :3], pred)       # use_input_norm = False
    x = pred.clone().requires_grad_(True)
    dxn = torch.randn(4, 8, H, W, generator=G(32))
    ref(x).backward(dxn[:2, :3])
    assert _within_1ulp(ops.vgg_prep_bwd(dxn.to(dev), 2, True, range_norm).cpu(), x.grad)
    assert _within_1ulp(ops.vgg_prep_bwd(dxn[:2, :3].contiguous().to(dev), 2, True, range_norm).cpu(), x.grad)     # batch stride 3 H W


# ---------------------------------------------------------------------------------------------- the loss
def _hip_loss_and_grad(dev, sd, x, gt, layer_weights, pw):
    from bem.percep import PerceptualLoss
    crit = PerceptualLoss(dict(layer_weights), perceptual_weight=pw, state_dict=sd).to(dev)
    xd = x.to(dev).requires_grad_(True)
    loss, style = crit(xd, gt.to(dev))
    assert style is None and loss.shape == ()
    loss.backward()
    return loss.detach().cpu(), xd.grad.cpu()


def _check_chain(what, loss, dx, loss_ref, dx_ref, loss32=None, dx32=None):
    """The pass bound, after printing the errors next to those of the f32 torch-CPU restatement."""
    el = abs(float(loss) - float(loss_ref)) / abs(float(loss_ref))
    eg = float((dx.double() - dx_ref.double()).abs().max()) / float(dx_ref.abs().max())
    msg = f"{what}: HIP loss rel err {el:.2e}, grad err / max {eg:.2e}"
    if loss32 is not None:
        cl = abs(float(loss32) - float(loss_ref)) / abs(float(loss_ref))
        cg = float((dx32.double() - dx_ref).abs().max()) / float(dx_ref.abs().max())
        msg += f"; torch CPU f32 {cl:.2e}, {cg:.2e}; ratios {el / max(cl, 1e-12):.2f}, {eg / max(cg, 1e-12):.2f}"
    print(msg)
    assert el <= 1e-5, msg
    assert eg <= 1e-5, msg


def test_reproduces_the_reference_fixture(dev):
    g = load_golden("g17_perceptual")
    sd = {k: v.float() for k, v in g["sd"].items()}
    lw = {k: float(v[0]) for k, v in g["layer_weight"].items()}
    loss, dx = _hip_loss_and_grad(dev, sd, g["x"], g["gt"], lw, float(g["perceptual_weight"][0]))
    _check_chain("fixture", loss, dx, g["loss"][0], g["dx"])
    from bem.percep import VGGFeatureExtractor
    feats = VGGFeatureExtractor(list(lw), state_dict=sd).to(dev)(g["x"].to(dev))
    for k in lw:
        f = feats[k].cpu()
        assert float((f - g["feat"][k]).abs().max()) <= 1e-5 * float(g["feat"][k].abs().max()), k


@pytest.fixture(scope="module")
def sd_full():
    return R.seeded_state_dict("conv5_4", seed=5)


@pytest.mark.parametrize("hw,lw", [((32, 32), {"conv5_4": 1.0}), ((36, 40), {"conv5_4": 1.0}),
                                   ((32, 32), {"relu2_2": 0.5, "conv3_1": 1.0, "conv5_4": 0.25})])
def test_full_depth_vs_float64(dev, sd_full, hw, lw):
    """32x32: conv5 on 2x2 planes.  36x40: planes 36x40, 18x20, 9x10 (odd pool input), 4x5 (odd width: conv2d's other routes, forward and
    backward), 2x2.  Three layers: gradients join the chain at two depths."""
    x, gt = torch.rand(2, 3, *hw, generator=G(40)), torch.rand(2, 3, *hw, generator=G(41))
    loss64, dx64 = R.loss_and_grad(sd_full, x, gt, lw, 0.01, dtype=torch.float64)
    loss32, dx32 = R.loss_and_grad(sd_full, x, gt, lw, 0.01, dtype=torch.float32)
    loss, dx = _hip_loss_and_grad(dev, sd_full, x, gt, lw, 0.01)
    _check_chain(f"{hw} {sorted(lw)}", loss, dx, loss64, dx64, loss32, dx32)


def test_no_gradient_for_gt_and_none_without_requires_grad(dev, sd_full):
    from bem.percep import PerceptualLoss
    sd = {k: v for k, v in sd_full.items() if int(k.split(".")[1]) <= 2}
    crit = PerceptualLoss({"relu1_2": 1.0}, perceptual_weight=0.5, state_dict=sd).to(dev)
    x, gt = torch.rand(1, 3, 8, 8, device=dev), torch.rand(1, 3, 8, 8, device=dev, requires_grad=True)
    loss, _ = crit(x, gt)
    assert not loss.requires_grad                                   # gt never gets one (basic_loss.py:210: gt.detach())
    assert PerceptualLoss({"relu1_2": 1.0}, perceptual_weight=0, state_dict=sd)(x, gt) == (None, None)
    ref = R.perceptual_loss(sd, x.cpu().double(), gt.detach().cpu().double(), {"relu1_2": 1.0}, 0.5)
    assert abs(float(loss) - float(ref)) <= 1e-5 * float(ref)


# ---------------------------------------------------------------------------------------------- the training step
PERCEP_OPT = dict(type="PerceptualLoss", layer_weights={"conv5_4": 1}, vgg_type="vgg19", use_input_norm=True, range_norm=False,
                  perceptual_weight=0.01, style_weight=0, criterion="l1")


def _opt(pixel=True, percep=True):
    train = dict(total_iter=10, warmup_iter=-1, max_grad_norm=1, use_amp=False,
                 scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=[6, 4], restart_weights=[1, 1], eta_mins=[0.0002, 0.000001]),
                 optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]))
    if pixel:
        train["pixel_opt"] = dict(type="L1Loss", loss_weight=1, reduction="mean")
    if percep:
        train["perceptual_opt"] = dict(PERCEP_OPT)
    return dict(model_type="ImageEnhancer", is_train=True, num_gpu=1, dist=False, manual_seed=100, condition=dict(type="mean", scale_down=16, noise_level=0.0),
                network_g=dict(type="DecompDualBranchDDWavelet", in_channels=6, out_channels=3, n_feat=16, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                               mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[1, 1, 1], decomp_model="model4"),
                path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None), train=train)


@pytest.fixture(scope="module")
def vgg_file(tmp_path_factory, sd_full):
    path = tmp_path_factory.mktemp("vgg") / "vgg19_seeded.pth"
    torch.save(sd_full, path)
    return str(path)


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


def test_training_step_with_the_perceptual_term(dev, vgg_file, monkeypatch):
    """Parameter gradients of L1 + perceptual = those of the two single-loss steps on the same weights and data (the two gradients of
    ``preds`` meet in ag.fork); the log carries both terms; two steps run and move the parameters."""
    monkeypatch.setenv("BEM_VGG19_WEIGHTS", vgg_file)
    data = _batch()
    both = _model(_opt(True, True))
    sd0 = {k: v.detach().clone() for k, v in both.net_g.state_dict().items()}
    runs = {}
    for tag, m in (("both", both), ("pix", _model(_opt(True, False), sd0)), ("per", _model(_opt(False, True), sd0))):
        m.feed_train_data(data)
        m.optimize_parameters(1)
        runs[tag] = (_grads(m), dict(m.log_dict))
    gb, gp, gq = runs["both"][0], runs["pix"][0], runs["per"][0]
    assert set(gb) == set(gp) == set(gq) and len(gb) > 50
    worst = 0.0
    for k in gb:
        s = gp[k] + gq[k]
        err, scale = float((gb[k] - s).abs().max()), float(s.abs().max())
        worst = max(worst, err / max(scale, 1e-30))
        assert err <= 1e-5 * scale, (k, err, scale)
    assert any(float(gq[k].abs().max()) > 1e-3 * float(gp[k].abs().max()) for k in gb), "the perceptual term must reach the parameters"
    print(f"gradient additivity: worst err / max {worst:.2e}")
    log = runs["both"][1]
    assert list(log) == ["l_pix", "l_percep"] and list(runs["per"][1]) == ["l_percep"] and list(runs["pix"][1]) == ["l_pix"]
    assert abs(float(log["l_pix"]) - float(runs["pix"][1]["l_pix"])) <= 1e-6 * float(log["l_pix"])
    # l_percep is the module's value / perceptual_weight (image_enhancer_model.py:188)
    both2 = _model(_opt(True, True), sd0)
    both2.feed_train_data(data)
    x = torch.empty(2, 6, 64, 64, device=dev)
    from bem import ops
    ops.copy_channels(both2.lq.contiguous(), x, 0)
    ops.bilinear_up(both2.conds, 16, dst=x, dst_c0=3)
    with torch.no_grad():
        value, _ = both2.cri_perceptual(both2.net_g(x, mask=None)[1], both2.gt)
    assert abs(float(log["l_percep"]) * 0.01 - float(value)) <= 1e-5 * float(value), (float(log["l_percep"]), float(value))
    before = {k: p.detach().clone() for k, p in both.net_g.named_parameters() if p.requires_grad}
    both.feed_train_data(data)
    both.optimize_parameters(2)
    moved = sum(int(not torch.equal(p.detach(), before[k])) for k, p in both.net_g.named_parameters() if k in before)
    assert moved >= 0.9 * len(before) and all(torch.isfinite(p).all() for p in both.net_g.parameters())


class _LaunchLog:
    """Stands in for the library handle of bem.ops and notes every ``bem_*`` call: its name and its non-pointer arguments."""

    def __init__(self, L, log):
        self._L, self._log = L, log

    def __getattr__(self, name):
        f = getattr(self._L, name)
        if not name.startswith("bem_"):
            return f

        def call(*a):
            self._log.append((name, tuple(v for v in a if type(v) in (int, float))))
            return f(*a)
        return call


def test_l1_only_step_is_todays_path(dev, monkeypatch):
    """Without ``perceptual_opt`` the step is the path of before the term existed, ``ag.l1_loss(net(x)[1], gt).backward()``: the SAME
    LAUNCHES -- every library call of the step up to the end of the backward pass, by name and by every non-pointer argument, equals
    that of the bare path, and only the clip and the AdamW kernel follow; no perceptual node, no fork of ``preds``, no added loss
    terms -- and the same gradients.

    The gradients are compared to 1e-5 of each tensor's maximum and not bit for bit: the parameter gradients of this net are accumulated
    with float atomics (include/bem_hip.h, "Training step"), so the bare path does not reproduce ITSELF bit for bit.  Measured on an
    MI355X: bare path against the step 178 of 207 tensors differ, worst 3.9e-7 of the maximum; the test prints bare against bare next
    to it and holds the first to 4 x the second.  Identical launches on identical inputs is the stronger statement."""
    from bem import autograd as ag
    from bem import native, ops

    def refuse(*a, **k):
        raise AssertionError("the L1-only step must not reach this")
    data = _batch()
    m = _model(_opt(True, False))
    sd0 = {k: v.detach().clone() for k, v in m.net_g.state_dict().items()}
    forks, adds, log = [], [], []
    real_fork, real_add, L = ag.fork, ag.AddFn.apply, native.lib()
    monkeypatch.setattr(ag, "fork", lambda x: (forks.append(tuple(x.shape)), real_fork(x))[1])        # the net forks its skips: counted
    monkeypatch.setattr(ag.AddFn, "apply", lambda *a: (adds.append(tuple(a[0].shape)), real_add(*a))[1])
    monkeypatch.setattr(ag.PerceptualFn, "forward", staticmethod(refuse))
    monkeypatch.setattr(ops, "lib", lambda: _LaunchLog(L, log))
    m.feed_train_data(data)
    m.optimize_parameters(1)
    g_step, n_forks, step_log = _grads(m), len(forks), list(log)
    assert () not in adds, "no loss terms are added on the L1 path"

    def bare():
        ref = _model(_opt(True, False), sd0)
        ref.feed_train_data(data)
        del forks[:], log[:]
        ref.optimizer_g.zero_grad()
        x = torch.empty(2, 6, 64, 64, device=dev)
        ops.copy_channels(ref.lq.contiguous(), x, 0)
        ops.bilinear_up(ref.conds, 16, dst=x, dst_c0=3)
        loss = ag.l1_loss(ref.net_g(x, mask=None)[1], ref.gt)
        loss.backward()
        return _grads(ref), float(loss.detach())
    g_ref, loss_ref = bare()
    assert len(forks) == n_forks and (2, 3, 64, 64) not in forks, "the step forks what the net alone forks: not preds"
    bare_log = list(log)
    assert len(bare_log) > 100 and step_log[:len(bare_log)] == bare_log, "the step's launches up to the end of backward are the bare path's"
    rest = {n for n, _ in step_log[len(bare_log):]}
    assert rest <= {"bem_grad_sumsq_f32", "bem_adamw_step_f32"}, rest
    g_ref2, _ = bare()
    monkeypatch.undo()
    assert float(m.log_dict["l_pix"]) == loss_ref
    assert set(g_ref) == set(g_step)

    def differ(a, b):
        return (sum(int(not torch.equal(a[k], b[k])) for k in a),
                max(float((a[k] - b[k]).abs().max()) / max(float(a[k].abs().max()), 1e-30) for k in a))
    n_step, w_step = differ(g_ref, g_step)
    n_self, w_self = differ(g_ref, g_ref2)
    print(f"L1-only step vs the bare path: {n_step} of {len(g_ref)} gradient tensors differ, worst err / max {w_step:.2e}; "
          f"bare path vs itself: {n_self} differ, worst {w_self:.2e}")
    for k in g_ref:
        assert float((g_ref[k] - g_step[k]).abs().max()) <= 1e-5 * float(g_ref[k].abs().max()), k
    # and no further from the bare path than the bare path is from itself: both differences are draws of the same atomic-order noise, whose
    # worst case over 207 tensors varies by a small factor from run to run (4 allowed), with one f32 ulp of the maximum as the floor
    assert w_step <= 4 * max(w_self, 2.0 ** -23), (w_step, w_self)


# ---------------------------------------------------------------------------------------------- the driver
def test_training_driver_reports_l_percep(dev, tmp_path, sd_full, capsys):
    """basicsr/train.py with an option file that carries ``perceptual_opt`` and --vgg_weights naming a file with the layers that
    {'conv2_2': 1} needs: two iterations, ``l_percep`` in the log line."""
    import yaml

    from basicsr.train import train_pipeline
    with open(os.path.join(PKG, "Options", "DecompDualBranch2DDWavelet_4.yml")) as f:
        opt = yaml.safe_load(f)
    opt["train"]["perceptual_opt"] = dict(PERCEP_OPT, layer_weights={"conv2_2": 1})
    yml = tmp_path / "DecompDualBranch2DDWavelet_4_percep.yml"
    with open(yml, "w") as f:
        yaml.safe_dump(opt, f)
    weights = tmp_path / "vgg19_upto_conv2_2.pth"
    torch.save({k: v for k, v in sd_full.items() if int(k.split(".")[1]) <= 7}, weights)
    old = os.environ.get("BEM_VGG19_WEIGHTS")
    try:
        torch.manual_seed(100)
        model, info = train_pipeline(str(tmp_path), argv=[
            "--opt", str(yml), "--synthetic", "8", "--vgg_weights", str(weights),
            "--force_yml", "network_g:n_feat=16", "network_g:num_blocks=[1,1,1]", "train:total_iter=2", "logger:save_checkpoint_freq=100",
            "logger:print_freq=1", "datasets:train:batch_size_per_gpu=2", "datasets:train:gt_size=64", "train:scheduler:periods=[4,4,4]"])
    finally:
        if old is None:
            os.environ.pop("BEM_VGG19_WEIGHTS", None)
        else:
            os.environ["BEM_VGG19_WEIGHTS"] = old
    assert info["iter"] == 2
    log = model.get_current_log()
    assert "l_pix" in log and float(log["l_percep"]) > 0 and torch.isfinite(torch.as_tensor(float(log["l_percep"])))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "l_percep:" in ln]
    assert len(lines) == 2 and all("l_pix:" in ln for ln in lines), lines
