"""CPU: the LPIPS loss term -- the pieces of its backward restated in torch (tests/lpips_loss_ref.py) against torch's own autograd in
float64, the loss registry, the refusals of LPIPSLoss, ConditionGenerator and ImageEnhancer.  Needs no GPU."""
import types

import pytest
import torch
import torch.nn.functional as F

import lpips_loss_ref as L
import lpips_ref as R


@pytest.fixture(autouse=True, scope="module")
def _backward_entries_declared():
    """The restatements below are the yardstick of the HIP backward; they stand next to the entry points they are the yardstick of."""
    from bem import native
    want = {"bem_lpips_layer_bwd_f32", "bem_relu_pool3s2_bwd_f32", "bem_lpips_prep_bwd_f32", "bem_lpips_mean_f32"}
    assert want <= set(native.SIGNATURES), sorted(want - set(native.SIGNATURES))


def _head_case(C=64, h=5, w=7, seed=0):
    """ref and pred features (2,C,h,w) with one pixel all-zero in pred only, one in ref only, one in both."""
    g = torch.Generator().manual_seed(seed)
    y0 = torch.relu(torch.randn(2, C, h, w, generator=g, dtype=torch.float64))
    y1 = torch.relu(torch.randn(2, C, h, w, generator=g, dtype=torch.float64))
    y1[0, :, 0, 0] = 0
    y0[0, :, 1, 2] = 0
    y0[1, :, h - 1, w - 1] = 0
    y1[1, :, h - 1, w - 1] = 0
    lin = torch.rand(C, generator=g, dtype=torch.float64) * 2 / C
    return y0, y1, lin


@pytest.mark.parametrize("C", [64, 192])
def test_closed_form_head_gradient_equals_autograd_of_the_safe_norm_form(C):
    y0, y1, lin = _head_case(C)
    y1g = y1.clone().requires_grad_(True)
    assert torch.equal(L.head_safe(y0, y1, lin), R.head(y0, y1, lin))                  # the same value; only the derivative at 0 differs
    (want,) = torch.autograd.grad(L.head_safe(y0, y1g, lin).sum(), y1g)
    got = L.head_grad(y0, y1, lin)
    err, top = float((got - want).abs().max()), float(want.abs().max())
    print(f"C={C}: max |closed form - autograd| {err:.2e} on a tensor whose maximum is {top:.2e}")
    assert bool(torch.isfinite(want).all()) and top > 1e5                              # the pred-only zero pixel: r = 1e10 times D
    assert err <= 1e-14 * top


def test_naive_autograd_is_nan_where_the_closed_form_with_the_relu_mask_is_zero():
    y0, y1, lin = _head_case()
    y1g = y1.clone().requires_grad_(True)
    (naive,) = torch.autograd.grad(R.head(y0, y1g, lin).sum(), y1g)
    assert bool(torch.isnan(naive[0, :, 0, 0]).all()) and bool(torch.isnan(naive[1, :, 4, 6]).all())
    got = L.head_bwd(torch.cat([y0, y1]), lin)
    assert bool(torch.isfinite(got).all()) and not got[0, :, 0, 0].any() and not got[1, :, 4, 6].any()
    keep = torch.ones(2, 1, 5, 7, dtype=torch.bool)
    keep[0, 0, 0, 0] = keep[1, 0, 4, 6] = False
    want = torch.where(keep & (y1 > 0), naive, torch.zeros_like(naive))                # everywhere else the two agree
    assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())
    # equal features: exactly zero
    assert not L.head_bwd(torch.cat([y1, y1]), lin).any()


@pytest.mark.parametrize("H,W", L.POOL_SIZES)
def test_pool_gather_equals_max_pool2d_autograd_on_ties(H, W):
    y, dpool = L.tied_pool_case(H, W)
    yg = y.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(F.max_pool2d(yg, 3, 2), yg, dpool)
    got = L.pool_bwd(y, dpool)
    win = y.unfold(2, 3, 2).unfold(3, 3, 2).reshape(2, 3, -1, 9)
    assert int((win == win.max(-1, keepdim=True).values).sum(-1).max()) > 1                # there are tied windows
    assert torch.equal(got, want)
    assert float(got.sum()) == float(dpool.sum())


def _unblock(xs, H, W):
    """Block form (R,48,Hb,Wb) -> the planar (R,3,H,W) image it holds (restated from the forward suite)."""
    Rn, _, Hb, Wb = xs.shape
    full = xs.reshape(Rn, 3, 4, 4, Hb, Wb).permute(0, 1, 4, 2, 5, 3).reshape(Rn, 3, 4 * Hb, 4 * Wb)
    return full[:, :, 2:2 + H, 2:2 + W]


@pytest.mark.parametrize("H,W", [(31, 31), (37, 53)])
def test_index_map_of_the_input_adjoint_is_the_inverse_block_layout(H, W):
    Hb, Wb = L.block_hw(H, W)
    assert 4 * Hb >= H + 2 and 4 * Wb >= W + 2
    gxs = torch.arange(2 * 48 * Hb * Wb, dtype=torch.float64).reshape(2, 48, Hb, Wb)         # every entry distinct
    got = L.unblock_grad(gxs, H, W)
    assert torch.equal(got, _unblock(gxs, H, W)) and got.unique().numel() == got.numel()
    scale = torch.tensor(R.SCALE, dtype=torch.float64)
    assert torch.equal(L.unblock_grad(gxs, H, W, 2.0, scale), 2.0 * got / scale.view(1, 3, 1, 1))


@pytest.mark.parametrize("H,W", [(31, 31), (37, 53), (64, 66)])
def test_conv1_input_gradient_as_a_block_convolution(H, W):
    """Autograd of the strided 11x11 convolution = the zero-bordered crop in the block grid, a 3x3 pad-1 convolution with the flipped,
    transposed block weight, and the un-blocking."""
    from bem.lpips import conv1_block_weight
    g = torch.Generator().manual_seed(H + W)
    w = torch.randn(64, 3, 11, 11, generator=g, dtype=torch.float64)
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, stride=4, padding=2)
    Ho, Wo = R.sizes(H)[0], R.sizes(W)[0]
    assert y.shape == (2, 64, Ho, Wo)
    d = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(y, x, d)
    Hb, Wb = L.block_hw(H, W)
    dz = torch.zeros(2, 64, Hb, Wb, dtype=torch.float64)
    dz[:, :, 1:1 + Ho, 1:1 + Wo] = d
    wb = conv1_block_weight(w).flip(2, 3).transpose(0, 1).contiguous()
    assert wb.shape == (48, 64, 3, 3)
    got = L.unblock_grad(F.conv2d(dz, wb, padding=1), H, W)
    err = float((got - want).abs().max())
    print(f"{H}x{W}: max |block form - autograd| {err:.2e}, max |grad| {float(want.abs().max()):.2e}")
    assert err <= 1e-12 * float(want.abs().max())


def test_loss_and_grad_is_zero_for_identical_images():
    sd, lin = R.seeded_state_dicts(0)
    a = torch.rand(1, 3, 31, 31, generator=torch.Generator().manual_seed(1))
    l, g = L.loss_and_grad(sd, lin, a, a, 0.5)
    assert float(l) == 0.0 and not g.any()


# ------------------------------------------------------------------------------ the host layer
@pytest.fixture()
def weights_dir(tmp_path):
    sd, lin = R.seeded_state_dicts(0)
    torch.save(sd, tmp_path / R.ALEXNET_FILE)
    torch.save(lin, tmp_path / R.LIN_FILE)
    return str(tmp_path)


def test_registered_and_built_by_build_loss(weights_dir, tmp_path, monkeypatch):
    import basicsr.losses as BL
    from basicsr.utils.registry import LOSS_REGISTRY
    from bem.lpips import LPIPS, WEIGHTS_ENV
    assert LOSS_REGISTRY.get("LPIPSLoss") is BL.LPIPSLoss and "LPIPSLoss" in BL.__all__
    crit = BL.build_loss(dict(type="LPIPSLoss", loss_weight=0.5, weights_dir=weights_dir))
    assert isinstance(crit, BL.LPIPSLoss) and isinstance(crit.lpips, LPIPS) and crit.loss_weight == 0.5
    assert (crit.reduction, crit.net, crit.normalize) == ("mean", "alex", True)
    sd, lin = R.seeded_state_dicts(0)
    assert torch.equal(crit.lpips.conv1_weight, sd["features.3.weight"]) and torch.equal(crit.lpips.lin4, lin["lin4.model.1.weight"].reshape(-1))
    assert not crit.state_dict() and not list(crit.parameters())                   # frozen buffers, kept out of checkpoints
    monkeypatch.setenv(WEIGHTS_ENV, weights_dir)
    assert BL.build_loss(dict(type="LPIPSLoss", normalize=False)).normalize is False
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match="LPIPS weights not found"):
        BL.build_loss(dict(type="LPIPSLoss", weights_dir=str(empty)))


@pytest.mark.parametrize("kw,name", [(dict(reduction="sum"), "reduction"), (dict(reduction="none"), "reduction"), (dict(net="vgg"), "net"),
                                     (dict(net="squeeze"), "net")])
def test_unsupported_settings_raise_by_name(kw, name, weights_dir):
    from basicsr.losses import build_loss
    with pytest.raises(ValueError, match=f"Unsupported {name}"):
        build_loss(dict(type="LPIPSLoss", weights_dir=weights_dir, **kw))


def test_backward_operands_are_the_flipped_transposed_weights(weights_dir):
    from basicsr.losses import build_loss
    net = build_loss(dict(type="LPIPSLoss", weights_dir=weights_dir)).lpips
    grads = lambda: [cw.input_grad() for cw, _, _ in net.conv_operands()]
    ops_b = grads()
    assert all(a is b for a, b in zip(ops_b, grads())) and len(ops_b) == 5         # held by the module, with the forward forms
    assert [tuple(o.w.shape) for o in ops_b] == [(48, 64, 3, 3), (64, 192, 5, 5), (192, 384, 3, 3), (384, 256, 3, 3), (256, 256, 3, 3)]
    assert torch.equal(ops_b[1].w[3, 7], net.conv1_weight[7, 3].flip(0, 1))
    net.float()                                                                     # moving the module drops the packed forms
    assert not any(a is b for a, b in zip(ops_b, grads()))


def test_condition_generator_refuses_lpips_opt_before_any_gpu_call():
    from basicsr.models.condition_generator_model import ConditionGenerator
    stub = types.SimpleNamespace(net_g=torch.nn.Identity(), device="cpu", opt=dict(train=dict(
        pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean"), lpips_opt=dict(type="LPIPSLoss", loss_weight=0.5))))
    with pytest.raises(NotImplementedError, match="lpips_opt") as e:
        ConditionGenerator.init_training_settings(stub)
    assert "8x8" in str(e.value) and "31x31" in str(e.value)


def test_image_enhancer_without_any_term_still_says_all_none():
    from basicsr.models.image_enhancer_model import ImageEnhancer
    stub = types.SimpleNamespace(net_g=torch.nn.Identity(), device="cpu", opt=dict(train=dict()))
    with pytest.raises(ValueError, match="all None") as e:
        ImageEnhancer.init_training_settings(stub)
    assert "LPIPS" in str(e.value)


def test_ops_wrappers_and_header(weights_dir):
    from bem import native, ops
    assert {"bem_lpips_layer_bwd_f32", "bem_relu_pool3s2_bwd_f32", "bem_lpips_prep_bwd_f32", "bem_lpips_mean_f32"} <= set(native.SIGNATURES)
    x = torch.zeros(2, 64, 5, 7)
    for call in (lambda: ops.lpips_layer_bwd(x, torch.zeros(64)), lambda: ops.relu_pool3s2_bwd(x, torch.zeros(2, 64, 2, 3)),
                 lambda: ops.lpips_prep_bwd(torch.zeros(1, 48, 9, 10), 31, 31)):
        with pytest.raises(native.BemNativeError):
            call()


def test_train_flag_sets_the_weights_variable(tmp_path, monkeypatch):
    import os

    import yaml
    from basicsr.utils.options import parse_options
    from bem.lpips import WEIGHTS_ENV
    from conftest import PKG
    monkeypatch.setenv(WEIGHTS_ENV, "elsewhere")                                    # restored by monkeypatch after the parse overwrote it
    with open(os.path.join(PKG, "Options", "DecompDualBranch2DDWavelet_4.yml")) as f:
        opt = yaml.safe_load(f)
    yml = tmp_path / "o.yml"
    with open(yml, "w") as f:
        yaml.safe_dump(opt, f)
    state = torch.random.get_rng_state()
    try:
        parse_options(str(tmp_path), is_train=True, argv=["--opt", str(yml), "--lpips_weights", str(tmp_path / "w")])
    finally:
        torch.random.set_rng_state(state)
    assert os.environ[WEIGHTS_ENV] == str(tmp_path / "w")
