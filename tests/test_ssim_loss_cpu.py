"""CPU: the SSIM loss term -- the float64 restatement against its own hand-written gradient (the formula the HIP backward implements),
the loss registry, the refusals of SSIMLoss and of ConditionGenerator, and the two C ABI symbols.  Needs no GPU and no library."""
import os
import re
import types

import pytest
import torch

import ssim_loss_ref as R
from conftest import ROOT


@pytest.mark.parametrize("hw", [(11, 11), (13, 17), (43, 75)])
def test_autograd_gradient_equals_the_hand_formula_in_float64(hw):
    pred, gt = R.pair((2, 3) + hw, seed=100 + hw[0])
    l, g = R.loss_and_grad(pred, gt, 0.5)
    f = R.grad_formula(pred, gt, 0.5)
    assert g.dtype == f.dtype == torch.float64 and g.shape == f.shape == pred.shape
    err = float((g - f).abs().max())
    print(f"{hw}: loss {float(l):.6f}, max |autograd - formula| {err:.2e}, max |grad| {float(g.abs().max()):.2e}")
    assert float(g.abs().max()) > 0 and err <= 1e-14


def test_identical_all_zero_images_give_loss_0_and_gradient_0():
    z = torch.zeros(1, 3, 16, 20)
    for dtype in (torch.float64, torch.float32):
        l, g = R.loss_and_grad(z, z, 1.0, dtype)
        assert float(l) == 0.0 and not g.any() and not R.grad_formula(z, z, 1.0, dtype).any()


def test_window_is_the_normalised_gaussian():
    g = R.window(torch.float64)
    assert g.shape == (11,) and abs(float(g.sum()) - 1) < 1e-15 and torch.equal(g, g.flip(0)) and int(g.argmax()) == 5
    assert abs(float(g[4] / g[5]) - float(torch.exp(torch.tensor(-1 / 4.5, dtype=torch.float64)))) < 1e-15


def test_registered_and_built_by_build_loss():
    import basicsr.losses as L
    from basicsr.utils.registry import LOSS_REGISTRY
    assert LOSS_REGISTRY.get("SSIMLoss") is L.SSIMLoss and "SSIMLoss" in L.__all__
    crit = L.build_loss({"type": "SSIMLoss", "loss_weight": 0.5})
    assert isinstance(crit, L.SSIMLoss) and crit.loss_weight == 0.5 and (crit.reduction, crit.window_size, crit.sigma) == ("mean", 11, 1.5)
    assert L.build_loss({"type": "SSIMLoss"}).loss_weight == 1.0


@pytest.mark.parametrize("kw,name", [(dict(reduction="sum"), "reduction"), (dict(reduction="none"), "reduction"),
                                     (dict(window_size=7), "window_size"), (dict(sigma=1.0), "sigma")])
def test_unsupported_settings_raise_by_name(kw, name):
    from basicsr.losses import build_loss
    with pytest.raises(ValueError, match=name):
        build_loss(dict(type="SSIMLoss", loss_weight=0.5, **kw))


def test_condition_generator_refuses_ssim_opt_before_any_gpu_call():
    """Stage I predicts 8x8 planes, smaller than the window: refused by name where the losses are built, ahead of everything else."""
    from basicsr.models.condition_generator_model import ConditionGenerator
    stub = types.SimpleNamespace(net_g=torch.nn.Identity(), device="cpu", opt=dict(train=dict(
        pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean"), ssim_opt=dict(type="SSIMLoss", loss_weight=0.5))))
    with pytest.raises(NotImplementedError, match="ssim_opt") as e:
        ConditionGenerator.init_training_settings(stub)
    assert "8x8" in str(e.value) and "11x11" in str(e.value)


def test_header_declares_both_entry_points_next_to_the_l1_loss():
    from bem import native
    with open(os.path.join(ROOT, "include", "bem_hip.h")) as f:
        text = f.read()
    assert {"bem_ssim_loss_f32", "bem_ssim_loss_bwd_f32", "bem_ssim_loss_tile", "bem_ssim_loss_ws_elems"} <= set(native.SIGNATURES)
    assert len(native.SIGNATURES["bem_ssim_loss_f32"]) == 10 and len(native.SIGNATURES["bem_ssim_loss_bwd_f32"]) == 10
    l1, fwd, bwd = (text.index(f"int {n}(") for n in ("bem_l1_loss_f32", "bem_ssim_loss_f32", "bem_ssim_loss_bwd_f32"))
    assert l1 < fwd < bwd and "int bem_" not in text[l1 + 10:text.index("int bem_ssim_loss_tile")]
    for at in (fwd, bwd):                          # each entry's comment cites the reference's lines
        assert re.search(r"basicsr/losses/my_loss\.py:37-38", text[text.rindex("/*", 0, at):at])


def test_ops_wrappers_refuse_cpu_tensors_and_state_their_cost():
    from bem import native, ops
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(native.BemNativeError):
        ops.ssim_loss(x, x)
    assert ops.ssim_loss_cost(x, want_grad=True) == (8.0 * x.numel() + 12.0 * 3 * 36, 3 * 36 * (220 + 40.0))
