"""CPU: the CombinedLoss term -- the float64 restatement of tests/pixstat_loss_ref.py against torch's own functions composed as
basicsr/losses/my_loss.py composes them, the loss registry and the recipe's defaults, the refusals by name (a negative alpha, Stage I, a
missing VGG file only with alpha2 > 0), PerceptualLoss with criterion l2, and the new C ABI entries.  Needs no GPU and no library."""
import ctypes
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

import pixstat_loss_ref as R
import vgg_ref
from conftest import ROOT


def _my_loss(y_true, y_pred):
    """my_loss.py:22-49 and the four alphas of :55-60 that weigh them, verbatim in torch's own functions."""
    color = torch.mean(torch.abs(torch.mean(y_true, dim=[1, 2, 3]) - torch.mean(y_pred, dim=[1, 2, 3])))
    mse = F.mse_loss(y_true, y_pred)
    psnr = 40.0 - torch.mean(20 * torch.log10(1.0 / torch.sqrt(mse)))
    sl1 = F.smooth_l1_loss(y_true, y_pred)
    ht, hp = torch.histc(y_true, bins=256, min=0.0, max=1.0), torch.histc(y_pred, bins=256, min=0.0, max=1.0)
    hist = torch.mean(torch.abs(ht / ht.sum() - hp / hp.sum()))
    return dict(loss=1.00 * sl1 + 0.05 * hist + 0.0083 * psnr + 0.25 * color, smooth_l1=sl1, mse=mse, psnr=psnr, color=color, hist=hist)


@pytest.mark.parametrize("shape", [(2, 3, 13, 17), (5, 1, 24, 40), (3, 1, 1, 4096)])
def test_restatement_equals_torchs_functions_in_float64(shape):
    pred, gt = R.pair(shape, seed=sum(shape))
    d = (pred - gt).abs()
    assert int((d > 1).sum()) >= 2 and int((pred < 0).sum()) >= 2 and int((pred > 1).sum()) >= 2          # the planted values are there
    assert bool((pred == 1.0).any()) and bool((pred == 0.0).any()) and bool((pred == 0.5).any())
    x = pred.double().requires_grad_(True)
    want = _my_loss(gt.double(), x)
    (gw,) = torch.autograd.grad(want["loss"], x)
    got, g = R.loss_and_grad(pred, gt, R.ALPHAS, torch.float64)
    for i, k in enumerate(R.VALUES):
        w = float(want[k].detach())
        err = abs(float(got[i]) - w)
        print(f"{shape} {k}: {float(got[i]):.12g} vs {w:.12g}")
        assert err <= 1e-14 * max(1.0, abs(w)), (k, err)
    assert float((g - gw).abs().max()) <= 1e-15 and float(gw.abs().max()) > 0
    assert not torch.histc(x, bins=256, min=0.0, max=1.0).requires_grad                    # the histogram term has no gradient


def test_histc_semantics_the_kernel_restates():
    x = torch.tensor([0.0, -0.0, 1.0, 0.5, float(torch.nextafter(torch.tensor(0.5), torch.tensor(0.0))), -1e-9, 1.0 + 2 ** -23, float("nan")])
    h = R.counts(x)
    assert int(h.sum()) == 5 and int(h[0]) == 2 and int(h[255]) == 1 and int(h[128]) == 1 and int(h[127]) == 1


def test_zero_alpha_leaves_its_term_out():
    z = torch.rand(1, 1, 4, 4, generator=torch.Generator().manual_seed(0))
    v = R.values(z, z, (1.0, 0.05, 0.0, 0.25))
    assert float(v["psnr"]) == float("-inf") and float(v["loss"]) == 0.0


def test_registered_with_the_references_six_weights():
    import basicsr.losses as L
    from basicsr.utils.registry import LOSS_REGISTRY
    assert LOSS_REGISTRY.get("CombinedLoss") is L.CombinedLoss and "CombinedLoss" in L.__all__
    crit = L.build_loss(dict(type="CombinedLoss", state_dict=vgg_ref.seeded_state_dict("conv3_3", seed=1)))
    assert [getattr(crit, k) for k in L.CombinedLoss.ALPHAS] == [1.00, 0.06, 0.05, 0.5, 0.0083, 0.25] and crit.loss_weight == 1.0     # my_loss.py:55-60
    assert crit.percep.criterion_type == "l2" and list(crit.percep.layer_weights) == ["relu3_3"] and crit.percep.perceptual_weight == 0.06
    assert not crit.percep.vgg.use_input_norm and not crit.percep.vgg.range_norm and crit.percep.vgg.names[-1] == "relu3_3"
    assert crit.ssim.loss_weight == 0.5 and crit.pix_alphas == (1.00, 0.05, 0.0083, 0.25)
    assert not crit.state_dict()                                                  # frozen buffers only
    half = L.build_loss(dict(type="CombinedLoss", alpha2=0, alpha4=0, loss_weight=2.0))
    assert half.percep is None and half.ssim is None and half.pix_alphas == (2.0, 0.1, 0.0166, 0.5)


@pytest.mark.parametrize("key", ["alpha1", "alpha2", "alpha3", "alpha4", "alpha5", "alpha6"])
def test_negative_alpha_raises_naming_the_key(key):
    from basicsr.losses import build_loss
    with pytest.raises(ValueError, match=key):
        build_loss({"type": "CombinedLoss", "alpha2": 0, key: -0.1})         # alpha2 = 0: no VGG file is needed to get as far as the check


def test_all_zero_alphas_and_bad_loss_weight_raise():
    from basicsr.losses import build_loss
    with pytest.raises(ValueError, match="all 0"):
        build_loss(dict(type="CombinedLoss", **{f"alpha{i}": 0 for i in range(1, 7)}))
    with pytest.raises(ValueError, match="loss_weight"):
        build_loss(dict(type="CombinedLoss", alpha2=0, loss_weight=0))


def test_missing_vgg_file_matters_only_with_alpha2(tmp_path, monkeypatch):
    from basicsr.losses import CombinedLoss, build_loss
    from bem.percep import VGG_PRETRAIN_PATH, WEIGHTS_ENV
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv(WEIGHTS_ENV, raising=False)
    with pytest.raises(FileNotFoundError) as e:
        build_loss(dict(type="CombinedLoss"))
    assert VGG_PRETRAIN_PATH in str(e.value) and WEIGHTS_ENV in str(e.value)
    with pytest.raises(FileNotFoundError, match="nowhere.pth"):
        build_loss(dict(type="CombinedLoss", vgg_weights=str(tmp_path / "nowhere.pth")))
    with pytest.raises(FileNotFoundError):
        CombinedLoss.find_weights(dict(type="CombinedLoss"))
    assert CombinedLoss.find_weights(dict(type="CombinedLoss", alpha2=0)) is None
    assert build_loss(dict(type="CombinedLoss", alpha2=0)).percep is None
    path = tmp_path / "vgg19_seeded.pth"
    torch.save(vgg_ref.seeded_state_dict("conv3_3", seed=2), path)
    monkeypatch.setenv(WEIGHTS_ENV, str(path))
    assert CombinedLoss.find_weights(dict(type="CombinedLoss")) == str(path)
    assert build_loss(dict(type="CombinedLoss")).percep is not None
    monkeypatch.delenv(WEIGHTS_ENV)
    assert build_loss(dict(type="CombinedLoss", vgg_weights=str(path))).percep is not None


def test_training_driver_looks_for_the_vgg_file_before_a_model_exists(tmp_path, monkeypatch):
    import basicsr.train as T
    from bem.percep import WEIGHTS_ENV
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv(WEIGHTS_ENV, raising=False)
    opt = dict(model_type="ImageEnhancer", train=dict(combined_opt=dict(type="CombinedLoss")))
    monkeypatch.setattr(T, "parse_options", lambda *a, **k: (opt, None))
    monkeypatch.setattr(T, "build_model", lambda *a, **k: pytest.fail("the model must not be built"))
    monkeypatch.setattr(T, "load_resume_state", lambda *a, **k: pytest.fail("nothing may be read or made before the file is found"))
    with pytest.raises(FileNotFoundError, match="vgg19"):
        T.train_pipeline(str(tmp_path), argv=[])


def test_condition_generator_refuses_combined_opt_before_any_file_is_looked_for(tmp_path, monkeypatch):
    from basicsr.models.condition_generator_model import ConditionGenerator
    from bem.percep import WEIGHTS_ENV
    monkeypatch.chdir(tmp_path)                                  # no weight file anywhere: a look for one would be a FileNotFoundError
    monkeypatch.delenv(WEIGHTS_ENV, raising=False)
    stub = types.SimpleNamespace(net_g=torch.nn.Identity(), device="cpu", opt=dict(train=dict(
        pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean"), combined_opt=dict(type="CombinedLoss"))))
    with pytest.raises(NotImplementedError, match="combined_opt") as e:
        ConditionGenerator.init_training_settings(stub)
    assert "8x8" in str(e.value) and "11x11" in str(e.value) and "VGG" in str(e.value)


def test_image_enhancer_names_the_new_term_when_every_loss_is_missing():
    from basicsr.models.image_enhancer_model import ImageEnhancer
    stub = types.SimpleNamespace(net_g=torch.nn.Identity(), device="cpu", opt=dict(train=dict()))
    with pytest.raises(ValueError, match="all None") as e:
        ImageEnhancer.init_training_settings(stub)
    assert "LPIPS" in str(e.value) and "combined" in str(e.value)


def test_perceptual_loss_constructs_with_criterion_l2():
    from bem.percep import PerceptualLoss
    crit = PerceptualLoss({"relu3_3": 1}, use_input_norm=False, criterion="l2", state_dict=vgg_ref.seeded_state_dict("conv3_3", seed=3))
    assert crit.criterion_type == "l2"
    assert PerceptualLoss({"conv1_2": 1}, state_dict=vgg_ref.seeded_state_dict("conv1_2", seed=3)).criterion_type == "l1"       # the default stays


def test_header_declares_the_new_entries_and_the_binding_agrees():
    from bem import native
    with open(os.path.join(ROOT, "include", "bem_hip.h")) as f:
        text = f.read()
    P, I64, D = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    want = {"bem_pixstat_loss_chunk": [], "bem_pixstat_loss_ws_bytes": [I64, I64],
            "bem_pixstat_loss_f32": [P, P, P, P, P, I64, I64, D, D, D, D, P],
            "bem_pixstat_loss_bwd_f32": [P, P, P, P, I64, I64, P, P],
            "bem_mse_loss_f32": native.SIGNATURES["bem_l1_loss_f32"]}
    for name, args in want.items():
        assert native.SIGNATURES[name] == args, name
    assert "bem_abi_version" in native.SIGNATURES
    ssim, mse, fwd, bwd = (text.index(f"int {n}(") for n in ("bem_ssim_loss_bwd_f32", "bem_mse_loss_f32", "bem_pixstat_loss_f32", "bem_pixstat_loss_bwd_f32"))
    assert ssim < mse < fwd < bwd and "int bem_" not in text[ssim + 10:mse]            # with the training step's other loss entries
    for at in (mse, fwd, bwd):                                                         # each entry's comment cites the reference's lines
        assert re.search(r"my_loss\.py:\d+", text[text.rindex("/*", 0, at):at])


def test_ops_wrappers_refuse_cpu_tensors_and_bad_operands_before_any_launch():
    from bem import native, ops
    x = torch.zeros(1, 3, 16, 16)
    for call in (lambda: ops.pixstat_loss(x, x, R.ALPHAS), lambda: ops.pixstat_loss_bwd(x, x, torch.zeros(3, dtype=torch.float64)),
                 lambda: ops.mse_loss(x, x), lambda: ops.mse_loss_bwd(x, x)):
        with pytest.raises(native.BemNativeError):
            call()
    assert ops.pixstat_loss_cost(x) == (8.0 * x.numel(), 12.0 * x.numel()) and ops.pixstat_loss_bwd_cost(x)[0] == 12.0 * x.numel()
    assert ops.PIXSTAT_VALUES == R.VALUES
