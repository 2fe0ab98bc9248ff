"""PerceptualLoss without a GPU: the torch restatement the GPU tests check against (tests/vgg_ref.py) reproduces what the reference's
own class recorded (tests/golden/g17_perceptual.npz), and the module's host side -- where the weights come from, which shapes they must
have, which options it refuses -- behaves as documented.  Nothing here launches a kernel: construction only reads and checks weights."""
import pytest
import torch

import vgg_ref as R
from conftest import load_golden


@pytest.fixture(scope="module")
def g17():
    g = load_golden("g17_perceptual")
    g["sd"] = {k: v.float() for k, v in g["sd"].items()}
    g["lw"] = {k: float(v[0]) for k, v in g["layer_weight"].items()}
    return g


def test_restatement_reproduces_the_reference_fixture(g17):
    """Same f32 torch ops on the same machine class: features, loss and input gradient within 1e-6 relative (bit-equal where the
    summation order is the same)."""
    g = g17
    assert list(g["lw"].items()) == [("conv1_2", 1.0), ("conv2_2", 0.5)] and abs(float(g["perceptual_weight"][0]) - 0.01) < 1e-9
    assert sum(v.numel() for v in g["sd"].values()) == 260160
    feats = R.features(g["sd"], g["x"], g["lw"])
    for k, f in feats.items():
        assert float((f - g["feat"][k]).abs().max()) <= 1e-6 * float(g["feat"][k].abs().max()), k
    loss, dx = R.loss_and_grad(g["sd"], g["x"], g["gt"], g["lw"], 0.01, dtype=torch.float32)
    assert abs(float(loss) - float(g["loss"][0])) <= 1e-6 * abs(float(g["loss"][0]))
    assert float((dx - g["dx"]).abs().max()) <= 1e-6 * float(g["dx"].abs().max())
    # and the float64 form the GPU tests use as their reference agrees with it to f32 rounding
    loss64, dx64 = R.loss_and_grad(g["sd"], g["x"], g["gt"], g["lw"], 0.01, dtype=torch.float64)
    assert abs(float(loss64) - float(g["loss"][0])) <= 1e-5 * abs(float(loss64))
    assert float((dx64 - g["dx"]).abs().max()) <= 1e-5 * float(dx64.abs().max())


def test_layer_table_matches_the_modules_names():
    from bem.percep import VGG19_NAMES, conv_shape
    tab = R.layer_table()
    assert [r[0] for r in tab] == VGG19_NAMES and [r[2] for r in tab] == list(range(len(VGG19_NAMES)))
    for name, kind, _, cin, cout in tab:
        if kind == "conv":
            assert conv_shape(name) == (cout, cin, 3, 3), name


def test_missing_weights_name_the_path_and_the_variable(tmp_path, monkeypatch):
    from basicsr.losses import build_loss
    from bem.percep import VGG_PRETRAIN_PATH, WEIGHTS_ENV
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv(WEIGHTS_ENV, raising=False)
    opt = dict(type="PerceptualLoss", layer_weights={"conv5_4": 1}, vgg_type="vgg19", use_input_norm=True, range_norm=False,
               perceptual_weight=0.01, style_weight=0, criterion="l1")
    with pytest.raises(FileNotFoundError) as e:
        build_loss(opt)
    assert VGG_PRETRAIN_PATH in str(e.value) and WEIGHTS_ENV in str(e.value)
    monkeypatch.setenv(WEIGHTS_ENV, str(tmp_path / "elsewhere.pth"))
    with pytest.raises(FileNotFoundError) as e:
        build_loss(opt)
    assert "elsewhere.pth" in str(e.value) and WEIGHTS_ENV in str(e.value)


def test_partial_state_dict_loads_and_wrong_shape_is_refused(tmp_path, monkeypatch):
    from basicsr.losses import build_loss
    from bem.percep import VGG_PRETRAIN_PATH, WEIGHTS_ENV
    sd = R.seeded_state_dict("conv2_2", seed=3)
    assert sorted(sd) == sorted(f"features.{i}.{k}" for i in (0, 2, 5, 7) for k in ("weight", "bias"))
    sd["classifier.0.weight"] = torch.zeros(2, 2)                  # other keys are ignored
    path = tmp_path / "vgg_small.pth"
    torch.save(sd, path)
    monkeypatch.setenv(WEIGHTS_ENV, str(path))
    crit = build_loss(dict(type="PerceptualLoss", layer_weights={"conv2_2": 1}, perceptual_weight=0.01))
    assert crit.vgg.names[-1] == "conv2_2" and torch.equal(crit.vgg.conv2_2_weight, sd["features.7.weight"])
    assert not list(crit.parameters()) and not crit.state_dict()   # frozen, and not part of any checkpoint
    with pytest.raises(KeyError, match="features.10.weight"):      # a deeper request needs layers the file does not hold
        build_loss(dict(type="PerceptualLoss", layer_weights={"conv3_1": 1}))
    # the default location, relative to the working directory
    monkeypatch.delenv(WEIGHTS_ENV)
    monkeypatch.chdir(tmp_path)
    (tmp_path / "experiments" / "pretrained_models").mkdir(parents=True)
    torch.save(sd, tmp_path / VGG_PRETRAIN_PATH)
    assert build_loss(dict(type="PerceptualLoss", layer_weights={"relu1_2": 1})).vgg.names[-1] == "relu1_2"
    bad = dict(sd)
    bad["features.5.weight"] = torch.zeros(128, 64, 3, 2)
    from bem.percep import PerceptualLoss
    with pytest.raises(ValueError, match="features.5.weight"):
        PerceptualLoss({"conv2_2": 1}, state_dict=bad)


@pytest.mark.parametrize("kw,word", [(dict(style_weight=1.0), "style_weight"), (dict(criterion="fro"), "fro"), (dict(vgg_type="vgg16"), "vgg16"),
                                     (dict(layer_weights={"pool3": 1.0}), "pool3")])
def test_unsupported_options_raise_by_name(kw, word):
    from bem.percep import PerceptualLoss
    args = dict(layer_weights={"conv1_2": 1.0}, state_dict=R.seeded_state_dict("pool3", seed=1))
    args.update(kw)
    with pytest.raises(NotImplementedError, match=word):
        PerceptualLoss(**args)


def test_registered_under_the_reference_names_and_l1_unchanged():
    from basicsr.losses import L1Loss, PerceptualLoss, VGGFeatureExtractor
    from basicsr.utils.registry import ARCH_REGISTRY, LOSS_REGISTRY
    assert LOSS_REGISTRY.get("PerceptualLoss") is PerceptualLoss and LOSS_REGISTRY.get("L1Loss") is L1Loss
    assert ARCH_REGISTRY.get("VGGFeatureExtractor") is VGGFeatureExtractor
    import inspect
    ref_kw = ["layer_weights", "vgg_type", "use_input_norm", "range_norm", "perceptual_weight", "style_weight", "criterion"]      # basic_loss.py:170-177
    assert list(inspect.signature(PerceptualLoss.__init__).parameters)[1:] == ref_kw + ["state_dict"]


def test_condition_generator_refuses_perceptual_opt_with_its_reason():
    """Stage I keeps refusing the term, before any weight file is looked for, and says why."""
    import types

    from basicsr.models.condition_generator_model import ConditionGenerator
    stub = types.SimpleNamespace(net_g=torch.nn.Identity(), device="cpu", opt=dict(train=dict(
        pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean"), perceptual_opt=dict(type="PerceptualLoss", layer_weights={"conv5_4": 1}))))
    with pytest.raises(NotImplementedError, match="8x8") as e:
        ConditionGenerator.init_training_settings(stub)
    assert "perceptual_opt" in str(e.value) and "captured graph" in str(e.value)
