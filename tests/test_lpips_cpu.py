"""LPIPS without a GPU: facts about the torch restatement the GPU tests check against (tests/lpips_ref.py), the host side of bem.lpips
(where the two weight files come from, which keys and shapes they must hold), the argument checks of the two drivers, which run before
any device work, and the argument checks of the new C entries, which return before any launch."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import lpips_ref as R
from conftest import PKG


@pytest.fixture(scope="module")
def sds():
    return R.seeded_state_dicts(0)


# ------------------------------------------------------------------------------ the restatement
def test_distance_of_an_image_to_itself_is_zero_and_d_is_symmetric(sds):
    sd, lin = sds
    g = torch.Generator().manual_seed(1)
    a, b = torch.rand(2, 3, 37, 53, generator=g) * 2 - 1, torch.rand(2, 3, 37, 53, generator=g) * 2 - 1
    for dt in (torch.float32, torch.float64):
        assert torch.equal(R.lpips(sd, lin, a, a, dt), torch.zeros(2, dtype=dt))
        dab, dba = R.lpips(sd, lin, a, b, dt), R.lpips(sd, lin, b, a, dt)
        assert torch.equal(dab, dba) and bool((dab > 0).all())


def test_head_by_hand():
    """Two channels, two pixels.  Pixel 0: y0 = (3, 4) -> (0.6, 0.8), y1 = (0, 5) -> (0, 1): w . (0.36, 0.04).  Pixel 1: y0 = (0, 0) -> 0 / 1e-10 =
    (0, 0), y1 = (1, 0) -> (1, 0): w . (1, 0).  Mean of the two."""
    y0 = torch.tensor([[[[3.0, 0.0]], [[4.0, 0.0]]]], dtype=torch.float64)      # (1, 2, 1, 2)
    y1 = torch.tensor([[[[0.0, 1.0]], [[5.0, 0.0]]]], dtype=torch.float64)
    w = np.array([0.25, 0.5])
    n = lambda v: v / (np.sqrt((v * v).sum()) + 1e-10)
    px0 = (w * (n(np.array([3.0, 4.0])) - n(np.array([0.0, 5.0]))) ** 2).sum()
    px1 = (w * (n(np.array([0.0, 0.0])) - n(np.array([1.0, 0.0]))) ** 2).sum()
    want = (px0 + px1) / 2
    assert abs(want - (0.25 * 0.36 + 0.5 * 0.04 + 0.25) / 2) < 1e-9
    assert abs(float(R.head(y0, y1, torch.from_numpy(w))[0]) - want) < 1e-15


@pytest.mark.parametrize("n,want", [(31, (7, 3, 1, 1, 1)), (37, (8, 3, 1, 1, 1)), (64, (15, 7, 3, 3, 3)), (400, (99, 49, 24, 24, 24))])
def test_feature_sizes(sds, n, want):
    assert R.sizes(n) == want
    m = {31: 64, 37: 400, 64: 31, 400: 37}[n]                       # W likewise, a different one per H
    f = R.features(sds[0], torch.zeros(1, 3, n, m))
    assert [t.shape[2] for t in f] == list(want) and [t.shape[3] for t in f] == list(R.sizes(m))
    assert [t.shape[1] for t in f] == list(R.WIDTHS)
    from bem import ops
    assert ops.lpips_conv1_hw(n, m) == (want[0], R.sizes(m)[0])


def test_conv1_block_weight_is_the_strided_convolution(sds):
    """The (64,48,3,3) block form over the 4x4 space-to-depth image is conv1 (11x11, stride 4, pad 2) shifted by one block."""
    from bem.lpips import conv1_block_weight
    w = sds[0]["features.0.weight"].double()
    g = torch.Generator().manual_seed(2)
    H, W = 37, 57
    x = torch.randn(1, 3, H, W, generator=g, dtype=torch.float64)
    Ho, Wo = R.sizes(H)[0], R.sizes(W)[0]
    Hb, Wb = Ho + 2, (Wo + 3) // 2 * 2
    xp = torch.zeros(1, 3, 4 * Hb, 4 * Wb, dtype=torch.float64)
    xp[:, :, 2:2 + H, 2:2 + W] = x
    xs = xp.view(1, 3, Hb, 4, Wb, 4).permute(0, 1, 3, 5, 2, 4).reshape(1, 48, Hb, Wb)
    got = torch.nn.functional.conv2d(xs, conv1_block_weight(w), padding=1)[:, :, 1:1 + Ho, 1:1 + Wo]
    want = torch.nn.functional.conv2d(x, w, stride=4, padding=2)
    assert got.shape == want.shape and float((got - want).abs().max()) < 1e-12


# ------------------------------------------------------------------------------ the loader
def test_module_refuses_other_nets_and_versions(sds):
    from bem.lpips import LPIPS
    with pytest.raises(NotImplementedError, match="vgg"):
        LPIPS(net="vgg", state_dict=sds[0], lin_state_dict=sds[1])
    with pytest.raises(NotImplementedError, match="0.0"):
        LPIPS(version="0.0", state_dict=sds[0], lin_state_dict=sds[1])


def test_loader_names_what_is_wrong(sds, tmp_path, monkeypatch):
    from bem import lpips as L
    sd, lin = sds
    extra = dict(sd)
    extra["classifier.1.weight"] = torch.zeros(4, 4)
    m = L.LPIPS(state_dict=extra, lin_state_dict=dict(lin, extra=torch.zeros(1)))          # extra keys are ignored
    assert m.conv1_weight.shape == (192, 64, 5, 5) and m.lin2.shape == (384,) and not m.state_dict()
    with pytest.raises(KeyError, match=r"features\.6\.bias"):
        L.LPIPS(state_dict={k: v for k, v in sd.items() if k != "features.6.bias"}, lin_state_dict=lin)
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight"):
        L.LPIPS(state_dict=sd, lin_state_dict={k: v for k, v in lin.items() if not k.startswith("lin3")})
    with pytest.raises(ValueError, match=r"features\.3\.weight"):
        L.LPIPS(state_dict=dict(sd, **{"features.3.weight": torch.zeros(192, 64, 3, 3)}), lin_state_dict=lin)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight"):
        L.LPIPS(state_dict=sd, lin_state_dict=dict(lin, **{"lin0.model.1.weight": torch.zeros(64)}))
    # files: a directory with one of the two is not enough, and the message names both files and the variable
    monkeypatch.delenv(L.WEIGHTS_ENV, raising=False)
    torch.save(sd, tmp_path / L.ALEXNET_FILE)
    with pytest.raises(FileNotFoundError) as e:
        L.LPIPS(weights_dir=str(tmp_path))
    assert L.ALEXNET_FILE in str(e.value) and L.LIN_FILE in str(e.value) and L.WEIGHTS_ENV in str(e.value)
    monkeypatch.setenv(L.WEIGHTS_ENV, str(tmp_path))
    with pytest.raises(FileNotFoundError, match=L.WEIGHTS_ENV):
        L.find_weight_files()
    torch.save(lin, tmp_path / L.LIN_FILE)
    assert L.find_weight_files() == (str(tmp_path / L.ALEXNET_FILE), str(tmp_path / L.LIN_FILE))
    m = L.LPIPS()                                                                              # through the variable
    assert torch.equal(m.conv4_weight, sd["features.10.weight"]) and torch.equal(m.lin4, lin["lin4.model.1.weight"].reshape(-1))
    monkeypatch.delenv(L.WEIGHTS_ENV)
    monkeypatch.chdir(tmp_path)                                                               # no experiments/pretrained_models here
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    with pytest.raises(FileNotFoundError, match="pretrained_models"):
        L.find_weight_files()
    os.makedirs(tmp_path / "experiments" / "pretrained_models")
    for f in (L.ALEXNET_FILE, L.LIN_FILE):
        os.replace(tmp_path / f, tmp_path / "experiments" / "pretrained_models" / f)
    assert L.find_weight_files() == (os.path.join(L.PRETRAIN_DIR, L.ALEXNET_FILE), os.path.join(L.PRETRAIN_DIR, L.LIN_FILE))


def test_small_images_are_refused_by_name(sds):
    from bem.lpips import LPIPS
    m = LPIPS(state_dict=sds[0], lin_state_dict=sds[1])
    with pytest.raises(ValueError, match="31 x 31"):
        m.distance01(torch.zeros(1, 3, 30, 64), torch.zeros(1, 3, 30, 64))
    with pytest.raises(ValueError, match="31 x 31"):
        m(torch.zeros(1, 3, 64, 30), torch.zeros(1, 3, 64, 30))


def test_im2tensor():
    from bem.lpips import im2tensor
    u = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) * 14
    t = im2tensor(u)
    assert t.shape == (1, 3, 2, 3) and t.dtype == torch.float32
    assert torch.equal(t, R.im2tensor(u).float())


# ------------------------------------------------------------------------------ the drivers
def _script(name):
    spec = importlib.util.spec_from_file_location("bem_" + name + "_lpips_cpu", os.path.join(PKG, "Enhancement", name + ".py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


def test_eval_lpips_checks_arguments_before_any_gpu_call(tmp_path, monkeypatch):
    from bem import lpips as L
    monkeypatch.delenv(L.WEIGHTS_ENV, raising=False)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    drv = _script("eval")
    with pytest.raises(SystemExit) as e:
        drv.main(["--lpips", "--input_dir", str(tmp_path)])
    assert "--lpips" in str(e.value) and "--target_dir" in str(e.value)
    with pytest.raises(SystemExit) as e:
        drv.main(["--lpips", "--input_dir", str(tmp_path), "--target_dir", str(tmp_path)])
    assert all(s in str(e.value) for s in ("--lpips", "--lpips_weights", L.ALEXNET_FILE, L.LIN_FILE))
    with pytest.raises(SystemExit) as e:
        drv.main(["--lpips", "--input_dir", str(tmp_path), "--target_dir", str(tmp_path), "--lpips_weights", str(tmp_path / "w")])
    assert all(s in str(e.value) for s in ("--lpips", "--lpips_weights", L.ALEXNET_FILE, L.LIN_FILE, str(tmp_path / "w")))


def test_cal_metrics_checks_arguments_before_any_gpu_call(tmp_path, monkeypatch):
    from bem import lpips as L
    monkeypatch.delenv(L.WEIGHTS_ENV, raising=False)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    drv = _script("cal_metrics_with_imgs")
    with pytest.raises(SystemExit) as e:
        drv.main(["--pred_dir", str(tmp_path), "--lpips"])
    assert "--lpips" in str(e.value) and "--target_dir" in str(e.value)
    with pytest.raises(SystemExit) as e:
        drv.main(["--pred_dir", str(tmp_path), "--target_dir", str(tmp_path), "--lpips"])
    assert all(s in str(e.value) for s in ("--lpips", "--lpips_weights", L.ALEXNET_FILE, L.LIN_FILE))
    with pytest.raises(SystemExit, match="--niqe_params"):
        drv.main(["--pred_dir", str(tmp_path), "--niqe"])
    with pytest.raises(SystemExit, match="--pred_dir"):
        drv.main(["--pred_dir", str(tmp_path / "missing"), "--niqe", "--niqe_params", "x.npz"])


# ------------------------------------------------------------------------------ the C entries
@pytest.fixture(scope="module")
def lib():
    from bem import native
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


def test_lpips_entries_reject_before_any_hip_call(lib):
    p = 16   # any non-null value: the checks reject before a pointer is touched
    assert lib.bem_abi_version() == 1
    assert lib.bem_lpips_prep_f32(None, p, p, 1, 64, 64, 1, None) == 1 and b"null" in lib.bem_last_error()
    assert lib.bem_lpips_prep_f32(p, p, None, 1, 64, 64, 1, None) == 1 and b"null" in lib.bem_last_error()
    assert lib.bem_lpips_prep_f32(p, p, p, 1, 30, 64, 1, None) == 1 and b"31 x 31" in lib.bem_last_error()
    assert lib.bem_lpips_prep_f32(p, p, p, 1, 64, 30, 1, None) == 1 and b"31 x 31" in lib.bem_last_error()
    assert lib.bem_lpips_prep_f32(p, p, p, 1, 64, 64, 3, None) == 1 and b"mode" in lib.bem_last_error()
    assert lib.bem_maxpool3s2_f32(None, 9, 3, p, 1, 3, 3, None) == 1 and b"null" in lib.bem_last_error()
    assert lib.bem_maxpool3s2_f32(p, 9, 3, p, 1, 2, 3, None) == 1 and b"3 x 3" in lib.bem_last_error()
    assert lib.bem_maxpool3s2_f32(p, 9, 3, p, 1, 3, 2, None) == 1 and b"3 x 3" in lib.bem_last_error()
    assert lib.bem_maxpool3s2_f32(p, 8, 3, p, 1, 3, 3, None) == 1 and b"strides" in lib.bem_last_error()
    ok = [p, 64 * 35, 35, 7, p, p, 2 * 2, p, 2, 64, 5, 7, 1, None]
    assert lib.bem_lpips_layer_ws_elems(2, 5, 7) == 4 and lib.bem_lpips_layer_ws_elems(1, 99, 149) == 1 + 231
    for i in (0, 4, 5, 7):
        bad = list(ok)
        bad[i] = None
        assert lib.bem_lpips_layer_f32(*bad) == 1 and b"null" in lib.bem_last_error()
    for i in (10, 11):
        bad = list(ok)
        bad[i] = 0
        assert lib.bem_lpips_layer_f32(*bad) == 1 and b"1 x 1" in lib.bem_last_error()
    bad = list(ok)
    bad[6] = 3
    assert lib.bem_lpips_layer_f32(*bad) == 1 and b"workspace" in lib.bem_last_error()
    bad = list(ok)
    bad[3] = 6
    assert lib.bem_lpips_layer_f32(*bad) == 1 and b"strides" in lib.bem_last_error()
    # the 5x5 tap form's refusals (odd widths, stride 2): tests/test_conv_route_cpu.py::test_forced_form_refuses_without_a_device
