"""GPU: UIQM / UCIQE on the device (bem.ops.uiqm_uciqe, bem_uiqm_uciqe_f32) against the reference's recorded parts and choices
(g16_uiqm.npz) and the restatement tests/uiqm_ref.py; the device-resized image against PIL and the device Lab against the restatement;
selection through bem.scorers.UiqmUciqe in BEMPipeline.enhance and Enhancement/eval.py --no_ref uiqm_uciqe."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import niqe_ref  # noqa: E402
import uiqm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("crop400x600", "crop193x290", "crop256", "portrait")
# UIQM is float32 in the reference (NumPy 2) and its EME terms use a float32 log that may sit 1 ulp from the device's; UCIQE is float64
RTOL = dict(uicm=1e-9, uism=1e-6, uiconm=1e-9, uiqm=1e-6, var_chr=1e-9, con_lum=0.0, aver_sat=1e-9, uciqe=1e-9)


@pytest.fixture(scope="module")
def g16():
    return np.load(os.path.join(GOLDEN, "g16_uiqm.npz"))


@pytest.fixture(scope="module")
def g13():
    return np.load(os.path.join(GOLDEN, "g13_niqe.npz"))


def _inputs(g13):
    out = {k: g13[f"in_{k}"] for k in NAMES[:3]}
    out["portrait"] = np.ascontiguousarray(g13["in_crop400x600"].transpose(1, 0, 2))
    return out


def _dev(u8s):
    """uint8 HWC images of one size -> (n,3,h,w) f32 on the device (u8 / 255)."""
    return torch.from_numpy(np.stack([niqe_ref.as_pred(u) for u in u8s])).permute(0, 3, 1, 2).contiguous().cuda()


def _check_parts(parts, want, label):
    for i, p in enumerate(R.PART_NAMES):
        assert abs(parts[i] - want[p]) <= RTOL[p] * abs(want[p]), (label, p, parts[i], want[p])


def test_uiqm_per_input_vs_reference(g16, g13):
    from bem import ops
    for name, img in _inputs(g13).items():
        u1, u2, v = ops.uiqm_uciqe(_dev([img]), debug=True)
        parts = v["parts"][0].cpu().numpy()
        _check_parts(parts, {p: float(g16[f"{p}_{name}"]) for p in R.PART_NAMES}, name)
        assert float(u1[0]) == parts[3] and float(u2[0]) == parts[7]
        assert float(u1[0]) == float(np.float32(u1[0].item()))          # rounded like the reference's np.float32 UIQM


@pytest.mark.parametrize("hw", [(400, 600), (193, 290), (600, 400), (120, 90), (31, 41)])
def test_device_resize_and_lab_bit_exact(g13, hw):
    """The workspace's resized image equals PIL.Image.resize (eval.py:257) and its Lab image equals the restated cv2 conversion."""
    from PIL import Image
    from bem import ops
    h, w = hw
    rng = np.random.default_rng(h + w)
    u8s = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8), np.ascontiguousarray(np.resize(g13["in_crop400x600"], (h, w, 3)))]
    _, _, v = ops.uiqm_uciqe(_dev(u8s), debug=True)
    rows = int(256 / w * h)
    rs, lab = v["resized"].permute(0, 2, 3, 1).cpu().numpy(), v["lab"].permute(0, 2, 3, 1).cpu().numpy()
    for i, u8 in enumerate(u8s):
        assert np.array_equal(rs[i], np.asarray(Image.fromarray(u8).resize((256, rows)))), (hw, i)
        assert np.array_equal(lab[i], R.rgb2lab_u8(u8)), (hw, i)


def test_uiqm_candidate_set_selects_reference_index(g16, g13):
    from bem import ops
    from bem.scorers import UiqmUciqe
    c = _dev(niqe_ref.fixture_candidates(g13))
    u1, u2, v = ops.uiqm_uciqe(c, debug=True)
    parts = v["parts"].cpu().numpy()
    for i in range(c.shape[0]):
        _check_parts(parts[i], {p: float(g16[f"cand_{p}"][i]) for p in R.PART_NAMES}, f"candidate {i}")
    for w, best in zip(g16["cand_w"], g16["cand_best_w"]):
        sel = UiqmUciqe(float(w)).select(c, None, c.shape[0])
        assert int(sel["best"][0]) == int(best), w
        assert torch.equal(sel["best_images"][0], c[int(best)])
        assert float(sel["best_s1"][0]) == np.float32(u1[int(best)].item()) and float(sel["best_s2"][0]) == np.float32(u2[int(best)].item())


def test_uiqm_rejects_small_images():
    from bem import ops
    from bem.native import BemNativeError, check, lib
    with pytest.raises(ValueError, match="at least 10 rows"):
        ops.uiqm_uciqe(torch.rand(1, 3, 9, 256, device="cuda"))
    with pytest.raises(ValueError, match="at least 10 rows"):
        ops.uiqm_uciqe(torch.rand(1, 3, 30, 800, device="cuda"))          # int(256 / 800 * 30) = 9
    ops.uiqm_uciqe(torch.rand(1, 3, 10, 256, device="cuda"))
    x = torch.rand(1, 3, 9, 256, device="cuda")
    ws = torch.empty(1 << 20, device="cuda", dtype=torch.uint8)
    out = torch.empty(2, device="cuda", dtype=torch.float64)
    p = ws.data_ptr()
    rc = lib().bem_uiqm_uciqe_f32(x.data_ptr(), p, p, p, 5, p, p, 5, out.data_ptr(), out.data_ptr() + 8, p, ws.numel(), 1, 9, 256, 9, None)
    assert rc == 1
    with pytest.raises(BemNativeError, match="10 rows"):
        check(rc, "uiqm_uciqe")


def test_flat_channel_nan_and_selection(g13):
    """A candidate whose blue plane is constant has no Sobel edges there: UISM and UIQM are NaN (as the reference's 255 / 0), UCIQE stays
    finite, nothing faults.  A NaN candidate is never chosen while another one has a score; when all are NaN the first is."""
    from bem import ops
    from bem.scorers import UiqmUciqe
    cand = niqe_ref.fixture_candidates(g13)
    flat = cand[3].copy()
    flat[..., 2] = 77
    u1, u2, v = ops.uiqm_uciqe(_dev([cand[0], flat, cand[2]]), debug=True)
    u1, u2 = u1.cpu().numpy(), u2.cpu().numpy()
    assert np.isnan(u1[1]) and np.isfinite(u1[[0, 2]]).all() and np.isfinite(u2).all()
    assert np.isnan(v["parts"][1, 1].item()) and np.isfinite(v["parts"][1, [0, 2]].cpu().numpy()).all()
    ref = R.scores(niqe_ref.as_pred(flat))
    assert np.isnan(ref["uiqm"]) and abs(u2[1] - ref["uciqe"]) <= 1e-9 * ref["uciqe"]
    for w in (1.0, 0.5):
        sel = UiqmUciqe(w).select(_dev([flat, cand[0], cand[2]]), None, 3)
        assert int(sel["best"][0]) != 0
    sel = UiqmUciqe(1.0).select(_dev([flat, flat]), None, 2)
    assert int(sel["best"][0]) == 0


def test_uicm_trimmed_sum_beyond_float32_exact_range():
    """A saturated red portrait: the trimmed R - G sum passes 2^24, where the reference's float32 sum in sorted order rounds (its mean
    moves by ~0.16 from the exact one); the device follows the float32 sum."""
    from bem import ops
    img = np.zeros((600, 400, 3), np.uint8)
    img[..., 0] = 255
    img[::9, ::13, 0] = 250
    img[::7, ::5, 1] = 90
    img[::3, ::11, 2] = 40
    _, _, v = ops.uiqm_uciqe(_dev([img]), debug=True)
    ref = R.scores(niqe_ref.as_pred(img))
    rs = R.pil_resize(img, 384, 256).astype(np.float32)
    rg = np.sort((rs[..., 0] - rs[..., 1]).ravel())
    K = rg.size
    exact = rg[int(np.ceil(0.1 * K)) + 1:K - int(0.1 * K)].astype(np.float64).sum() / (K - int(np.ceil(0.1 * K)) - int(0.1 * K))
    assert abs(float(R.mu_a(rg)) - exact) > 0.1
    _check_parts(v["parts"][0].cpu().numpy(), ref, "saturated")


def test_uiqm_bit_reproducible_and_batch_independent(g13):
    from bem import ops
    x = _dev(niqe_ref.fixture_candidates(g13))
    a1, a2 = ops.uiqm_uciqe(x)
    b1, b2 = ops.uiqm_uciqe(x)
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    alone = [ops.uiqm_uciqe(x[i:i + 1].contiguous()) for i in range(x.shape[0])]
    assert torch.equal(a1, torch.cat([s[0] for s in alone])) and torch.equal(a2, torch.cat([s[1] for s in alone]))
    torch.manual_seed(0)
    y = torch.rand(3, 3, 150, 220, device="cuda")
    y1, y2 = ops.uiqm_uciqe(y)
    for i in range(3):
        ref = R.scores(y[i].permute(1, 2, 0).cpu().numpy())
        assert abs(y1[i].item() - ref["uiqm"]) <= 1e-6 * abs(ref["uiqm"]) and abs(y2[i].item() - ref["uciqe"]) <= 1e-9 * ref["uciqe"]


@pytest.mark.parametrize("with_target", [False, True])
def test_pipeline_uiqm_selection(with_target):
    """BEMPipeline.enhance with the UiqmUciqe scorer on seeded random-init nets (N = 4): the scores are the restatement's on the returned
    candidates, and the chosen sample is the reference's rule applied to them."""
    from bem.pipeline import BEMPipeline, build_nets, synthetic_pair
    from bem.scorers import UiqmUciqe
    net1, net2 = build_nets(n_feat=8, num_blocks=(1, 1, 1), seed=21, device="cuda")
    lq, gt = synthetic_pair((1, 3, 120, 180), seed=4)
    N = 4
    out = BEMPipeline(net1, net2).enhance(lq.cuda(), gt.cuda() if with_target else None, N, gt_mean=with_target, scorer=UiqmUciqe(0.5), seed=9)
    fin = out["final"].permute(0, 2, 3, 1).cpu().numpy()
    ref = [R.scores(fin[i]) for i in range(N)]
    u1, u2 = out["scores"].cpu().numpy(), out["scores2"].cpu().numpy()
    np.testing.assert_allclose(u1, [np.float32(r["uiqm"]) for r in ref], rtol=1e-6)
    np.testing.assert_allclose(u2, [np.float32(r["uciqe"]) for r in ref], rtol=1e-6)
    s = 0.5 * u1.astype(np.float64) / np.nanmax(u1) + 0.5 * u2.astype(np.float64) / np.nanmax(u2)
    assert out["best"][0] == int(np.argmax(np.where(np.isnan(s), -np.inf, s)))       # a NaN score never wins (scorers.UiqmUciqe)


def test_eval_driver_uiqm(tmp_path):
    from PIL import Image
    from bem.pipeline import build_nets, synthetic_pair
    spec = importlib.util.spec_from_file_location("bem_eval_driver_uiqm_gpu", os.path.join(PKG, "Enhancement", "eval.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    net1, net2 = build_nets(device="cpu")
    torch.save({"params": net1.state_dict()}, tmp_path / "cg.pth")
    torch.save({"params": net2.state_dict()}, tmp_path / "s2.pth")
    (tmp_path / "in").mkdir()
    (tmp_path / "gt").mkdir()
    lq, gt = synthetic_pair((2, 3, 64, 96))
    for i in range(2):
        Image.fromarray(np.rint(lq[i].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(tmp_path / "in" / f"{i}.png")
        Image.fromarray(np.rint(gt[i].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(tmp_path / "gt" / f"{i}.png")
    out = drv.main(["--opt", os.path.join(PKG, "Options", "CG_UNet_LOLv1.yml"), "--cond_opt", os.path.join(PKG, "Options", "DecompDualBranch2DDWavelet_4.yml"),
                    "--weights", str(tmp_path / "cg.pth"), "--cond_weights", str(tmp_path / "s2.pth"), "--input_dir", str(tmp_path / "in"),
                    "--target_dir", str(tmp_path / "gt"), "--GT_mean", "--result_dir", str(tmp_path / "res"), "--dataset", "synthetic",
                    "--num_samples", "3", "--seed", "11", "--no_ref", "uiqm_uciqe", "--uiqm_weight", "0.5"])
    assert sorted(os.listdir(out["result_dir"])) == ["0.png", "1.png", "result.txt"]
    assert len(out["uiqm"]) == 2 and len(out["uciqe"]) == 2 and np.isfinite(out["uciqe"]).all()
    lines = open(os.path.join(out["result_dir"], "result.txt")).read().splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["Best_PSNR", "Best_SSIM", "Best_UIQM", "Best_UCIQE"]
    assert lines[2:] == [f"Best_UIQM: {np.mean(out['uiqm']):.4f} ", f"Best_UCIQE: {np.mean(out['uciqe']):.4f} "]
