"""GPU: NIQE on the device (bem.ops.niqe, bem_niqe_f32) against the reference's recorded features and scores (g13_niqe.npz) and the
restatement tests/niqe_ref.py; selection through bem.scorers.Niqe in BEMPipeline.enhance and Enhancement/eval.py --no_ref niqe."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import niqe_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
NPZ = os.path.join(GOLDEN, "g13_niqe.npz")


@pytest.fixture(scope="module")
def g13():
    return np.load(NPZ)


@pytest.fixture(scope="module")
def params():
    from bem.scorers import NiqeParams
    return NiqeParams.load(NPZ)


def _dev(u8s):
    """uint8 HWC images of one size -> (n,3,h,w) f32 on the device (u8 / 255)."""
    return torch.from_numpy(np.stack([R.as_pred(u) for u in u8s])).permute(0, 3, 1, 2).contiguous().cuda()


def _features(final, params):
    """Runs ops.niqe and returns the per-block feature rows it left in its workspace (the last region, f64, idx_w-major)."""
    from bem import ops
    from bem.native import lib
    s = ops.niqe(final, params)
    Bn, _, h, w = final.shape
    nb = (h // 96) * (w // 96)
    total = int(lib().bem_niqe_ws_bytes(Bn, h, w))
    ws = ops._scratch("niqe", final.device, total, torch.uint8)         # the buffer the call just used: same stream, no larger request
    start = total - ((Bn * nb * 36 * 8 + 255) // 256) * 256
    feat = ws[start:start + Bn * nb * 36 * 8].view(torch.float64).reshape(Bn, nb, 36)
    return s, feat.cpu().numpy()


def test_niqe_per_input_vs_reference(g13, params):
    steps_all = []
    for name, img in R.fixture_inputs(g13).items():
        s, feat = _features(_dev([img]), params)
        s = float(s[0])
        ref = g13[f"feat_{name}"]
        assert abs(s / float(g13[f"score_{name}"]) - 1) <= 1e-4, (name, s, float(g13[f"score_{name}"]))
        assert np.array_equal(np.isnan(feat[0]), np.isnan(ref)), name
        a, ra = feat[0][:, R.ALPHA_COLS], ref[:, R.ALPHA_COLS]
        steps = np.rint(np.abs(a - ra) / 1e-3)
        assert steps.max() <= 1, name
        steps_all.append(steps.ravel())
        same = np.repeat((steps == 0).all(axis=1, keepdims=True), 36, axis=1) & ~np.isnan(ref)
        np.testing.assert_allclose(feat[0][same], ref[same], rtol=1e-3, atol=2e-5, err_msg=name)
        if name == "saturated":
            assert np.isnan(ref).any() and np.isfinite(s)
    assert (np.concatenate(steps_all) == 0).mean() >= 0.99


def test_niqe_candidate_set_selects_reference_index(g13, params):
    from bem import ops
    from bem.scorers import Niqe
    c = _dev(R.fixture_candidates(g13))
    s = ops.niqe(c, params)
    np.testing.assert_allclose(s.cpu().numpy(), g13["cand_scores"], rtol=1e-4)
    sel = Niqe(params).select(c, None, c.shape[0])
    assert int(sel["best"][0]) == int(g13["cand_best"])
    assert torch.equal(sel["best_images"][0], c[int(g13["cand_best"])])


def test_niqe_flat_image_nan_and_never_chosen_unless_first(g13, params):
    from bem.scorers import Niqe
    cand = R.fixture_candidates(g13)
    flat = np.full_like(cand[0], 128)
    x = _dev([cand[0], flat, cand[2]])
    sel = Niqe(params).select(x, None, 3)
    s = sel["s1"].cpu().numpy()
    assert np.isnan(s[1]) and np.isfinite(s[[0, 2]]).all()
    assert int(sel["best"][0]) == int(np.argmin(s[[0, 2]])) * 2
    sel = Niqe(params).select(_dev([flat, cand[0], cand[2]]), None, 3)   # python min() of a list that starts with NaN keeps the NaN
    assert int(sel["best"][0]) == 0


def test_niqe_rejects_small_images(params):
    from bem import ops
    from bem.native import BemNativeError, check, lib
    with pytest.raises(ValueError, match="96"):
        ops.niqe(torch.rand(1, 3, 95, 200, device="cuda"), params)
    x = torch.rand(1, 3, 95, 200, device="cuda")
    ws = torch.empty(1 << 20, device="cuda", dtype=torch.uint8)
    out = torch.empty(1, device="cuda", dtype=torch.float64)
    rc = lib().bem_niqe_f32(x.data_ptr(), params.mu.data_ptr(), params.cov.data_ptr(), params.window.data_ptr(), ws.data_ptr(), 9801,
                            ws.data_ptr(), ws.data_ptr(), 8, ws.data_ptr(), ws.data_ptr(), 8, out.data_ptr(), ws.data_ptr(), ws.numel(),
                            1, 95, 200, None)
    assert rc == 1
    with pytest.raises(BemNativeError, match="96"):
        check(rc, "niqe")


def test_niqe_bit_reproducible_and_batch_independent(g13, params):
    from bem import ops
    x = _dev(R.fixture_candidates(g13))
    a, b = ops.niqe(x, params), ops.niqe(x, params)
    assert torch.equal(a, b)
    alone = torch.cat([ops.niqe(x[i:i + 1].contiguous(), params) for i in range(x.shape[0])])
    assert torch.equal(a, alone)
    torch.manual_seed(0)
    y = torch.rand(3, 3, 200, 300, device="cuda")
    ys = ops.niqe(y, params)
    ref = [R.niqe(y[i].cpu().numpy(), g13) for i in range(3)]
    np.testing.assert_allclose(ys.cpu().numpy(), ref, rtol=1e-4)


@pytest.mark.parametrize("with_target", [False, True])
def test_pipeline_niqe_selection(g13, params, with_target):
    """BEMPipeline.enhance with the Niqe scorer on seeded random-init nets (n_feat 8, N = 4): the chosen sample is the argmin of the restatement over
    the returned candidates wherever the best score beats the runner-up by more than 1e-4 relative.  Random-init nets give degenerate,
    partly saturated images (NIQE ~60), where the f32 cancellation next to saturated patches moves single features: the scores
    themselves agree to 1e-3 here."""
    from bem.pipeline import BEMPipeline, build_nets, synthetic_pair
    from bem.scorers import Niqe
    net1, net2 = build_nets(n_feat=8, num_blocks=(1, 1, 1), seed=21, device="cuda")
    lq, gt = synthetic_pair((1, 3, 200, 300), seed=4)       # 2 x 3 blocks: a single 96 x 96 block cannot form a covariance
    N = 4
    out = BEMPipeline(net1, net2).enhance(lq.cuda(), gt.cuda() if with_target else None, N, gt_mean=with_target, scorer=Niqe(params), seed=9)
    fin = out["final"].cpu().numpy()
    ref = np.array([R.niqe(fin[i], g13) for i in range(N)])
    dev = out["scores"].cpu().numpy().astype(np.float64)
    ok = np.isfinite(ref)
    np.testing.assert_allclose(dev[ok], ref[ok], rtol=1e-3)
    assert np.array_equal(np.isnan(dev), np.isnan(ref))
    order = np.argsort(np.where(ok, ref, np.inf))
    if ok.sum() >= 2 and (ref[order[1]] - ref[order[0]]) > 1e-4 * abs(ref[order[0]]):
        assert out["best"][0] == int(order[0])


def test_eval_driver_niqe(tmp_path, g13):
    from PIL import Image
    from bem.pipeline import build_nets, synthetic_pair
    spec = importlib.util.spec_from_file_location("bem_eval_driver_niqe_gpu", os.path.join(PKG, "Enhancement", "eval.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    net1, net2 = build_nets(device="cpu")
    torch.save({"params": net1.state_dict()}, tmp_path / "cg.pth")
    torch.save({"params": net2.state_dict()}, tmp_path / "s2.pth")
    (tmp_path / "in").mkdir()
    lq, _ = synthetic_pair((2, 3, 200, 200))
    for i in range(2):
        Image.fromarray(np.rint(lq[i].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(tmp_path / "in" / f"{i}.png")
    out = drv.main(["--opt", os.path.join(PKG, "Options", "CG_UNet_LOLv1.yml"), "--cond_opt", os.path.join(PKG, "Options", "DecompDualBranch2DDWavelet_4.yml"),
                    "--weights", str(tmp_path / "cg.pth"), "--cond_weights", str(tmp_path / "s2.pth"), "--input_dir", str(tmp_path / "in"),
                    "--result_dir", str(tmp_path / "res"), "--dataset", "synthetic", "--num_samples", "3", "--seed", "11",
                    "--no_ref", "niqe", "--niqe_params", NPZ])
    assert sorted(os.listdir(out["result_dir"])) == ["0.png", "1.png", "result.txt"]
    assert len(out["niqe"]) == 2 and all(np.isfinite(out["niqe"]))
    lines = [ln for ln in open(os.path.join(out["result_dir"], "result.txt")).read().splitlines() if ln.startswith("Best_NIQE")]
    assert lines == [f"Best_NIQE: {np.mean(out['niqe']):.4f} "]
