"""CPU: UIQM / UCIQE no-reference selection (eval.py --no_ref uiqm_uciqe).  The numpy restatement (tests/uiqm_ref.py) against the
reference's recorded parts and choices (g16_uiqm.npz) and against the reference live (skipped without the reference tree); bem.tables'
host-built tables against Pillow and against the restatement; the OpenCV Lab restatement against known anchors and an analytic
CIE-Lab; the argument checks that come before any GPU call."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, PKG

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, GOLDEN)
import make_golden_uiqm as M  # noqa: E402
import niqe_ref  # noqa: E402
import uiqm_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def g16():
    return np.load(os.path.join(GOLDEN, "g16_uiqm.npz"))


@pytest.fixture(scope="module")
def g13():
    return np.load(os.path.join(GOLDEN, "g13_niqe.npz"))


def _close(name, got, want):
    """uicm sums its squares in another order than the reference (1e-13); UIQM is float32 in the reference; the rest is exact here."""
    rtol = {"uicm": 1e-11}.get(name, 0.0)
    assert abs(got - want) <= rtol * abs(want), (name, got, want)


@pytest.mark.parametrize("name", M.NAMES)
def test_restatement_matches_reference(g16, g13, name):
    img = M.fixture_inputs(g13)[name]
    s = R.scores(niqe_ref.as_pred(img))
    for p in R.PART_NAMES:
        _close(p, s[p], float(g16[f"{p}_{name}"]))


def test_restatement_candidate_set(g16, g13):
    ss = [R.scores(niqe_ref.as_pred(c)) for c in M.fixture_candidates(g13)]
    for p in R.PART_NAMES:
        for i, s in enumerate(ss):
            _close(p, s[p], float(g16[f"cand_{p}"][i]))
    for w, best in zip(g16["cand_w"], g16["cand_best_w"]):
        assert R.select([s["uiqm"] for s in ss], [s["uciqe"] for s in ss], float(w)) == int(best)
    assert len(set(int(b) for b in g16["cand_best_w"])) > 1       # the weight matters for this set


def test_restatement_matches_reference_live(g13):
    """A crop that is not in the golden file (upsampled: 90 columns -> 256), through the reference's own getUIQM / getUCIQE."""
    import ref_harness
    if not ref_harness.available():
        pytest.skip("reference tree not present")
    mod = M.load_reference()
    img = niqe_ref.variant(g13["in_crop193x290"][20:140, 100:190], 0.8, 1.1)
    pred = niqe_ref.as_pred(img)
    ref, s = M.reference_parts(mod, pred), R.scores(pred)
    for p in R.PART_NAMES:
        _close(p, s[p], float(ref[p]))


@pytest.mark.parametrize("hw", [(400, 600), (193, 290), (256, 256), (600, 400), (120, 90), (45, 700), (31, 41)])
def test_pil_resize_tables_bit_exact(hw):
    """bem.tables' coefficient tables equal the restatement's, and the fixed-point two-pass resize with them equals PIL.Image.resize
    (BICUBIC) at eval.py:257's target size, down- and upsampling."""
    from PIL import Image
    from bem import tables
    h, w = hw
    rows = tables.uiqm_resized_rows(h, w)
    assert rows == R.resized_size(h, w)[0] == int(256 / w * h)
    for n_in, n_out in ((w, 256), (h, rows)):
        b, k = tables.pil_resize_table(n_in, n_out)
        rb, rk = R.pil_coeffs(n_in, n_out)
        assert np.array_equal(b, rb) and np.array_equal(k, rk)
        assert (b[:, 0] >= 0).all() and (b.sum(axis=1) <= n_in).all() and (b[:, 1] <= k.shape[1]).all()
    u8 = np.random.default_rng(h * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(u8).resize((256, rows)))
    assert np.array_equal(R.pil_resize(u8, rows, 256), want)


def test_lab_tables_and_anchors():
    """The restated cv2.cvtColor(RGB2LAB) on 8-bit data: white, black and the grey axis (a = b = 128), and the primaries' widely published
    cv2 outputs (recalled values, not recorded with cv2 here)."""
    from bem import tables
    g, c, m = R.lab_tables()
    assert np.array_equal(tables.lab_tables(), np.concatenate([g, c, m.ravel()]).astype(np.int32))
    anchors = {(255, 255, 255): (255, 128, 128), (0, 0, 0): (0, 128, 128), (255, 0, 0): (136, 208, 195), (0, 255, 0): (224, 42, 211),
               (0, 0, 255): (82, 207, 20)}
    for rgb, lab in anchors.items():
        assert tuple(R.rgb2lab_u8(np.array([rgb], np.uint8))[0]) == lab, rgb
    grey = R.rgb2lab_u8(np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1))
    assert (grey[:, 1:] == 128).all() and (np.diff(grey[:, 0].astype(int)) >= 0).all()


def test_lab_within_bound_of_analytic_cielab():
    """Over all 2^24 colours the integer path stays within (2, 3, 2) levels of float CIE-Lab (D65, sRGB), scaled as OpenCV's 8-bit
    output (L * 255 / 100, a + 128, b + 128): the restated tables are the right functions, not merely matching the anchors."""
    M3 = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    white = np.array([0.950456, 1.0, 1.088754])
    g = np.arange(256)
    G, B = np.meshgrid(g, g, indexing="ij")
    worst = np.zeros(3)
    for r in range(256):
        u8 = np.stack([np.full_like(G, r), G, B], -1).reshape(-1, 3).astype(np.uint8)
        x = u8 / 255.0
        lin = np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)
        xyz = lin @ M3.T / white
        f = np.where(xyz > 0.008856, np.cbrt(xyz), 7.787 * xyz + 16 / 116)
        ref = np.stack([(116 * f[:, 1] - 16) * 255 / 100, 500 * (f[:, 0] - f[:, 1]) + 128, 200 * (f[:, 1] - f[:, 2]) + 128], -1)
        worst = np.maximum(worst, np.abs(R.rgb2lab_u8(u8) - np.clip(ref, 0, 255)).max(axis=0))
    assert (worst <= [2, 3, 2]).all(), worst


def test_con_lum_from_level_counts_matches_np_histogram():
    """The device's route to con_lum (a 256-level count histogram of L plus numpy's bin rule) equals np.histogram(lum, 65536)."""
    rng = np.random.default_rng(5)
    cases = [np.array([7] * 50), np.array([0, 255]), np.arange(256), np.array([3] * 99 + [200]), np.array([1] + [250] * 99)]
    for _ in range(300):
        lo, hi = sorted(rng.integers(0, 256, 2))
        cases.append(rng.integers(lo, hi + 1, int(rng.integers(1, 2000))))
    for lv in cases:
        lab = np.zeros((lv.size, 3), np.uint8)
        lab[:, 0], lab[:, 1], lab[:, 2] = lv, 140, 120
        assert R.con_lum_levels(np.bincount(lv, minlength=256)) == R.uciqe_parts(lab)[1], lv[:8]


def _driver():
    spec = importlib.util.spec_from_file_location("bem_eval_driver_uiqm", os.path.join(PKG, "Enhancement", "eval.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


def test_eval_uiqm_checks_arguments_before_any_gpu_call(tmp_path):
    drv = _driver()
    with pytest.raises(SystemExit) as e:
        drv.main(["--no_ref", "uiqm_uciqe", "--input_dir", str(tmp_path / "missing")])
    assert "uiqm_uciqe" in str(e.value) and "--input_dir" in str(e.value)
    with pytest.raises(SystemExit) as e:
        drv.main(["--no_ref", "uiqm_uciqe", "--input_dir", str(tmp_path), "--uiqm_weight", "nan"])
    assert "uiqm_uciqe" in str(e.value) and "--uiqm_weight" in str(e.value)
    with pytest.raises(SystemExit) as e:
        drv.main(["--lpips", "--input_dir", str(tmp_path)])
    assert "--lpips" in str(e.value)


def test_uiqm_entry_rejects_before_any_hip_call():
    from bem import native
    if not os.path.exists(native.LIB_PATH):
        native.build()
    lib = native.lib()
    rc = lib.bem_uiqm_uciqe_f32(None, None, None, None, 11, None, None, 11, None, None, None, 0, 2, 400, 600, 170, None)
    assert rc == 1 and b"null" in lib.bem_last_error()
    p = 16   # any non-null value: the checks below reject before a pointer is touched
    args = [p, p, p, p, 11, p, p, 11, p, p, p, 1 << 40]
    assert lib.bem_uiqm_uciqe_f32(*args, 2, 9, 256, 9, None) == 1 and b"10 rows" in lib.bem_last_error()
    assert lib.bem_uiqm_uciqe_f32(*(args[:-1] + [16]), 2, 400, 600, 170, None) == 1 and b"workspace" in lib.bem_last_error()
    assert lib.bem_uiqm_ws_bytes(2, 400, 600, 170) > 0 and lib.bem_uiqm_ws_bytes(2, 9, 256, 9) == 0
