"""CPU: NIQE no-reference selection (eval.py --no_ref niqe).  The float64 restatement (tests/niqe_ref.py) against the reference's recorded
features and scores (g13_niqe.npz), the host-built tables of bem.tables against the reference's own formulas (live, skipped without the
reference tree), and the argument checks that come before any GPU call."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, PKG

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import niqe_ref as R  # noqa: E402

REGULAR = ("crop400x600", "crop193x290", "crop256")


@pytest.fixture(scope="module")
def g13():
    return np.load(os.path.join(GOLDEN, "g13_niqe.npz"))


def _alpha_steps(a, b):
    return np.rint(np.abs(a - b) / 1e-3).astype(int)


@pytest.mark.parametrize("name", REGULAR)
def test_restatement_matches_reference(g13, name):
    """Inputs without saturated areas: score to 1e-5 relative, every alpha exactly, the other features to 1e-4 relative
    (2e-5 absolute for the small (beta_r - beta_l) means, which cancel)."""
    img = R.fixture_inputs(g13)[name]
    feat = R.features(R.y_channel(R.as_pred(img)), g13["gaussian_window"])
    ref = g13[f"feat_{name}"]
    assert feat.shape == ref.shape == ((img.shape[0] // 96) * (img.shape[1] // 96), 36)
    assert np.array_equal(feat[:, R.ALPHA_COLS], ref[:, R.ALPHA_COLS])
    np.testing.assert_allclose(feat, ref, rtol=1e-4, atol=2e-5)
    score, mu_d, cov_d = R.mvg(feat, g13["mu_pris_param"], g13["cov_pris_param"])
    np.testing.assert_allclose(mu_d, g13[f"mud_{name}"], rtol=1e-4, atol=2e-6)
    np.testing.assert_allclose(cov_d, g13[f"covd_{name}"], rtol=1e-3, atol=1e-7)
    assert abs(score / float(g13[f"score_{name}"]) - 1) <= 1e-5


def test_restatement_saturated_and_candidates(g13):
    """Saturated areas: the NaN rows (blocks without negative or positive coefficients) sit where the reference's do and the score is
    finite.  Next to a saturated patch sigma = sqrt(|E[x^2] - mu^2|) cancels in float32, so a 1-ulp difference in the resized image
    (torch's BLAS summation order) can move one alpha by a grid step: score to 1e-4, alphas within one step, >= 99 % equal.
    The candidate set: the reference's index(min)."""
    img = R.fixture_inputs(g13)["saturated"]
    feat = R.features(R.y_channel(R.as_pred(img)), g13["gaussian_window"])
    ref = g13["feat_saturated"]
    nan = np.isnan(ref).any(axis=1)
    assert nan.any() and not nan.all()
    assert np.array_equal(np.isnan(feat), np.isnan(ref))
    steps = _alpha_steps(feat[:, R.ALPHA_COLS], ref[:, R.ALPHA_COLS])
    assert steps.max() <= 1 and (steps == 0).mean() >= 0.99
    score = R.mvg(feat, g13["mu_pris_param"], g13["cov_pris_param"])[0]
    assert np.isfinite(score) and abs(score / float(g13["score_saturated"]) - 1) <= 1e-4
    scores = [R.niqe(R.as_pred(c), g13) for c in R.fixture_candidates(g13)]
    np.testing.assert_allclose(scores, g13["cand_scores"], rtol=1e-4)
    assert scores.index(min(scores)) == int(g13["cand_best"])


def test_flat_image_scores_nan(g13):
    """Every block of a flat image has no negative and no positive coefficient: all rows NaN, no covariance (the reference raises)."""
    assert np.isnan(R.niqe(np.full((192, 192, 3), 0.4, np.float32), g13))


@pytest.fixture
def reference():
    """The reference's NIQE modules (make_golden_niqe.load_reference).  Loading them swaps the reference's basicsr in for this
    package's mirror; the mirror and sys.path are put back afterwards so that later tests in the process see the product again."""
    sys.path.insert(0, GOLDEN)
    import ref_harness
    if not ref_harness.available():
        pytest.skip("reference tree not present")
    import make_golden_niqe
    mine = lambda k: k == "basicsr" or k.startswith("basicsr.")
    saved = {k: v for k, v in sys.modules.items() if mine(k)}
    path = list(sys.path)
    try:
        yield make_golden_niqe.load_reference()
    finally:
        for k in [k for k in sys.modules if mine(k)]:
            del sys.modules[k]
        sys.modules.update(saved)
        sys.path[:] = path


def test_host_tables_match_reference(reference):
    """bem.tables' gamma table and resize tables against the reference's formulas, live: the gamma ratios of estimate_aggd_param
    (niqe.py:24-26,35-36,59) with scipy's gamma, and calculate_weights_indices (matlab_functions.py:16-81) with its padding."""
    import math
    from scipy.special import gamma
    from bem import tables
    niqe_mod, _, mf = reference
    tab = tables.niqe_gamma_table()
    gam = np.arange(0.2, 10.001, 0.001)
    rec = np.reciprocal(gam)
    assert tab.shape == (4, 9801) and np.array_equal(tab[0], gam)
    np.testing.assert_allclose(tab[1], np.square(gamma(rec * 2)) / (gamma(rec) * gamma(rec * 3)), rtol=1e-13)
    np.testing.assert_allclose(tab[2], np.sqrt(gamma(1 / gam) / gamma(3 / gam)), rtol=1e-13)
    np.testing.assert_allclose(tab[3], gamma(2 / gam) / gamma(1 / gam), rtol=1e-13)
    # the same alpha as the reference's own estimate for a few AGGD-like blocks
    rng = np.random.default_rng(3)
    for s in (0.5, 1.0, 2.0):
        x = (rng.standard_normal((96, 96)) * rng.random((96, 96)) ** s).astype(np.float32)
        a = niqe_mod.estimate_aggd_param(x)[0]
        assert a == R.aggd(x)[1]
    for n in (96, 192, 288, 384, 576, 1056):
        wt, ix = tables.niqe_resize_table(n)
        rw, ri, s0, _ = mf.calculate_weights_indices(n, math.ceil(n * 0.5), 0.5, "cubic", 4, True)
        assert np.array_equal(wt, rw.numpy()), n
        src = ri.numpy().astype(np.int64) - s0                # padded-array position -> 0-based source, then the symmetric fold
        src = np.where(src < 0, -src - 1, np.where(src >= n, 2 * n - 1 - src, src))
        assert np.array_equal(ix, src), n


def test_eval_niqe_needs_params_before_any_gpu_call():
    spec = importlib.util.spec_from_file_location("bem_eval_driver_niqe", os.path.join(PKG, "Enhancement", "eval.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    with pytest.raises(SystemExit) as e:
        drv.main(["--no_ref", "niqe", "--input_dir", "/nonexistent"])
    assert "niqe_pris_params.npz" in str(e.value) and "--niqe_params" in str(e.value)
    with pytest.raises(SystemExit) as e:
        drv.main(["--no_ref", "uiqm_uciqe", "--input_dir", "/nonexistent"])
    assert "uiqm_uciqe" in str(e.value) and "niqe " not in str(e.value)


def test_niqe_entry_rejects_before_any_hip_call():
    from bem import native
    if not os.path.exists(native.LIB_PATH):
        native.build()
    lib = native.lib()
    rc = lib.bem_niqe_f32(*([None] * 5), 9801, None, None, 8, None, None, 8, None, None, 0, 2, 400, 600, None)
    assert rc == 1 and b"null" in lib.bem_last_error()
    p = 16   # any non-null value: the checks below reject before a pointer is touched
    args = [p] * 5 + [9801, p, p, 8, p, p, 8, p, p, 1 << 40]
    assert lib.bem_niqe_f32(*args, 2, 95, 600, None) == 1 and b"96" in lib.bem_last_error()
    assert lib.bem_niqe_f32(*args, 2, 400, 90, None) == 1 and b"96" in lib.bem_last_error()
    assert lib.bem_niqe_f32(*(args[:-1] + [16]), 2, 400, 600, None) == 1 and b"workspace" in lib.bem_last_error()
    assert lib.bem_niqe_ws_bytes(2, 400, 600) > 0 and lib.bem_niqe_ws_bytes(2, 95, 600) == 0
