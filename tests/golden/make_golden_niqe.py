"""Writes tests/golden/g13_niqe.npz: NIQE (basicsr/metrics/niqe.py) as Enhancement/eval.py:248-254 calls it, recorded from the reference
on the CPU.  The reference is imported the way ref_harness.py does it, plus a stub ``cv2`` (niqe.py imports it; only its
convert_to='gray' branch uses it, which eval.py never takes).

Contents: the pristine-model arrays (mu_pris_param, cov_pris_param, gaussian_window); uint8 HWC inputs (used as /255 float32 candidates)
and, per input, the reference's per-block feature matrix (nblocks x 36, idx_w-major), mu_d, cov_d and score; a candidate set of 6
gamma / gain variants of one crop with their scores and index(min(scores)) (eval.py:272-274).  To stay small, the saturated input is
stored as its box (rows, cols saturated to 255 in the 400 x 600 crop) and the candidates as their source crop plus (gamma, gain) pairs:
``saturate`` and ``variant`` below rebuild them exactly.

    python tests/golden/make_golden_niqe.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness  # noqa: E402


SAT_BOX = (96, 296, 192, 442)
CAND_GK = ((0.35, 1.0), (0.45, 1.0), (0.6, 1.0), (0.45, 1.3), (0.8, 1.2), (1.0, 2.0))


def saturate(img, box):
    out = img.copy()
    out[box[0]:box[1], box[2]:box[3]] = 255
    return out


def variant(u8, g, k):
    """uint8 -> uint8: clip(k * (u8 / 255) ** g, 0, 1) * 255, rounded."""
    return np.rint(np.clip(k * (u8.astype(np.float64) / 255.0) ** g, 0, 1) * 255).astype(np.uint8)


def load_reference():
    ref_harness.load()
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    import importlib
    cu = importlib.import_module("basicsr.utils.color_util")
    sys.modules["basicsr.utils"].bgr2ycbcr = cu.bgr2ycbcr
    ref_harness._ns("basicsr.metrics", os.path.join(ref_harness.REF, "basicsr", "metrics"))
    return importlib.import_module("basicsr.metrics.niqe"), importlib.import_module("basicsr.metrics.metric_util"), \
        importlib.import_module("basicsr.utils.matlab_functions")


def reference_walk(niqe_mod, mu_, mf, pred, pris):
    """calculate_niqe(pred * 255, crop_border=0) with niqe()'s loop re-walked through the reference's own pieces so that the feature
    matrix is kept; the score must equal calculate_niqe's."""
    from scipy.ndimage import convolve
    win = pris["gaussian_window"]
    img = np.squeeze(mu_.to_y_channel(mu_.reorder_image((pred * 255).astype(np.float32), input_order="HWC"))).round()
    h, w = img.shape
    nbh, nbw = h // 96, w // 96
    img = img[:nbh * 96, :nbw * 96]
    rows = []
    for scale in (1, 2):
        mu = convolve(img, win, mode="nearest")
        sigma = np.sqrt(np.abs(convolve(np.square(img), win, mode="nearest") - np.square(mu)))
        n = (img - mu) / (sigma + 1)
        bs = 96 // scale
        rows.append(np.array([niqe_mod.compute_feature(n[bh * bs:(bh + 1) * bs, bw * bs:(bw + 1) * bs])
                              for bw in range(nbw) for bh in range(nbh)]))
        if scale == 1:
            img = mf.imresize(img / 255., scale=0.5, antialiasing=True) * 255.
    feat = np.concatenate(rows, axis=1)
    mu_d = np.nanmean(feat, axis=0)
    cov_d = np.cov(feat[~np.isnan(feat).any(axis=1)], rowvar=False)
    score = niqe_mod.calculate_niqe(pred * 255, crop_border=0)
    d = pris["mu_pris_param"] - mu_d
    again = float(np.sqrt(np.squeeze(d @ np.linalg.pinv((pris["cov_pris_param"] + cov_d) / 2) @ d.T)))
    assert abs(again - score) <= 1e-9 * abs(score), (again, score)
    return feat, mu_d, cov_d, score


def main():
    import warnings
    warnings.simplefilter("ignore")
    from PIL import Image
    niqe_mod, mu_, mf = load_reference()
    pris = dict(np.load(os.path.join(ref_harness.REF, "basicsr", "metrics", "niqe_pris_params.npz")))
    demo = np.asarray(Image.open(os.path.join(ref_harness.REF, "assets", "input_demo.png")).convert("RGB"), dtype=np.float64) / 255.0
    bright = lambda a, g: np.rint(np.clip(a ** g, 0, 1) * 255).astype(np.uint8)
    base = bright(demo[100:500, 200:800], 0.45)
    inputs = {"crop400x600": base, "saturated": saturate(base, SAT_BOX), "crop193x290": bright(demo[300:493, 500:790], 0.45),
              "crop256": bright(demo[200:456, 700:956], 0.5)}
    out = {k: v for k, v in pris.items()}
    names = list(inputs)
    out["names"], out["sat_box"] = np.array(names), np.array(SAT_BOX)
    for k in names:
        pred = inputs[k].astype(np.float32) / np.float32(255)
        feat, mu_d, cov_d, score = reference_walk(niqe_mod, mu_, mf, pred, pris)
        if k != "saturated":
            out[f"in_{k}"] = inputs[k]
        out[f"feat_{k}"], out[f"mud_{k}"], out[f"covd_{k}"], out[f"score_{k}"] = feat, mu_d, cov_d, np.float64(score)
        print(f"{k}: {inputs[k].shape} blocks {feat.shape[0]} NaN rows {int(np.isnan(feat).any(axis=1).sum())} score {score:.6f}")
    crop = bright(demo[150:342, 300:588], 0.7)
    cands = np.stack([variant(crop, g, k) for g, k in CAND_GK])
    scores = [niqe_mod.calculate_niqe(c.astype(np.float32) / np.float32(255) * 255, crop_border=0) for c in cands]
    out["cand_src"], out["cand_gk"], out["cand_scores"], out["cand_best"] = crop, np.array(CAND_GK), np.array(scores), np.int64(scores.index(min(scores)))
    print("candidates:", np.round(scores, 4), "best", scores.index(min(scores)))
    np.savez_compressed(os.path.join(HERE, "g13_niqe.npz"), **out)


if __name__ == "__main__":
    main()
