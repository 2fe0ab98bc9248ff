"""Writes tests/golden/g16_uiqm.npz: UIQM and UCIQE (basicsr/metrics/uciqe_uiqm.py) as Enhancement/eval.py:255-260 calls them, and the
candidate choice of eval.py:276-280, recorded from the reference on the CPU.

The reference module imports cv2 and skimage at the top.  skimage is never used by getUIQM / getUCIQE, so an empty module stands in for
it.  cv2 is used once, by getUCIQE's cvtColor(RGB2LAB); the stand-in here is tests/uiqm_ref.rgb2lab_u8, the restatement of OpenCV's
8-bit RGB2Lab_b.  Everything in UCIQE after the colour conversion, and all of UIQM with Pillow's real resize, is the reference's own
code.  img_as_ubyte (skimage) is rint(255 x) in float32, as skimage computes it for float32 input.

The inputs are not copied: they are named entries of g13_niqe.npz (crop400x600, crop193x290, crop256, and the six gamma / gain
candidates rebuilt from cand_src and cand_gk), plus ``portrait``, the transposed 400 x 600 crop (resized to 384 x 256).
Contents per input k: uicm_k, uism_k, uiconm_k, uiqm_k, var_chr_k, con_lum_k, aver_sat_k, uciqe_k; for the candidate set the same
parts as (6,) arrays cand_<part>, and cand_best_w (3,) the chosen index for uiqm_weight in cand_w = (1.0, 0.5, 0.0).

    python tests/golden/make_golden_uiqm.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, TESTS)
import ref_harness  # noqa: E402
import uiqm_ref as R  # noqa: E402
import niqe_ref  # noqa: E402

NAMES = ("crop400x600", "crop193x290", "crop256", "portrait")
CAND_W = (1.0, 0.5, 0.0)


def load_reference():
    """The reference's uciqe_uiqm.py as a module, with the cv2 / skimage stand-ins described above."""
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_RGB2LAB = 45
    cv2.cvtColor = lambda img, code: R.rgb2lab_u8(img) if code == 45 else (_ for _ in ()).throw(NotImplementedError(code))
    sk = types.ModuleType("skimage")
    sk.filters, sk.color = types.ModuleType("skimage.filters"), types.ModuleType("skimage.color")
    saved = {k: sys.modules.get(k) for k in ("cv2", "skimage")}
    sys.modules.update({"cv2": cv2, "skimage": sk})
    try:
        spec = importlib.util.spec_from_file_location("ref_uciqe_uiqm", os.path.join(ref_harness.REF, "basicsr", "metrics", "uciqe_uiqm.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def img_as_ubyte(pred):
    return np.rint(pred.astype(np.float32) * np.float32(255)).astype(np.uint8)


def reference_parts(mod, pred):
    """eval.py:256-260 for one candidate, with getUCIQE's lines :44-73 re-walked to keep its three parts (the total must equal
    getUCIQE's) and getUIQM's parts from its own helpers (their combination must equal getUIQM's)."""
    from PIL import Image
    img_rgb = np.array(Image.fromarray(img_as_ubyte(pred)).resize((256, int(256 / pred.shape[1] * pred.shape[0]))))
    uiqm = mod.getUIQM(img_rgb)
    x = img_rgb.astype(np.float32)
    uicm, uism, uiconm = mod._uicm(x), mod._uism(x), mod._uiconm(x, 10)
    assert (0.0282 * uicm) + (0.2953 * uism) + (3.5753 * uiconm) == uiqm
    u8 = img_as_ubyte(pred)
    uciqe = mod.getUCIQE(u8)
    lab = R.rgb2lab_u8(u8)
    lum, a, b = lab[..., 0] / 255, lab[..., 1] / 255, lab[..., 2] / 255
    chr_ = np.sqrt(np.square(a) + np.square(b))
    aver_sat = np.mean(chr_ / np.sqrt(np.square(chr_) + np.square(lum)))
    var_chr = np.sqrt(np.mean(abs(1 - np.square(np.mean(chr_) / chr_))))
    hist, _ = np.histogram(lum, 65536)
    cdf = np.cumsum(hist) / np.sum(hist)
    con_lum = (np.where(cdf >= 0.99)[0][0] - 1) / 65535 - (np.where(cdf > 0.01)[0][0] - 1) / 65535
    assert 0.4680 * var_chr + 0.2745 * con_lum + 0.2576 * aver_sat == uciqe
    return dict(uicm=uicm, uism=uism, uiconm=uiconm, uiqm=uiqm, var_chr=var_chr, con_lum=con_lum, aver_sat=aver_sat, uciqe=uciqe)


def fixture_inputs(g13):
    """{name: uint8 (h,w,3)} for NAMES, from g13_niqe.npz."""
    out = {k: g13[f"in_{k}"] for k in NAMES[:3]}
    out["portrait"] = np.ascontiguousarray(g13["in_crop400x600"].transpose(1, 0, 2))
    return out


def fixture_candidates(g13):
    return niqe_ref.fixture_candidates(g13)


def main():
    import warnings
    warnings.simplefilter("ignore")
    mod = load_reference()
    g13 = np.load(os.path.join(HERE, "g13_niqe.npz"))
    out = {"names": np.array(NAMES), "cand_w": np.array(CAND_W)}
    for k, img in fixture_inputs(g13).items():
        p = reference_parts(mod, niqe_ref.as_pred(img))
        for part, v in p.items():
            out[f"{part}_{k}"] = np.float64(v)
        print(k, img.shape, {n: round(float(v), 6) for n, v in p.items()})
    cand = [reference_parts(mod, niqe_ref.as_pred(c)) for c in fixture_candidates(g13)]
    for part in R.PART_NAMES:
        out[f"cand_{part}"] = np.array([float(c[part]) for c in cand])
    uiqm, uciqe = [c["uiqm"] for c in cand], [c["uciqe"] for c in cand]
    best = []
    for w in CAND_W:      # eval.py:277-278, verbatim
        best_one_list = (w * np.array(uiqm) / max(uiqm) + (1 - w) * np.array(uciqe) / max(uciqe)).tolist()
        best.append(best_one_list.index(max(best_one_list)))
    out["cand_best_w"] = np.array(best, np.int64)
    print("candidates uiqm", np.round(out["cand_uiqm"], 4), "uciqe", np.round(out["cand_uciqe"], 4), "best", best)
    np.savez_compressed(os.path.join(HERE, "g16_uiqm.npz"), **out)


if __name__ == "__main__":
    main()
