"""Writes tests/golden/g18_data.npz: what the reference's own data-preparation functions return on small seeded inputs (data only).

Loads data/transforms.py, utils/mask.py, utils/labelnoise.py and data/data_sampler.py of the reference by path, with an empty stand-in
module for cv2 (none of the recorded functions calls it).  Run once where the reference tree is available:

    python tests/golden/make_golden_data.py [reference root]
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# the three label-noise factors, as the float32 values a plan row carries
FACTORS = tuple(float(np.float32(v)) for v in (1.02, 1.2, 0.9))


def _load(root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main(root):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    tr = _load(root, "basicsr/data/transforms.py", "_ref_transforms")
    mk = _load(root, "basicsr/utils/mask.py", "_ref_mask")
    ln = _load(root, "basicsr/utils/labelnoise.py", "_ref_labelnoise")
    sm = _load(root, "basicsr/data/data_sampler.py", "_ref_sampler")
    out = {}
    rng = np.random.RandomState(18)
    img = rng.randint(0, 256, (6, 6, 3)).astype(np.uint8)
    out["aug_in"] = img
    for mode in range(8):
        out[f"aug_{mode}"] = np.ascontiguousarray(tr.data_augmentation(img, mode))
    for tag, args in (("a", (8, 1, 1, 0.75)), ("b", (8, 2, 1, 0.4))):
        np.random.seed(18)
        gen = mk.MaskGenerator(*args)
        out[f"mask_{tag}"] = np.stack([gen() for _ in range(4)]).astype(np.int64)
        out[f"mask_{tag}_args"] = np.array(args, np.float64)
    for epoch in (0, 1):
        for rank in range(3):
            s = sm.EnlargedSampler(list(range(10)), 3, rank, 1)
            s.set_epoch(epoch)
            out[f"sampler_e{epoch}_r{rank}"] = np.array(list(s), np.int64)
    bgr = rng.rand(4, 4, 3).astype(np.float32)
    bgr[0, 0] = (0.0, 1.0, 0.995)              # the clips are exercised
    t, b, c = FACTORS
    out["noise_in_bgr"] = bgr
    out["noise_factors"] = np.array(FACTORS, np.float64)
    tem = ln.adjust_color_temperature(bgr, t)
    out["noise_temperature_f64"] = tem
    out["noise_brightness"] = ln.adjust_brightness(bgr, b)
    out["noise_contrast"] = ln.adjust_contrast(bgr, c)
    out["noise_chain"] = ln.adjust_contrast(ln.adjust_brightness(tem, b), c)       # add_label_noise's order (labelnoise.py:59-67)
    assert out["noise_temperature_f64"].dtype == np.float64 and out["noise_chain"].dtype == np.float32
    np.savez_compressed(os.path.join(HERE, "g18_data.npz"), **out)
    print({k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    sys.path.insert(0, HERE)
    from ref_harness import REF
    main(sys.argv[1] if len(sys.argv) > 1 else REF)
