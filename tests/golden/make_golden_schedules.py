"""Writes tests/golden/g20_schedules.npz from the reference's own scheduler classes and BaseModel wiring, on CPU.

  python tests/golden/make_golden_schedules.py

The reference's ``BaseModel`` (basicsr/models/base_model.py) is imported from its real file next to a namespace stand-in for
``basicsr.models``; for each configuration below an instance gets one SGD optimizer over a single CPU parameter, builds its scheduler with
its own ``setup_schedulers`` (:124-161) and is driven like basicsr/train.py drives it: ``update_learning_rate(i, warmup_iter)`` for
i = 1 .. n (:209-230), the learning rate of group 0 read after each call.  Two configurations per class -- repeated milestones, a
restart, eta_min > 0, uneven periods, both envelope changes of VibrateLR -- and one of them once more under a linear warm-up.

Recorded numbers only: ``configs`` is a JSON string {name: {"train": the train block, "warmup_iter": w, "n": iterations}}, ``lr/<name>``
the float64 sequence of that run.
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

BASE_LR = 2e-4
CONFIGS = {
    "multistep_repeated": ({"scheduler": {"type": "MultiStepLR", "milestones": [50, 50, 120, 200], "gamma": 0.5}}, -1, 300),
    "multistep_restart": ({"scheduler": {"type": "MultiStepRestartLR", "milestones": [40, 90, 160, 220], "gamma": 0.1, "restarts": [0, 150],
                                         "restart_weights": [1, 0.5]}}, -1, 300),
    "cosine_uneven": ({"scheduler": {"type": "CosineAnnealingRestartLR", "periods": [100, 60, 140], "restart_weights": [1, 0.5, 0.25],
                                     "eta_min": 1e-6}}, -1, 300),
    "cosine_even": ({"scheduler": {"type": "CosineAnnealingRestartLR", "periods": [150, 150], "restart_weights": [1, 1], "eta_min": 0}}, -1, 300),
    "cosine_uneven_warmup": ({"scheduler": {"type": "CosineAnnealingRestartLR", "periods": [100, 60, 140], "restart_weights": [1, 0.5, 0.25],
                                            "eta_min": 1e-6}}, 30, 300),
    "linear_300": ({"scheduler": {"type": "LinearLR"}, "total_iter": 300}, -1, 300),
    "linear_257": ({"scheduler": {"type": "LinearLR"}, "total_iter": 257}, -1, 250),
    "vibrate_400": ({"scheduler": {"type": "VibrateLR"}, "total_iter": 400}, -1, 400),
    "vibrate_960": ({"scheduler": {"type": "VibrateLR"}, "total_iter": 960}, -1, 700),
}


def main():
    rh.load()
    rh._ns("basicsr.models", os.path.join(rh.REF, "basicsr", "models"))
    base_model = importlib.import_module("basicsr.models.base_model")
    out = {"configs": np.array(json.dumps({k: {"train": t, "warmup_iter": w, "n": n} for k, (t, w, n) in CONFIGS.items()}))}
    for name, (train, warmup, n) in CONFIGS.items():
        model = base_model.BaseModel({"num_gpu": 0, "is_train": True, "train": json.loads(json.dumps(train))})     # setup_schedulers pops 'type'
        model.optimizers = [torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=BASE_LR)]
        model.setup_schedulers()
        lrs = []
        for i in range(1, n + 1):
            model.update_learning_rate(i, warmup_iter=warmup)
            lrs.append(model.get_current_learning_rate()[0])
        out[f"lr/{name}"] = np.asarray(lrs, dtype=np.float64)
        print(f"  {name:22s} {type(model.schedulers[0]).__name__:26s} n {n}  lr[0] {lrs[0]:.6e}  min {min(lrs):.6e}  last {lrs[-1]:.6e}")
    out["base_lr"] = np.array([BASE_LR])
    path = os.path.join(HERE, "g20_schedules.npz")
    np.savez_compressed(path, **out)
    print(f"  g20_schedules.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
