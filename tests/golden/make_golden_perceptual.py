"""Writes tests/golden/g17_perceptual.npz from the reference's own PerceptualLoss class, on CPU.

  python tests/golden/make_golden_perceptual.py

The reference builds its VGG19 through ``torchvision.models.vgg.vgg19`` and fetches pretrained weights; neither torchvision nor the
weights are needed for a fixture, so a stand-in module provides ``vgg19``: configuration E (an ``nn.Sequential`` ``features`` of
Conv2d / ReLU(inplace) / MaxPool2d in torchvision's order) with seeded Kaiming-normal weights and small non-zero biases.  The class
that runs -- input normalisation, the walk with its in-place ReLU and ``clone()``, the L1 terms, the weights -- is the reference's
(basicsr/losses/basic_loss.py:146-238, basicsr/archs/vgg_arch.py:54-161), imported from its real files next to a namespace stand-in
for ``basicsr.losses``.

Recorded for layer_weights {'conv1_2': 1.0, 'conv2_2': 0.5}, perceptual_weight 0.01, two (2,3,20,24) inputs in [0,1]: the eight weight /
bias tensors of features.0 .. features.7, both inputs, the two features of x, the loss and d loss / d x.  The weights are rounded to
float16 BEFORE the reference runs and stored as float16 (exact), which keeps the file under 1 MiB; the tests widen them to float32.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

LAYER_WEIGHTS = {"conv1_2": 1.0, "conv2_2": 0.5}
PERCEPTUAL_WEIGHT = 0.01
CFG_E = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"]


class _VGG(nn.Module):
    def __init__(self, features):
        super().__init__()
        self.features = features


def _vgg19(pretrained=False, **kw):
    g = torch.Generator().manual_seed(1719)
    layers, cin = [], 3
    for v in CFG_E:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            continue
        conv = nn.Conv2d(cin, v, kernel_size=3, padding=1)
        with torch.no_grad():
            conv.weight.copy_((torch.randn(conv.weight.shape, generator=g) * (2.0 / (v * 9)) ** 0.5).half().float())
            conv.bias.copy_((torch.randn(v, generator=g) * 0.05).half().float())
        layers += [conv, nn.ReLU(inplace=True)]
        cin = v
    return _VGG(nn.Sequential(*layers))


def main():
    rh.load()
    tv, tvm, tvv = types.ModuleType("torchvision"), types.ModuleType("torchvision.models"), types.ModuleType("torchvision.models.vgg")
    tv.__path__, tvm.__path__ = [], []
    tvv.vgg19 = _vgg19
    tv.models, tvm.vgg = tvm, tvv
    sys.modules.update({"torchvision": tv, "torchvision.models": tvm, "torchvision.models.vgg": tvv})
    rh._ns("basicsr.losses", os.path.join(rh.REF, "basicsr", "losses"))
    basic_loss = importlib.import_module("basicsr.losses.basic_loss")
    with rh.ref_ctor_env():          # cwd = the reference root, where experiments/pretrained_models/ does not exist: vgg19(pretrained=True) above
        crit = basic_loss.PerceptualLoss(layer_weights=dict(LAYER_WEIGHTS), vgg_type="vgg19", use_input_norm=True, range_norm=False,
                                         perceptual_weight=PERCEPTUAL_WEIGHT, style_weight=0, criterion="l1")
    g = torch.Generator().manual_seed(1720)
    x = torch.rand(2, 3, 20, 24, generator=g).requires_grad_(True)
    gt = torch.rand(2, 3, 20, 24, generator=g)
    loss, style = crit(x, gt)
    assert style is None
    (dx,) = torch.autograd.grad(loss, x)
    with torch.no_grad():
        feats = crit.vgg(x)
    out = {"x": x.detach(), "gt": gt, "loss": loss.detach().reshape(1), "dx": dx, "perceptual_weight": torch.tensor([PERCEPTUAL_WEIGHT])}
    for k, w in LAYER_WEIGHTS.items():
        out[f"feat/{k}"] = feats[k]
        out[f"layer_weight/{k}"] = torch.tensor([w])
    names = importlib.import_module("basicsr.archs.vgg_arch").NAMES["vgg19"]
    for k, v in crit.vgg.vgg_net.state_dict().items():          # keys conv1_1.weight ...: stored under torchvision's features.{i} names
        name, kind = k.split(".")
        out[f"sd/features.{names.index(name)}.{kind}"] = v.half()
    path = os.path.join(HERE, "g17_perceptual.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print(f"  g17_perceptual.npz  {os.path.getsize(path) / 1024:.1f} KiB, loss {float(loss.detach()):.9e}, {sum(v.numel() for k, v in out.items() if k.startswith('sd/'))} weight floats")


if __name__ == "__main__":
    main()
