"""build_loss (basicsr/losses/__init__.py) for the losses of the hot path's training step.

``L1Loss`` runs as one HIP reduction kernel forward and one elementwise kernel backward (bem.autograd.L1LossFn).  ``PerceptualLoss``
(VGG19 features, criterion l1) is bem.percep's module: one autograd node of HIP kernels (bem.autograd.PerceptualFn); its weights are
read from a torchvision state dict on disk (bem.percep.weights_path), never fetched."""
from copy import deepcopy

import torch.nn as nn

from basicsr.utils.registry import LOSS_REGISTRY
from basicsr.utils.registry import ARCH_REGISTRY
from bem import autograd as _ag
from bem.percep import PerceptualLoss, VGGFeatureExtractor

__all__ = ["build_loss", "L1Loss", "PerceptualLoss", "VGGFeatureExtractor"]

LOSS_REGISTRY.register(PerceptualLoss)
if "VGGFeatureExtractor" not in ARCH_REGISTRY:
    ARCH_REGISTRY.register(VGGFeatureExtractor)                # basicsr/archs/vgg_arch.py:54


@LOSS_REGISTRY.register()
class L1Loss(nn.Module):
    """basicsr/losses/losses.py:28-52: loss_weight * mean |pred - target| (reduction 'mean'; per-element weights unsupported)."""

    def __init__(self, loss_weight=1.0, reduction="mean"):
        super().__init__()
        if reduction != "mean":
            raise ValueError(f"Unsupported reduction mode: {reduction}. The HIP path implements 'mean' (the shipped option files).")
        self.loss_weight, self.reduction = loss_weight, reduction

    def forward(self, pred, target, weight=None, **kwargs):
        if weight is not None:
            raise NotImplementedError("L1Loss: element-wise weights are not used on the BEM path")
        return _ag.l1_loss(pred, target, self.loss_weight)


def build_loss(opt):
    opt = deepcopy(opt)
    loss_type = opt.pop("type")
    return LOSS_REGISTRY.get(loss_type)(**opt)
