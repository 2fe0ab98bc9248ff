"""build_loss (basicsr/losses/__init__.py) for the losses of the hot path's training step.

``L1Loss`` runs as one HIP reduction kernel forward and one elementwise kernel backward (bem.autograd.L1LossFn).  ``PerceptualLoss``
(VGG19 features, criterion l1) is bem.percep's module: one autograd node of HIP kernels (bem.autograd.PerceptualFn); its weights are
read from a torchvision state dict on disk (bem.percep.weights_path), never fetched.  ``SSIMLoss`` is one tiled HIP kernel forward (plus
the fixed-order sum of its partials) and one backward (bem.autograd.SSIMLossFn)."""
from copy import deepcopy

import torch.nn as nn

from basicsr.utils.registry import LOSS_REGISTRY
from basicsr.utils.registry import ARCH_REGISTRY
from bem import autograd as _ag
from bem.percep import PerceptualLoss, VGGFeatureExtractor

__all__ = ["build_loss", "L1Loss", "SSIMLoss", "PerceptualLoss", "VGGFeatureExtractor"]

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


@LOSS_REGISTRY.register()
class SSIMLoss(nn.Module):
    """The structural term of basicsr/losses/my_loss.py:37-38: loss_weight * (1 - pytorch_msssim.ssim(pred, target, data_range=1.0,
    size_average=True)): 11x11 Gaussian window (sigma 1.5), valid region, every (b,c) plane on its own, mean over all positions."""

    def __init__(self, loss_weight=1.0, reduction="mean", window_size=11, sigma=1.5):
        super().__init__()
        if reduction != "mean":
            raise ValueError(f"Unsupported reduction mode: {reduction}. The HIP path implements 'mean' (size_average=True).")
        if window_size != 11:
            raise ValueError(f"Unsupported window_size: {window_size}. The HIP path implements the 11x11 window (pytorch_msssim's default).")
        if sigma != 1.5:
            raise ValueError(f"Unsupported sigma: {sigma}. The HIP path implements sigma 1.5 (pytorch_msssim's default).")
        self.loss_weight, self.reduction, self.window_size, self.sigma = loss_weight, reduction, window_size, sigma

    def forward(self, pred, target, weight=None, **kwargs):
        if weight is not None:
            raise NotImplementedError("SSIMLoss: element-wise weights are not used on the BEM path")
        return _ag.ssim_loss(pred, target, self.loss_weight)


def build_loss(opt):
    opt = deepcopy(opt)
    loss_type = opt.pop("type")
    return LOSS_REGISTRY.get(loss_type)(**opt)
