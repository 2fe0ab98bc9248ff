"""build_loss (basicsr/losses/__init__.py) for the losses of the hot path's training step.

``L1Loss`` runs as one HIP reduction kernel forward and one elementwise kernel backward (bem.autograd.L1LossFn).  ``PerceptualLoss``
(VGG19 features, criterion l1) is bem.percep's module: one autograd node of HIP kernels (bem.autograd.PerceptualFn); its weights are
read from a torchvision state dict on disk (bem.percep.weights_path), never fetched.  ``SSIMLoss`` is one tiled HIP kernel forward (plus
the fixed-order sum of its partials) and one backward (bem.autograd.SSIMLossFn).  ``LPIPSLoss`` is the metric of bem.lpips (v0.1, AlexNet)
without its quantisation, as one autograd node of HIP kernels (bem.autograd.LPIPSFn); its two weight files are found on disk
(bem.lpips.find_weight_files), never fetched."""
from copy import deepcopy

import torch.nn as nn

from basicsr.utils.registry import LOSS_REGISTRY
from basicsr.utils.registry import ARCH_REGISTRY
from bem import autograd as _ag
from bem.lpips import LPIPS
from bem.percep import PerceptualLoss, VGGFeatureExtractor

__all__ = ["build_loss", "L1Loss", "SSIMLoss", "LPIPSLoss", "PerceptualLoss", "VGGFeatureExtractor"]

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


@LOSS_REGISTRY.register()
class LPIPSLoss(nn.Module):
    """loss_weight * mean_b d(target_b, pred_b), d what ``lpips.LPIPS(net='alex')(target, pred, normalize=normalize)`` computes (bem.lpips:
    no quantisation, no clipping).  ``normalize=True``: images in [0,1], as the training step holds them; False: already in [-1,1].
    Gradient goes to pred alone; the AlexNet and linear-layer weights are frozen buffers, absent from any state dict.  ``weights_dir``
    names the directory of the two weight files (otherwise BEM_LPIPS_WEIGHTS / experiments/pretrained_models, bem.lpips)."""

    def __init__(self, loss_weight=1.0, reduction="mean", net="alex", normalize=True, weights_dir=None):
        super().__init__()
        if reduction != "mean":
            raise ValueError(f"Unsupported reduction mode: {reduction}. The HIP path implements 'mean' (over the batch).")
        if net != "alex":
            raise ValueError(f"Unsupported net: {net}. The HIP path implements 'alex' (the trunk the evaluation scripts report).")
        self.loss_weight, self.reduction, self.net, self.normalize = loss_weight, reduction, net, bool(normalize)
        self.lpips = LPIPS(net=net, weights_dir=weights_dir)

    def forward(self, pred, target, weight=None, **kwargs):
        if weight is not None:
            raise NotImplementedError("LPIPSLoss: element-wise weights are not used on the BEM path")
        return _ag.lpips_loss(pred, target, self)


def build_loss(opt):
    opt = deepcopy(opt)
    loss_type = opt.pop("type")
    return LOSS_REGISTRY.get(loss_type)(**opt)
