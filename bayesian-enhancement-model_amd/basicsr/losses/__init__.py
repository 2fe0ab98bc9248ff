"""build_loss (basicsr/losses/__init__.py) for the losses of the hot path's training step.

``L1Loss`` runs as one HIP reduction kernel forward and one elementwise kernel backward (bem.autograd.L1LossFn); ``MSELoss`` and
``CharbonnierLoss``, the other two pixel losses of basic_loss.py, have the same shape (MSELossFn, CharbonnierLossFn).  ``PerceptualLoss``
(VGG19 features, criterion l1 or l2) is bem.percep's module: one autograd node of HIP kernels (bem.autograd.PerceptualFn); its weights are
read from a torchvision state dict on disk (bem.percep.weights_path), never fetched.  ``SSIMLoss`` is one tiled HIP kernel forward (plus
the fixed-order sum of its partials) and one backward (bem.autograd.SSIMLossFn).  ``LPIPSLoss`` is the metric of bem.lpips (v0.1, AlexNet)
without its quantisation, as one autograd node of HIP kernels (bem.autograd.LPIPSFn); its two weight files are found on disk
(bem.lpips.find_weight_files), never fetched.  ``CombinedLoss`` is the reference's six-term recipe (my_loss.py:51-74): its four
per-pixel statistics in one HIP pass (bem.autograd.PixStatLossFn) beside ``SSIMLoss`` and ``PerceptualLoss`` with criterion l2."""
from copy import deepcopy

import torch.nn as nn

from basicsr.utils.registry import LOSS_REGISTRY
from basicsr.utils.registry import ARCH_REGISTRY
from bem import autograd as _ag
from bem.lpips import LPIPS
from bem.ops import PIXSTAT_VALUES
from bem.percep import PerceptualLoss, VGGFeatureExtractor

__all__ = ["build_loss", "L1Loss", "MSELoss", "CharbonnierLoss", "SSIMLoss", "LPIPSLoss", "CombinedLoss", "PerceptualLoss", "VGGFeatureExtractor"]
_PIXSTAT_AT = {name: i for i, name in enumerate(PIXSTAT_VALUES)}

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


def _mean_or_sum(name, reduction):
    """'mean' and 'sum' are one kernel: a sum is the mean under the weight times the element count (``_weight``)."""
    if reduction not in ("mean", "sum"):
        raise ValueError(f"Unsupported reduction mode: {reduction}. {name} on the HIP path implements 'mean' and 'sum' (a scalar loss).")
    return reduction


def _weight(mod, pred):
    return mod.loss_weight * pred.numel() if mod.reduction == "sum" else mod.loss_weight


@LOSS_REGISTRY.register()
class MSELoss(nn.Module):
    """basicsr/losses/basic_loss.py:55-80: loss_weight * mean (or sum) of (pred - target)^2; per-element weights unsupported."""

    def __init__(self, loss_weight=1.0, reduction="mean"):
        super().__init__()
        self.loss_weight, self.reduction = loss_weight, _mean_or_sum("MSELoss", reduction)

    def forward(self, pred, target, weight=None, **kwargs):
        if weight is not None:
            raise NotImplementedError("MSELoss: element-wise weights are not used on the BEM path")
        return _ag.mse_loss(pred, target, _weight(self, pred))


@LOSS_REGISTRY.register()
class CharbonnierLoss(nn.Module):
    """basicsr/losses/basic_loss.py:83-114: loss_weight * mean (or sum) of sqrt((pred - target)^2 + eps); per-element weights unsupported."""

    def __init__(self, loss_weight=1.0, reduction="mean", eps=1e-12):
        super().__init__()
        self.loss_weight, self.reduction, self.eps = loss_weight, _mean_or_sum("CharbonnierLoss", reduction), eps

    def forward(self, pred, target, weight=None, **kwargs):
        if weight is not None:
            raise NotImplementedError("CharbonnierLoss: element-wise weights are not used on the BEM path")
        return _ag.charbonnier_loss(pred, target, _weight(self, pred), self.eps)


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


@LOSS_REGISTRY.register()
class CombinedLoss(nn.Module):
    """basicsr/losses/my_loss.py:51-74, the reference's own loss recipe with its weights as defaults:
        loss_weight * (alpha1 smooth_l1 + alpha2 VGG19[:16]-MSE + alpha3 histogram + alpha4 (1 - SSIM) + alpha5 psnr_loss + alpha6 color_loss)
    Three autograd nodes: the four per-pixel statistics in one pass (bem.autograd.PixStatLossFn, csrc/pixstat_loss.hip), ``SSIMLoss`` and
    ``PerceptualLoss({'relu3_3': 1}, criterion='l2')`` on the raw images (``vgg19.features[:16]`` with F.mse_loss, my_loss.py:12-19); their
    gradients into pred are summed by bem_add_f32 (ag.fork_n).  A zero alpha switches its part off entirely: alpha2 = 0 needs no VGG file,
    alpha4 = 0 allows images below 11x11.  ``vgg_weights`` names the torchvision vgg19 state dict (otherwise bem.percep.weights_path);
    ``state_dict`` hands one over directly (keys features.0 .. features.14).  After a forward ``parts`` holds the unweighted values of
    the active parts as device scalars, in the order of PARTS."""
    ALPHAS = ("alpha1", "alpha2", "alpha3", "alpha4", "alpha5", "alpha6")
    PARTS = ("smooth_l1", "percep", "hist", "psnr", "color", "ssim")              # the part alpha1 .. alpha6 weighs

    def __init__(self, alpha1=1.00, alpha2=0.06, alpha3=0.05, alpha4=0.5, alpha5=0.0083, alpha6=0.25, loss_weight=1.0, vgg_weights=None,
                 state_dict=None):
        super().__init__()
        for k, v in zip(self.ALPHAS, (alpha1, alpha2, alpha3, alpha4, alpha5, alpha6)):
            if not v >= 0:
                raise ValueError(f"CombinedLoss: {k}={v}: a weight of the recipe is >= 0 (0 switches its part off)")
            setattr(self, k, float(v))
        if not loss_weight > 0:
            raise ValueError(f"CombinedLoss: loss_weight={loss_weight} must be positive (set an alpha to 0 to switch a part off)")
        if not any(getattr(self, k) > 0 for k in self.ALPHAS):
            raise ValueError("CombinedLoss: alpha1 .. alpha6 are all 0: no part is left")
        self.loss_weight = float(loss_weight)
        self.percep = self.ssim = None
        if self.alpha2 > 0:
            if state_dict is None and vgg_weights is not None:
                from bem.percep import load_vgg19_state_dict
                state_dict = load_vgg19_state_dict(vgg_weights)
            self.percep = PerceptualLoss({"relu3_3": 1}, use_input_norm=False, range_norm=False, criterion="l2",
                                         perceptual_weight=self.alpha2 * self.loss_weight, state_dict=state_dict)
        if self.alpha4 > 0:
            self.ssim = SSIMLoss(loss_weight=self.alpha4 * self.loss_weight)
        self.pix_alphas = tuple(a * self.loss_weight for a in (self.alpha1, self.alpha3, self.alpha5, self.alpha6))
        self.parts = {}

    @staticmethod
    def find_weights(opt):
        """For a ``train.combined_opt`` block: the path of the VGG19 state dict its alpha2 part will read (FileNotFoundError if the file
        is missing), None where that part is off.  The training driver asks before a model exists."""
        from bem.percep import find_vgg19_weights
        if not opt.get("alpha2", 0.06) > 0 or opt.get("state_dict") is not None:
            return None
        return find_vgg19_weights(opt.get("vgg_weights"))

    def forward(self, pred, target, weight=None, **kwargs):
        if weight is not None:
            raise NotImplementedError("CombinedLoss: element-wise weights are not used on the BEM path")
        pix = any(a > 0 for a in self.pix_alphas)
        heads = iter(_ag.fork_n(pred, int(pix) + (self.percep is not None) + (self.ssim is not None)))
        terms, parts = [], {}
        if pix:
            l, vals = _ag.pixstat_loss(next(heads), target, self.pix_alphas)
            terms.append(l)
            for name, a in zip(("smooth_l1", "hist", "psnr", "color"), self.pix_alphas):
                if a > 0:
                    parts[name] = vals[_PIXSTAT_AT[name]]
        if self.percep is not None:
            l, _ = self.percep(next(heads), target)
            terms.append(l)
            parts["percep"] = l.detach() / self.percep.perceptual_weight
        if self.ssim is not None:
            l = self.ssim(next(heads), target)
            terms.append(l)
            parts["ssim"] = l.detach() / self.ssim.loss_weight
        self.parts = {k: parts[k] for k in self.PARTS if k in parts}
        total = terms[0]
        for l in terms[1:]:
            total = _ag.AddFn.apply(total, l)
        return total


def build_loss(opt):
    opt = deepcopy(opt)
    loss_type = opt.pop("type")
    return LOSS_REGISTRY.get(loss_type)(**opt)
