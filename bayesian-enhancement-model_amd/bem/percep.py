"""VGG19 perceptual loss of the Stage-II training step (basicsr/losses/basic_loss.py:146-238 over basicsr/archs/vgg_arch.py:54-161).

``VGGFeatureExtractor`` owns the frozen convolution weights and the operand forms the kernels read; ``PerceptualLoss`` is the
reference's module around it.  The feature pass, the per-layer L1 (criterion l2: MSE) terms and the whole backward are one autograd node of HIP
kernels (bem.autograd.PerceptualFn).  Weights come from a torchvision ``vgg19`` state dict on disk; nothing is ever downloaded."""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import ops

VGG_PRETRAIN_PATH = "experiments/pretrained_models/vgg19-dcbb9e9d.pth"          # vgg_arch.py:9, relative to the working directory
WEIGHTS_ENV = "BEM_VGG19_WEIGHTS"
# vgg_arch.py:27-32; position in the list = index of the layer in torchvision's ``vgg19().features``
VGG19_NAMES = [
    "conv1_1", "relu1_1", "conv1_2", "relu1_2", "pool1", "conv2_1", "relu2_1", "conv2_2", "relu2_2", "pool2",
    "conv3_1", "relu3_1", "conv3_2", "relu3_2", "conv3_3", "relu3_3", "conv3_4", "relu3_4", "pool3", "conv4_1",
    "relu4_1", "conv4_2", "relu4_2", "conv4_3", "relu4_3", "conv4_4", "relu4_4", "pool4", "conv5_1", "relu5_1",
    "conv5_2", "relu5_2", "conv5_3", "relu5_3", "conv5_4", "relu5_4", "pool5"]
_BLOCK_WIDTH = {1: 64, 2: 128, 3: 256, 4: 512, 5: 512}


def conv_shape(name):
    """(Cout, Cin, 3, 3) of a 'convB_I' layer of configuration E."""
    blk, i = int(name[4]), int(name[6:])
    cout = _BLOCK_WIDTH[blk]
    return (cout, (3 if blk == 1 else _BLOCK_WIDTH[blk - 1]) if i == 1 else cout, 3, 3)


def weights_path():
    return os.environ.get(WEIGHTS_ENV) or VGG_PRETRAIN_PATH


def find_vgg19_weights(path=None):
    """The state dict's path (``path`` or weights_path()) if the file is there, FileNotFoundError naming where it is looked for otherwise."""
    path = path or weights_path()
    if not os.path.isfile(path):
        raise FileNotFoundError(f"VGG19 weights not found at '{path}': put torchvision's vgg19-dcbb9e9d.pth at {VGG_PRETRAIN_PATH} (relative to "
                                f"the working directory) or point the environment variable {WEIGHTS_ENV} at it; nothing is downloaded")
    return path


def load_vgg19_state_dict(path=None):
    return torch.load(find_vgg19_weights(path), map_location="cpu", weights_only=True)


class VGGFeatureExtractor(nn.Module):
    """vgg_arch.py:54-161 for ``vgg19``: the layers up to the deepest requested name, frozen.  ``forward(x)`` returns {name: feature}
    ('conv*': before its ReLU); the training step does not go through it but through PerceptualLoss, which walks both images at once."""

    def __init__(self, layer_name_list, vgg_type="vgg19", use_input_norm=True, range_norm=False, requires_grad=False,
                 remove_pooling=False, pooling_stride=2, state_dict=None):
        super().__init__()
        if vgg_type != "vgg19":
            raise NotImplementedError(f"VGGFeatureExtractor: vgg_type '{vgg_type}' is not on the HIP path (vgg19 only, as in every shipped option file)")
        if requires_grad or remove_pooling or pooling_stride != 2:
            raise NotImplementedError(f"VGGFeatureExtractor: requires_grad={requires_grad}, remove_pooling={remove_pooling}, "
                                      f"pooling_stride={pooling_stride}: the HIP path has the frozen net with MaxPool2d(2, 2) only")
        self.layer_name_list = list(layer_name_list)
        if not self.layer_name_list:
            raise ValueError("VGGFeatureExtractor: no layer requested")
        for n in self.layer_name_list:
            if n not in VGG19_NAMES:
                raise ValueError(f"VGGFeatureExtractor: '{n}' is not a vgg19 layer name")
            if n.startswith("pool"):
                raise NotImplementedError(f"VGGFeatureExtractor: feature '{n}': pooled features are not on the HIP path (conv* / relu* names only)")
        self.use_input_norm, self.range_norm = bool(use_input_norm), bool(range_norm)
        self.names = VGG19_NAMES[:max(VGG19_NAMES.index(n) for n in self.layer_name_list) + 1]
        sd = state_dict if state_dict is not None else load_vgg19_state_dict()
        for i, n in enumerate(self.names):
            if not n.startswith("conv"):
                continue
            shp = conv_shape(n)
            for kind, want in (("weight", shp), ("bias", shp[:1])):
                key = f"features.{i}.{kind}"
                if key not in sd:
                    raise KeyError(f"VGG19 state dict has no '{key}' ({n})")
                if tuple(sd[key].shape) != want:
                    raise ValueError(f"VGG19 state dict: '{key}' ({n}) has shape {tuple(sd[key].shape)}, expected {want}")
                self.register_buffer(f"{n}_{kind}", sd[key].detach().to(torch.float32).contiguous().clone(), persistent=False)
        self._ops = None

    def _apply(self, fn, *a, **k):
        self._ops = None                   # the operand forms below belong to the buffers they were packed from
        return super()._apply(fn, *a, **k)

    def conv_operands(self):
        """{conv name: (ConvWeight, bias)}, made on first use and held here for the life of the module: the weights are frozen, so no
        optimizer step invalidates a packed form.  The input gradients read ConvWeight.input_grad()."""
        if self._ops is None:
            with torch.no_grad():
                d = {}
                for n in self.names:
                    if not n.startswith("conv"):
                        continue
                    w = getattr(self, n + "_weight")
                    cw = ops.ConvWeight(w)
                    if n == "conv1_1":           # eight input channels (five of zeros): the Cin % 8 == 0 matrix-core route; its gradient weight is the 3-channel one
                        wf = torch.zeros(w.shape[0], 8, 3, 3, device=w.device, dtype=w.dtype)
                        wf[:, :3] = w
                        cw = ops.ConvWeight(wf, input_grad=cw.input_grad())
                    d[n] = (cw, getattr(self, n + "_bias"))
                self._ops = d
        return self._ops

    def forward(self, x):
        from . import autograd as ag
        with torch.no_grad():
            return ag.vgg_features(self, x.contiguous())


class PerceptualLoss(nn.Module):
    """basic_loss.py:146-238: (percep_loss, style_loss), ``None`` for a disabled term.  ``state_dict=`` (not a reference keyword) hands
    the VGG19 weights over directly instead of reading the file."""

    def __init__(self, layer_weights, vgg_type="vgg19", use_input_norm=True, range_norm=False, perceptual_weight=1.0, style_weight=0.,
                 criterion="l1", state_dict=None):
        super().__init__()
        if style_weight > 0:
            raise NotImplementedError(f"PerceptualLoss: style_weight={style_weight}: the style (Gram) term is not on the HIP path (every shipped option file has 0)")
        if criterion not in ("l1", "l2"):
            raise NotImplementedError(f"PerceptualLoss: criterion '{criterion}' is not on the HIP path (l1, as in every shipped option file, "
                                      "and l2, basic_loss.py:191-192)")
        self.perceptual_weight, self.style_weight, self.criterion_type = perceptual_weight, style_weight, criterion
        self.layer_weights = dict(layer_weights)
        self.vgg = VGGFeatureExtractor(list(self.layer_weights.keys()), vgg_type=vgg_type, use_input_norm=use_input_norm,
                                       range_norm=range_norm, state_dict=state_dict)

    def forward(self, x, gt):
        if not self.perceptual_weight > 0:
            return None, None
        from . import autograd as ag
        return ag.perceptual_loss(x, gt, self), None
