"""LPIPS v0.1 with the AlexNet trunk (Zhang et al. 2018): the ``--lpips`` metric of Enhancement/eval.py:143-145,301-306 and
Enhancement/cal_metrics_with_imgs.py:39-41,51-55, with the call signature of ``lpips.LPIPS(net='alex')``, forward only; the loss term
``train.lpips_opt`` differentiates the same distance through bem.autograd.LPIPSFn, which takes its weights from this module.

Input stage, the two pools and the distance heads are the kernels of csrc/lpips.hip; the five convolutions run on the convolution kernels
bem.ops.conv2d dispatches to.  Weights come from two files the user supplies -- torchvision's ``alexnet-owt-7be5be79.pth`` and the ``lpips``
package's ``weights/v0.1/alex.pth`` -- and nothing is ever downloaded.  Neither package is a dependency, so agreement with the package's own
numbers is not pinned by a test: the definition in DESIGN.md section 4.7 is what is checked."""
from __future__ import annotations

import importlib.util
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops

ALEXNET_FILE = "alexnet-owt-7be5be79.pth"            # torchvision.models.alexnet(weights=IMAGENET1K_V1)
LIN_FILE = "alex.pth"                                # lpips/weights/v0.1/alex.pth
WEIGHTS_ENV = "BEM_LPIPS_WEIGHTS"
PRETRAIN_DIR = "experiments/pretrained_models"       # relative to the working directory, where the VGG19 file of the perceptual loss goes too
# (index in torchvision's ``alexnet().features``, Cin, Cout, kernel, stride, pad); a feature is taken after the ReLU of each
ALEX_CONVS = ((0, 3, 64, 11, 4, 2), (3, 64, 192, 5, 1, 2), (6, 192, 384, 3, 1, 1), (8, 384, 256, 3, 1, 1), (10, 256, 256, 3, 1, 1))
MIN_HW = ops.LPIPS_MIN_HW


def _missing(where):
    return FileNotFoundError(f"LPIPS weights not found {where}: both {ALEXNET_FILE} (torchvision's AlexNet) and {LIN_FILE} (weights/v0.1/{LIN_FILE} of "
                             f"the lpips package) are needed; put them in one directory and pass it as weights_dir / --lpips_weights, or point "
                             f"the environment variable {WEIGHTS_ENV} at it, or put them in {PRETRAIN_DIR}/ under the working directory; "
                             f"nothing is downloaded")


def find_weight_files(weights_dir=None):
    """(path of the AlexNet file, path of the lin file).  An explicit ``weights_dir`` or the environment variable is binding; otherwise
    experiments/pretrained_models/, then an installed lpips package (located, not imported) and torch's hub checkpoint directory."""
    for d, where in ((weights_dir, f"in '{weights_dir}'"), (os.environ.get(WEIGHTS_ENV), f"in '{os.environ.get(WEIGHTS_ENV)}' ({WEIGHTS_ENV})")):
        if d:
            a, l = os.path.join(d, ALEXNET_FILE), os.path.join(d, LIN_FILE)
            if os.path.isfile(a) and os.path.isfile(l):
                return a, l
            raise _missing(where)
    a, l = os.path.join(PRETRAIN_DIR, ALEXNET_FILE), os.path.join(PRETRAIN_DIR, LIN_FILE)
    if os.path.isfile(a) and os.path.isfile(l):
        return a, l
    a = l = None
    try:
        spec = importlib.util.find_spec("lpips")
    except (ImportError, ValueError):
        spec = None
    if spec is not None and spec.origin:
        l = os.path.join(os.path.dirname(spec.origin), "weights", "v0.1", LIN_FILE)
    a = os.path.join(torch.hub.get_dir(), "checkpoints", ALEXNET_FILE)
    if l and os.path.isfile(l) and os.path.isfile(a):
        return a, l
    raise _missing(f"in {PRETRAIN_DIR}/, an installed lpips package or torch's hub checkpoints")


def check_state_dicts(sd, lin_sd):
    """Every key and shape the metric reads; extra keys (the classifier's) are ignored."""
    for idx, cin, cout, k, _, _ in ALEX_CONVS:
        for kind, want in (("weight", (cout, cin, k, k)), ("bias", (cout,))):
            key = f"features.{idx}.{kind}"
            if key not in sd:
                raise KeyError(f"AlexNet state dict ({ALEXNET_FILE}) has no '{key}'")
            if tuple(sd[key].shape) != want:
                raise ValueError(f"AlexNet state dict ({ALEXNET_FILE}): '{key}' has shape {tuple(sd[key].shape)}, expected {want}")
    for i, (_, _, cout, _, _, _) in enumerate(ALEX_CONVS):
        key = f"lin{i}.model.1.weight"
        if key not in lin_sd:
            raise KeyError(f"LPIPS linear-layer state dict ({LIN_FILE}) has no '{key}'")
        if tuple(lin_sd[key].shape) != (1, cout, 1, 1):
            raise ValueError(f"LPIPS linear-layer state dict ({LIN_FILE}): '{key}' has shape {tuple(lin_sd[key].shape)}, expected {(1, cout, 1, 1)}")


def im2tensor(image, imtype=np.uint8, cent=1., factor=255. / 2.):
    """lpips.im2tensor: uint8 (H,W,3) -> float32 (1,3,H,W) in [-1,1]."""
    return torch.Tensor((image / factor - cent)[:, :, :, np.newaxis].transpose((3, 2, 0, 1)))


def conv1_block_weight(w):
    """(64,3,11,11) -> (64,48,3,3): zero-padded to 12x12 and cut into 4x4 blocks, channel 16 c + 4 dy + dx, the layout ops.lpips_prep writes."""
    co, ci = w.shape[:2]
    wp = torch.zeros(co, ci, 12, 12, device=w.device, dtype=w.dtype)
    wp[:, :, :11, :11] = w
    return wp.view(co, ci, 3, 4, 3, 4).permute(0, 1, 3, 5, 2, 4).reshape(co, ci * 16, 3, 3).contiguous()


class LPIPS(nn.Module):
    """``LPIPS(net='alex')`` of the lpips package, spatial=False, eval mode.  ``weights_dir`` / ``state_dict`` + ``lin_state_dict`` are not the
    package's keywords: the directory holding the two files, or the two state dicts handed over directly."""

    def __init__(self, net="alex", version="0.1", verbose=False, weights_dir=None, state_dict=None, lin_state_dict=None):
        super().__init__()
        if net != "alex":
            raise NotImplementedError(f"LPIPS: net '{net}' is not on the HIP path (alex only, as the evaluation scripts build it)")
        if version != "0.1":
            raise NotImplementedError(f"LPIPS: version '{version}' is not on the HIP path (0.1 only)")
        if (state_dict is None) != (lin_state_dict is None):
            raise ValueError("LPIPS: state_dict and lin_state_dict go together")
        if state_dict is None:
            a, l = find_weight_files(weights_dir)
            state_dict = torch.load(a, map_location="cpu", weights_only=True)
            lin_state_dict = torch.load(l, map_location="cpu", weights_only=True)
            if verbose:
                print(f"LPIPS: AlexNet from {a}, linear layers from {l}")
        check_state_dicts(state_dict, lin_state_dict)
        for i, (idx, *_rest) in enumerate(ALEX_CONVS):
            for kind in ("weight", "bias"):
                self.register_buffer(f"conv{i}_{kind}", state_dict[f"features.{idx}.{kind}"].detach().to(torch.float32).contiguous().clone(),
                                     persistent=False)
            self.register_buffer(f"lin{i}", lin_state_dict[f"lin{i}.model.1.weight"].detach().to(torch.float32).reshape(-1).contiguous().clone(),
                                 persistent=False)
        self._ops = None
        self.eval()

    def _apply(self, fn, *a, **k):
        self._ops = None                   # the operand forms below belong to the buffers they were packed from
        return super()._apply(fn, *a, **k)

    def conv_operands(self):
        """[(ConvWeight, bias, pad)] per convolution, conv1 in its block form; packed on first use and held for the life of the module (the
        weights are frozen, so nothing invalidates a packed form).  The input gradient of a convolution is ops.conv2d(d, its ConvWeight's
        input_grad(), None, pad=its pad); conv1's comes from its block form ((64,48,3,3) -> (48,64,3,3))."""
        if self._ops is None:
            with torch.no_grad():
                self._ops = [(ops.ConvWeight(conv1_block_weight(self.conv0_weight) if i == 0 else getattr(self, f"conv{i}_weight")),
                              getattr(self, f"conv{i}_bias"), 1 if i == 0 else c[5]) for i, c in enumerate(ALEX_CONVS)]
        return self._ops

    def features(self, xs, H, W):
        """The five ReLU outputs for the block-form input of ops.lpips_prep; the first is a crop of conv1's block grid (a view, not a copy)."""
        cw = self.conv_operands()
        Ho, Wo = ops.lpips_conv1_hw(H, W)
        ys = [ops.conv2d(xs, cw[0][0], cw[0][1], pad=1, relu=True)[:, :, 1:1 + Ho, 1:1 + Wo]]
        ys.append(ops.conv2d(ops.maxpool3s2(ys[0]), cw[1][0], cw[1][1], pad=2, relu=True))
        ys.append(ops.conv2d(ops.maxpool3s2(ys[1]), cw[2][0], cw[2][1], pad=1, relu=True))
        ys.append(ops.conv2d(ys[2], cw[3][0], cw[3][1], pad=1, relu=True))
        ys.append(ops.conv2d(ys[3], cw[4][0], cw[4][1], pad=1, relu=True))
        return ys

    def _distance(self, ref, pred, quantise, normalize):
        if ref.dim() != 4 or ref.shape[1] != 3 or ref.shape != pred.shape:
            raise ValueError(f"LPIPS: two (B,3,H,W) tensors of one shape required, got {tuple(ref.shape)} and {tuple(pred.shape)}")
        H, W = ref.shape[2:]
        if H < MIN_HW or W < MIN_HW:
            raise ValueError(f"LPIPS: images of at least {MIN_HW} x {MIN_HW} required (AlexNet's second pool has no output below that), got {H} x {W}")
        with torch.no_grad():
            xs = ops.lpips_prep(ref.contiguous(), pred.contiguous(), quantise=quantise, normalize=normalize)
            out = ws = None
            for i, y in enumerate(self.features(xs, H, W)):
                out, ws = ops.lpips_layer(y, getattr(self, f"lin{i}"), ws=ws, out=out, first=i == 0)
        return out

    def forward(self, in0, in1, retPerLayer=False, normalize=False):
        """in0, in1 (B,3,H,W) in [-1,1], or in [0,1] with ``normalize`` -> (B,1,1,1)."""
        if retPerLayer:
            raise NotImplementedError("LPIPS: retPerLayer is not on the HIP path")
        return self._distance(in0, in1, False, normalize).view(-1, 1, 1, 1)

    def distance01(self, ref01, pred01):
        """loss_fn.forward(im2tensor(img_as_ubyte(ref)), im2tensor(img_as_ubyte(pred))) for float images in [0,1], the quantisation fused into
        the input kernel -> (B) on the device."""
        return self._distance(ref01, pred01, True, False)
