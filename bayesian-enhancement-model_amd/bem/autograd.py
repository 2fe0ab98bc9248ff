"""Training path of the Stage-II nets: ``torch.autograd.Function``s whose forward AND backward are sequences of hand-written
gfx950 kernels (bem.ops).  torch's autograd engine only walks the graph; no gradient is computed by a torch op.

What is differentiated: ``DecompDualBranchDDWavelet.forward`` and its siblings
(basicsr/archs/DecompDualBranchDDWavelet_arch.py:301-369) as driven by ``ImageEnhancer.optimize_parameters``
(basicsr/models/image_enhancer_model.py:165-216): Hamilton product / IWT, dense 3x3 and 4x4-stride-2 convolutions,
ConvTranspose2d(2,2), 1x1 fuse layers and the 18 ``VSSBlock``s (vmamba.py:1319-1334: LayerNorm2d, Linear2d, depthwise 3x3 +
SiLU, the four-direction selective scan with x_proj / dt_proj -- the reference's CrossScanF / SelectiveScanCuda /
CrossMergeF backward, csm_triton.py:207-273, csms6s.py:95-113 -- and the gdMlp).

Parameter gradients are accumulated by the kernels straight into ``param.grad`` (allocated zero-filled on first use, or a view
of the flat buffer of ``bem.train.FlatParams``); the Functions return ``None`` for parameter inputs.  Use ``loss.backward()``
(as the reference's training step does) -- ``torch.autograd.grad`` with respect to parameters is not supported.
"""
from __future__ import annotations

import torch
from torch.autograd import Function

from . import ops
from .native import BemNativeError


def grad_of(p):
    """The buffer the kernels accumulate this parameter's gradient into; None for an absent parameter (a layer without a bias)."""
    if p is None:
        return None
    if p.grad is None:
        p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
    elif not p.grad.is_contiguous():
        raise RuntimeError("bem.autograd: parameter .grad must be contiguous")
    return p.grad


def _pack(holder, key, srcs, make):
    """pack_pw_weight of ``make()`` (an (M,K) matrix), cached on ``holder``."""
    return ops.derived(holder).get(key, srcs, lambda: ops.pack_pw_weight(make()))


def _w2d(w):
    return w.detach().reshape(w.shape[0], -1)


def _packT(layer, w):
    """The transposed weight of a 1x1 layer as GEMM operand (its input-gradient GEMM), cached on the layer under "T"."""
    return _pack(layer, "T", [w], lambda: _w2d(w).t())


def _det(t):
    return None if t is None else t.detach()


def wb(m):
    """(weight, bias | None) tensors of a leaf: nn.Conv2d / nn.Linear parameters, or -- for a Bayesian leaf in a training forward -- the
    weights it sampled for this forward (``m.sample``, a bayes.Sample); their .grad is the buffer the reparameterisation kernel
    later folds into mu / rho."""
    if hasattr(m, "mu_weight"):
        if m.deterministic:
            return m.mu_weight, (m.mu_bias if m.bias else None)
        if m.sample is None:
            raise RuntimeError("Bayesian leaf: no weight sample is active (training forwards run under Network.forward)")
        return m.sample.w, m.sample.b
    return m.weight, m.bias


def out_width(m):
    return m.out_features if hasattr(m, "out_features") else m.out_channels


def ln_pw(x, norm, layer, asked=None, **kw):
    """layer(LayerNorm2d(x)) for a 1x1 layer, the normalisation in the GEMM's prologue; ``kw`` goes to ops.pw_gemm (res, x2 / in_mode).
    ``asked``: the layer's ``gemm_weights`` where the caller has asked for them already.  A Bayesian leaf draws when it is asked, and
    its Philox streams follow the asking order in_proj, conv2d, out_proj, project_in, dwconv, project_out: a
    caller that needs another leaf's weights before this GEMM is launched asks both itself, in that order, and no leaf twice."""
    Wp, b = asked if asked is not None else layer.gemm_weights(x.shape[0])
    return ops.pw_gemm(x, Wp, out_width(layer), ln=(norm.weight.detach(), norm.bias.detach()), ln_eps=norm.eps, bias=b, **kw)


def _ln_pw_bwd(x, d, norm, layer, x2=None, dres=None):
    """Backward of ln_pw(x [+ x2], norm, layer) for the output gradient d: the layer's weight / bias and the norm's gradients are
    accumulated, the gradient of x (+ dres, a residual branch's) is returned."""
    w, b = wb(layer)
    dn = ops.pw_gemm(d, _packT(layer, w), x.shape[1])
    dx, nrm = ops.ln_bwd(x, dn, norm.weight.detach(), norm.bias.detach(), norm.eps, grad_of(norm.weight), grad_of(norm.bias), x2=x2, dres=dres)
    del dn
    ops.pw_wgrad_(d, nrm, grad_of(w), dbias=grad_of(b))
    return dx


def _dw_bwd(layer, t, d, mode):
    """Backward of the depthwise 3x3 + activation (mode 1: SiLU, 2: GELU gate) over t: the gradient of t; weight / bias gradients accumulated."""
    w, b = wb(layer)
    dpre = ops.dwact_bwd(t, w.detach(), _det(b), d, grad_of(w), grad_of(b), mode)
    return ops.dwconv3x3(dpre, ops.derived(layer).get("flip", [w], lambda: w.detach().flip(2, 3).contiguous()), None, mode=0)


# ------------------------------------------------------------------------------------------------------------------
# small nodes
# ------------------------------------------------------------------------------------------------------------------
class ForkFn(Function):
    """A tensor with two consumers: the two incoming gradients are summed by bem_add_f32 (not by the engine's own add)."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, g1, g2):
        if g1 is None:
            return g2
        if g2 is None:
            return g1
        return ops.add(g1.contiguous(), g2.contiguous())


def fork(x):
    return ForkFn.apply(x) if x.requires_grad else (x, x)


def fork_n(x, n):
    """x for n >= 1 consumers, as a list: a chain of n - 1 two-way forks, so every sum of incoming gradients is a bem_add_f32
    (g1 + (g2 + (g3 + ...))); one consumer gets x itself."""
    heads = []
    for _ in range(n - 1):
        h, x = fork(x)
        heads.append(h)
    return heads + [x]


class L1LossFn(Function):
    """basicsr/losses/losses.py L1Loss(loss_weight, reduction='mean')."""

    @staticmethod
    def forward(ctx, pred, gt, weight):
        pred, gt = pred.contiguous(), gt.contiguous()
        ctx.save_for_backward(pred, gt)
        ctx.weight = weight
        return ops.l1_loss(pred, gt, weight).reshape(())

    @staticmethod
    def backward(ctx, g):
        pred, gt = ctx.saved_tensors
        # g = dL/dloss as a device scalar (1.0 in the reference's step; an AMP scaler passes its scale): folded into the kernel
        return ops.l1_loss_bwd(pred, gt, ctx.weight, g.reshape(1).contiguous().float()), None, None


def l1_loss(pred, gt, weight=1.0):
    return L1LossFn.apply(pred, gt, float(weight))


class MSELossFn(Function):
    """basicsr/losses/basic_loss.py MSELoss(loss_weight, reduction='mean'); only pred takes a gradient."""

    @staticmethod
    def forward(ctx, pred, gt, weight):
        pred, gt = pred.contiguous(), gt.contiguous()
        ctx.save_for_backward(pred, gt)
        ctx.weight = weight
        return ops.mse_loss(pred, gt, weight).reshape(())

    @staticmethod
    def backward(ctx, g):
        pred, gt = ctx.saved_tensors
        return ops.mse_loss_bwd(pred, gt, ctx.weight, g.reshape(1).contiguous().float()), None, None


def mse_loss(pred, gt, weight=1.0):
    return MSELossFn.apply(pred, gt, float(weight))


class CharbonnierLossFn(Function):
    """basicsr/losses/basic_loss.py CharbonnierLoss(loss_weight, reduction='mean', eps); only pred takes a gradient."""

    @staticmethod
    def forward(ctx, pred, gt, weight, eps):
        pred, gt = pred.contiguous(), gt.contiguous()
        ctx.save_for_backward(pred, gt)
        ctx.weight, ctx.eps = weight, eps
        return ops.charbonnier_loss(pred, gt, weight, eps).reshape(())

    @staticmethod
    def backward(ctx, g):
        pred, gt = ctx.saved_tensors
        return ops.charbonnier_loss_bwd(pred, gt, ctx.weight, ctx.eps, g.reshape(1).contiguous().float()), None, None, None


def charbonnier_loss(pred, gt, weight=1.0, eps=1e-12):
    return CharbonnierLossFn.apply(pred, gt, float(weight), float(eps))


class SSIMLossFn(Function):
    """basicsr/losses/my_loss.py:37-38: weight * (1 - ssim(pred, gt)), 11x11 Gaussian window, data range 1.  The forward launch writes the
    three coefficient maps of the backward when pred wants a gradient; gt takes none."""

    @staticmethod
    def forward(ctx, pred, gt, weight):
        pred, gt = pred.contiguous(), gt.contiguous()
        ctx.weight = weight
        if not ctx.needs_input_grad[0]:
            return ops.ssim_loss(pred, gt, weight).reshape(())
        loss, coef = ops.ssim_loss(pred, gt, weight, want_grad=True)
        ctx.save_for_backward(pred, gt, coef)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        pred, gt, coef = ctx.saved_tensors
        return ops.ssim_loss_bwd(pred, gt, coef, ctx.weight, g.reshape(1).contiguous().float()), None, None


def ssim_loss(pred, gt, weight=1.0):
    return SSIMLossFn.apply(pred, gt, float(weight))


class PixStatLossFn(Function):
    """The per-pixel statistics of basicsr/losses/my_loss.py:51-74 (csrc/pixstat_loss.hip): a1 smooth_l1 + a3 hist + a5 psnr + a6 color
    as a 0-d loss; the (6,) device tensor ops.PIXSTAT_VALUES (the loss and the five unweighted values) is appended to ``values`` for the log.  The
    forward's second launch writes the backward's record when pred wants a gradient; gt takes none, and neither does the histogram term:
    with a1 = a5 = a6 = 0 the gradient is zero and no kernel is launched for it."""

    @staticmethod
    def forward(ctx, pred, gt, alphas, values):
        pred, gt = pred.contiguous(), gt.contiguous()
        ctx.has_grad = any(alphas[i] != 0 for i in (0, 2, 3))
        if ctx.needs_input_grad[0] and ctx.has_grad:
            vals, rec = ops.pixstat_loss(pred, gt, alphas, want_grad=True)
            ctx.save_for_backward(pred, gt, rec)
        else:
            vals = ops.pixstat_loss(pred, gt, alphas)
            if ctx.needs_input_grad[0]:
                ctx.save_for_backward(pred)                    # its shape, for the zero gradient
        values.append(vals)
        return vals[:1].reshape(())

    @staticmethod
    def backward(ctx, g):
        if not ctx.has_grad:
            return torch.zeros_like(ctx.saved_tensors[0]), None, None, None
        pred, gt, rec = ctx.saved_tensors
        return ops.pixstat_loss_bwd(pred, gt, rec, g.reshape(1).contiguous().float()), None, None, None


def pixstat_loss(pred, gt, alphas):
    """(loss, values) of PixStatLossFn; ``alphas`` = (a1, a3, a5, a6), values = the (6,) tensor of ops.PIXSTAT_VALUES."""
    values = []
    loss = PixStatLossFn.apply(pred, gt, tuple(float(a) for a in alphas), values)
    return loss, values[0]


# ------------------------------------------------------------------------------------------------------------------
# VGG19 perceptual loss (basic_loss.py:198-222 over vgg_arch.py:141-161)
# ------------------------------------------------------------------------------------------------------------------
def _vgg_walk(vgg, x, keep=None, rows=None):
    """The conv / ReLU / pool walk of ``vgg.names`` over the normalised batch x (N,8,H,W).  Returns {requested name: feature}; ``keep``
    (a dict) receives the first ``rows`` batch rows of the post-ReLU output of every convolution whose ReLU is part of the walk, copied
    out as soon as it exists (a view where the whole tensor is a requested relu* feature and stays alive anyway), so that the N-row
    tensor itself is released once the next layer has read it.  A convolution carries its ReLU in its epilogue unless its own value is
    requested: then the value before the ReLU is the feature and bem_relu_f32 continues the walk."""
    names, want, w = vgg.names, set(vgg.layer_name_list), vgg.conv_operands()
    feats = {}
    for i, n in enumerate(names):
        if n.startswith("conv"):
            cw, bias = w[n]
            has_relu = i + 1 < len(names)
            if n in want:
                feats[n] = pre = ops.conv2d(x, cw, bias, relu=False)
                x = ops.relu(pre) if has_relu else pre
            else:
                x = ops.conv2d(x, cw, bias, relu=True)
            if has_relu and keep is not None:
                keep[n] = x[:rows] if names[i + 1] in want else _rows(x, rows)
        elif n.startswith("relu"):
            if n in want:
                feats[n] = x
        else:
            x = ops.maxpool2(x)
    return feats


def vgg_features(vgg, x):
    """VGGFeatureExtractor.forward for one image batch (no gradient): {name: feature}."""
    B = x.shape[0]
    return _vgg_walk(vgg, ops.vgg_prep(x, x, vgg.use_input_norm, vgg.range_norm)[:B])


class PerceptualFn(Function):
    """percep_loss of PerceptualLoss.forward(pred, gt), criterion l1 or l2.  Forward: both images as one 2B-row batch through the walk, one
    bem_l1_loss_f32 (l2: bem_mse_loss_f32) per requested layer between the two halves, the values summed on the device.  Backward: the pred half only, against
    the frozen weights: no weight gradient, none for gt.  Saved: the post-ReLU activations of the pred rows (ReLU masks, pool argmax)
    and the requested features."""

    @staticmethod
    def forward(ctx, pred, gt, mod):
        vgg = mod.vgg
        pred, gt = pred.contiguous(), gt.contiguous()
        B = pred.shape[0]
        need_bwd = ctx.needs_input_grad[0]
        keep = {} if need_bwd else None
        feats = _vgg_walk(vgg, ops.vgg_prep(pred, gt, vgg.use_input_norm, vgg.range_norm), keep, B)
        total = None
        crit = ops.mse_loss if mod.criterion_type == "l2" else ops.l1_loss
        for n, f in feats.items():
            l = crit(f[:B], f[B:], float(mod.layer_weights[n]) * float(mod.perceptual_weight))
            total = l if total is None else ops.add(total, l)
        if need_bwd:
            ctx.mod, ctx.B = mod, B
            ctx.feat_names, ctx.act_names = list(feats), list(keep)
            ctx.save_for_backward(*feats.values(), *keep.values())
        return total.reshape(())

    @staticmethod
    def backward(ctx, g):
        mod, B = ctx.mod, ctx.B
        vgg = mod.vgg
        names, w = vgg.names, vgg.conv_operands()
        nf = len(ctx.feat_names)
        feats = dict(zip(ctx.feat_names, ctx.saved_tensors[:nf]))
        acts = dict(zip(ctx.act_names, ctx.saved_tensors[nf:]))
        gmul = g.reshape(1).contiguous().float()

        crit_bwd = ops.mse_loss_bwd if mod.criterion_type == "l2" else ops.l1_loss_bwd

        def dfeat(n):
            f = feats[n]
            return crit_bwd(f[:B], f[B:], float(mod.layer_weights[n]) * float(mod.perceptual_weight), gmul)

        d, masked = None, False          # d: gradient at the output of layer i; masked: the mask of the ReLU it leaves is already in it
        for i in range(len(names) - 1, -1, -1):
            n = names[i]
            if n.startswith("pool"):
                d, masked = ops.relu_pool_bwd(acts["conv" + names[i - 1][4:]], d), True
            elif n.startswith("relu"):
                if n in feats:
                    gf = dfeat(n)
                    if d is None:
                        d, masked = gf, False
                    elif masked:
                        d = ops.add(d, ops.relu_bwd(acts["conv" + n[4:]], gf, inplace=True))
                    else:
                        d = ops.add(d, gf)
            else:
                if d is not None and not masked:
                    d = ops.relu_bwd(acts[n], d, inplace=True)       # d is this node's own tensor
                if n in feats:
                    gf = dfeat(n)
                    d = gf if d is None else ops.add(d, gf)
                d, masked = ops.conv2d(d, w[n][0].input_grad(), None), False
        return ops.vgg_prep_bwd(d, B, vgg.use_input_norm, vgg.range_norm), None, None


def _rows(t, B):
    """The first B batch rows of a contiguous (N,C,H,W) tensor as a tensor of their own (bem_copy_channels_f32)."""
    out = torch.empty((B,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
    ops.copy_channels(t[:B], out, 0)
    return out


def perceptual_loss(pred, gt, mod):
    return PerceptualFn.apply(pred, gt.detach(), mod)          # basic_loss.py:210


# ------------------------------------------------------------------------------------------------------------------
# LPIPS (v0.1, AlexNet) as a loss term
# ------------------------------------------------------------------------------------------------------------------
class LPIPSFn(Function):
    """mod.loss_weight * mean_b d(gt_b, pred_b), d the distance of ``mod.lpips`` (a bem.lpips.LPIPS) on unquantised inputs: in [0,1] with
    ``mod.normalize``, in [-1,1] without.  Forward: the launches of LPIPS.forward and one bem_lpips_mean_f32.  Backward: the pred rows only,
    against the frozen weights -- per layer from the top the head backward (which adds the gradient from the layer above and applies
    the ReLU mask) and the convolution's input gradient, a pool backward before layers 1 and 0, the input stage's adjoint last; none
    for gt.  Saved: the five 2B-row features (the head backward needs the reference rows too)."""

    @staticmethod
    def forward(ctx, pred, gt, mod):
        net = mod.lpips
        pred, gt = pred.contiguous(), gt.contiguous()
        if pred.dim() != 4 or pred.shape[1] != 3 or pred.shape != gt.shape:
            raise ValueError(f"lpips_loss: two (B,3,H,W) tensors of one shape required, got {tuple(pred.shape)} and {tuple(gt.shape)}")
        B, _, H, W = pred.shape
        ys = net.features(ops.lpips_prep(gt, pred, quantise=False, normalize=mod.normalize), H, W)
        out = ws = None
        for i, y in enumerate(ys):
            out, ws = ops.lpips_layer(y, getattr(net, f"lin{i}"), ws=ws, out=out, first=i == 0)
        if ctx.needs_input_grad[0]:
            ctx.mod, ctx.hw = mod, (H, W)
            ctx.save_for_backward(*ys)
        return ops.lpips_mean(ws, B, float(mod.loss_weight)).reshape(())

    @staticmethod
    def backward(ctx, g):
        mod, (H, W), ys = ctx.mod, ctx.hw, ctx.saved_tensors
        net, B = mod.lpips, ys[0].shape[0] // 2
        cw = net.conv_operands()
        gmul, scale = g.reshape(1).contiguous().float(), float(mod.loss_weight) / B
        gin = None
        for i in (4, 3, 2, 1):
            d = ops.lpips_layer_bwd(ys[i], getattr(net, f"lin{i}"), gin, gmul, scale)
            gin = ops.conv2d(d, cw[i][0].input_grad(), None, pad=cw[i][2])
            if i <= 2:                                               # conv2 and conv3 read a pooled feature
                gin = ops.relu_pool3s2_bwd(ys[i - 1][B:], gin)
        # layer 0 is a crop of conv1's block grid: its gradient goes back into the whole grid, zero around the crop
        Ho, Wo = ops.lpips_conv1_hw(H, W)
        d = torch.empty(B, ys[0].shape[1], Ho + 2, (Wo + 3) // 2 * 2, device=gin.device, dtype=torch.float32)
        ops.lpips_layer_bwd(ys[0], net.lin0, gin, gmul, scale, out=d, origin=(1, 1))
        return ops.lpips_prep_bwd(ops.conv2d(d, cw[0][0].input_grad(), None, pad=cw[0][2]), H, W, normalize=mod.normalize), None, None


def lpips_loss(pred, gt, mod):
    return LPIPSFn.apply(pred, gt.detach(), mod)


class IwtHamiltonFn(Function):
    @staticmethod
    def forward(ctx, q1w, q2w):
        q1w, q2w = q1w.contiguous(), q2w.contiguous()
        ctx.save_for_backward(q1w, q2w)
        return ops.iwt_hamilton(q1w, q2w)

    @staticmethod
    def backward(ctx, dout):
        q1w, q2w = ctx.saved_tensors
        return ops.iwt_hamilton_bwd(q1w, q2w, dout.contiguous())


# ------------------------------------------------------------------------------------------------------------------
# 1x1 layers without a LayerNorm prologue (fuse, bottleneck_fuse, bottleneck_to_Q*)
# ------------------------------------------------------------------------------------------------------------------
class PwFn(Function):
    @staticmethod
    def forward(ctx, x1, x2, weight, bias, holder):
        x1 = x1.contiguous()
        M = weight.shape[0]
        Wp, _ = holder.gemm_weights(x1.shape[0])
        if x2 is not None:
            x2 = x2.contiguous()
            out = ops.pw_gemm(x1, Wp, M, x2=x2, in_mode=2, bias=_det(bias))
        else:
            out = ops.pw_gemm(x1, Wp, M, bias=_det(bias))
        ctx.save_for_backward(x1, x2)
        ctx.holder, ctx.weight, ctx.bias = holder, weight, bias
        return out

    @staticmethod
    def backward(ctx, dout):
        x1, x2 = ctx.saved_tensors
        dout = dout.contiguous()
        w, b, h = ctx.weight, ctx.bias, ctx.holder
        C1 = x1.shape[1]
        ops.pw_wgrad_(dout, x1, grad_of(w), x2=x2, dbias=grad_of(b))
        w2 = _w2d(w)
        dx1 = dx2 = None
        if ctx.needs_input_grad[0]:
            dx1 = ops.pw_gemm(dout, _pack(h, "T1", [w], lambda: w2[:, :C1].t()), C1)
        if x2 is not None and ctx.needs_input_grad[1]:
            C2 = x2.shape[1]
            dx2 = ops.pw_gemm(dout, _pack(h, "T2", [w], lambda: w2[:, C1:].t()), C2)
        return dx1, dx2, None, None, None


class ConvT2x2Fn(Function):
    """nn.ConvTranspose2d(C, C/2, 2, 2): forward = 1x1 GEMM to 4*Co rows + 2x2 scatter (modules.ConvT2x2)."""

    @staticmethod
    def forward(ctx, x, weight, bias, holder):
        x = x.contiguous()
        ctx.save_for_backward(x)
        ctx.holder, ctx.weight, ctx.bias = holder, weight, bias
        return holder._forward_nograd(x)

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        w, b, h = ctx.weight, ctx.bias, ctx.holder
        Cin, Co = w.shape[0], w.shape[1]
        dy4 = ops.pixel_unshuffle2(dout.contiguous())                 # (B, 4 Co, H, W), channel = co*4 + dy*2 + dx
        ops.pw_wgrad_(x, dy4, grad_of(w))                            # (Cin, Co*4) = weight.grad's own layout
        ops.channel_sum_(dout, grad_of(b))
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.pw_gemm(dy4, _pack(h, "T", [w], lambda: w.detach().reshape(Cin, 4 * Co)), Cin)
        return dx, None, None, None


# ------------------------------------------------------------------------------------------------------------------
# dense convolutions (3x3 stride 1 pad 1; 4x4 stride 2 pad 1)
# ------------------------------------------------------------------------------------------------------------------
def _wT4(w):
    """Input gradient of the 4x4 stride-2 pad-1 convolution as a 3x3 convolution over dout producing 4*Cin phase channels
    (PixelShuffle order ci*4 + py*2 + px), then pixel_shuffle2."""
    w = w.detach()
    Co, Ci = w.shape[0], w.shape[1]
    w3 = torch.zeros(Ci, 2, 2, Co, 3, 3, device=w.device, dtype=w.dtype)
    taps = {0: ((0, 1), (-1, 3)), 1: ((1, 0), (0, 2))}                 # phase -> ((offset, kernel index), ...)
    for py in (0, 1):
        for di, ky in taps[py]:
            for px in (0, 1):
                for dj, kx in taps[px]:
                    w3[:, py, px, :, di + 1, dj + 1] = w[:, :, ky, kx].t()
    return w3.reshape(Ci * 4, Co, 3, 3).contiguous()


class Conv2dFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, holder, cin_slice):
        if holder.dilation[0] != 1:
            raise BemNativeError("Conv2dFn: the training path covers undilated convolutions only (the dilated QD model2 layers are frozen)")
        x = x.contiguous()
        ctx.save_for_backward(x)
        ctx.holder, ctx.weight, ctx.bias, ctx.cin_slice = holder, weight, bias, cin_slice
        return ops.conv2d(x, holder.conv_weight(), _det(bias), stride=holder.stride[0], pad=holder.padding[0],
                          cin_slice=cin_slice)

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        w, b, h = ctx.weight, ctx.bias, ctx.holder
        dout = dout.contiguous()
        s, p = h.stride[0], h.padding[0]
        ops.conv_wgrad_(dout, x, grad_of(w), grad_of(b), stride=s, pad=p, cin_slice=ctx.cin_slice)
        dx = None
        if ctx.needs_input_grad[0]:
            if ctx.cin_slice is not None:
                raise NotImplementedError("Conv2dFn: input gradient of a channel-sliced input")
            k = tuple(w.shape[2:])
            if (k, s, p) == ((3, 3), 1, 1):
                dx = ops.conv2d(dout, h.conv_weight().input_grad(), None, stride=1, pad=1)     # correlation with the flipped kernel
            elif (k, s, p) == ((4, 4), 2, 1):
                d4 = ops.conv2d(dout, ops.derived(h).get("T4", [w], lambda: ops.ConvWeight(_wT4(w))), None, stride=1, pad=1)
                dx = ops.pixel_shuffle2(d4)
            else:
                raise NotImplementedError(f"Conv2dFn: input gradient for kernel {k} stride {s} pad {p}")
        return dx, None, None, None, None


# ------------------------------------------------------------------------------------------------------------------
# VSSBlock (vmamba.py:1319-1334) as one node
# ------------------------------------------------------------------------------------------------------------------
class VSSBlockFn(Function):
    @staticmethod
    def forward(ctx, x, blk, *params):
        x = x.contiguous()
        x2, (t, xc, xd, xd1, y0, y1) = blk.op.forward_fused(x, blk.norm, keep=True)
        out, t2, g = blk.mlp.chain(x2, blk.norm2)
        ctx.blk = blk
        ctx.save_for_backward(x, t, xc, xd, xd1, y0, y1, x2, t2, g)
        return out

    @staticmethod
    def backward(ctx, dout):
        blk = ctx.blk
        x, t, xc, xd, xd1, y0, y1, x2, t2, g = ctx.saved_tensors
        dout = dout.contiguous()
        op, mlp = blk.op, blk.mlp
        B, C, H, W = x.shape
        Ci, R, L = op.d_inner, op.dt_rank, H * W
        # ---- gdMlp: out = x2 + W_o g + b_o, g = GELU(h1) h2, h = dw(t2) + b, t2 = W_i LN2(x2) + b_i
        pow_, pob = wb(mlp.project_out)
        ops.pw_wgrad_(dout, g, grad_of(pow_), dbias=grad_of(pob))
        dt2 = _dw_bwd(mlp.dwconv, t2, ops.pw_gemm(dout, _packT(mlp.project_out, pow_), pow_.shape[1]), 2)
        dx2 = _ln_pw_bwd(x2, dt2, blk.norm2, mlp.project_in, dres=dout)
        del dt2
        # ---- SS2D: x2 = x + W_out LN_on(y0 + y1), (y0, y1) = scan(xc, x_proj xc), xc = SiLU(dw(t)), t = W_in LN(x)
        dys = _ln_pw_bwd(y0, dx2, op.out_norm, op.out_proj, x2=y1)
        wall, dtw, dtb, A, Ds, _ = op._scan_params()
        M = R + 2 * op.d_state                           # x_dbl rows per direction
        dysT = ops.transpose_planes(dys)
        xcT = ops.transpose_planes(xc)
        scan_bwd = ops.ss2d_scan_n_bwd if op.d_state > 1 else ops.ss2d_scan_bwd
        dx0, dx1T, dxd0, dxd1 = scan_bwd(
            xc.view(B, Ci, L), xcT.view(B, Ci, L), xd.view(B, 4, M, L)[:, :2], xd1.view(B, 2, M, L), dys.view(B, Ci, L), dysT.view(B, Ci, L),
            dtw, dtb, A, Ds, grad_of(op.A_logs), grad_of(op.Ds), grad_of(op.dt_projs_weight), grad_of(op.dt_projs_bias))
        del dysT, xcT, dys
        # x_dbl gradient back in the stacked row order of the forward GEMM: [dir 0 | dir 2 | dir 1 | dir 3], row-major pixels
        dxd = torch.empty(B, 4 * M, H, W, device=x.device, dtype=x.dtype)
        ops.copy_channels(dxd0.view(B, 2 * M, H, W), dxd, 0)
        ops.transpose_planes_into(dxd1.view(B, 2 * M, W, H), dxd, 2 * M)
        ops.pw_wgrad_(dxd, xc, grad_of(op.x_proj_weight), blk_rows=M, perm=(0, 2, 1, 3))
        xw = op.x_proj_weight
        wallT = _pack(op, "wallT", [xw], lambda: torch.cat([xw.detach()[0], xw.detach()[2], xw.detach()[1], xw.detach()[3]], 0).t())
        dxc = ops.pw_gemm(dxd, wallT, Ci, res=dx0.view(B, Ci, H, W))
        dxc = ops.add(dxc, ops.transpose_planes(dx1T.view(B, Ci, W, H)))
        del dx0, dx1T, dxd, dxd0, dxd1
        dt = _dw_bwd(op.conv2d, t, dxc, 1)
        del dxc
        dx = _ln_pw_bwd(x, dt, blk.norm, op.in_proj, dres=dx2)
        return (dx if ctx.needs_input_grad[0] else None, None) + (None,) * (len(ctx.needs_input_grad) - 2)


def vssblock_params(blk):
    return [p for p in blk.parameters() if p.requires_grad]


def vssblock(blk, x):
    return VSSBlockFn.apply(x, blk, *vssblock_params(blk))


# ------------------------------------------------------------------------------------------------------------------
# Stage-I U-Net pieces (basicsr/archs/UNet_arch.py): PatchMerging, DualUpSample, MIM token mix, outer residual
# ------------------------------------------------------------------------------------------------------------------
class AddFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        return ops.add(a.contiguous(), b.contiguous())

    @staticmethod
    def backward(ctx, g):
        return g, g


class LnPwFn(Function):
    """LayerNorm2d + bias-free / biased 1x1 layer (PatchMerging.reduction(norm(x)), UNet_arch.py:80)."""

    @staticmethod
    def forward(ctx, x, norm, layer, *params):
        x = x.contiguous()
        ctx.save_for_backward(x)
        ctx.norm, ctx.layer = norm, layer
        return ln_pw(x, norm, layer)

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        dx = _ln_pw_bwd(x, dout.contiguous(), ctx.norm, ctx.layer)
        return (dx if ctx.needs_input_grad[0] else None, None, None) + (None,) * (len(ctx.needs_input_grad) - 3)


class SpaceToDepthFn(Function):
    @staticmethod
    def forward(ctx, x):
        return ops.space_to_depth(x.contiguous())

    @staticmethod
    def backward(ctx, g):
        return ops.depth_to_space(g.contiguous())


class PixelShuffle2Fn(Function):
    @staticmethod
    def forward(ctx, x):
        return ops.pixel_shuffle2(x.contiguous())

    @staticmethod
    def backward(ctx, g):
        return ops.pixel_unshuffle2(g.contiguous())


class BilinearUpFn(Function):
    @staticmethod
    def forward(ctx, x, s):
        ctx.s = s
        return ops.bilinear_up(x.contiguous(), s)

    @staticmethod
    def backward(ctx, g):
        return ops.bilinear_up_bwd(g.contiguous(), ctx.s), None


class PReLUFn(Function):
    @staticmethod
    def forward(ctx, x, slope):
        x = x.contiguous()
        ctx.save_for_backward(x)
        ctx.slope = slope
        return ops.prelu(x, slope.detach())

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.prelu_bwd(x, ctx.slope.detach(), g.contiguous(), grad_of(ctx.slope)), None


class MaskTokenFn(Function):
    """fea * (1 - w) + mask_token * w  (UNet_arch.py:463-466)."""

    @staticmethod
    def forward(ctx, fea, mask, token):
        mask = mask.to(fea.dtype).contiguous()
        ctx.save_for_backward(mask)
        ctx.token = token
        return ops.mask_token(fea.contiguous(), mask, token.detach().reshape(-1).contiguous())

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return ops.mask_token_bwd(g.contiguous(), mask, grad_of(ctx.token).view(-1)), None, None


class ScaledSumFn(Function):
    """a + c * b for two device scalars (l_total = l_pix + 0.01 / mini_batch * l_kl, condition_generator_model.py:185-190)."""

    @staticmethod
    def forward(ctx, a, b, c):
        ctx.c = c
        return ops.add(a.reshape(1).contiguous(), b.reshape(1).contiguous(), c).reshape(())

    @staticmethod
    def backward(ctx, g):
        g1 = g.reshape(1).contiguous()
        return g, ops.add(torch.zeros_like(g1), g1, ctx.c).reshape(()), None


# ------------------------------------------------------------------------------------------------------------------
# DecompDualBranch's bottleneck blocks in training (basicsr/archs/DecompModel_arch.py:57-99)
# ------------------------------------------------------------------------------------------------------------------
class GateAddFn(Function):
    """x_tgt + gate * t  (CrossFusionBlock after its 1x1 transform, :62-66): dt = gate dy, dx_tgt = dy, dgate[c] += sum dy t."""

    @staticmethod
    def forward(ctx, t, gate, x_tgt):
        t, x_tgt = t.contiguous(), x_tgt.contiguous()
        ctx.save_for_backward(t)
        ctx.gate = gate
        return ops.chan_scale(t, gate.detach().reshape(-1).contiguous(), add=x_tgt)

    @staticmethod
    def backward(ctx, dy):
        (t,) = ctx.saved_tensors
        dy = dy.contiguous()
        g = ctx.gate
        ops.chan_dot(dy, t, grad_of(g).view(-1))
        return ops.chan_scale(dy, g.detach().reshape(-1).contiguous()), None, dy


class SEBlockFn(Function):
    """x * sigmoid(W2 relu(W1 mean_hw(x)))  (SEBlock, :68-83)."""

    @staticmethod
    def forward(ctx, x, w1, w2):
        x = x.contiguous()
        y, mean = ops.se_gate(x, w1.detach(), w2.detach(), want_mean=True)
        ctx.save_for_backward(x, y, mean)
        ctx.w = (w1, w2)
        return ops.chan_scale(x, y)

    @staticmethod
    def backward(ctx, dout):
        x, y, mean = ctx.saved_tensors
        w1, w2 = ctx.w
        dout = dout.contiguous()
        dy = ops.chan_dot(dout, x)                                                     # (B,C): gradient of the gate
        dmean = ops.se_gate_bwd(mean, w1.detach(), w2.detach(), y, dy, grad_of(w1), grad_of(w2))
        return ops.chan_scale(dout, y, add_bc=dmean, add_bc_scale=1.0 / x[0, 0].numel()), None, None


class SpatialAttnFn(Function):
    """x * sigmoid(conv_kxk([mean_c x, max_c x]))  (SpatialAttention, :85-99)."""

    @staticmethod
    def forward(ctx, x, w):
        x = x.contiguous()
        out, amap = ops.spatial_attention(x, w.detach(), want_map=True)
        ctx.save_for_backward(x, amap)
        ctx.w = w
        return out

    @staticmethod
    def backward(ctx, dout):
        x, amap = ctx.saved_tensors
        w = ctx.w
        return ops.spatial_attention_bwd(x, dout.contiguous(), amap, w.detach(), grad_of(w)), None


class HamiltonFn(Function):
    """hamilton_product(p, q)[:, 1:] of two (B,4,H,W) maps at full resolution (DecompModel_arch.py:351-352)."""

    @staticmethod
    def forward(ctx, p, q):
        B, _, H, W = p.shape
        q8 = torch.empty(B, 8, H, W, device=p.device, dtype=p.dtype)
        ops.copy_channels(p.contiguous(), q8, 0)
        ops.copy_channels(q.contiguous(), q8, 4)
        ctx.save_for_backward(q8)
        return ops.hamilton(q8)

    @staticmethod
    def backward(ctx, dout):
        (q8,) = ctx.saved_tensors
        d = ops.hamilton_bwd(q8, dout.contiguous())
        B, _, H, W = q8.shape
        dp, dq = torch.empty(B, 4, H, W, device=d.device, dtype=d.dtype), torch.empty(B, 4, H, W, device=d.device, dtype=d.dtype)
        ops.copy_channels(d, dp, 0, src_c0=0, C=4)
        ops.copy_channels(d, dq, 0, src_c0=4, C=4)
        return dp, dq


class Hamilton8Fn(Function):
    """The same on one (B,8,H,W) tensor [p | q] (DecompSingleBranch_arch.py:229-231: the single U-Net's 8 output channels)."""

    @staticmethod
    def forward(ctx, q8):
        q8 = q8.contiguous()
        ctx.save_for_backward(q8)
        return ops.hamilton(q8)

    @staticmethod
    def backward(ctx, dout):
        (q8,) = ctx.saved_tensors
        return ops.hamilton_bwd(q8, dout.contiguous())


# ------------------------------------------------------------------------------------------------------------------
# Output heads of the two-branch archs without a decomposition (TunedModel_arch.py:315-319,406, TwoBranchNaive_arch.py:268)
# ------------------------------------------------------------------------------------------------------------------
class FusionHeadFn(Function):
    """fusion(cat(o1, o2)) = Conv2d(6,3,3) -> ReLU -> Conv2d(3,3,3) as one kernel.  Only the two inputs are saved: the backward
    recomputes the pre-activation."""

    @staticmethod
    def forward(ctx, o1, o2, w1, b1, w2, b2):
        o1, o2 = o1.contiguous(), o2.contiguous()
        ctx.save_for_backward(o1, o2)
        ctx.w = (w1, b1, w2, b2)
        return ops.fusion_head(o1, o2, w1.detach(), b1.detach(), w2.detach(), b2.detach())

    @staticmethod
    def backward(ctx, dout):
        o1, o2 = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.w
        do1, do2 = ops.fusion_head_bwd_(o1, o2, dout.contiguous(), w1.detach(), b1.detach(), w2.detach(), grad_of(w1), grad_of(b1),
                                        grad_of(w2), grad_of(b2))
        return do1, do2, None, None, None, None


class BranchMeanFn(Function):
    """(o1 + o2) / 2; both input gradients are dout / 2."""

    @staticmethod
    def forward(ctx, o1, o2):
        return ops.fusion_head(o1.contiguous(), o2.contiguous(), mean=True)

    @staticmethod
    def backward(ctx, dout):
        return ops.fusion_head_bwd_(None, None, dout.contiguous(), mean=True)
