"""Architectures of the hot path, mirroring the reference's constructors and state-dict keys:

  Network                     basicsr/archs/UNet_arch.py:364-474          (Stage-I, Bayesian after convert2bnn)
  DecompDualBranchDDWavelet   basicsr/archs/DecompDualBranchDDWavelet_arch.py:146-369
  DecompSingleBranch          basicsr/archs/DecompSingleBranch_arch.py:53-237
  Decomp (model1 / model4)    basicsr/QD/model1.py, model4.py:167-262 (+ the wavelet-domain MyDecomp :71-132)
  VMUNet                      basicsr/archs/VMUnet_arch.py:68-240
  NaiveVMUNetTwoBranch        basicsr/archs/TwoBranchNaive_arch.py:68-271
  TunedModel                  basicsr/archs/TunedModel_arch.py:162-406
  FusedTunedModel             basicsr/archs/FusedModel_arch.py:101-332

forward(x, mask=None) -> [x, out] like the reference.  All compute goes through bem.ops (HIP).
"""
from __future__ import annotations

import math
import os

import torch
import torch.nn as nn

from . import autograd as ag
from . import bayes
from . import ops
from .modules import Conv2dK, ConvT2x2, LayerNorm2d, PwConv2d, VSSBlock, _need_cuda, fold_up_fuse, grad_mode, make_vss_level
from .native import BemNativeError

_QD_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "basicsr", "QD", "checkpoints")


def _trunc_normal_(t, std=0.02):
    return nn.init.trunc_normal_(t, mean=0.0, std=std, a=-2.0, b=2.0)


def _init_weights(m):
    # UNet_arch.py:344-351 / DecompDualBranchDDWavelet_arch.py:264-271
    if isinstance(m, nn.Linear):
        _trunc_normal_(m.weight, std=0.02)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, nn.LayerNorm):
        nn.init.constant_(m.weight, 1.0)
        nn.init.constant_(m.bias, 0)


def conv_down(c):
    return Conv2dK(c, c * 2, 4, 2, 1, bias=False)


# ------------------------------------------------------------------------------------------------
# Quaternion-Retinex decomposition (frozen)
# ------------------------------------------------------------------------------------------------
class _CrossAttnParams(nn.Module):
    """SymmetricCrossAttention (QD/model4.py:81-139) parameter holder; evaluated folded (bem_attn_fold).  ``p``: the probability of its
    attn_drop (QD/model3.py:98: 0.1; model2 builds it with 0.0, model1 / model4 have none), live in train() mode only."""

    def __init__(self, dim, p=0.0):
        super().__init__()
        self.p = float(p)
        for n in ("q1_proj", "k2_proj", "v2_proj", "q2_proj", "k1_proj", "v1_proj", "out1", "out2"):
            setattr(self, n, nn.Conv2d(dim, dim, 1))


def attn_drop_stream_id(rank, iteration, call=0):
    """Philox stream id of one decomposition call's attention-dropout draw, in a key space of its own:
    bit 61 | rank : 16 bits at bit 44 | iteration : 36 bits at bit 8 | call index within the forward : 8 bits.
    The weight samples' ids (SampleCtx.next_stream) end at bit 59 and the condition noise sets bit 62, so no two kinds of draw share a
    stream."""
    if not (0 <= rank < 1 << 16 and 0 <= iteration < 1 << 36 and 0 <= call < 1 << 8):
        raise ValueError(f"attn_drop_stream_id: rank {rank}, iteration {iteration} or call {call} outside the 16 / 36 / 8 bit fields")
    return (1 << 61) | (rank << 44) | (iteration << 8) | call


class AttnDrop:
    """What identifies the attention-dropout draws of ONE forward of a net: its owner (ImageEnhancer.optimize_parameters) sets it as
    ``decomp.attn_drop`` before the forward.  ``base_stream_id`` = attn_drop_stream_id(rank, iteration); the decomposition counts its calls
    within the forward into the low 8 bits (the *DD archs decompose the image and the condition).  ``masks``: injected keep flags, one
    (B,2,32,32) tensor of 0 / 1 per call in call order (parity runs) instead of the in-kernel draw."""

    def __init__(self, seed=0, base_stream_id=1 << 61, masks=None):
        self.seed, self.base_stream_id, self.masks, self.calls = int(seed), int(base_stream_id), masks, 0


class Decomp(nn.Module):
    """wavelet=True : MyDecomp.forward -> one (B,32,h,w) tensor laid out [Q1_w (16) | Q2_w (16)].
    wavelet=False: Decomp.forward     -> one (B,8,H,W) tensor laid out [Q1 (4) | Q2 (4)] (after IWT and,
    for model4, PostSmooth).  The even/odd channel interleave of the reference is absorbed into a
    one-time permutation of the conv_out / sharpening weights."""

    def __init__(self, model="model4", wavelet_out=True, num_filters=32):
        super().__init__()
        if model not in ("model1", "model2", "model3", "model4"):
            raise ValueError(f"Unknown decomp_model: {model}")
        self.model, self.wavelet_out = model, wavelet_out
        nf = num_filters
        self.conv_in = Conv2dK(32, nf, 3, padding=1)
        if model == "model3":
            # QD/model3.py:175-178 mini U-Net.  The wavelet-domain MyDecomp of the DDWavelet arch overrides forward() with the
            # model1 / model4 op sequence, so there these three layers hold weights but are never applied (DDWavelet_arch.py:104-107).
            self.down_conv = Conv2dK(nf, nf, 3, stride=2, padding=1)
            self.mid_conv = Conv2dK(nf, nf, 3, padding=1)
            self.up_conv = ConvT2x2(nf, nf)
        d = 2 if model == "model2" else 1        # QD/model2.py:171-181: the second convolution of each branch is dilated
        self.branch_q1 = nn.Sequential(Conv2dK(nf, nf, 3, padding=1), nn.ReLU(inplace=True), Conv2dK(nf, nf, 3, padding=d, dilation=d))
        self.branch_q2 = nn.Sequential(Conv2dK(nf, nf, 3, padding=1), nn.ReLU(inplace=True), Conv2dK(nf, nf, 3, padding=d, dilation=d))
        self.cross_attn = _CrossAttnParams(nf, p=0.1 if model == "model3" else 0.0)
        self.attn_drop = None                    # AttnDrop of the forward under way, set by the net's owner; None: process-wide counter
        self.fuse = nn.Conv2d(nf * 2, nf, 1)
        self.conv_out = Conv2dK(nf, 32, 3, padding=1)
        self.sharpening = Conv2dK(32, 32, 3, padding=1, bias=True)
        if model == "model4" and not wavelet_out:
            self.smooth_q1 = nn.Module(); self.smooth_q1.conv = nn.Conv2d(4, 4, 3, padding=1, groups=4, bias=True)
            self.smooth_q2 = nn.Module(); self.smooth_q2.conv = nn.Conv2d(4, 4, 3, padding=1, groups=4, bias=True)

    @classmethod
    def from_shipped(cls, model, wavelet_out):
        from safetensors.torch import load_file
        m = cls(model, wavelet_out)
        sd = load_file(os.path.join(_QD_DIR, f"{model}_999.safetensors"))
        res = m.load_state_dict(sd, strict=False)      # strict=False: MyDecomp drops smooth_q* (DDWavelet_arch.py:138)
        bad = [k for k in res.unexpected_keys if not k.startswith(("smooth_q1.", "smooth_q2."))]
        if res.missing_keys or bad:
            raise RuntimeError(f"frozen decomposition weights {model}_999: missing {res.missing_keys}, unexpected {bad}")
        m.eval()
        for p in m.parameters():
            p.requires_grad = False
        return m

    def _perm(self, dev):
        if self.wavelet_out:   # [band*8 + 2j] then [band*8 + 2j + 1]
            idx = [b * 8 + 2 * j for b in range(4) for j in range(4)] + [b * 8 + 2 * j + 1 for b in range(4) for j in range(4)]
        else:                  # within each band: q1 comps then q2 comps -> IWT output is [Q1 | Q2]
            idx = [b * 8 + q for b in range(4) for q in (0, 2, 4, 6, 1, 3, 5, 7)]
        return torch.tensor(idx, device=dev, dtype=torch.long)

    def _prepared(self):
        srcs = [self.conv_out.weight, self.conv_out.bias, self.sharpening.weight, self.sharpening.bias, self.fuse.weight]

        def prep():
            dev = self.conv_out.weight.device
            p = self._perm(dev)
            ca = self.cross_attn
            aw = torch.cat([torch.cat([getattr(ca, n).weight.detach().reshape(-1), getattr(ca, n).bias.detach().reshape(-1)])
                            for n in ("q1_proj", "k2_proj", "v2_proj", "q2_proj", "k1_proj", "v1_proj", "out1", "out2")]).contiguous()
            d = dict(co_w=ops.ConvWeight(self.conv_out.weight.detach()[p].contiguous()), co_b=self.conv_out.bias.detach()[p].contiguous(),
                     sh_w=ops.ConvWeight(self.sharpening.weight.detach()[p][:, p].contiguous()), sh_b=self.sharpening.bias.detach()[p].contiguous(),
                     aw=aw, fw=self.fuse.weight.detach().reshape(32, 64).contiguous(), fb=self.fuse.bias.detach().contiguous())
            if hasattr(self, "smooth_q1"):
                d["sm_w"] = torch.cat([self.smooth_q1.conv.weight.detach(), self.smooth_q2.conv.weight.detach()], 0).contiguous()
                d["sm_b"] = torch.cat([self.smooth_q1.conv.bias.detach(), self.smooth_q2.conv.bias.detach()], 0).contiguous()
            return d
        return ops.derived(self).get("prep", srcs, prep)

    _drop_calls = 0     # process-wide count of dropout draws made without an AttnDrop record: successive calls never share a stream

    def _next_drop(self):
        """ops.attn_fold's ``drop`` for this call: None unless the attention dropout is live (train() mode, p > 0; nn.Dropout follows
        module.training alone, so grad mode does not matter -- QD/model3.py:98,124-131, and the wavelet-domain MyDecomp keeps the same
        cross_attn, DecompDualBranchDDWavelet_arch.py:55-143)."""
        p = self.cross_attn.p
        if not (self.training and p > 0):
            return None
        rec = self.attn_drop
        if rec is None:
            Decomp._drop_calls += 1
            return p, 0, (1 << 61) | (Decomp._drop_calls & ((1 << 44) - 1))
        call, rec.calls = rec.calls, rec.calls + 1
        if rec.masks is not None:
            if call >= len(rec.masks):
                raise BemNativeError(f"Decomp: call {call} of this forward has no injected dropout mask ({len(rec.masks)} given)")
            return p, rec.masks[call]
        if call >= 1 << 8:
            raise BemNativeError("Decomp: more than 256 decomposition calls under one AttnDrop record (set a fresh one per forward)")
        return p, rec.seed, rec.base_stream_id | call

    def forward(self, x, c0=0):
        """x (B,Ct,H,W); channels [c0, c0+3) hold the RGB image to decompose."""
        _need_cuda(x)
        return self.forward_from_dwt(ops.quat_dwt(x, c0))

    def forward_from_dwt(self, d):
        """d (B,32,h,w) = quat_dwt of the image: the entry for callers that form it themselves (ops.cond_dwt)."""
        _need_cuda(d)
        P = self._prepared()
        feat = self.conv_in(d)
        if self.model == "model3" and not self.wavelet_out:
            mid = self.mid_conv(self.down_conv(feat, relu=True), relu=True)
            feat = ops.add(feat, self.up_conv._forward_nograd(mid))
        dil = self.branch_q1[2].dilation[0]
        b1, b2 = self.branch_q1[2], self.branch_q2[2]
        f1 = ops.conv2d(self.branch_q1[0](feat, relu=True), b1.conv_weight(), b1.bias.detach(), pad=dil, dilation=dil, res1=feat)
        f2 = ops.conv2d(self.branch_q2[0](feat, relu=True), b2.conv_weight(), b2.bias.detach(), pad=dil, dilation=dil, res1=feat)
        Wp, bias = ops.attn_fold(f1, f2, P["aw"], P["fw"], P["fb"], drop=self._next_drop())
        fused = ops.pw_gemm(f1, Wp, 32, x2=f2, in_mode=2, bias=bias)
        out = ops.conv2d(fused, P["co_w"], P["co_b"], pad=1)
        out = ops.conv2d(out, P["sh_w"], P["sh_b"], pad=1, res1=out)
        if self.wavelet_out:
            return out
        q = ops.iwt(out)                               # (B,8,H,W) = [Q1 | Q2]
        if "sm_w" in P:
            q = ops.dwconv3x3(q, P["sm_w"], P["sm_b"], mode=3)
        return q


# ------------------------------------------------------------------------------------------------
# Stage-II: the U-Net pieces every arch is built from
# ------------------------------------------------------------------------------------------------
class _Dec(nn.ModuleDict):
    pass


def _check_last_act(last_act):
    if last_act is not None:
        raise NotImplementedError("last_act: only None occurs in the shipped option files")
    return nn.Identity()


def _first_conv(cin, n_feat):
    fc = Conv2dK(cin, n_feat, 3, 1, 1, bias=True)
    nn.init.kaiming_normal_(fc.weight, mode="fan_out", nonlinearity="linear")
    nn.init.zeros_(fc.bias)
    return fc


def _hamilton(o1, o2, train):
    """Hamilton(o1, o2)[1:] of two (B,4,H,W) quaternion maps -> (B,3,H,W): an autograd node in training, the kernel otherwise."""
    if train:
        return ag.HamiltonFn.apply(o1, o2)
    B, _, H, W = o1.shape
    out8 = torch.empty(B, 8, H, W, device=o1.device, dtype=o1.dtype)
    ops.copy_channels(o1, out8, 0)
    ops.copy_channels(o2, out8, 4)
    return ops.hamilton(out8)


class _Stage2(nn.Module):
    """Construction helpers and U-Net walks shared by the Stage-II archs.  The helpers register ``first_conv<sfx>``, ``encoders<sfx>``,
    ``down_layers<sfx>``, ``decoders<sfx>`` and ``proj<sfx>`` on the arch itself, so the state-dict keys are the reference's; each arch
    calls them in its own registration order (which fixes parameters() order and the RNG draws of the initialisation)."""

    def _setup(self, stage, num_blocks, d_state, ssm_ratio, mlp_ratio, mlp_type, decomp_model, wavelet_out):
        """Loads the frozen decomposition (none for decomp_model=None); returns level(dim, i), the VSS stack of U-Net level i (i = -1: the
        bottleneck)."""
        self.stage, self.num_levels = stage, len(num_blocks)
        if isinstance(d_state, int):
            d_state = [d_state] * self.num_levels
        if decomp_model is not None:
            self.decomp = Decomp.from_shipped(decomp_model, wavelet_out=wavelet_out)
        return lambda dim, i: make_vss_level(dim, num_blocks[i], d_state[i], ssm_ratio, mlp_ratio, mlp_type)

    def _add_encoder(self, sfx, cin, n_feat, level):
        """first_conv<sfx> and encoders<sfx>; returns the bottleneck width."""
        setattr(self, "first_conv" + sfx, _first_conv(cin, n_feat))
        enc, cur = nn.ModuleList(), n_feat
        for i in range(self.num_levels - 1):
            enc.append(level(cur, i))
            cur *= 2
        setattr(self, "encoders" + sfx, enc)
        return cur

    def _add_down_layers(self, sfx, n_feat):
        setattr(self, "down_layers" + sfx, nn.ModuleList([conv_down(n_feat * (2 ** i)) for i in range(self.num_levels - 1)]))

    def _add_decoder(self, sfx, cur, n_feat, out_ch, level):
        """decoders<sfx> from the bottleneck width ``cur`` back to n_feat, then proj<sfx> (n_feat -> out_ch)."""
        decs = nn.ModuleList()
        for i in range(self.num_levels - 2, -1, -1):
            decs.append(_Dec({"up": ConvT2x2(cur, cur // 2), "fuse": PwConv2d(cur, cur // 2, bias=False), "block": level(cur // 2, i)}))
            cur //= 2
        setattr(self, "decoders" + sfx, decs)
        pj = Conv2dK(n_feat, out_ch, 3, 1, 1, bias=True)
        nn.init.zeros_(pj.bias)
        setattr(self, "proj" + sfx, pj)

    def _encode(self, sfx, x, **first_kw):
        """first_conv, then (encoder, fork, down) per level; returns the deepest features and the skips."""
        f = getattr(self, "first_conv" + sfx)(x, **first_kw)
        skips = []
        for enc, down in zip(getattr(self, "encoders" + sfx), getattr(self, "down_layers" + sfx)):
            # two consumers (down layer, decoder skip): their gradients meet in bem_add_f32; a no-op without a graph
            f, s = ag.fork(enc(f))
            skips.append(s)
            f = down(f)
        return f, skips

    def _decode(self, sfx, f, skips, pre=None):
        """(up, fuse with the skip, block) per level, then proj.  ``pre``: a bias-free 1x1 layer applied to f ahead of the first level.
        Inference: up and fuse (and pre) are linear with nothing in between, so a level runs them as one folded kernel (ops.up_fuse,
        modules.fold_up_fuse) and the up-sampled tensor is never formed; training keeps the layers as their own autograd nodes."""
        folded = ops.USE_UPFUSE and not grad_mode(self)
        if pre is not None and not (folded and pre.bias is None):
            f, pre = pre(f), None
        for dec, skip in zip(getattr(self, "decoders" + sfx), reversed(skips)):
            if folded and dec["fuse"].bias is None:
                f = ops.up_fuse(f, skip, fold_up_fuse(dec["up"], dec["fuse"], pre, holder=dec))
            else:
                f = dec["fuse"](dec["up"](f if pre is None else pre(f)), x2=skip, in_mode=2)
            f, pre = dec["block"](f), None
        return getattr(self, "proj" + sfx)(f)

    def _cross_fuse(self, f1, f2):
        """The one cross-fusion at the deepest encoder level of DecompDualBranch / FusedTunedModel: branch 2 takes from branch 1 first, then
        branch 1 from the fused branch 2 (DecompModel_arch.py:311-312, FusedModel_arch.py:299-300)."""
        fa, fb = ag.fork(f1)                                            # branch 1's deepest features feed both cross-fusions
        f2 = self.cross_fusion_12(fa, f2)
        f2a, f2b = ag.fork(f2)
        return self.cross_fusion_21(f2a, fb), f2b

    def _attn_bottleneck(self, sfx, f, train):
        """bottleneck<sfx>, then SE and spatial attention: the SE gate is applied inside the attention kernel in inference."""
        f = getattr(self, "bottleneck" + sfx)(f)
        se, sa = getattr(self, "bottleneck_se" + sfx), getattr(self, "spatial_attention" + sfx)
        return sa(se(f)) if train else sa(f, chan_scale=se.gate(f))


# ------------------------------------------------------------------------------------------------
# Stage-II: two U-Nets (Q1, Q2) around one shared bottleneck -- DecompDualBranchDDWavelet and the sibling archs
# DecompDualBranch2DD / DecompDualBranch2 (same blocks and kernels, different wiring of the condition)
# ------------------------------------------------------------------------------------------------
class _DualBranch(_Stage2):
    """Subclasses set the decomposition's output domain and the widths of the U-Net input and of proj."""
    _wavelet, _in_ch, _out_ch = False, 4, 4

    def __init__(self, in_channels=3, out_channels=3, n_feat=40, stage=1, num_blocks=[2, 2, 2], d_state=1, ssm_ratio=1,
                 mlp_ratio=4, mlp_type="gdmlp", use_pixelshuffle=False, drop_path=0.0, use_illu=False, sam=False,
                 last_act=None, decomp_model="model1"):
        super().__init__()
        level = self._setup(stage, num_blocks, d_state, ssm_ratio, mlp_ratio, mlp_type, decomp_model, self._wavelet)
        for br in ("_Q1", "_Q2"):
            cur = self._add_encoder(br, self._in_ch, n_feat, level)
            self._add_down_layers(br, n_feat)
        self.bottleneck_fuse = PwConv2d(cur * 2, cur, bias=False)
        self.bottleneck_block = level(cur, -1)
        self.bottleneck_to_Q1 = PwConv2d(cur, cur, bias=False)
        self.bottleneck_to_Q2 = PwConv2d(cur, cur, bias=False)
        for br in ("_Q1", "_Q2"):
            self._add_decoder(br, cur, n_feat, self._out_ch, level)
        self.last_act = _check_last_act(last_act)
        self.apply(_init_weights)
        # the registration order above differs from the reference only inside this constructor;
        # state-dict KEYS and shapes are identical (tests/test_host_contract.py)

    def _dual_unet(self, qs, first_kw=({}, {})):
        """qs: the inputs of U-Net Q1 and Q2, taken one at a time as each branch starts; first_kw: per branch, further arguments of its
        first_conv.  Returns the two proj outputs."""
        feats, skips = [], []
        for br, q, kw in zip(("_Q1", "_Q2"), qs, first_kw):
            f, sk = self._encode(br, q, **kw)
            feats.append(f)
            skips.append(sk)
        fused = self.bottleneck_block(self.bottleneck_fuse(feats[0], x2=feats[1], in_mode=2))
        return [self._decode(br, fz, sk, pre=getattr(self, "bottleneck_to" + br)) for br, fz, sk in zip(("_Q1", "_Q2"), ag.fork(fused), skips)]

    def _full_res(self, qs):
        """Full-resolution tail: q1, q2 (B,Cin,H,W) -> Hamilton(Q1_out, Q2_out)[1:] (B,3,H,W).  Kernels only in inference, bem.autograd
        nodes in train() mode with autograd on (q1, q2 come from the frozen decomposition and carry no graph)."""
        train = grad_mode(self)
        with torch.enable_grad() if train else torch.no_grad():
            return _hamilton(*self._dual_unet(qs), train)


class DecompDualBranchDDWavelet(_DualBranch):
    _wavelet, _in_ch, _out_ch = True, 32, 16

    # -- pieces reused by the Monte-Carlo pipeline (decomp(img) hoisted out of the sample loop) --
    def decompose(self, x, c0):
        return self.decomp(x, c0)

    def decompose_cond(self, conds, scale):
        """decompose(bilinear_up(conds, scale), 0) of the Stage-I conditions (R,3,hd,wd), without the enlarged condition image."""
        return self.decomp.forward_from_dwt(ops.cond_dwt(conds, scale))

    def first_conv_image(self, d_img):
        """Per branch, the image half of first_conv with its bias: (Bi,n_feat,h,w) each.  first_conv is linear in its input channels and
        its image half does not depend on the sample, so it is evaluated once per image; forward_decomposed adds it to the condition
        half of every sample of that image."""
        fcs = [getattr(self, "first_conv" + br) for br in ("_Q1", "_Q2")]
        return [ops.conv2d(d_img, fc.conv_weight((0, 16)), fc.bias.detach(), pad=1, cin_slice=(16 * bi, 16)) for bi, fc in enumerate(fcs)]

    def forward_decomposed(self, d_img, d_cond, img_index=None, p_img=None):
        """d_img (Bi,32,h,w), d_cond (B,32,h,w); img_index: None (Bi == B) or samples-per-image count
        (image i serves batch rows [i*n, (i+1)*n)); p_img: first_conv_image(d_img) where the caller has it already.
        Inference: first_conv(cat(d_img[16 bi : 16 bi + 16] per sample, d_cond[16 bi : 16 bi + 16])) runs as the condition half on the B
        rows with the per-image half as its residual -- the concatenation is never formed.  Training keeps the concatenated input."""
        B, _, h, w = d_cond.shape
        spi = 1 if img_index is None else int(img_index)
        if d_img.shape[0] * spi != B:
            raise ValueError("forward_decomposed: image / sample batch mismatch")
        if not grad_mode(self):
            if p_img is None:
                p_img = self.first_conv_image(d_img)
            o1, o2 = self._dual_unet((d_cond, d_cond), [dict(cin_slice=(16 * bi, 16), w_part=(16, 16), use_bias=False, res1=p_img[bi], res1_rep=spi)
                                                        for bi in range(2)])
            return ops.iwt_hamilton(o1, o2)

        def branch_input(bi):
            q = torch.empty(B, 32, h, w, device=d_cond.device, dtype=d_cond.dtype)
            if spi == 1:
                ops.copy_channels(d_img, q, 0, src_c0=16 * bi, C=16)
            else:
                ops.copy_channels_rep(d_img, q, 0, spi, src_c0=16 * bi, C=16)
            ops.copy_channels(d_cond, q, 16, src_c0=16 * bi, C=16)
            return q
        o1, o2 = self._dual_unet(branch_input(bi) for bi in range(2))
        if o1.requires_grad or o2.requires_grad:
            return ag.IwtHamiltonFn.apply(o1, o2)
        return ops.iwt_hamilton(o1, o2)

    def forward(self, x, mask=None):
        """Inference: kernels only, nothing recorded.  ``train()`` mode with autograd enabled (image_enhancer_model.py:165-216):
        the frozen decomposition still runs without a graph (DDWavelet_arch.py:307), the U-Nets record bem.autograd nodes."""
        _need_cuda(x)
        train = grad_mode(self)
        with torch.no_grad():
            x = x.contiguous()
            if x.shape[1] != 6:
                raise ValueError("DecompDualBranchDDWavelet expects 6 input channels (image || condition)")
            d_img, d_cond = self.decomp(x, 0), self.decomp(x, 3)
        with torch.enable_grad() if train else torch.no_grad():
            out = self.forward_decomposed(d_img, d_cond)
        return [x, out]


class DecompDualBranch2DD(_DualBranch):
    """basicsr/archs/DecompDualBranchDD_arch.py:53-302: Q = cat(Q_img, Q_cond) (8 channels per branch)."""
    _in_ch = 8

    def forward(self, x, mask=None):
        _need_cuda(x)
        with torch.no_grad():
            x = x.contiguous()
            B, _, H, W = x.shape
            qi, qc = self.decomp(x, 0), self.decomp(x, 3)              # each (B,8,H,W) = [Q1 | Q2]
            qs = []
            for bi in range(2):
                q = torch.empty(B, 8, H, W, device=x.device, dtype=x.dtype)
                ops.copy_channels(qi, q, 0, src_c0=4 * bi, C=4)
                ops.copy_channels(qc, q, 4, src_c0=4 * bi, C=4)
                qs.append(q)
        return [x, self._full_res(qs)]


class DecompDualBranch2(_DualBranch):
    """basicsr/archs/DecompDualBranch_arch.py:51-298: Q = Q_img + [cond, 0] (4 channels per branch); returns
    [x[:, 0:3], out] like the reference."""

    def forward(self, x, mask=None):
        _need_cuda(x)
        with torch.no_grad():
            x = x.contiguous()
            B, _, H, W = x.shape
            qi = self.decomp(x, 0)
            qs = []
            for bi in range(2):
                q = torch.empty(B, 4, H, W, device=x.device, dtype=x.dtype)
                ops.copy_channels(qi, q, 0, src_c0=4 * bi, C=4)
                ops.add_channels(x, q, 0, src_c0=3, C=3)               # + [cond, 0]
                qs.append(q)
        return [x[:, 0:3], self._full_res(qs)]


# ------------------------------------------------------------------------------------------------
# Stage-II: DecompDualBranch (basicsr/archs/DecompModel_arch.py:101-366) -- two U-Nets, one cross-fusion, SE + spatial attention
# ------------------------------------------------------------------------------------------------
class CrossFusionBlock(nn.Module):
    """DecompModel_arch.py:57-66: x_tgt + gate * transform(x_src).  The gate is folded into the 1x1 weights and bias (row scaling, cached per
    weight version), so the block is one limb GEMM with x_tgt as its residual."""

    def __init__(self, ch):
        super().__init__()
        self.transform = PwConv2d(ch, ch, bias=True)
        self.gate = nn.Parameter(torch.ones(1, ch, 1, 1))

    def forward(self, x_src, x_tgt):
        _need_cuda(x_src)
        if grad_mode(self):                      # training: the transform as its own autograd node, then x_tgt + gate * t
            return ag.GateAddFn.apply(self.transform(x_src), self.gate, x_tgt)
        t, C = self.transform, self.transform.out_channels
        Wp, b = ops.derived(self).get("gated", [t.weight, t.bias, self.gate], lambda: (
            ops.pack_pw_weight(ops.row_scale(t.weight.detach().reshape(C, C).contiguous(), self.gate.detach().reshape(C).contiguous())),
            ops.row_scale(t.bias.detach().contiguous(), self.gate.detach().reshape(C).contiguous())))
        return ops.pw_gemm(x_src, Wp, C, bias=b, res=x_tgt)


class SEBlock(nn.Module):
    """DecompModel_arch.py:68-83.  ``gate(x)`` returns the (B,C) channel factors; the multiplication happens inside the spatial attention
    that follows it."""

    def __init__(self, channel, reduction=16):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(channel, channel // reduction, bias=False), nn.ReLU(inplace=True),
                                nn.Linear(channel // reduction, channel, bias=False), nn.Sigmoid())

    def gate(self, x):
        _need_cuda(x)
        return ops.se_gate(x, self.fc[0].weight.detach(), self.fc[2].weight.detach())

    def forward(self, x):
        """Training form (the scaled tensor is materialised: the backward needs it); inference goes through gate() + SpatialAttention."""
        _need_cuda(x)
        if grad_mode(self):
            return ag.SEBlockFn.apply(x, self.fc[0].weight, self.fc[2].weight)
        return ops.chan_scale(x.contiguous(), self.gate(x))


class SpatialAttention(nn.Module):
    """DecompModel_arch.py:85-99 (kernel 7, or 3)."""

    def __init__(self, kernel_size=7):
        super().__init__()
        if kernel_size not in (3, 7):
            raise ValueError("kernel size must be 3 or 7")
        self.conv = nn.Conv2d(2, 1, kernel_size, padding=kernel_size // 2, bias=False)

    def forward(self, x, chan_scale=None):
        _need_cuda(x)
        if grad_mode(self):
            if chan_scale is not None:
                raise BemNativeError("SpatialAttention: the training form takes the SE-scaled tensor (SEBlock.forward), not a gate")
            return ag.SpatialAttnFn.apply(x, self.conv.weight)
        return ops.spatial_attention(x, self.conv.weight.detach(), chan_scale)


class DecompDualBranch(_Stage2):
    """DecompModel_arch.py:101-366: the image's two quaternion maps (4 channels each; the condition half of the 6-channel input is not
    read, :294) through two U-Nets with their own bottlenecks.  State-dict keys follow the reference: branch 1 without suffix, branch 2
    with the suffix ``2``."""

    def __init__(self, in_channels=3, out_channels=3, n_feat=40, stage=1, num_blocks=[2, 2, 2], d_state=1, ssm_ratio=1,
                 mlp_ratio=4, mlp_type="gdmlp", use_pixelshuffle=False, drop_path=0.0, use_illu=False, sam=False,
                 last_act=None, decomp_model="model1"):
        super().__init__()
        level = self._setup(stage, num_blocks, d_state, ssm_ratio, mlp_ratio, mlp_type, decomp_model, False)
        for s_ in ("", "2"):
            cur = self._add_encoder(s_, 4, n_feat, level)
            setattr(self, "bottleneck" + s_, level(cur, -1))
            self._add_decoder(s_, cur, n_feat, 4, level)
            self._add_down_layers(s_, n_feat)
        self.last_act = _check_last_act(last_act)
        self.cross_fusion_12, self.cross_fusion_21 = CrossFusionBlock(cur), CrossFusionBlock(cur)
        self.bottleneck_se, self.bottleneck_se2 = SEBlock(cur), SEBlock(cur)
        self.spatial_attention, self.spatial_attention2 = SpatialAttention(), SpatialAttention()
        self.apply(_init_weights)

    def forward(self, x, mask=None):
        """Inference: kernels only.  ``train()`` mode with autograd enabled (image_enhancer_model.py:165-216): the frozen decomposition runs
        without a graph, the two U-Nets, the cross-fusions, SE / attention blocks and the Hamilton product record bem.autograd nodes."""
        _need_cuda(x)
        train = grad_mode(self)
        with torch.no_grad():
            x = x.contiguous()
            qi = self.decomp(x, 0)                                      # (B,8,H,W) = [Q1 | Q2] of the image channels
        with torch.enable_grad() if train else torch.no_grad():
            f1, sk1 = self._encode("", qi, cin_slice=(0, 4))
            f2, sk2 = self._encode("2", qi, cin_slice=(4, 4))
            f1, f2 = self._cross_fuse(f1, f2)
            outs = [self._decode(s_, self._attn_bottleneck(s_, f, train), sk) for s_, f, sk in (("", f1, sk1), ("2", f2, sk2))]
            out = _hamilton(outs[0], outs[1], train)
        return [x, out]


# ------------------------------------------------------------------------------------------------
# Stage-II: DecompSingleBranch (BASELINE config 1)
# ------------------------------------------------------------------------------------------------
class DecompSingleBranch(_Stage2):
    def __init__(self, in_channels=6, out_channels=3, n_feat=40, stage=1, num_blocks=[2, 2, 2], d_state=1, ssm_ratio=1,
                 mlp_ratio=4, mlp_type="gdmlp", use_pixelshuffle=False, drop_path=0.0, use_illu=False, sam=False,
                 last_act=None, decomp_model="model1"):
        super().__init__()
        level = self._setup(stage, num_blocks, d_state, ssm_ratio, mlp_ratio, mlp_type, decomp_model, False)
        self.conditioning_channels = 3
        cur = self._add_encoder("", 11, n_feat, level)
        self.bottleneck = level(cur, -1)
        self._add_decoder("", cur, n_feat, 8, level)
        self.last_act = _check_last_act(last_act)
        self._add_down_layers("", n_feat)
        self.drop_path = nn.Identity()
        self.apply(_init_weights)

    def forward(self, x, mask=None):
        _need_cuda(x)
        with torch.no_grad():
            x = x.contiguous()
            B, _, H, W = x.shape
            q = self.decomp(x, 0)                                    # (B,8,H,W) = [Q1 | Q2]
            fea = torch.empty(B, 11, H, W, device=x.device, dtype=x.dtype)
            ops.copy_channels(q, fea, 0)
            ops.copy_channels(x, fea, 8, src_c0=3, C=3)
        return [x, self._run(fea)]

    def _run(self, fea):
        """The U-Net + Hamilton product on the assembled input: kernels only in inference, bem.autograd nodes in train() mode with autograd on
        (the frozen decomposition that produced ``fea`` never records)."""
        train = grad_mode(self)
        with torch.enable_grad() if train else torch.no_grad():
            f, sk = self._encode("", fea)
            out = self._decode("", self.bottleneck(f), sk)
            return ag.Hamilton8Fn.apply(out) if train else ops.hamilton(out)


class DecompSingleBranchDD(DecompSingleBranch):
    """basicsr/archs/DecompSingleBranchDD_arch.py:53-251: the condition is decomposed too; the single U-Net sees
    cat(Q1_img, Q2_img, Q1_cond, Q2_cond) (16 channels)."""

    def __init__(self, in_channels=6, out_channels=3, n_feat=40, stage=1, num_blocks=[2, 2, 2], d_state=1, ssm_ratio=1,
                 mlp_ratio=4, mlp_type="gdmlp", use_pixelshuffle=False, drop_path=0.0, use_illu=False, sam=False,
                 last_act=None, decomp_model="model1"):
        super().__init__(in_channels, out_channels, n_feat, stage, num_blocks, d_state, ssm_ratio, mlp_ratio, mlp_type,
                         use_pixelshuffle, drop_path, use_illu, sam, last_act, decomp_model)
        del self.conditioning_channels
        self.first_conv = _first_conv(16, n_feat)       # replaces the parent's 11-channel one after its draws, like the reference

    def forward(self, x, mask=None):
        _need_cuda(x)
        with torch.no_grad():
            x = x.contiguous()
            B, _, H, W = x.shape
            fea = torch.empty(B, 16, H, W, device=x.device, dtype=x.dtype)
            ops.copy_channels(self.decomp(x, 0), fea, 0)
            ops.copy_channels(self.decomp(x, 3), fea, 8)
        return [x, self._run(fea)]
# ------------------------------------------------------------------------------------------------
# Stage-II without a decomposition: U-Nets on the 6-channel cat(image, upsampled condition) -- VMUNet and its two-branch kin
# ------------------------------------------------------------------------------------------------
def _check_head_width(arch, out_channels):
    """Before any parameter is drawn: the head kernel takes two 3-channel branch outputs only (C_out 3, C_in 6)."""
    if out_channels != 3:
        raise NotImplementedError(f"{arch}: out_channels={out_channels}; only out_channels 3 is supported by the two-branch head kernel")


class FusionHead(nn.Sequential):
    """fusion = Sequential(Conv2d(2C, C, 3, p=1), ReLU, Conv2d(C, C, 3, p=1)) on cat(out_1, out_2) (TunedModel_arch.py:315-319,406,
    FusedModel_arch.py:234-238,330), evaluated by one kernel from the two branch outputs (the concatenation is never formed).  C = 3
    only: the width of every option file."""

    def __init__(self, out_channels):
        if out_channels != 3:
            raise NotImplementedError(f"fusion head: out_channels={out_channels}; only out_channels 3 (Conv2d(6,3) -> ReLU -> Conv2d(3,3)) "
                                      "is supported")
        super().__init__(nn.Conv2d(6, 3, 3, 1, 1, bias=True), nn.ReLU(inplace=True), nn.Conv2d(3, 3, 3, 1, 1, bias=True))

    def forward(self, o1, o2):
        _need_cuda(o1)
        c1, c2 = self[0], self[2]
        if grad_mode(self):
            return ag.FusionHeadFn.apply(o1, o2, c1.weight, c1.bias, c2.weight, c2.bias)
        return ops.fusion_head(o1, o2, c1.weight.detach(), c1.bias.detach(), c2.weight.detach(), c2.bias.detach())


class _ImageDomain(_Stage2):
    """The reference builds these archs branch by branch (first_conv, encoders, bottleneck, decoders, proj, last_act, down_layers; branch 2
    with the suffix ``2``), then their extra blocks; each subclass registers in its reference's order, so parameters() order, state-dict
    keys and the RNG draws of the initialisation are the reference's."""

    def _add_unet(self, sfx, cin, n_feat, out_ch, level, last_act):
        cur = self._add_encoder(sfx, cin, n_feat, level)
        setattr(self, "bottleneck" + sfx, level(cur, -1))
        self._add_decoder(sfx, cur, n_feat, out_ch, level)
        setattr(self, "last_act" + sfx, _check_last_act(last_act))
        self._add_down_layers(sfx, n_feat)
        return cur

    def forward(self, x, mask=None):
        """Inference: kernels only, nothing recorded.  ``train()`` mode with autograd enabled (image_enhancer_model.py:165-216): every block
        records its bem.autograd node."""
        _need_cuda(x)
        train = grad_mode(self)
        x = x.contiguous()
        with torch.enable_grad() if train else torch.no_grad():
            out = self._body(x, train)
        return [x, out]


class VMUNet(_ImageDomain):
    """VMUnet_arch.py:68-240: one U-Net."""

    def __init__(self, in_channels=3, out_channels=3, n_feat=40, stage=1, num_blocks=[2, 2, 2], d_state=1, ssm_ratio=1, mlp_ratio=4,
                 mlp_type="gdmlp", use_pixelshuffle=False, drop_path=0.0, use_illu=False, sam=False, last_act=None):
        super().__init__()
        level = self._setup(stage, num_blocks, d_state, ssm_ratio, mlp_ratio, mlp_type, None, False)
        self._add_unet("", in_channels, n_feat, out_channels, level, last_act)
        self.drop_path = nn.Identity()
        self.apply(_init_weights)

    def _body(self, x, train):
        f, sk = self._encode("", x)
        return self._decode("", self.bottleneck(f), sk)


class NaiveVMUNetTwoBranch(_ImageDomain):
    """TwoBranchNaive_arch.py:68-271: two U-Nets on the same input, outputs averaged."""

    def __init__(self, in_channels=3, out_channels=3, n_feat=40, stage=1, num_blocks=[2, 2, 2], d_state=1, ssm_ratio=1, mlp_ratio=4,
                 mlp_type="gdmlp", use_pixelshuffle=False, drop_path=0.0, use_illu=False, sam=False, last_act=None):
        super().__init__()
        _check_head_width("NaiveVMUNetTwoBranch", out_channels)
        level = self._setup(stage, num_blocks, d_state, ssm_ratio, mlp_ratio, mlp_type, None, False)
        for s_ in ("", "2"):
            self._add_unet(s_, in_channels, n_feat, out_channels, level, last_act)
        self.drop_path = nn.Identity()
        self.apply(_init_weights)

    def _body(self, x, train):
        o1, o2 = [self._decode(s_, getattr(self, "bottleneck" + s_)(f), sk) for s_, (f, sk) in (("", self._encode("", x)), ("2", self._encode("2", x)))]
        return ag.BranchMeanFn.apply(o1, o2) if train else ops.fusion_head(o1, o2, mean=True)


class TunedModel(_ImageDomain):
    """TunedModel_arch.py:162-406: two U-Nets with SE + spatial attention after each bottleneck, outputs fused by the 3x3 head."""

    def __init__(self, in_channels=3, out_channels=3, n_feat=40, stage=1, num_blocks=[2, 2, 2], d_state=1, ssm_ratio=1, mlp_ratio=4,
                 mlp_type="gdmlp", use_pixelshuffle=False, drop_path=0.0, use_illu=False, sam=False, last_act=None):
        super().__init__()
        _check_head_width("TunedModel", out_channels)
        level = self._setup(stage, num_blocks, d_state, ssm_ratio, mlp_ratio, mlp_type, None, False)
        for s_ in ("", "2"):
            cur = self._add_unet(s_, in_channels, n_feat, out_channels, level, last_act)
        self.drop_path = nn.Identity()
        self.spatial_attention, self.spatial_attention2 = SpatialAttention(), SpatialAttention()
        self.fusion = FusionHead(out_channels)
        self.bottleneck_se, self.bottleneck_se2 = SEBlock(cur), SEBlock(cur)
        self.apply(_init_weights)

    def _body(self, x, train):
        outs = []
        for s_ in ("", "2"):
            f, sk = self._encode(s_, x)
            outs.append(self._decode(s_, self._attn_bottleneck(s_, f, train), sk))
        return self.fusion(*outs)


class FusedTunedModel(_ImageDomain):
    """FusedModel_arch.py:101-332: TunedModel with one cross-fusion at the deepest encoder level, the sequence of DecompDualBranch."""

    def __init__(self, in_channels=3, out_channels=3, n_feat=40, stage=1, num_blocks=[2, 2, 2], d_state=1, ssm_ratio=1, mlp_ratio=4,
                 mlp_type="gdmlp", use_pixelshuffle=False, drop_path=0.0, use_illu=False, sam=False, last_act=None):
        super().__init__()
        _check_head_width("FusedTunedModel", out_channels)
        level = self._setup(stage, num_blocks, d_state, ssm_ratio, mlp_ratio, mlp_type, None, False)
        for s_ in ("", "2"):
            cur = self._add_unet(s_, in_channels, n_feat, out_channels, level, last_act)
        self.drop_path = nn.Identity()
        self.cross_fusion_12, self.cross_fusion_21 = CrossFusionBlock(cur), CrossFusionBlock(cur)
        self.bottleneck_se, self.bottleneck_se2 = SEBlock(cur), SEBlock(cur)
        self.spatial_attention, self.spatial_attention2 = SpatialAttention(), SpatialAttention()
        self.fusion = FusionHead(out_channels)
        self.apply(_init_weights)

    def _body(self, x, train):
        f1, sk1 = self._encode("", x)
        f2, sk2 = self._encode("2", x)
        f1, f2 = self._cross_fuse(f1, f2)
        outs = [self._decode(s_, self._attn_bottleneck(s_, f, train), sk) for s_, f, sk in (("", f1, sk1), ("2", f2, sk2))]
        return self.fusion(*outs)


# ------------------------------------------------------------------------------------------------
# Stage-I: Network (UNet_arch.py)
# ------------------------------------------------------------------------------------------------
class PatchMerging(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.norm = LayerNorm2d(4 * dim)
        self.reduction = PwConv2d(4 * dim, 2 * dim, bias=False)

    def forward(self, x):
        if grad_mode(self):
            ps = [p for p in (self.norm.weight, self.norm.bias, self.reduction.weight) if p.requires_grad]
            return ag.LnPwFn.apply(ag.SpaceToDepthFn.apply(x), self.norm, self.reduction, *ps)
        return ag.ln_pw(ops.space_to_depth(x), self.norm, self.reduction)


class _Shuffle(nn.Module):
    def forward(self, x):
        return ops.pixel_shuffle2(x)


class _Up2(nn.Module):
    def forward(self, x):
        return ops.bilinear_up(x, 2)


class DualUpSample(nn.Module):
    """scale_factor 2 only (the factor the U-Net uses, UNet_arch.py:283)."""

    def __init__(self, in_channels, scale_factor=2):
        super().__init__()
        if scale_factor != 2:
            raise NotImplementedError("DualUpSample: scale_factor 2 only")
        c = in_channels
        self.factor = scale_factor
        self.conv = PwConv2d(c, c // 2, bias=False)
        self.up_p = nn.Sequential(PwConv2d(c, 2 * c, bias=False), nn.PReLU(), _Shuffle(), PwConv2d(c // 2, c // 2, bias=False))
        self.up_b = nn.Sequential(PwConv2d(c, c, bias=True), nn.PReLU(), _Up2(), PwConv2d(c, c // 2, bias=False))

    def forward(self, x):
        if grad_mode(self):
            xa, xb = ag.fork(x)
            p = self.up_p[3](ag.PixelShuffle2Fn.apply(ag.PReLUFn.apply(self.up_p[0](xa), self.up_p[1].weight)))
            b = self.up_b[3](ag.BilinearUpFn.apply(ag.PReLUFn.apply(self.up_b[0](xb), self.up_b[1].weight), 2))
            return self.conv(p, x2=b, in_mode=2)
        p = self.up_p[3](self.up_p[2](self.up_p[0](x, prelu=self.up_p[1].weight.detach())))
        b = self.up_b[3](self.up_b[2](self.up_b[0](x, prelu=self.up_b[1].weight.detach())))
        return self.conv(p, x2=b, in_mode=2)


class BasicBlock(nn.Module):
    def __init__(self, dim, num_blocks=2, d_state=1, ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp", sam=False,
                 condition=False, bayesian=False):
        super().__init__()
        if sam or condition:
            raise NotImplementedError("BasicBlock: sam / condition are off in every shipped option file")
        self.bayesian, self.sam, self.condition = bayesian, sam, condition
        self.blocks = nn.ModuleList(list(make_vss_level(dim, num_blocks, d_state, ssm_ratio, mlp_ratio, mlp_type)))

    def forward(self, x):
        for b in self.blocks:
            x = b(x)
        return x


class SubNetwork(nn.Module):
    def __init__(self, dim=31, num_blocks=[2, 4, 4], d_state=1, ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp",
                 use_pixelshuffle=False, drop_path=0.0, sam=False):
        super().__init__()
        if not use_pixelshuffle:
            raise NotImplementedError("SubNetwork: use_pixelshuffle=True (PatchMerging/DualUpSample) is the shipped configuration")
        if drop_path:
            raise NotImplementedError("drop_path > 0")
        self.dim, self.level = dim, len(num_blocks) - 1
        if isinstance(d_state, int):
            d_state = [d_state] * len(num_blocks)
        self.encoder_layers = nn.ModuleList()
        self.drop_path = nn.Identity()
        cur = dim
        for i in range(self.level):
            self.encoder_layers.append(nn.ModuleList([
                BasicBlock(cur, num_blocks[i], d_state[i], ssm_ratio, mlp_ratio, mlp_type, sam, bayesian=True), PatchMerging(cur)]))
            cur *= 2
        self.bottleneck = BasicBlock(cur, num_blocks[-1], d_state[self.level], ssm_ratio, mlp_ratio, sam=sam, bayesian=True)
        self.decoder_layers = nn.ModuleList()
        for i in range(self.level):
            self.decoder_layers.append(nn.ModuleList([
                DualUpSample(cur, 2), PwConv2d(cur, cur // 2, bias=False),
                BasicBlock(cur // 2, num_blocks[self.level - 1 - i], d_state[self.level - 1 - i], ssm_ratio, mlp_ratio, sam=sam, bayesian=True)]))
            cur //= 2
        self.apply(_init_weights)

    def forward(self, x):
        """returns the decoder output WITHOUT the outer residual (added by Network through proj's linearity)."""
        fea, enc = x, []
        for blk, down in self.encoder_layers:
            fea = blk(fea)
            if grad_mode(self):
                fea, skip = ag.fork(fea)
                enc.append(skip)
            else:
                enc.append(fea)
            fea = down(fea)
        fea = self.bottleneck(fea)
        for i, (up, fusion, blk) in enumerate(self.decoder_layers):
            fea = up(fea)
            fea = fusion(fea, x2=enc[self.level - 1 - i], in_mode=2)
            fea = blk(fea)
        return fea


class Network(nn.Module):
    def __init__(self, in_channels=3, out_channels=3, n_feat=40, stage=1, num_blocks=[1, 1, 1], d_state=1, ssm_ratio=1,
                 mlp_ratio=4, mlp_type="gdmlp", use_pixelshuffle=False, drop_path=0.0, use_illu=False, sam=False,
                 last_act=None):
        super().__init__()
        if stage != 1:
            raise NotImplementedError("Network: stage = 1 (the shipped configuration)")
        self.stage = stage
        self.mask_token = nn.Parameter(torch.zeros(1, n_feat, 1, 1))
        _trunc_normal_(self.mask_token, std=0.02)
        self.first_conv = Conv2dK(in_channels, n_feat, 3, 1, 1, bias=True)
        nn.init.kaiming_normal_(self.first_conv.weight, mode="fan_out", nonlinearity="linear")
        nn.init.zeros_(self.first_conv.bias)
        self.subnets = nn.ModuleList()
        self.proj = Conv2dK(n_feat, out_channels, 3, 1, 1, bias=True)
        nn.init.zeros_(self.proj.bias)
        self.last_act = _check_last_act(last_act)
        for _ in range(stage):
            self.subnets.append(SubNetwork(n_feat, num_blocks, d_state, ssm_ratio, mlp_ratio, mlp_type, use_pixelshuffle, drop_path, sam))

    def forward(self, x, mask=None):
        _need_cuda(x)
        if grad_mode(self):
            return self._forward_train(x, mask)
        # without an enclosing context: one weight sample per batch element, fresh Philox streams for this forward
        ctx = bayes.scope.ctx or bayes.SampleCtx(x.shape[0], None, seed=torch.initial_seed() & 0xFFFFFFFF)
        with torch.no_grad(), bayes.eval_sampling(self, ctx):
            x = x.contiguous()
            fea0 = self.first_conv(x)
            dec = self.subnets[0](fea0)
            # proj(fea0 + dec) = proj_nobias(fea0) + proj(dec)   (UNet_arch.py:361,470-472; conv is linear)
            base = ops.conv2d(fea0, self.proj.conv_weight(), None, pad=1)
            out = self.proj(dec, res1=base)
        return [x, out]

    def _forward_train(self, x, mask):
        """Training forward (UNet_arch.py:447-474 with module.training): one weight sample per Bayesian leaf for the whole batch
        (conv.py:100-104 draws eps once per forward), EMA prior update before the draw, optional MIM token mix, autograd nodes over the
        HIP kernels.  The returned prediction carries the anchor that folds the sampled-weight gradients into mu / rho after backward."""
        ctx = bayes.scope.ctx or bayes.SampleCtx(1, None, seed=torch.initial_seed() & 0xFFFFFFFF)
        if ctx.nsets != 1:
            raise BemNativeError("Network: a training forward shares one weight sample across the batch (SampleCtx(nsets=1))")
        with bayes.train_sampling(self, ctx) as step:
            fea = self.first_conv(x.contiguous())
            if mask is not None:
                fea = ag.MaskTokenFn.apply(fea, mask, self.mask_token)
            fa, fb = ag.fork(fea)
            dec = self.subnets[0](fa)
            out = self.proj(ag.AddFn.apply(fb, dec))
            out = bayes.BayesAnchorFn.apply(out, step)
        return [x, out]
