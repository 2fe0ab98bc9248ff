"""nn.Module mirrors of the reference's hot-path modules, computing through the HIP C ABI.

Same class names, constructor arguments, parameter names/shapes (state-dict contract, SURVEY.md
section 8b) and ``forward(x)`` meaning as the reference modules cited in each docstring -- but every
forward is a sequence of hand-written gfx950 kernels (bem.ops).  There is no CPU implementation:
calling a module on CPU tensors raises ``BemNativeError``.  In eval() mode, or with autograd disabled, a forward
runs the inference kernels and its output carries no graph; in train() mode with autograd enabled it records the
``bem.autograd`` nodes, whose backward is HIP kernels too.  The Bayesian leaves are ``bem.bayes``.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from . import autograd as ag
from . import ops
from .bayes import BayesBank, Conv2dReparameterization, EvalSampleBank, Linear2dReparameterization, SampleCtx, sampling, set_module_paths  # noqa: F401
from .native import BemNativeError


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def grad_mode(m: nn.Module) -> bool:
    """True when a forward has to record the training graph: module in train() mode with autograd enabled (the reference's
    training step, image_enhancer_model.py:165-216).  Everything else runs the inference kernels only."""
    return m.training and torch.is_grad_enabled()


def _need_cuda(x):
    if not x.is_cuda:
        raise BemNativeError("BEM modules run on the GPU through libbem_hip.so only (no CPU fallback); "
                             "move the model and input to a HIP device")


# ------------------------------------------------------------------------------------------------
# leaves
# ------------------------------------------------------------------------------------------------
class LayerNorm2d(nn.LayerNorm):
    """basicsr/vmamba/models/vmamba.py:58-63.  Parameter holder: the normalisation itself is always
    fused into the prologue of the 1x1 GEMM that consumes it."""

    def forward(self, x):
        raise BemNativeError("LayerNorm2d is fused into its consumer GEMM; it has no standalone forward here")


class Linear2d(nn.Linear):
    """basicsr/vmamba/models/vmamba.py:42-55: 1x1 conv with a 2-D weight (4-D accepted on load)."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.module_path = ""

    def _load_from_state_dict(self, state_dict, prefix, *args):
        if prefix + "weight" in state_dict:
            state_dict[prefix + "weight"] = state_dict[prefix + "weight"].view(self.weight.shape)
        return super()._load_from_state_dict(state_dict, prefix, *args)

    def gemm_weights(self, B):
        Wp = ops.derived(self).get("p", [self.weight], lambda: ops.pack_pw_weight(self.weight.detach().contiguous()))
        return Wp, (self.bias.detach() if self.bias is not None else None)

    def forward(self, x, **kw):
        _need_cuda(x)
        if grad_mode(self):
            return _pw_train(self, x, kw)
        Wp, b = self.gemm_weights(x.shape[0])
        return ops.pw_gemm(x, Wp, self.out_features, bias=b, **kw)


def _pw_train(m, x, kw):
    """Training-mode forward of a plain 1x1 layer (optionally over the concatenation of two inputs)."""
    extra = set(kw) - {"x2", "in_mode"}
    if extra or (("x2" in kw) != (kw.get("in_mode", 0) == 2)):
        raise BemNativeError(f"1x1 layer: the training path covers plain and concat-input forms only (got {sorted(kw)})")
    return ag.PwFn.apply(x, kw.get("x2"), m.weight, m.bias, m)


class PwConv2d(nn.Conv2d):
    """nn.Conv2d(kernel_size=1) holder running on the MFMA pointwise GEMM."""

    def __init__(self, cin, cout, bias=True):
        super().__init__(cin, cout, 1, 1, 0, bias=bias)
        self.module_path = ""

    def gemm_weights(self, B):
        Wp = ops.derived(self).get("p", [self.weight], lambda: ops.pack_pw_weight(
            self.weight.detach().reshape(self.out_channels, self.in_channels).contiguous()))
        return Wp, (self.bias.detach() if self.bias is not None else None)

    def forward(self, x, **kw):
        _need_cuda(x)
        if grad_mode(self):
            return _pw_train(self, x, kw)
        Wp, b = self.gemm_weights(x.shape[0])
        return ops.pw_gemm(x, Wp, self.out_channels, bias=b, **kw)


class DwConv2d(nn.Conv2d):
    """Depthwise 3x3, padding 1 (holder; epilogue chosen by the caller)."""

    def __init__(self, ch, bias=True):
        super().__init__(ch, ch, 3, 1, 1, groups=ch, bias=bias)
        self.module_path = ""

    def dw_weights(self, B):
        return self.weight.detach(), (self.bias.detach() if self.bias is not None else None)


class Conv2dK(nn.Conv2d):
    """Dense conv through ops.conv2d (holder); ops.conv2d_route names the kernel form a call takes."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)

    def conv_weight(self, part=None):
        """ops.ConvWeight of the weight, or for ``part=(c0, n)`` of its input channels [c0, c0+n), made once per weight version."""
        w = self.weight
        return ops.derived(self).get(("part", part), [w], lambda: ops.ConvWeight(
            w.detach() if part is None else w.detach()[:, part[0]:part[0] + part[1]].contiguous()))

    def forward(self, x, relu=False, res1=None, res2=None, cin_slice=None, res1_rep=1, w_part=None, use_bias=True):
        """``w_part=(c0, n)``: the convolution over input channels [c0, c0+n) of the weight only (a convolution is linear in its input
        channels: the parts of a split layer are summed through ``res1``); ``use_bias=False`` leaves the bias to another part."""
        _need_cuda(x)
        if grad_mode(self) and self.weight.requires_grad:
            if relu or res1 is not None or res2 is not None or w_part is not None or not use_bias:
                raise BemNativeError("Conv2dK: the training path covers the plain convolution (+ bias) only")
            return ag.Conv2dFn.apply(x, self.weight, self.bias, self, cin_slice)
        return ops.conv2d(x, self.conv_weight(w_part), self.bias.detach() if (use_bias and self.bias is not None) else None,
                          stride=self.stride[0], pad=self.padding[0], relu=relu, res1=res1, res2=res2, cin_slice=cin_slice, dilation=self.dilation[0],
                          res1_rep=res1_rep)


class ConvT2x2(nn.ConvTranspose2d):
    """nn.ConvTranspose2d(C, C/2, kernel 2, stride 2) = a 1x1 GEMM to 4*Cout rows + 2x2 scatter."""

    def __init__(self, cin, cout):
        super().__init__(cin, cout, kernel_size=2, stride=2, padding=0, output_padding=0)

    def forward(self, x):
        _need_cuda(x)
        if grad_mode(self):
            return ag.ConvT2x2Fn.apply(x, self.weight, self.bias, self)
        return self._forward_nograd(x)

    def _forward_nograd(self, x):
        co = self.out_channels

        def prep():
            w = self.weight.detach()                                  # (Cin, Cout, 2, 2)
            w4 = w.permute(2, 3, 1, 0).reshape(4 * co, self.in_channels).contiguous()   # row = (dy*2+dx)*Co + co
            return ops.pack_pw_weight(w4), self.bias.detach().repeat(4).contiguous()
        Wp, b4 = ops.derived(self).get("p", [self.weight, self.bias], prep)
        return ops.pw_gemm(x, Wp, 4 * co, bias=b4, convT_Win=x.shape[3])


def compose_up_fuse(up_w, up_b, fuse_w, pre_w=None):
    """The algebra of the folded decoder level, in float64 (plain torch, any device).  up_w (C, C/2, 2, 2) and up_b (C/2) of the
    ConvTranspose2d, fuse_w (C/2, C[, 1, 1]) = [Wf1 | Wf2] of the bias-free 1x1 conv over cat(up(f), skip), pre_w (C, C[, 1, 1]) of a
    bias-free 1x1 conv applied to f first.  Returns Wc (4, C/2, C), phase 2a + b = Wf1 Wt[:, :, a, b]^T [pre_w]; bc (C/2) = Wf1 bt; Wf2:
        out[:, 2i+a, 2j+b] = Wc[2a+b] f[:, i, j] + Wf2 skip[:, 2i+a, 2j+b] + bc"""
    co = up_w.shape[1]
    wf = fuse_w.double().reshape(fuse_w.shape[0], -1)
    wf1, wf2 = wf[:, :co], wf[:, co:]
    wc = torch.einsum("mc,kcab->abmk", wf1, up_w.double())
    if pre_w is not None:
        wc = wc @ pre_w.double().reshape(pre_w.shape[0], -1)
    return wc.reshape(4, wf.shape[0], -1), wf1 @ up_b.double(), wf2


def fold_up_fuse(up: "ConvT2x2", fuse: PwConv2d, pre: Optional[PwConv2d] = None, holder: Optional[nn.Module] = None) -> "ops.UpFuseWeights":
    """ops.UpFuseWeights of fuse(cat(up(pre(f)), skip)): composed in float64 on the weights' device, rounded once to f32 and packed.  The
    result lives in the Derived cache of ``holder`` (the decoder level; default ``up``), valid for one version of the source weights and
    one weight epoch.  A ``fuse`` or ``pre`` with a bias is refused (no shipped arch has one)."""
    if fuse.bias is not None or (pre is not None and pre.bias is not None):
        raise ValueError("fold_up_fuse: a fuse / pre layer with a bias is not folded")
    c, co = up.in_channels, up.out_channels
    if c != 2 * co or (fuse.in_channels, fuse.out_channels) != (c, co) or (pre is not None and (pre.in_channels, pre.out_channels) != (c, c)):
        raise ValueError(f"fold_up_fuse: needs up C -> C/2, fuse C -> C/2 and pre C -> C (got up {c} -> {co}, fuse {fuse.in_channels} -> "
                         f"{fuse.out_channels}" + (f", pre {pre.in_channels} -> {pre.out_channels})" if pre is not None else ")"))
    srcs = [up.weight, up.bias, fuse.weight] + ([pre.weight] if pre is not None else [])

    def prep():
        wc, bc, wf2 = compose_up_fuse(up.weight.detach(), up.bias.detach(), fuse.weight.detach(), None if pre is None else pre.weight.detach())
        return ops.UpFuseWeights(ops.pack_pw_weight(wc.float().contiguous()), ops.pack_pw_weight(wf2.float().contiguous()),
                                 bc.float().contiguous(), c)
    return ops.derived(up if holder is None else holder).get(("upfuse", pre is not None), srcs, prep)


# ------------------------------------------------------------------------------------------------
# SS2D / gdMlp / VSSBlock  (basicsr/vmamba/models/vmamba.py:116-133, 438-716, 1241-1334)
# ------------------------------------------------------------------------------------------------
class gdMlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0, channels_first=False):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.project_in = PwConv2d(in_features, hidden_features * 2)
        self.dwconv = DwConv2d(hidden_features * 2)
        self.project_out = PwConv2d(hidden_features, out_features)
        self.act = act_layer()

    def fused_supported(self, C):
        """The whole branch runs as one kernel (ops.gdmlp_x6): deterministic leaves and a supported width."""
        return isinstance(self.project_in, PwConv2d) and isinstance(self.dwconv, DwConv2d) and isinstance(self.project_out, PwConv2d) \
            and ops.gdmlp_x6_supported(C, self.project_in.out_channels // 2)

    def forward_fused(self, x, norm: LayerNorm2d, pre=None):
        """x + project_out(GELU(h1) * h2), h = dwconv(project_in(LN(x))).  pre (ops.gdmlp_x6): the SS2D tail that forms x inside the kernel."""
        B, C = x.shape[0], x.shape[1]
        Hd = self.project_in.out_channels // 2
        if self.fused_supported(C):
            # the whole branch in one kernel (bem_gdmlp_x6_f32): neither the 2Hd-channel nor the Hd-channel tensor reaches HBM
            pi, dw, po = self.project_in, self.dwconv, self.project_out

            def prep():
                perm = ops.gate_interleave(Hd, pi.weight.device)
                bg = pi.bias.detach()[perm].contiguous() if pi.bias is not None else torch.zeros(2 * Hd, device=pi.weight.device)
                return (ops.pack_pw_weight(pi.weight.detach().reshape(2 * Hd, C)[perm].contiguous(), x6=True), bg,
                        ops.dw_gate_params10(dw.weight.detach(), None if dw.bias is None else dw.bias.detach(), Hd),
                        ops.pack_pw_weight(po.weight.detach().reshape(po.out_channels, Hd).contiguous(), x6=True),
                        None if po.bias is None else po.bias.detach().contiguous())
            Wg, bg, w10, Wo, bo = ops.derived(self).get("gdmlp_x6", [t for t in (pi.weight, pi.bias, dw.weight, dw.bias, po.weight, po.bias) if t is not None], prep)
            return ops.gdmlp_x6(x, norm.weight.detach(), norm.bias.detach(), norm.eps, Wg, bg, w10, Wo, bo, Hd, pre=pre)
        if pre is not None:
            raise BemNativeError("gdMlp: the SS2D tail can be folded into the one-kernel branch only")
        return self.chain(x, norm)[0]

    def chain(self, x, norm: LayerNorm2d):
        """The branch as three kernels; returns (out, t2, g): the output and the two intermediates VSSBlockFn.backward needs,
        t2 = project_in(LN(x)) and g = GELU(h1) * h2."""
        B = x.shape[0]
        t2 = ag.ln_pw(x, norm, self.project_in)
        w, b = self.dwconv.dw_weights(B)
        g = ops.dwconv3x3(t2, w, b, mode=2)
        Wp, b = self.project_out.gemm_weights(B)
        return ops.pw_gemm(g, Wp, ag.out_width(self.project_out), bias=b, res=x), t2, g


SS2D_MAX_D_STATE = 16       # bem_ss2d_scan_n_f32 / bem_ss2d_scan_n_bwd_f32


class SS2D(nn.Module):
    """forward_type 'v05_noz' only (the one every arch on this path selects, UNet_arch.py:219)."""

    def __init__(self, d_model=96, d_state=16, ssm_ratio=2.0, dt_rank="auto", act_layer=nn.SiLU, d_conv=3,
                 conv_bias=True, dropout=0.0, bias=False, dt_min=0.001, dt_max=0.1, dt_init="random", dt_scale=1.0,
                 dt_init_floor=1e-4, initialize="v0", forward_type="v2", channel_first=False, **kwargs):
        super().__init__()
        if forward_type != "v05_noz" or not channel_first or d_conv != 3 or initialize != "v0":
            raise NotImplementedError("SS2D: only forward_type='v05_noz', channel_first, d_conv=3, init v0 are on the BEM path")
        N = int(d_state)
        if not 1 <= N <= SS2D_MAX_D_STATE:
            raise NotImplementedError(f"SS2D: d_state = {N}: the fused HIP scans take 1 <= d_state <= {SS2D_MAX_D_STATE}")
        d_inner = int(ssm_ratio * d_model)
        R = math.ceil(d_model / 16) if dt_rank == "auto" else dt_rank
        self.d_inner, self.dt_rank, self.d_state = d_inner, R, N
        self.in_proj = Linear2d(d_model, d_inner, bias=bias)
        self.act = act_layer()
        self.conv2d = DwConv2d(d_inner, bias=conv_bias)
        K = 4
        self.x_proj_weight = nn.Parameter(torch.stack([nn.Linear(d_inner, R + 2 * N, bias=False).weight.detach() for _ in range(K)], 0))
        self.out_proj = Linear2d(d_inner, d_model, bias=bias)
        # mamba_init.init_dt_A_D (vmamba.py:222-289)
        std = R ** -0.5 * dt_scale
        dtw, dtb = [], []
        for _ in range(K):
            w = torch.empty(d_inner, R).uniform_(-std, std)
            dt = torch.exp(torch.rand(d_inner) * (math.log(dt_max) - math.log(dt_min)) + math.log(dt_min)).clamp(min=dt_init_floor)
            dtw.append(w)
            dtb.append(dt + torch.log(-torch.expm1(-dt)))
        self.dt_projs_weight = nn.Parameter(torch.stack(dtw, 0))
        self.dt_projs_bias = nn.Parameter(torch.stack(dtb, 0))
        self.A_logs = nn.Parameter(torch.log(torch.arange(1, N + 1, dtype=torch.float32)).view(1, -1).repeat(K * d_inner, 1).contiguous())
        self.Ds = nn.Parameter(torch.ones(K * d_inner))
        self.out_norm = LayerNorm2d(d_inner)

    def _scan_params(self):
        R = self.dt_rank

        def prep():
            xw = self.x_proj_weight.detach()                                # (4, R+2N, C)
            # one x_proj GEMM over the row-major planes for all four directions: rows [dir 0 | dir 2 | dir 1 | dir 3]
            rows = torch.cat([xw[0], xw[2], xw[1], xw[3]], 0).float().contiguous()     # raw f32: what bem_ss2d_core_small_f32 reads
            wall = ops.pack_pw_weight(rows)
            A = -torch.exp(self.A_logs.detach().float())                    # (4C, N): flat (4C) for the d_state = 1 kernels
            A = (A.reshape(-1) if self.d_state == 1 else A).contiguous()
            return (wall, self.dt_projs_weight.detach().contiguous(), self.dt_projs_bias.detach().contiguous(), A,
                    self.Ds.detach().float().contiguous(), rows)
        return ops.derived(self).get("scan", [self.x_proj_weight, self.dt_projs_weight, self.dt_projs_bias, self.A_logs, self.Ds], prep)

    def tail_deferrable(self, C):
        """out_norm + out_proj + residual can run inside the kernel of the block's gdMlp branch (bem_vss_back_x6_f32): deterministic
        out_proj weights (a Bayesian leaf has one set per sample) and d_inner == d_model."""
        return type(self.out_proj) is Linear2d and self.d_inner == C

    def forward_fused(self, x, norm: LayerNorm2d, keep=False, defer_tail=False):
        """x + out_proj(out_norm(y0 + y1)), (y0, y1) = scan(SiLU(dw(in_proj(LN(x)))))  (vmamba.py:700-716 + 547-698), for every d_state.
        keep=True (the training forward, VSSBlockFn) returns (out, (t, xc, xd, xd1, y0, y1)): the intermediates the backward
        reads, y0 / y1 row-major (B, Ci, H, W).  defer_tail=True returns no output but the ``pre`` operands of ops.gdmlp_x6:
        (y0, y1, out_norm weight, bias, eps, packed row-permuted out_proj weight, out_proj bias).  With neither, d_state 1 and a plane of
        at most 256 pixels (ops.ss2d_core_small_supported) everything between in_proj and out_proj is one kernel."""
        B, C, H, W = x.shape
        Ci, R, N, L = self.d_inner, self.dt_rank, self.d_state, H * W
        M = R + 2 * N                                    # x_dbl rows per direction: [dt_0..dt_{R-1} | B_0..B_{N-1} | C_0..C_{N-1}]
        wall, dtw, dtb, A, Ds, xrows = self._scan_params()
        on = self.out_norm
        # Bayesian leaves draw when they are asked, and their Philox streams follow the asking order in_proj, conv2d, out_proj (DESIGN.md
        # section 4.2): both are asked here, ahead of every launch of this forward, and in_proj's answer is handed on to ag.ln_pw
        ip = self.in_proj.gemm_weights(B)
        w, bw = self.conv2d.dw_weights(B)
        # small planes (Stage I's 16x16 .. 4x4 maps): depthwise conv + SiLU, x_proj and the four scans in one kernel with a sample's planes
        # in LDS (bem_ss2d_core_small_f32) -- no xc, x_dbl or transposed plane in memory, one y instead of y0 / y1.  The fused tail
        # (defer_tail) and the training forward (keep) need y0 / y1 and keep the chain.
        if ops.USE_SS2D_CORE and not keep and not defer_tail and ops.ss2d_core_small_supported(Ci, H, W, R, N):
            y = ops.ss2d_core_small(ag.ln_pw(x, norm, self.in_proj, asked=ip), w, bw, xrows, dtw, dtb, A, Ds)
            return ag.ln_pw(y, on, self.out_proj, res=x)
        # row-major scan (d_state = 1): no transposed copy of xc, y1 comes back row-major (the column orientation goes through LDS)
        rm = N == 1 and ops.ss2d_scan_rm_supported(H, W, R)
        # LayerNorm + in_proj + depthwise 3x3 + SiLU + x_proj in one kernel (bem_ss2d_front_x6_f32).  The in_proj output t stays in
        # LDS, so never with keep.  At d_state = 1 it is taken only ahead of the row-major scan: it was wired into that branch
        # alone when it was added, no reason for leaving the transposed-plane scan out is recorded; d_state > 1 has no such condition.
        front = not keep and (rm or N > 1) and ops.ss2d_front_supported(C, 4 * M) and Ci == C \
            and type(self.in_proj) is Linear2d and type(self.conv2d) is DwConv2d
        t = None
        if front:
            xc, xd = ops.ss2d_front(x, norm.weight.detach(), norm.bias.detach(), norm.eps, *ip, w, bw, wall, 4 * M)
        else:
            t = ag.ln_pw(x, norm, self.in_proj, asked=ip)
            xc = ops.dwconv3x3(t, w, bw, mode=1)
            xd = ops.pw_gemm(xc, wall, 4 * M)            # (B, 4M, H, W), rows [dir 0 | dir 2 | dir 1 | dir 3]
        # x_dbl of the column-major directions = the row-major GEMM's rows in transposed pixel order: 2M planes to transpose
        # instead of a second GEMM pass over the C planes of xcT
        xd1 = ops.transpose_plane_slice(xd, 2 * M, 2 * M)                             # (B, 2M, W, H)
        xd0v, xd1v = xd.view(B, 4, M, L)[:, :2], xd1.view(B, 2, M, L)
        if rm:
            y0, y1 = ops.ss2d_scan_rm(xc, xd0v, xd1v, dtw, dtb, A, Ds)
        else:
            x0, x1 = xc.view(B, Ci, L), ops.transpose_planes(xc).view(B, Ci, L)
            if N > 1:
                y0, y1 = ops.ss2d_scan_n(x0, x1, xd0v, xd1v, dtw, dtb, A, Ds)
            else:
                y0, y1 = ops.ss2d_scan(x0, x1, xd0v, xd1v, dtw, dtb, A, Ds)
            y0, y1 = y0.view(B, Ci, H, W), ops.transpose_planes(y1.view(B, Ci, W, H))
        if defer_tail:
            op = self.out_proj
            Wpp = ops.derived(self).get("vss_back", [op.weight], lambda: ops.pack_vss_back_outproj(op.weight.detach()))
            return y0, y1, on.weight.detach(), on.bias.detach(), on.eps, Wpp, (op.bias.detach() if op.bias is not None else None)
        out = ag.ln_pw(y0, on, self.out_proj, x2=y1, in_mode=1, res=x)
        return (out, (t, xc, xd, xd1, y0, y1)) if keep else out

    def forward(self, x):
        raise BemNativeError("SS2D runs fused with its VSSBlock (norm prologue + residual epilogue); call the block")


class VSSBlock(nn.Module):
    def __init__(self, hidden_dim=0, drop_path=0.0, norm_layer=LayerNorm2d, channel_first=True, ssm_d_state=16,
                 ssm_ratio=2.0, ssm_dt_rank="auto", ssm_act_layer=nn.SiLU, ssm_conv=3, ssm_conv_bias=True,
                 ssm_drop_rate=0.0, ssm_init="v0", forward_type="v2", mlp_ratio=4.0, mlp_act_layer=nn.GELU,
                 mlp_drop_rate=0.0, mlp_type="mlp", use_checkpoint=False, post_norm=False, grid_size=None, **kwargs):
        super().__init__()
        if post_norm or grid_size or drop_path or mlp_type != "gdmlp" or not channel_first:
            raise NotImplementedError("VSSBlock: only pre-norm, gdmlp, channel-first, drop_path=0 are on the BEM path")
        self.norm = LayerNorm2d(hidden_dim)
        self.op = SS2D(d_model=hidden_dim, d_state=ssm_d_state, ssm_ratio=ssm_ratio, dt_rank=ssm_dt_rank,
                       act_layer=ssm_act_layer, d_conv=ssm_conv, conv_bias=ssm_conv_bias, dropout=ssm_drop_rate,
                       initialize=ssm_init, forward_type=forward_type, channel_first=channel_first)
        self.drop_path = nn.Identity()
        self.norm2 = LayerNorm2d(hidden_dim)
        self.mlp = gdMlp(in_features=hidden_dim, hidden_features=int(hidden_dim * mlp_ratio), act_layer=mlp_act_layer,
                         drop=mlp_drop_rate, channels_first=channel_first)

    def forward(self, x):
        _need_cuda(x)
        if grad_mode(self):
            return ag.vssblock(self, x)
        x = x.contiguous()
        C = x.shape[1]
        # the SS2D tail inside the gdMlp kernel: x1 = x + out_proj(out_norm(y0 + y1)) is never written
        if ops.USE_VSS_BACK and self.op.tail_deferrable(C) and self.mlp.fused_supported(C) \
                and ops.vss_back_supported(C, self.mlp.project_in.out_channels // 2, x.shape[2] * x.shape[3]):
            return self.mlp.forward_fused(x, self.norm2, pre=self.op.forward_fused(x, self.norm, defer_tail=True))
        x = self.op.forward_fused(x, self.norm)
        return self.mlp.forward_fused(x, self.norm2)


def make_vss_level(dim, num_block, d_state, ssm_ratio, mlp_ratio, mlp_type):
    return nn.Sequential(*[VSSBlock(hidden_dim=dim, drop_path=0, norm_layer=LayerNorm2d, channel_first=True,
                                    ssm_d_state=d_state, ssm_ratio=ssm_ratio, ssm_dt_rank="auto", ssm_act_layer=nn.SiLU,
                                    ssm_conv=3, ssm_conv_bias=False, ssm_drop_rate=0, ssm_init="v0",
                                    forward_type="v05_noz", mlp_ratio=mlp_ratio, mlp_act_layer=nn.GELU,
                                    mlp_drop_rate=0.0, mlp_type=mlp_type, use_checkpoint=False, post_norm=False)
                           for _ in range(num_block)])
