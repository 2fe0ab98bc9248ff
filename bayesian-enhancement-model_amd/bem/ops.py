"""Tensor-level wrappers over the C ABI (include/bem_hip.h).

Each wrapper checks operand shapes on the host before anything is launched (a kernel fault can take
the whole GPU host down), allocates the output with torch (device memory is torch's job here) and
launches on torch's current stream.  No wrapper computes anything itself: the constant tables some kernels read are built by
bem.tables (numpy, on the host) and uploaded once per device (``_tables``); scratch buffers that outlive a call are kept per stream
(``_scratch``), all others are allocated by the call."""
from __future__ import annotations

import ctypes
import os
from inspect import signature as _signature
from functools import wraps as _wraps
from math import prod as _prod
from typing import Optional

import torch

from . import native
from .native import PwArgs, check, lib
from .tables import UIQM_WIDTH, lab_tables, niqe_gamma_table, niqe_resize_table, pil_resize_table, uiqm_resized_rows  # noqa: F401  (host builders; callers of ops.<name> keep working)


_U64 = (1 << 64) - 1


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _chk(t: Optional[torch.Tensor], name: str, dtype=torch.float32, optional=False):
    if t is None:
        if optional:
            return
        raise ValueError(f"{name} is required")
    if not t.is_cuda:
        raise native.BemNativeError(f"{name} must be a CUDA/HIP tensor: the BEM hot path has no CPU implementation")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


# --------------------------------------------------------------------------- launch timing ----
# bench.py asks for ONE op's launches to be bracketed by HIP events on the launch stream (torch's
# current stream is the stream every wrapper launches on), together with that launch's algorithmic
# bytes / flops.  Disabled (one None test and one Python frame per bracketed op) outside bench.py.
_PROF = None
# profile key -> (op wrapper it belongs to, roofline bound, kernel symbol reported to bench.py, predicate on the call)
_KEYS = {
    # the register-resident x6 GEMM for K <= 48 (level-0 in_proj / project_in / x_proj and the small Stage-I layers):
    # every launch of the (vectorised, single-input or concat) instance, whatever M and L
    "pw_x6_res<3,2,1>": ("pw_gemm", "hbm", "pw_x6_res_kernel<3, 2, 1, false, true>",
                         lambda K, M, ln, L, mode: K <= 48 and L % 2 == 0 and mode != 1),
    # the streaming x6 GEMM with two M-tiles per pass (project_out / out_proj / fuse 1x1 at K > 48 without LayerNorm):
    # the kernel with the largest share of the step in profiles/r01_bench_kernel_stats.csv
    "pw_x6_stream<2>": ("pw_gemm", "hbm", "pw_x6_stream_kernel<2, 2, false, true, false>",
                        lambda K, M, ln, L, mode: K > 48 and not ln and M > 32 and L % 2 == 0 and mode != 1),
    "pw_gemm": ("pw_gemm", "mfma", "pw_gemm* (all variants)", lambda K, M, ln, L, mode: True),
    # the whole gdMlp branch in one kernel: x in, out out -- 8 bytes per element of x are its algorithmic bytes
    # (HBM: 42 us at level 0) -- but its two GEMMs (2Hd x C and C x Hd per pixel) evaluated as six bf16 limb products are 242 GFLOP on the
    # matrix cores (97 us at the dense bf16 peak): the matrix pipe is the roofline that bounds it.  flops = 6 x the f32 GEMM flops
    # (what the x6 scheme must issue for the output pixels; halo and padding MFMAs are waste, not work).
    # In the eval step the level-0 launches carry the SS2D tail as well (``pre``): vss_back_x6_kernel, + y0, y1 in and the C x C out_proj GEMM.
    "gdmlp_x6<3>": ("gdmlp_x6", "mfma_bf16", "vss_back_x6_kernel<3, 2, 2> (with the SS2D tail; gdmlp_x6_kernel<3, 2, 2, false> without)", lambda C: 32 < C <= 48),
    "gdmlp_x6<5>": ("gdmlp_x6", "mfma_bf16", "gdmlp_x6_kernel<5, 3, 1, false>", lambda C: 64 < C <= 80),
    "conv2d": ("conv2d", "mfma", "conv2d_kernel", None),
    "dwconv3x3": ("dwconv3x3", "hbm", "dwconv3x3_kernel", None),
    "ss2d_scan": ("ss2d_scan", "hbm", "ss2d_scan_kernel", None),
    "transpose_planes": ("transpose_planes", "hbm", "transpose_planes_kernel", None),
    # a decoder level's up + fuse as one kernel: f in, skip in, out out are its algorithmic bytes
    "up_fuse": ("up_fuse", "hbm", "upfuse_x6_kernel<2>", None),
    # training step (bench.py --config train)
    "pw_wgrad": ("pw_wgrad_", "hbm", "wgrad_x6_kernel<2, 2> + wgrad_x6_reduce_kernel (1x1 weight gradients; wgrad_kernel<*> for L % 32 != 0)", None),
    "conv_wgrad": ("conv_wgrad_", "mfma", "wgrad_kernel<*> (dense conv weight gradients)", None),
    "ss2d_scan_bwd": ("ss2d_scan_bwd", "hbm", "ss2d_scan_bwd_kernel", None),
    "dwact_bwd": ("dwact_bwd", "hbm", "dwact_bwd_kernel", None),
    "ln_bwd": ("ln_bwd", "hbm", "ln_bwd_kernel", None),
}


def profile_start(key: str):
    global _PROF
    if key not in _KEYS:
        raise ValueError(f"profile_start: unknown key {key}; choose from {sorted(_KEYS)}")
    op, bound, symbol, pred = _KEYS[key]
    _PROF = {"kernel": op, "symbol": symbol, "bound": bound, "pred": pred, "events": [], "bytes": 0.0, "flops": 0.0}


def profile_stop():
    global _PROF
    p, _PROF = _PROF, None
    if p is None:
        return None
    torch.cuda.synchronize()
    ms = sum(s.elapsed_time(e) for s, e in p["events"])
    return {"kernel": p["symbol"], "bound": p["bound"], "launches": len(p["events"]), "ms": ms,
            "bytes": p["bytes"], "flops": p["flops"]}


def _bracket(cost, sees=None):
    """Makes an op one that a profile key (_KEYS) can time.  ``cost`` and ``sees`` are handed the call's arguments by the op's own
    parameter names, defaults filled in, and name the ones they read (``**_`` takes the rest): cost returns the (algorithmic bytes,
    flops) of the call, sees the tuple handed to the key's predicate (keys without a predicate count every call)."""
    def deco(fn):
        name, sig = fn.__name__, _signature(fn)
        if sees is None and any(op == name and pred is not None for op, _, _, pred in _KEYS.values()):
            raise TypeError(f"_bracket: a key of {name} has a predicate, so the op needs ``sees``")

        @_wraps(fn)
        def op(*a, **kw):
            p = _PROF
            if p is None or p["kernel"] != name:
                return fn(*a, **kw)
            args = sig.bind(*a, **kw)
            args.apply_defaults()
            if p["pred"] is not None and not p["pred"](*sees(**args.arguments)):
                return fn(*a, **kw)
            nb, nf = cost(**args.arguments)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = fn(*a, **kw)
            e.record()
            p["bytes"] += nb
            p["flops"] += nf
            p["events"].append((s, e))
            return out
        return op
    return deco


# ----------------------------------------------------------------- cached device memory ----
_SCRATCH = {}            # (tag, device, stream) -> a kernel's scratch buffer
_TABLES = {}             # (key, device) -> constant table(s) of bem.tables on the device


def _scratch(tag, device, n, dtype):
    """The scratch buffer ``tag`` of at least n elements for a launch on ``device``'s current stream.  Launches on one stream are ordered, so
    they share one buffer, which grows and never shrinks; another stream (or another tag) gets its own, so two streams never meet in one."""
    key = (tag, str(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _SCRATCH.get(key)
    if ws is None or ws.numel() < n:
        ws = _SCRATCH[key] = torch.empty(n, device=device, dtype=dtype)
    return ws


def _tables(key, device, build):
    """What ``build()`` returns (one numpy array or a tuple of them), uploaded once per device."""
    k = (key, str(device))
    if k not in _TABLES:
        t = build()
        _TABLES[k] = tuple(torch.from_numpy(a).to(device) for a in t) if isinstance(t, tuple) else torch.from_numpy(t).to(device)
    return _TABLES[k]


_GRID_MAX = 65535        # the y and z extent of a launch grid: planes, candidates (x 3 channels) or images go there
# The tile kernels (gdmlp_x6, ss2d_front) address one image's planes with 32-bit byte offsets below _TILE_NARROW elements and with 64-bit
# ones up to _TILE_MAX, where the int pixel indices end; the library states the same two bounds (gdmlp_x6.hip, ss2d_front_x6.hip).
_TILE_NARROW, _TILE_MAX = 1 << 30, 1 << 31


def _tile_plane_set(op, elems):
    """Refuses a plane set the tile kernels cannot index, with the library's message, before anything is allocated for it."""
    if elems >= _TILE_MAX:
        raise native.BemNativeError(f"{op}: plane set too large for 32-bit offsets ({elems} elements per image, at most {_TILE_MAX - 1})")


def _pslice(t, c0):
    """Channel c0 of a contiguous float32 (B, Ct, *spatial) tensor as a pointer, and the tensor's batch stride in elements."""
    Ct = t.shape[1]
    if not 0 <= c0 <= Ct:
        raise ValueError(f"channel offset {c0} outside a tensor of {Ct} channels")
    L = _prod(t.shape[2:])
    return ctypes.c_void_p(t.data_ptr() + 4 * c0 * L), Ct * L


# --------------------------------------------------------------------------- operator seam ----
def selective_scan_fwd(u, delta, A, B, C, D=None, delta_bias=None, delta_softplus=True):
    """u, delta (Bt,KC,L); A (KC,N); B, C (Bt,K,N,L); D, delta_bias (KC) -> y (Bt,KC,L) f32."""
    for n, t in (("u", u), ("delta", delta), ("A", A), ("B", B), ("C", C)):
        _chk(t, n)
    _chk(D, "D", optional=True)
    _chk(delta_bias, "delta_bias", optional=True)
    Bt, KC, L = u.shape
    if delta.shape != u.shape:
        raise ValueError(f"delta {tuple(delta.shape)} != u {tuple(u.shape)}")
    if B.dim() != 4 or B.shape[0] != Bt or B.shape[3] != L or C.shape != B.shape:
        raise ValueError(f"B/C must be (batch, groups, dstate, L); got {tuple(B.shape)} {tuple(C.shape)}")
    K, N = B.shape[1], B.shape[2]
    if A.shape != (KC, N):
        raise ValueError(f"A must be ({KC},{N}), got {tuple(A.shape)}")
    if KC % K:
        raise ValueError("dim must be a multiple of the number of groups")
    for n, t in (("D", D), ("delta_bias", delta_bias)):
        if t is not None and t.shape != (KC,):
            raise ValueError(f"{n} must be ({KC},)")
    out = torch.empty_like(u)
    check(lib().bem_selective_scan_fwd_f32(_p(u), _p(delta), _p(A), _p(B), _p(C), _p(D), _p(delta_bias), _p(out),
                                           Bt, KC, L, N, K, int(bool(delta_softplus)), _stream()), "selective_scan_fwd")
    return out


def selective_scan_bwd(u, delta, A, B, C, D, delta_bias, dout, delta_softplus=True):
    """Gradients (du, ddelta, dA, dB, dC, dD|None, ddelta_bias|None) of selective_scan_fwd w.r.t. its inputs."""
    for n, t in (("u", u), ("delta", delta), ("A", A), ("B", B), ("C", C), ("dout", dout)):
        _chk(t, n)
    _chk(D, "D", optional=True); _chk(delta_bias, "delta_bias", optional=True)
    Bt, KC, L = u.shape
    K, N = B.shape[1], B.shape[2]
    if delta.shape != u.shape or dout.shape != u.shape or A.shape != (KC, N) or C.shape != B.shape or B.shape[0] != Bt or B.shape[3] != L or KC % K:
        raise ValueError("selective_scan_bwd: shapes")
    du, dd = torch.empty_like(u), torch.empty_like(u)
    dA, dB, dC = torch.empty_like(A), torch.empty_like(B), torch.empty_like(C)
    dD = torch.empty_like(D) if D is not None else None
    db = torch.empty_like(delta_bias) if delta_bias is not None else None
    ws = torch.empty(int(lib().bem_selective_scan_bwd_ws_elems(Bt, KC, L, N)), device=u.device, dtype=torch.float32)
    check(lib().bem_selective_scan_bwd_f32(_p(u), _p(delta), _p(A), _p(B), _p(C), _p(D), _p(delta_bias), _p(dout), _p(ws), _p(du), _p(dd),
                                           _p(dA), _p(dB), _p(dC), _p(dD), _p(db), Bt, KC, L, N, K, int(bool(delta_softplus)), _stream()),
          "selective_scan_bwd")
    return du, dd, dA, dB, dC, dD, db


def cross_scan(x):
    _chk(x, "x")
    B, C, H, W = x.shape
    xs = torch.empty(B, 4, C, H * W, device=x.device, dtype=x.dtype)
    check(lib().bem_cross_scan_f32(_p(x), _p(xs), B, C, H, W, _stream()), "cross_scan")
    return xs


def cross_merge(ys):
    _chk(ys, "ys")
    B, K, C, H, W = ys.shape
    if K != 4:
        raise ValueError("cross_merge expects 4 directions")
    y = torch.empty(B, C, H * W, device=ys.device, dtype=ys.dtype)
    check(lib().bem_cross_merge_f32(_p(ys), _p(y), B, C, H, W, _stream()), "cross_merge")
    return y


# --------------------------------------------------------------------------- fused SS2D -------
def ss2d_scan_n_supported(N):
    return bool(lib().bem_ss2d_scan_n_supported(int(N)))


def _scan_operands(op, n_from_A, acts, xd0, xd1, dtw, dtb, A, Ds, grads=None):
    """The operand checks of every SS2D scan wrapper; returns (B, C, L, R, N, batch stride of xd0, of xd1).
    acts: (name, tensor) pairs, all (B,C,L) (x0, x1 and, backward, dy0, dy1).  xd0 / xd1 (B,2,R+2N,L): contiguous, or channel slices
    of a wider (B,*,L) buffer, whose batch stride is taken from the view.  n_from_A: A is (4C, N) and gives the d_state; otherwise A
    holds 4C elements and N = 1.  grads: the accumulators (dAlog, dDs, ddtw, ddtb) of a backward."""
    params = (("dtw", dtw), ("dtb", dtb), ("A", A), ("Ds", Ds))
    if grads is not None:
        params += tuple(zip(("dAlog", "dDs", "ddtw", "ddtb"), grads))
    for n, t in acts + params:
        _chk(t, n)
    x = acts[0][1]
    B, C, L = x.shape
    R, N = dtw.shape[2], 1
    if n_from_A:
        if A.dim() != 2 or A.shape[0] != 4 * C:
            raise ValueError(f"{op}: A {tuple(A.shape)} is not (4C, N)")
        N = A.shape[1]
        if not ss2d_scan_n_supported(N):
            raise NotImplementedError(f"{op}: d_state {N} outside 1..16")
    rows = R + 2 * N
    if any(t.shape != x.shape for _, t in acts) or xd0.shape != (B, 2, rows, L) or xd1.shape != xd0.shape:
        raise ValueError(f"{op}: activation shapes: {[tuple(t.shape) for _, t in acts]} xd {tuple(xd0.shape)}/{tuple(xd1.shape)} R={R} N={N}")
    if dtw.shape != (4, C, R) or dtb.shape != (4, C) or A.numel() != 4 * C * N or Ds.numel() != 4 * C:
        raise ValueError(f"{op}: parameter shapes")
    if grads is not None and [g.numel() for g in grads] != [4 * C * N, 4 * C, 4 * C * R, 4 * C]:
        raise ValueError(f"{op}: gradient accumulator sizes")
    bs = []
    for n, t in (("xd0", xd0), ("xd1", xd1)):
        if not t.is_cuda or t.dtype != torch.float32:
            raise native.BemNativeError(f"{n} must be a float32 CUDA/HIP tensor")
        if t.stride()[1:] != (rows * L, L, 1) or (B > 1 and (t.stride(0) < 2 * rows * L or (L % 4 == 0 and t.stride(0) % 4))):
            raise ValueError(f"{op}: {n}: only the batch stride may differ from a contiguous (B,2,R+2N,L) tensor")
        bs.append(t.stride(0) if B > 1 else 0)
    return B, C, L, R, N, bs[0], bs[1]


@_bracket(lambda x0, xd0, **_: (4.0 * (2 * x0.numel() + 2 * xd0.numel() + 2 * x0.numel()), 0.0))
def ss2d_scan(x0, x1, xd0, xd1, dtw, dtb, A, Ds):
    """xd0 / xd1 (B,2,R+2,L): contiguous, or channel slices of a wider (B,*,L) buffer (batch stride taken from the view)."""
    B, C, L, R, _, bs0, bs1 = _scan_operands("ss2d_scan", False, (("x0", x0), ("x1", x1)), xd0, xd1, dtw, dtb, A, Ds)
    y0, y1 = torch.empty_like(x0), torch.empty_like(x0)
    check(lib().bem_ss2d_scan_strided_f32(_p(x0), _p(x1), _p(xd0), _p(xd1), _p(dtw), _p(dtb), _p(A), _p(Ds), _p(y0), _p(y1),
                                          B, C, L, R, bs0, bs1, _stream()), "ss2d_scan")
    return y0, y1


def ss2d_scan_n(x0, x1, xd0, xd1, dtw, dtb, A, Ds):
    """d_state N form of ss2d_scan (bem_ss2d_scan_n_f32): xd0 / xd1 (B,2,R+2N,L) with rows [dt | B_0..B_{N-1} | C_0..C_{N-1}]
    (contiguous or batch-strided channel slices), A (4C, N) = -exp(A_logs)."""
    B, C, L, R, N, bs0, bs1 = _scan_operands("ss2d_scan_n", True, (("x0", x0), ("x1", x1)), xd0, xd1, dtw, dtb, A, Ds)
    y0, y1 = torch.empty_like(x0), torch.empty_like(x0)
    check(lib().bem_ss2d_scan_n_f32(_p(x0), _p(x1), _p(xd0), _p(xd1), _p(dtw), _p(dtb), _p(A), _p(Ds), _p(y0), _p(y1),
                                    B, C, L, R, N, bs0, bs1, _stream()), "ss2d_scan_n")
    return y0, y1


def ss2d_scan_rm_supported(H, W, R):
    return bool(lib().bem_ss2d_scan_rm_supported(H, W, R))


def ss2d_scan_rm(x, xd0, xd1, dtw, dtb, A, Ds):
    """Row-major form: x (B,C,H,W); xd0 (B,2,R+2,L) row-major order, xd1 (B,2,R+2,L) transposed pixel order (either may be
    a batch-strided channel slice); returns y0, y1 both (B,C,H,W) row-major."""
    for n, t in (("x", x), ("dtw", dtw), ("dtb", dtb), ("A", A), ("Ds", Ds)):      # a wrong tensor is reported before an unsupported plane
        _chk(t, n)
    B, C, H, W = x.shape
    if not ss2d_scan_rm_supported(H, W, dtw.shape[2]):
        raise ValueError(f"ss2d_scan_rm: plane {H}x{W} / dt_rank {dtw.shape[2]} not supported")
    _, _, _, R, _, bs0, bs1 = _scan_operands("ss2d_scan_rm", False, (("x", x.view(B, C, H * W)),), xd0, xd1, dtw, dtb, A, Ds)
    y0, y1 = torch.empty_like(x), torch.empty_like(x)
    check(lib().bem_ss2d_scan_rm_f32(_p(x), _p(xd0), _p(xd1), _p(dtw), _p(dtb), _p(A), _p(Ds), _p(y0), _p(y1), B, C, H, W, R, bs0, bs1, _stream()),
          "ss2d_scan_rm")
    return y0, y1


# SS2D's conv + x_proj + scans as one kernel on small planes (bem_ss2d_core_small_f32): a test reaches the six-launch chain by switching it off.
USE_SS2D_CORE = True


def ss2d_core_small_supported(C, H, W, R, N=1):
    """d_state N = 1, H W <= 256 and a sample's planes within one CU's LDS (the library states the exact bound)."""
    return N == 1 and bool(lib().bem_ss2d_core_small_supported(int(C), int(H), int(W), int(R)))


def ss2d_core_small(t, dww, dwb, xw, dtw, dtb, A, Ds):
    """t (B,C,H,W) -> y (B,C,H,W) = (y_dir0 + y_dir2) + (y_dir1 + y_dir3) of the four-direction scan over xc = SiLU(dw3x3(t) + dwb) with
    x_dbl = xw xc, in one launch.  dww (C,1,3,3) or (B,C,1,3,3), dwb (C) | (B,C) | None as for dwconv3x3; xw (4(R+2),C) the raw x_proj rows
    in the order [dir 0 | dir 2 | dir 1 | dir 3]; dtw (4,C,R), dtb (4,C), A (4C), Ds (4C)."""
    for n, v in (("t", t), ("dww", dww), ("xw", xw), ("dtw", dtw), ("dtb", dtb), ("A", A), ("Ds", Ds)):
        _chk(v, n)
    _chk(dwb, "dwb", optional=True)
    B, C, H, W = t.shape
    if dtw.dim() != 3 or dtw.shape[:2] != (4, C):
        raise ValueError(f"ss2d_core_small: dtw {tuple(dtw.shape)} is not (4, {C}, R)")
    R = dtw.shape[2]
    if not ss2d_core_small_supported(C, H, W, R, 1 if A.dim() == 1 else A.shape[1]):
        raise ValueError(f"ss2d_core_small: C = {C}, plane {H}x{W}, dt_rank {R} not supported")
    per_b = dww.dim() == 5
    if tuple(dww.shape[-4:]) != (C, 1, 3, 3) or (per_b and dww.shape[0] != B) or dww.dim() not in (4, 5):
        raise ValueError(f"ss2d_core_small: depthwise weight {tuple(dww.shape)} vs {C} channels, batch {B}")
    bb = 0
    if dwb is not None:
        if dwb.shape[-1] != C or dwb.dim() > 2 or (dwb.dim() == 2 and dwb.shape[0] not in (1, B)):
            raise ValueError("ss2d_core_small: bias shape")
        bb = C if (dwb.dim() == 2 and dwb.shape[0] == B and B > 1) else 0
    if xw.shape != (4 * (R + 2), C) or dtb.shape != (4, C) or A.numel() != 4 * C or Ds.numel() != 4 * C:
        raise ValueError("ss2d_core_small: parameter shapes")
    y = torch.empty_like(t)
    check(lib().bem_ss2d_core_small_f32(_p(t), _p(dww), (C * 9 if per_b else 0), _p(dwb), bb, _p(xw), _p(dtw), _p(dtb), _p(A), _p(Ds), _p(y),
                                        B, C, H, W, R, _stream()), "ss2d_core_small")
    return y


def _transpose(src, src_c0, C, dst=None, dst_c0=0):
    """dst[:, dst_c0:dst_c0+C] (B,*,W,H) = the planes of src[:, src_c0:src_c0+C] (B,*,H,W) transposed.  The planes of a launch go into
    gridDim.z: one launch per _GRID_MAX // C batch rows.  C None: every channel from src_c0 on; dst None: a new (B,C,W,H) tensor.  Returns dst."""
    _chk(src, "src")
    B, Cs, H, W = src.shape
    C = Cs - src_c0 if C is None else C
    if C < 0 or src_c0 < 0 or src_c0 + C > Cs:
        raise ValueError(f"transpose_planes: channels [{src_c0}, {src_c0 + C}) of a source with {Cs}")
    if C > _GRID_MAX:
        raise ValueError(f"transpose_planes: at most {_GRID_MAX} planes per batch row, got {C}")
    if dst is None:
        dst = torch.empty(B, C, W, H, device=src.device, dtype=src.dtype)
    _chk(dst, "dst")
    if dst.dim() != 4 or dst.shape[0] != B or tuple(dst.shape[2:]) != (W, H) or dst_c0 < 0 or dst_c0 + C > dst.shape[1]:
        raise ValueError(f"transpose_planes: {C} transposed planes of src {tuple(src.shape)} do not fit dst {tuple(dst.shape)} at channel {dst_c0}")
    (sp, sbs), (dp, dbs) = _pslice(src, src_c0), _pslice(dst, dst_c0)
    step = _GRID_MAX // max(C, 1)
    for b0 in range(0, max(B, 1), step):
        check(lib().bem_transpose_planes_f32(ctypes.c_void_p((sp.value or 0) + 4 * b0 * sbs), sbs, ctypes.c_void_p((dp.value or 0) + 4 * b0 * dbs), dbs,
                                             min(step, B - b0), C, H, W, _stream()), "transpose_planes")
    return dst


def transpose_plane_slice(x, c0, C):
    """x (B,Ct,H,W) contiguous -> transposed planes of channels [c0, c0+C): (B,C,W,H) contiguous."""
    return _transpose(x, c0, C)


def transpose_planes_into(src, dst, dst_c0):
    """dst[:, dst_c0:dst_c0+C] = src.transpose(2, 3) for src (B,C,H,W) and dst (B,*,W,H), both contiguous; dst's other channels stay."""
    return _transpose(src, 0, None, dst, dst_c0)


# --------------------------------------------------------------------------- pointwise GEMM ---
# Two packed operand formats: "x6" (three bf16 limbs per f32 value, six limb products on v_mfma_f32_32x32x16_bf16, bem_pw_gemm_x6_f32 --
# f32-level error at 6/16 of the f32 matrix-pipe cost), what every pointwise GEMM consumes; and "f32" (v_mfma_f32_32x32x2_f32 operand
# order, pack_pw_weight(x6=False)), the weight format of the implicit-GEMM convolutions (ConvWeight.f32).
# Bumped whenever parameters are rewritten behind torch's back (the fused optimizer step, bem.train.BemAdamW): every Derived
# cache (packed / transposed / flipped copies of weights) is keyed on it as well as on the tensors' data_ptr / _version.
WEIGHT_EPOCH = [0]


def bump_weight_epoch():
    WEIGHT_EPOCH[0] += 1


def tensor_version(t) -> int:
    """t._version for cache keys; tensors created under torch.inference_mode() (the reference's eval.py runs there) carry no
    version counter and cannot be modified in place later, so a constant serves."""
    return -1 if t.is_inference() else t._version


class Derived:
    """The tensors one holder derives from its parameters: packed, transposed, flipped or folded copies.  An entry is valid for one
    weight epoch and one (data_ptr, version, device) of each source; a changed signature replaces it, which frees the old value."""

    def __init__(self):
        self.d = {}

    @staticmethod
    def _sig(srcs):
        return (WEIGHT_EPOCH[0],) + tuple((t.data_ptr(), tensor_version(t), t.device) for t in srcs)

    def get(self, key, srcs, fn):
        sig = self._sig(srcs)
        hit = self.d.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1]
        with torch.no_grad():
            val = fn()
        self.d[key] = (sig, val)
        return val

    def put(self, key, srcs, val):
        """Store a value made elsewhere (BayesBank packs all its leaves' operands in one launch) as ``get(key, srcs, ...)`` would."""
        self.d[key] = (self._sig(srcs), val)


def derived(holder) -> Derived:
    """The one Derived cache of a module (or any object), created on first use; it is no parameter, buffer or submodule."""
    c = holder.__dict__.get("_derived")
    if c is None:
        c = holder.__dict__["_derived"] = Derived()
    return c


def packed_elems(M: int, K: int, x6: bool = False) -> int:
    return int(lib().bem_pw_x6_packed_elems(M, K) if x6 else lib().bem_pw_packed_elems(M, K))


def pack_pw_weight(W, x6=True):
    """(M,K) or (nsets,M,K) natural weights -> packed MFMA operand order, shape (nsets, packed).
    x6: True = bf16-limb operands (every pointwise GEMM), False = f32 operands (what the MFMA convolution consumes)."""
    if W.dim() == 2:
        W = W[None]
    ns, M, K = W.shape
    out = torch.empty(ns, packed_elems(M, K, x6), device=W.device, dtype=W.dtype)
    if x6 and not W.is_contiguous():            # a transposed / sliced view (W^T of an input-gradient GEMM): packed where it lies
        if not W.is_cuda or W.dtype != torch.float32:
            raise native.BemNativeError("pack_pw_weight: a float32 CUDA/HIP tensor")
        check(lib().bem_pack_pw_weight_x6_strided(_p(W), _p(out), ns, M, K, W.stride(0), W.stride(1), W.stride(2), _stream()), "pack_pw_weight")
        out._bem_mk = (M, K)
        return out
    _chk(W, "W")
    fn = lib().bem_pack_pw_weight_x6 if x6 else lib().bem_pack_pw_weight_f32
    check(fn(_p(W), _p(out), ns, M, K, _stream()), "pack_pw_weight")
    out._bem_mk = (M, K)          # the x6 size only pins ceil(K/16): keep the exact logical shape for pw_gemm's check
    return out


def _pw_gemm_sees(x1, M, x2, in_mode, ln, **_):
    return x1.shape[1] + (x2.shape[1] if in_mode == 2 else 0), M, ln is not None, x1[0, 0].numel(), in_mode


def _pw_gemm_cost(x1, Wp, M, x2, in_mode, res, **_):
    B, L = x1.shape[0], x1[0, 0].numel()
    C2 = 0 if x2 is None else x2.shape[1]
    K = x1.shape[1] + (C2 if in_mode == 2 else 0)
    return 4.0 * B * L * (x1.shape[1] + C2 + M + (M if res is not None else 0)) + 4.0 * Wp.numel(), 2.0 * M * K * L * B


@_bracket(_pw_gemm_cost, _pw_gemm_sees)
def pw_gemm(x1, Wp, M, *, x2=None, in_mode=0, ln=None, ln_eps=1e-5, bias=None, res=None, prelu=None,
            convT_Win: int = 0, out=None):
    """x1 (B,C1,*spatial); Wp packed (1|B, packed(M,K)); returns (B,M,*spatial) (or (B,M/4,2H,2W) for convT)."""
    _chk(x1, "x1"); _chk(Wp, "Wp"); _chk(x2, "x2", optional=True); _chk(bias, "bias", optional=True)
    _chk(res, "res", optional=True); _chk(prelu, "prelu", optional=True)
    B, C1 = x1.shape[0], x1.shape[1]
    sp = tuple(x1.shape[2:])
    L = 1
    for s in sp:
        L *= s
    C2 = 0
    if in_mode:
        if x2 is None or x2.shape[0] != B or tuple(x2.shape[2:]) != sp:
            raise ValueError("pw_gemm: x2 shape")
        C2 = x2.shape[1]
    K = C1 + C2 if in_mode == 2 else C1
    if in_mode == 1 and C1 != C2:
        raise ValueError("pw_gemm sum mode: channel mismatch")
    if getattr(Wp, "_bem_mk", (M, K)) != (M, K):
        raise ValueError(f"pw_gemm: weights packed for (M, K) = {Wp._bem_mk}, called with M={M} K={K}")
    if Wp.dim() != 2 or Wp.shape[1] != packed_elems(M, K, True) or Wp.shape[0] not in (1, B):
        raise ValueError(f"pw_gemm: packed weight shape {tuple(Wp.shape)} does not match M={M} K={K} B={B} (x6 format, pack_pw_weight)")
    a = PwArgs()
    a.x1, a.x2, a.C1, a.C2, a.in_mode = x1.data_ptr(), (x2.data_ptr() if x2 is not None else 0), C1, C2, in_mode
    if ln is not None:
        lw, lb = ln
        _chk(lw, "ln_w"); _chk(lb, "ln_b")
        if lw.numel() != K or lb.numel() != K:
            raise ValueError("pw_gemm: LayerNorm size != K")
        a.ln_w, a.ln_b = lw.data_ptr(), lb.data_ptr()
    a.ln_eps = ln_eps
    a.Wp, a.w_bstride = Wp.data_ptr(), (Wp.shape[1] if Wp.shape[0] > 1 else 0)
    if bias is not None:
        if bias.shape[-1] != M or (bias.dim() == 2 and bias.shape[0] not in (1, B)):
            raise ValueError("pw_gemm: bias shape")
        a.bias, a.bias_bstride = bias.data_ptr(), (M if (bias.dim() == 2 and bias.shape[0] > 1) else 0)
    if prelu is not None:
        if prelu.numel() != 1:
            raise ValueError("pw_gemm: PReLU with one slope only")
        a.prelu, a.act = prelu.data_ptr(), 1
    if convT_Win:
        if len(sp) != 2 or sp[1] != convT_Win or M % 4 or res is not None:
            raise ValueError("pw_gemm convT mode: bad arguments")
        oshape = (B, M // 4, 2 * sp[0], 2 * sp[1])
        a.out_mode, a.Win = 1, convT_Win
    else:
        oshape = (B, M) + sp
    if res is not None:
        if tuple(res.shape) != oshape:
            raise ValueError(f"pw_gemm: residual shape {tuple(res.shape)} != {oshape}")
        a.res = res.data_ptr()
    if out is None:
        out = torch.empty(oshape, device=x1.device, dtype=x1.dtype)
    elif tuple(out.shape) != oshape or not out.is_contiguous():
        raise ValueError("pw_gemm: out shape")
    a.out = out.data_ptr()
    a.B, a.M, a.K, a.L = B, M, K, L
    check(lib().bem_pw_gemm_x6_f32(ctypes.byref(a), _stream()), "pw_gemm")
    return out


# Reaches the unfolded decoder chain (ConvT2x2 -> concat-input 1x1 GEMM) from a test; the shipped path is the folded kernel.
USE_UPFUSE = True


class UpFuseWeights:
    """The folded operands of one decoder level (bem.modules.fold_up_fuse): Wc = pack_pw_weight of the four composed phase matrices
    (4, Cin/2, Cin), Wf2 = pack_pw_weight of the skip half of the fuse weight (Cin/2, Cin/2), bias (Cin/2) the composed bias."""

    def __init__(self, Wc, Wf2, bias, cin):
        self.Wc, self.Wf2, self.bias, self.cin = Wc, Wf2, bias, int(cin)


def _up_fuse_cost(f, skip, folded, **_):
    return 4.0 * (f.numel() + 2 * skip.numel() + folded.Wc.numel() + folded.Wf2.numel()), 2.0 * skip.numel() * (f.shape[1] + skip.shape[1])


@_bracket(_up_fuse_cost)
def up_fuse(f, skip, folded: UpFuseWeights):
    """fuse(cat(up(f), skip)) of a decoder level as one kernel: f (B,Cin,h,w), skip (B,Cin/2,2h,2w) -> (B,Cin/2,2h,2w)."""
    _chk(f, "f"); _chk(skip, "skip"); _chk(folded.Wc, "Wc"); _chk(folded.Wf2, "Wf2"); _chk(folded.bias, "bias")
    if f.dim() != 4:
        raise ValueError("up_fuse: f must be (B, Cin, h, w)")
    B, C, h, w = f.shape
    if C != folded.cin or C < 2 or C % 2:
        raise ValueError(f"up_fuse: f has {C} channels, the folded weights were made for {folded.cin} (even, >= 2)")
    Co = C // 2
    if tuple(skip.shape) != (B, Co, 2 * h, 2 * w):
        raise ValueError(f"up_fuse: skip shape {tuple(skip.shape)} != {(B, Co, 2 * h, 2 * w)}")
    if tuple(folded.Wc.shape) != (4, packed_elems(Co, C, True)) or getattr(folded.Wc, "_bem_mk", (Co, C)) != (Co, C):
        raise ValueError(f"up_fuse: Wc packed shape {tuple(folded.Wc.shape)} does not match four ({Co}, {C}) matrices")
    if tuple(folded.Wf2.shape) != (1, packed_elems(Co, Co, True)) or getattr(folded.Wf2, "_bem_mk", (Co, Co)) != (Co, Co):
        raise ValueError(f"up_fuse: Wf2 packed shape {tuple(folded.Wf2.shape)} does not match one ({Co}, {Co}) matrix")
    if folded.bias.numel() != Co:
        raise ValueError("up_fuse: bias size")
    out = torch.empty_like(skip)
    check(lib().bem_upfuse_x6_f32(_p(f), _p(skip), _p(folded.Wc), _p(folded.Wf2), _p(folded.bias), _p(out), B, C, h, w, _stream()), "up_fuse")
    return out


def empty_padded(shape, device, pad=4):
    """Contiguous float32 tensor of ``shape`` that may be read ``pad`` elements before its first and after its last element
    (it is a view into a larger allocation; the 16-byte alignment of a fresh allocation is kept for pad % 4 == 0)."""
    n = 1
    for s_ in shape:
        n *= s_
    buf = torch.empty(n + 2 * pad, device=device, dtype=torch.float32)
    return buf[pad:pad + n].view(shape)


def _chk_packed1(op, weights):
    """Each (name, Wp, M, K): Wp is ONE x6-packed (M, K) weight set (the fused kernels take no per-sample weights)."""
    for nm, Wp, M, K in weights:
        if Wp.dim() != 2 or Wp.shape[0] != 1 or Wp.shape[1] != packed_elems(M, K, True) or getattr(Wp, "_bem_mk", (M, K)) != (M, K):
            raise ValueError(f"{op}: {nm} {tuple(Wp.shape)} does not match M={M} K={K} (x6 format, one weight set)")


# SS2D front half (LayerNorm + in_proj + depthwise 3x3 + SiLU + x_proj) in one kernel, deterministic weights; wider blocks run the three-kernel chain.
def ss2d_front_supported(C, Mx):
    return C <= 48 and C % 8 == 0 and Mx <= 32


def ss2d_front(x, ln_w, ln_b, ln_eps, Wp_in, bias_in, dww, dwb, Wp_x, Mx):
    """xc = SiLU(dw3x3(in_proj(LayerNorm2d(x)))) (B,C,H,W) and xd = x_proj(xc) (B,Mx,H,W) in ONE kernel (bem_ss2d_front_x6_f32).
    Wp_in = pack_pw_weight(W_in (C,C), x6=True), Wp_x = pack_pw_weight(W_x (Mx,C), x6=True); dww (C,1,3,3) or (C,9)."""
    for n_, t in (("x", x), ("ln_w", ln_w), ("ln_b", ln_b), ("Wp_in", Wp_in), ("dww", dww), ("Wp_x", Wp_x)):
        _chk(t, n_)
    _chk(bias_in, "bias_in", optional=True); _chk(dwb, "dwb", optional=True)
    B, C, H, W = x.shape
    if not ss2d_front_supported(C, Mx):
        raise ValueError(f"ss2d_front: C = {C} (<= 48, % 8) / Mx = {Mx} (<= 32) not supported")
    if ln_w.numel() != C or ln_b.numel() != C or dww.numel() != 9 * C or (dwb is not None and dwb.numel() != C) or (bias_in is not None and bias_in.numel() != C):
        raise ValueError("ss2d_front: parameter shapes")
    _chk_packed1("ss2d_front", (("Wp_in", Wp_in, C, C), ("Wp_x", Wp_x, Mx, C)))
    _tile_plane_set("ss2d_front", max(C, Mx) * H * W)
    xc = torch.empty_like(x)
    xd = torch.empty(B, Mx, H, W, device=x.device, dtype=x.dtype)
    check(lib().bem_ss2d_front_x6_f32(_p(x), _p(ln_w), _p(ln_b), float(ln_eps), _p(Wp_in), _p(bias_in), _p(dww), _p(dwb), _p(Wp_x), _p(xc), _p(xd),
                                      B, C, Mx, H, W, _stream()), "ss2d_front")
    return xc, xd


def gate_interleave(Hd, device):
    """row permutation of a (2Hd, ...) project_in parameter into the gate-interleaved order of bem_gdmlp_x6_f32:
    new row 32 j + 2 c + s = old row s Hd + 16 j + c."""
    j = torch.arange(Hd // 16, device=device)[:, None, None]
    c = torch.arange(16, device=device)[None, :, None]
    s_ = torch.arange(2, device=device)[None, None, :]
    return (s_ * Hd + 16 * j + c).reshape(-1)


# the fully fused gdMlp branch (bem_gdmlp_x6_f32), deterministic weights; wider blocks run the kernel chains.
def gdmlp_x6_supported(C, Hd):
    return C <= 80 and Hd % 16 == 0


def dw_gate_params10(dww, dwb, Hd):
    """depthwise (2Hd,1,3,3) / (2Hd)|None parameters -> the (Hd,10,2) block of bem_gdmlp_x6_f32: per gate channel nine (w1, w2) tap pairs
    and the (b1, b2) bias pair (zeros without a bias) -- 80 bytes per channel, moved chunk-wise into LDS by the kernel."""
    w = dww.reshape(2, Hd, 9).permute(1, 2, 0)
    b = torch.zeros(Hd, 1, 2, device=dww.device, dtype=dww.dtype) if dwb is None else dwb.reshape(2, Hd).t().reshape(Hd, 1, 2)
    return torch.cat([w, b], 1).contiguous()


# The SS2D tail folded into the fused gdMlp kernel (bem_vss_back_x6_f32): a test reaches the two-kernel chain by switching it off.
# C > 48 stays on the chain: the wider forms of the kernel spill in their prologue.
USE_VSS_BACK = True


def vss_back_supported(C, Hd, L):
    """L = H W of the image: the kernel addresses with 32-bit byte offsets and has no wide form, so a plane set of 2^30 elements or more
    belongs to the two-kernel chain (bem_gdmlp_x6_f32 has 64-bit forms up to 2^31)."""
    return C <= 48 and C % 8 == 0 and Hd % 16 == 0 and C * L < _TILE_NARROW


def vss_back_rows(C):
    """Row order of the out_proj operand of bem_vss_back_x6_f32, as a list over the 32 MT packed rows: the out_proj row (channel) that
    packed row holds, or -1 for a zero row.  Accumulator register r of M-tile mt in lane half kh is packed row
    32 mt + (r & 3) + 8 (r >> 2) + 4 kh; as slot s = 16 mt + r of the lane it must be channel 16 (s >> 3) + 8 kh + (s & 7), the
    channel the lane holds there as the B operand of project_in."""
    KB = (C + 15) // 16
    MT = (8 * KB + 15) // 16
    rows = [-1] * (32 * MT)
    for mt in range(MT):
        for kh in range(2):
            for r in range(16):
                s = 16 * mt + r
                ch = 16 * (s >> 3) + 8 * kh + (s & 7)
                if s < 8 * KB and ch < C:
                    rows[32 * mt + (r & 3) + 8 * (r >> 2) + 4 * kh] = ch
    return rows


def pack_vss_back_outproj(W):
    """(C, C) out_proj weight -> the x6-packed, row-permuted operand Wp_outproj of bem_vss_back_x6_f32."""
    C = W.shape[0]
    rows = torch.tensor(vss_back_rows(C), device=W.device)
    Wz = torch.cat([W, W.new_zeros(1, W.shape[1])], 0)              # index -1 = the zero row
    return pack_pw_weight(Wz[rows].contiguous(), x6=True)


def _gdmlp_x6_cost(x, Hd, pre, **_):
    B, C, H, W = x.shape
    nb, nf = 8.0 * x.numel(), 6.0 * 2.0 * B * H * W * (2 * Hd * C + Hd * C)
    if pre is not None:                                             # + y0, y1 in and the C x C out_proj GEMM
        nb, nf = nb + 8.0 * x.numel(), nf + 6.0 * 2.0 * B * H * W * C * C
    return nb, nf


@_bracket(_gdmlp_x6_cost, lambda x, **_: (x.shape[1],))
def gdmlp_x6(x, ln_w, ln_b, ln_eps, Wp_gate, bias_gate, dw10, Wp_out, bias_out, Hd, *, pre=None):
    """x + project_out(GELU(h1) * h2) + b_o with [h1; h2] = dw3x3(project_in(LayerNorm2d(x))) in ONE kernel (bem_gdmlp_x6_f32).
    Wp_gate = pack_pw_weight(W_i[gate_interleave(Hd)], x6=True), bias_gate = b_i[gate_interleave(Hd)] (zeros without a bias);
    dw10 = dw_gate_params10(...); Wp_out = pack_pw_weight(W_o, x6=True).
    pre = (y0, y1, on_w, on_b, on_eps, Wp_outproj, bias_outproj): x is the SS2D branch's input and the branch is applied to
    x1 = x + out_proj(out_norm(y0 + y1)) + bias_outproj, formed inside the kernel (bem_vss_back_x6_f32; Wp_outproj = pack_vss_back_outproj(W_op))."""
    for n_, t in (("x", x), ("ln_w", ln_w), ("ln_b", ln_b), ("Wp_gate", Wp_gate), ("bias_gate", bias_gate), ("dw10", dw10), ("Wp_out", Wp_out)):
        _chk(t, n_)
    _chk(bias_out, "bias_out", optional=True)
    B, C, H, W = x.shape
    if not gdmlp_x6_supported(C, Hd):
        raise ValueError(f"gdmlp_x6: C = {C} (<= 80) / Hd = {Hd} (% 16) not supported")
    if tuple(dw10.shape) != (Hd, 10, 2):
        raise ValueError("gdmlp_x6: depthwise parameters must come from dw_gate_params10")
    if ln_w.numel() != C or ln_b.numel() != C or bias_gate.numel() != 2 * Hd or (bias_out is not None and bias_out.numel() != C):
        raise ValueError("gdmlp_x6: parameter shapes")
    _chk_packed1("gdmlp_x6", (("Wp_gate", Wp_gate, 2 * Hd, C), ("Wp_out", Wp_out, C, Hd)))
    _tile_plane_set("gdmlp_x6", C * H * W)
    if pre is not None:
        y0, y1, on_w, on_b, on_eps, Wp_op, b_op = pre
        for n_, t in (("y0", y0), ("y1", y1), ("on_w", on_w), ("on_b", on_b), ("Wp_outproj", Wp_op)):
            _chk(t, n_)
        _chk(b_op, "bias_outproj", optional=True)
        if not vss_back_supported(C, Hd, H * W):
            raise ValueError(f"gdmlp_x6 with pre: C = {C} (<= 48, % 8) with {C * H * W} elements per image (< {_TILE_NARROW}) not supported")
        if y0.shape != x.shape or y1.shape != x.shape or on_w.numel() != C or on_b.numel() != C or (b_op is not None and b_op.numel() != C):
            raise ValueError("gdmlp_x6 with pre: y0 / y1 must have the shape of x, out_norm and the out_proj bias C entries")
        _chk_packed1("gdmlp_x6", (("Wp_outproj", Wp_op, 32 * ((8 * ((C + 15) // 16) + 15) // 16), C),))      # len(vss_back_rows(C)) rows
    out = torch.empty_like(x)
    if pre is not None:
        check(lib().bem_vss_back_x6_f32(_p(x), _p(ln_w), _p(ln_b), float(ln_eps), _p(Wp_gate), _p(bias_gate), _p(dw10), _p(Wp_out),
                                        _p(bias_out), _p(out), B, C, Hd, H, W, _p(y0), _p(y1), _p(on_w), _p(on_b), float(on_eps),
                                        _p(Wp_op), _p(b_op), _stream()), "gdmlp_x6")
        return out
    check(lib().bem_gdmlp_x6_f32(_p(x), _p(ln_w), _p(ln_b), float(ln_eps), _p(Wp_gate), _p(bias_gate), _p(dw10), _p(Wp_out),
                                 _p(bias_out), _p(out), B, C, Hd, H, W, _stream()), "gdmlp_x6")
    return out


def _dwconv3x3_cost(x, mode, **_):
    B, Cin, H, W = x.shape
    return 4.0 * B * H * W * (Cin + (Cin // 2 if mode == 2 else Cin)), 18.0 * B * Cin * H * W


@_bracket(_dwconv3x3_cost)
def dwconv3x3(x, w, bias=None, mode=0):
    """mode 0 plain, 1 SiLU, 2 gdMlp gate (x has 2*Cout channels), 3 PostSmooth.  w (Cw,1,3,3) or (B,Cw,1,3,3)."""
    _chk(x, "x"); _chk(w, "w"); _chk(bias, "bias", optional=True)
    B, Cin, H, W = x.shape
    Cout = Cin // 2 if mode == 2 else Cin
    per_b = w.dim() == 5
    Cw = w.shape[1] if per_b else w.shape[0]
    if Cw != Cin or tuple(w.shape[-3:]) != (1, 3, 3) or (per_b and w.shape[0] != B):
        raise ValueError(f"dwconv3x3: weight {tuple(w.shape)} vs input channels {Cin}")
    bb = 0
    if bias is not None:
        if bias.shape[-1] != Cin:
            raise ValueError("dwconv3x3: bias shape")
        bb = Cin if (bias.dim() == 2 and bias.shape[0] == B and B > 1) else 0
        if bias.dim() == 2 and bias.shape[0] not in (1, B):
            raise ValueError("dwconv3x3: bias batch")
    out = torch.empty(B, Cout, H, W, device=x.device, dtype=x.dtype)
    check(lib().bem_dwconv3x3_f32(_p(x), _p(w), (Cin * 9 if per_b else 0), _p(bias), bb, _p(out), B, Cout, H, W, mode,
                                  _stream()), "dwconv3x3")
    return out


# Which kernel form takes a dense convolution is the library's decision (bem_conv2d_route; its comment in bem_hip.h is the route table).  These two
# constants only build its `allow` argument: tests and scripts/lpips_rate.py clear one to reach the kernels that stand behind the x6 / f32-MFMA forms.
USE_CONV_MFMA = True
USE_CONV_X6 = True


class ConvWeight:
    """A dense-conv weight (Cout, Cin, KH, KW) and the operand forms conv2d's matrix-core kernels read, each packed on first request and
    kept as long as this object.  Whoever owns the weight keeps the ConvWeight (modules.Conv2dK.conv_weight: in its Derived cache)."""

    def __init__(self, w, input_grad=None):
        self.w, self._x6, self._f32, self._grad = w, None, None, input_grad      # input_grad: given where it is not the flip of w itself

    def x6(self):
        """(KH*KW taps, x6-packed (Cout, Cin)), tap = ky * KW + kx: the row and the shifted-tap forms."""
        if self._x6 is None:
            w = self.w
            self._x6 = pack_pw_weight(w.permute(2, 3, 0, 1).reshape(w.shape[2] * w.shape[3], w.shape[0], w.shape[1]).contiguous(), x6=True)
        return self._x6

    def f32(self):
        """Packed (Cout, Cin*KH*KW) f32 operand of the implicit-GEMM form."""
        if self._f32 is None:
            self._f32 = pack_pw_weight(self.w.reshape(self.w.shape[0], -1).contiguous(), x6=False)
        return self._f32

    def input_grad(self):
        """ConvWeight of a stride-1 convolution's input gradient (taps flipped, channel axes swapped): dx = conv2d(dy, this, None, pad=K - 1 - pad)."""
        if self._grad is None:
            self._grad = ConvWeight(self.w.flip(2, 3).transpose(0, 1).contiguous())
        return self._grad


# BEM_CONV_* of bem_hip.h -> the form's name and the operand form of the weight its kernel reads
_CONV_FORMS = {1: ("rows", ConvWeight.x6), 2: ("taps", ConvWeight.x6), 3: ("mfma", ConvWeight.f32), 4: ("direct", lambda cw: cw.w)}
_CONV_ROUTES = {}           # bem_conv2d_route's answers, by everything it reads


def _conv_out_hw(H, W, KH, KW, stride, pad, dilation=1):
    return (H + 2 * pad - dilation * (KH - 1) - 1) // stride + 1, (W + 2 * pad - dilation * (KW - 1) - 1) // stride + 1


def _conv2d_cost(x, w, stride, pad, res1, res2, dilation, **_):
    B, _, H, W = x.shape
    Co, Ci, KH, KW = (w.w if isinstance(w, ConvWeight) else w).shape
    Ho, Wo = _conv_out_hw(H, W, KH, KW, stride, pad, dilation)
    nres = (res1 is not None) + (res2 is not None)
    return 4.0 * B * (Ci * H * W + Co * Ho * Wo * (1 + nres)) + 4.0 * Co * Ci * KH * KW, 2.0 * B * Co * Ci * KH * KW * Ho * Wo


def _conv2d_ask(x, w, bias, stride, pad, res1, res2, cin_slice, dilation, res1_rep):
    """conv2d's operand check and its question to bem_conv2d_route -> (BEM_CONV_* form, ConvWeight, (pointer, batch stride) of the sliced x, output
    shape); a convolution no kernel takes raises the library's reason.  out, conv2d's own allocation, is NULL to the route.  The route reads a pointer's
    low four bits only, so _CONV_ROUTES keeps the answer per argument tuple (asking costs 2 us of host time, in every launch-bound step)."""
    cw = w if isinstance(w, ConvWeight) else ConvWeight(w)
    w = cw.w
    _chk(x, "x"); _chk(w, "w"); _chk(bias, "bias", optional=True)
    _chk(res1, "res1", optional=True); _chk(res2, "res2", optional=True)
    B, Ct, H, W = x.shape
    Cout, Cin, KH, KW = w.shape
    c0 = 0
    if cin_slice is not None:
        c0, cs = cin_slice
        if cs != Cin or c0 + Cin > Ct:
            raise ValueError("conv2d: channel slice out of range")
    elif Ct != Cin:
        raise ValueError(f"conv2d: input has {Ct} channels, weight expects {Cin}")
    if bias is not None and bias.shape != (Cout,):
        raise ValueError("conv2d: bias shape")
    if res1_rep < 1 or (res1_rep != 1 and res1 is None):
        raise ValueError("conv2d: res1_rep must be >= 1 and needs res1")
    oshape = (B, Cout) + _conv_out_hw(H, W, KH, KW, stride, pad, dilation)
    for n, r, shp in (("res1", res1, (B // res1_rep if B % res1_rep == 0 else -1,) + oshape[1:]), ("res2", res2, oshape)):
        if r is not None and tuple(r.shape) != shp:
            raise ValueError(f"conv2d: {n} shape")
    xs = _pslice(x, c0)
    key = (Cout, Cin, KH, KW, H, W, xs[1], stride, pad, dilation, USE_CONV_X6, USE_CONV_MFMA, (xs[0].value or 0) & 15,
           None if res1 is None else res1.data_ptr() & 15, None if res2 is None else res2.data_ptr() & 15)
    form = _CONV_ROUTES.get(key) or _CONV_ROUTES.setdefault(key, lib().bem_conv2d_route(
        *xs, _p(res1), _p(res2), None, Cin, H, W, Cout, KH, KW, stride, pad, dilation, USE_CONV_X6 | 2 * USE_CONV_MFMA))
    if form == 0:
        raise native.BemNativeError(lib().bem_last_error().decode())
    return form, cw, xs, oshape


def conv2d_route(x, w, stride=1, pad=1, res1=None, res2=None, cin_slice=None, dilation=1, res1_rep=1):
    """The kernel form conv2d runs for these operands, "rows", "taps", "mfma" or "direct", without running anything."""
    return _CONV_FORMS[_conv2d_ask(x, w, None, stride, pad, res1, res2, cin_slice, dilation, res1_rep)[0]][0]


@_bracket(_conv2d_cost)
def conv2d(x, w, bias=None, stride=1, pad=1, relu=False, res1=None, res2=None, cin_slice=None, dilation=1, res1_rep=1):
    """Dense conv.  ``cin_slice=(c0, Cin)`` convolves channels [c0, c0+Cin) of a wider contiguous x.
    ``res1_rep=n``: res1 has B / n rows and output row b adds res1[b // n] (a per-image term shared by the n samples of an image).
    Which kernel runs, and which convolutions none takes (BemNativeError): bem_conv2d_route; conv2d_route asks it alone.
    ``w``: a ConvWeight, whose packed forms are reused, or a plain (Cout, Cin, KH, KW) tensor, packed for this call alone."""
    res1_rep = int(res1_rep)
    form, cw, xs, oshape = _conv2d_ask(x, w, bias, stride, pad, res1, res2, cin_slice, dilation, res1_rep)
    out = torch.empty(oshape, device=x.device, dtype=x.dtype)
    name, operand = _CONV_FORMS[form]
    (B, _, H, W), (Cout, Cin, KH, KW) = x.shape, cw.w.shape
    check(lib().bem_conv2d_f32(form, *xs, _p(operand(cw)), _p(bias), _p(res1), _p(res2), _p(out), B, Cin, H, W, Cout, KH, KW, stride, pad, dilation,
                               int(relu), res1_rep, _stream()), "conv2d " + name)
    return out


# --------------------------------------------------------------------------- quaternion / Haar -
def quat_dwt(x, c0=0):
    """x (B,Ct,H,W); channels [c0,c0+3) are RGB -> (B,32,H/2,W/2)."""
    _chk(x, "x")
    B, Ct, H, W = x.shape
    if c0 + 3 > Ct or H % 2 or W % 2:
        raise ValueError("quat_dwt: needs 3 channels and even H, W")
    out = torch.empty(B, 32, H // 2, W // 2, device=x.device, dtype=x.dtype)
    check(lib().bem_quat_dwt_f32(*_pslice(x, c0), _p(out), B, H, W, _stream()), "quat_dwt")
    return out


def cond_dwt(conds, s):
    """conds (R,3,hd,wd) -> (R,32,hd*s/2,wd*s/2) = quat_dwt(bilinear_up(conds, s)), bit for bit, in one kernel: the enlarged condition
    image is never written."""
    _chk(conds, "conds")
    s = int(s)
    R, C, H, W = conds.shape
    if C != 3 or s < 1 or (H * s) % 2 or (W * s) % 2:
        raise ValueError("cond_dwt: needs 3 channels and even enlarged H, W")
    out = torch.empty(R, 32, H * s // 2, W * s // 2, device=conds.device, dtype=conds.dtype)
    check(lib().bem_cond_dwt_f32(_p(conds), _p(out), R, H, W, s, _stream()), "cond_dwt")
    return out


def dwt(x):
    _chk(x, "x")
    B, C, H, W = x.shape
    if H % 2 or W % 2:
        raise ValueError("dwt: even H, W required")
    out = torch.empty(B, 4 * C, H // 2, W // 2, device=x.device, dtype=x.dtype)
    check(lib().bem_dwt_f32(_p(x), _p(out), B, C, H, W, _stream()), "dwt")
    return out


def iwt(x):
    _chk(x, "x")
    B, C4, H, W = x.shape
    if C4 % 4:
        raise ValueError("iwt: channels must be a multiple of 4")
    out = torch.empty(B, C4 // 4, 2 * H, 2 * W, device=x.device, dtype=x.dtype)
    check(lib().bem_iwt_f32(_p(x), _p(out), B, C4, H, W, _stream()), "iwt")
    return out


def iwt_hamilton(q1w, q2w):
    _chk(q1w, "q1w"); _chk(q2w, "q2w")
    B, C, h, w = q1w.shape
    if C != 16 or q2w.shape != q1w.shape:
        raise ValueError("iwt_hamilton: expects two (B,16,h,w) tensors")
    out = torch.empty(B, 3, 2 * h, 2 * w, device=q1w.device, dtype=q1w.dtype)
    check(lib().bem_iwt_hamilton_f32(_p(q1w), _p(q2w), _p(out), B, h, w, _stream()), "iwt_hamilton")
    return out


def hamilton(q):
    _chk(q, "q")
    B, C, H, W = q.shape
    if C != 8:
        raise ValueError("hamilton: expects (B,8,H,W)")
    out = torch.empty(B, 3, H, W, device=q.device, dtype=q.dtype)
    check(lib().bem_hamilton_f32(_p(q), _p(out), B, H, W, _stream()), "hamilton")
    return out


def hamilton_bwd(q8, dout):
    """Backward of hamilton(): q8 (B,8,H,W), dout (B,3,H,W) -> (B,8,H,W) = [dp | dq]."""
    _chk(q8, "q8"); _chk(dout, "dout")
    B, C, H, W = q8.shape
    if C != 8 or tuple(dout.shape) != (B, 3, H, W):
        raise ValueError("hamilton_bwd: shapes")
    d = torch.empty_like(q8)
    check(lib().bem_hamilton_bwd_f32(_p(q8), _p(dout), _p(d), B, H, W, _stream()), "hamilton_bwd")
    return d


def hamilton_full(q1, q2):
    """QD/quaternion.py hamilton_product: (B,4,H,W) x (B,4,H,W) -> (B,4,H,W) = [real, i, j, k]."""
    _chk(q1, "q1"); _chk(q2, "q2")
    B, C, H, W = q1.shape
    if C != 4 or q2.shape != q1.shape:
        raise ValueError("hamilton_full: expects two (B,4,H,W) tensors")
    out = torch.empty_like(q1)
    check(lib().bem_hamilton_full_f32(_p(q1), _p(q2), _p(out), B, H, W, _stream()), "hamilton_full")
    return out


def attn_fold(f1, f2, attn_w, fuse_w, fuse_b, drop=None):
    """Channel cross attention + fuse conv folded into per-image (32x64) weights: returns (Wp (B, x6-packed(32,64)), bias (B,32)).
    drop: the attention dropout of QD/model3.py:98,124-131 on the two softmaxed maps, (p, seed, stream_id) for keep flags drawn in the
    kernel (Philox, bem_attn_fold_drop_f32) or (p, mask) with mask (B,2,32,32) of 0 / 1 values, map 0 = attn_1, map 1 = attn_2."""
    for n, t in (("f1", f1), ("f2", f2), ("attn_w", attn_w), ("fuse_w", fuse_w), ("fuse_b", fuse_b)):
        _chk(t, n)
    mask = None
    if drop is not None:
        if len(drop) == 2:
            (p, mask), seed, stream_id = drop, 0, 0
            _chk(mask, "mask")
        elif len(drop) == 3:
            p, seed, stream_id = drop
        else:
            raise ValueError("attn_fold: drop is (p, seed, stream_id) or (p, mask)")
        if not 0.0 <= float(p) < 1.0:
            raise ValueError(f"attn_fold: dropout probability {p} is not in [0, 1)")
    B, C, H, W = f1.shape
    if C != 32 or f2.shape != f1.shape or attn_w.numel() != 8 * (32 * 32 + 32) or fuse_w.numel() != 32 * 64 or fuse_b.numel() != 32:
        raise ValueError("attn_fold: shapes")
    if mask is not None and tuple(mask.shape) != (B, 2, 32, 32):
        raise ValueError(f"attn_fold: mask {tuple(mask.shape)} is not (B, 2, 32, 32) = {(B, 2, 32, 32)}")
    L = H * W
    stats = torch.empty(B, 32 * 32 + 64, device=f1.device, dtype=torch.float64)
    check(lib().bem_attn_stats_f64(_p(f1), _p(f2), _p(stats), B, L, _stream()), "attn_stats")
    Wn = torch.empty(B, 32, 64, device=f1.device, dtype=torch.float32)
    bias = torch.empty(B, 32, device=f1.device, dtype=torch.float32)
    if drop is None:
        check(lib().bem_attn_fold_f32(_p(stats), _p(attn_w), _p(fuse_w), _p(fuse_b), _p(Wn), _p(bias), B, L, _stream()), "attn_fold")
    else:
        check(lib().bem_attn_fold_drop_f32(_p(stats), _p(attn_w), _p(fuse_w), _p(fuse_b), _p(mask), float(p), int(seed) & _U64, int(stream_id) & _U64,
                                           _p(Wn), _p(bias), B, L, _stream()), "attn_fold_drop")
    return pack_pw_weight(Wn, x6=True), bias


# --------------------------------------------------------------------------- layout helpers ---
@_bracket(lambda x, **_: (8.0 * x.numel(), 0.0))
def transpose_planes(x):
    """(B,C,H,W) -> (B,C,W,H), contiguous."""
    _chk(x, "x")
    B, C, H, W = x.shape
    out = torch.empty(B, C, W, H, device=x.device, dtype=x.dtype)
    n = B * C
    xf, of = x.view(1, n, H, W), out.view(1, n, W, H)
    for s in range(0, n, _GRID_MAX):            # large batches: one launch per _GRID_MAX planes
        _transpose(xf, s, min(_GRID_MAX, n - s), of, s)
    return out


def _channels(op, fn, src, dst, dst_c0, src_c0, C, rep=None):
    """The body of copy_channels, copy_channels_rep and add_channels: ``op`` names the wrapper in messages, ``fn`` is its library function."""
    _chk(src, "src"); _chk(dst, "dst")
    Cs = src.shape[1]
    C = Cs - src_c0 if C is None else C
    L = _prod(src.shape[2:])
    Bd = src.shape[0] * (1 if rep is None else int(rep))
    if dst.shape[0] != Bd or _prod(dst.shape[2:]) != L or C < 0 or dst_c0 + C > dst.shape[1] or src_c0 + C > Cs:
        raise ValueError(f"{op}: shapes")
    rep_arg = () if rep is None else (int(rep),)
    check(fn(*_pslice(src, src_c0), *_pslice(dst, dst_c0), Bd, C, L, *rep_arg, _stream()), op)
    return dst


def copy_channels(src, dst, dst_c0, src_c0=0, C=None):
    """dst[:, dst_c0:dst_c0+C] = src[:, src_c0:src_c0+C] (same spatial size)."""
    return _channels("copy_channels", lib().bem_copy_channels_f32, src, dst, dst_c0, src_c0, C)


def copy_channels_rep(src, dst, dst_c0, rep, src_c0=0, C=None):
    """dst[b, dst_c0:dst_c0+C] = src[b // rep, src_c0:src_c0+C]  (dst has rep times the rows of src)."""
    return _channels("copy_channels_rep", lib().bem_copy_channels_rep_f32, src, dst, dst_c0, src_c0, C, rep)


def add_channels(src, dst, dst_c0, src_c0=0, C=None):
    """dst[:, dst_c0:dst_c0+C] += src[:, src_c0:src_c0+C] (same spatial size)."""
    return _channels("add_channels", lib().bem_add_channels_f32, src, dst, dst_c0, src_c0, C)


def bilinear_up(src, s, dst=None, dst_c0=0):
    _chk(src, "src")
    B, C, H, W = src.shape
    if dst is None:
        dst = torch.empty(B, C, H * s, W * s, device=src.device, dtype=src.dtype)
        dst_c0 = 0
    _chk(dst, "dst")
    if dst.shape[0] != B or dst.shape[2] != H * s or dst.shape[3] != W * s or dst_c0 + C > dst.shape[1]:
        raise ValueError("bilinear_up: dst shape")
    check(lib().bem_bilinear_up_f32(_p(src), C * H * W, *_pslice(dst, dst_c0), B, C, H, W, s, _stream()), "bilinear_up")
    return dst


def space_to_depth(x):
    _chk(x, "x")
    B, C, H, W = x.shape
    if H % 2 or W % 2:
        raise ValueError("space_to_depth: even H, W required")
    out = torch.empty(B, 4 * C, H // 2, W // 2, device=x.device, dtype=x.dtype)
    check(lib().bem_space_to_depth_f32(_p(x), _p(out), B, C, H, W, _stream()), "space_to_depth")
    return out


def pixel_shuffle2(x):
    _chk(x, "x")
    B, C4, H, W = x.shape
    if C4 % 4:
        raise ValueError("pixel_shuffle2: channels % 4")
    out = torch.empty(B, C4 // 4, 2 * H, 2 * W, device=x.device, dtype=x.dtype)
    check(lib().bem_pixel_shuffle2_f32(_p(x), _p(out), B, C4 // 4, H, W, _stream()), "pixel_shuffle2")
    return out


# ------------------------------------------------------------------- Stage-I training pieces ----
def store_words(dst, host, n):
    """dst[:n] (device, 32-bit elements) = host[:n] (CPU tensor of a 32-bit dtype), n <= 512, as the arguments of one launch."""
    _chk(dst, "dst")
    if host.is_cuda or host.element_size() != 4 or not host.is_contiguous() or n > host.numel() or n > dst.numel():
        raise ValueError("store_words: a contiguous CPU tensor of 32-bit elements")
    check(lib().bem_store_words(_p(dst), ctypes.c_void_p(host.data_ptr()), int(n), _stream()), "store_words")


def bnn_prior_ema_(prior_mu, prior_rho, mu, rho, decay, decay_dev=None):
    for t, nm in ((prior_mu, "prior_mu"), (prior_rho, "prior_rho"), (mu, "mu"), (rho, "rho")):
        _chk(t, nm)
    if not (prior_mu.shape == prior_rho.shape == mu.shape == rho.shape):
        raise ValueError("bnn_prior_ema_: shapes differ")
    check(lib().bem_bnn_prior_ema_f32(_p(prior_mu), _p(prior_rho), _p(mu), _p(rho), float(decay), _p(decay_dev), mu.numel(), _stream()), "bnn_prior_ema")


def bnn_bank_sample(bank, decay, decay_dev, seed, stream_base, stream_add):
    check(lib().bem_bnn_bank_sample_f32(_p(bank.segs), _p(bank.blks), bank.nblk, _p(bank.pm), _p(bank.pr), _p(bank.w), _p(bank.eps), _p(bank.gw),
                                        float(decay), _p(decay_dev), seed, stream_base, _p(stream_add), _stream()), "bnn_bank_sample")


def bnn_ebank_sample(bank, seed, stream_base):
    check(lib().bem_bnn_ebank_sample_f32(_p(bank.segs), _p(bank.blks), bank.nblk, _p(bank.arena), seed, stream_base, _stream()), "bnn_ebank_sample")


def pack_pw_weight_jobs(jobs, blks, nblk, arena):
    check(lib().bem_pack_pw_weight_x6_jobs(_p(jobs), _p(blks), nblk, _p(arena), _stream()), "pack_pw_weight_x6_jobs")


def bnn_bank_kl_(bank, out):
    _chk(out, "out")
    check(lib().bem_bnn_bank_kl_f32(_p(bank.segs), _p(bank.blks), bank.nblk, _p(bank.pm), _p(bank.pr), _p(out), _stream()), "bnn_bank_kl")


def bnn_bank_kl_bwd_(bank, g):
    _chk(g, "g")
    check(lib().bem_bnn_bank_kl_bwd_f32(_p(bank.segs), _p(bank.blks), bank.nblk, _p(bank.pm), _p(bank.pr), _p(g), _stream()), "bnn_bank_kl_bwd")


def bnn_bank_reparam_bwd_(bank):
    check(lib().bem_bnn_bank_reparam_bwd_f32(_p(bank.segs), _p(bank.blks), bank.nblk, _p(bank.gw), _p(bank.eps), _stream()), "bnn_bank_reparam_bwd")


def bnn_kl_(mu, rho, prior_mu, prior_rho, out):
    """out[0] += kl_div(mu, softplus(rho), prior_mu, softplus(prior_rho)).mean()"""
    for t, nm in ((prior_mu, "prior_mu"), (prior_rho, "prior_rho"), (mu, "mu"), (rho, "rho"), (out, "out")):
        _chk(t, nm)
    if not (prior_mu.shape == prior_rho.shape == mu.shape == rho.shape) or out.numel() != 1:
        raise ValueError("bnn_kl_: shapes")
    check(lib().bem_bnn_kl_f32(_p(mu), _p(rho), _p(prior_mu), _p(prior_rho), mu.numel(), _p(out), _stream()), "bnn_kl")


def bnn_kl_bwd_(mu, rho, prior_mu, prior_rho, g, dmu, drho):
    for t, nm in ((prior_mu, "prior_mu"), (prior_rho, "prior_rho"), (mu, "mu"), (rho, "rho"), (g, "g"), (dmu, "dmu"), (drho, "drho")):
        _chk(t, nm)
    if not (prior_mu.shape == prior_rho.shape == mu.shape == rho.shape == dmu.shape == drho.shape) or g.numel() != 1:
        raise ValueError("bnn_kl_bwd_: shapes")
    check(lib().bem_bnn_kl_bwd_f32(_p(mu), _p(rho), _p(prior_mu), _p(prior_rho), mu.numel(), _p(g), _p(dmu), _p(drho), _stream()), "bnn_kl_bwd")


def bnn_reparam_bwd_(gw, eps, rho, dmu, drho):
    for t, nm in ((gw, "gw"), (eps, "eps"), (rho, "rho"), (dmu, "dmu"), (drho, "drho")):
        _chk(t, nm)
    if not (gw.numel() == eps.numel() == rho.numel() == dmu.numel() == drho.numel()):
        raise ValueError("bnn_reparam_bwd_: sizes differ")
    check(lib().bem_bnn_reparam_bwd_f32(_p(gw), _p(eps), _p(rho), _p(dmu), _p(drho), rho.numel(), _stream()), "bnn_reparam_bwd")


def mask_token(fea, mask, token):
    _chk(fea, "fea"); _chk(mask, "mask"); _chk(token, "token")
    B, C, H, W = fea.shape
    if tuple(mask.shape) != (B, H, W) or token.numel() != C:
        raise ValueError(f"mask_token: mask {tuple(mask.shape)} / token {tuple(token.shape)} vs features {tuple(fea.shape)}")
    out = torch.empty_like(fea)
    check(lib().bem_mask_token_f32(_p(fea), _p(mask), _p(token), _p(out), B, C, H, W, _stream()), "mask_token")
    return out


def mask_token_bwd(dout, mask, dtoken):
    _chk(dout, "dout"); _chk(mask, "mask"); _chk(dtoken, "dtoken")
    B, C, H, W = dout.shape
    if tuple(mask.shape) != (B, H, W) or dtoken.numel() != C:
        raise ValueError("mask_token_bwd: shapes")
    dfea = torch.empty_like(dout)
    check(lib().bem_mask_token_bwd_f32(_p(dout), _p(mask), _p(dfea), _p(dtoken), B, C, H, W, _stream()), "mask_token_bwd")
    return dfea


def depth_to_space(d4):
    _chk(d4, "d4")
    B, C4, h, w = d4.shape
    if C4 % 4:
        raise ValueError("depth_to_space: channels % 4")
    dx = torch.empty(B, C4 // 4, 2 * h, 2 * w, device=d4.device, dtype=d4.dtype)
    check(lib().bem_depth_to_space_f32(_p(d4), _p(dx), B, C4 // 4, 2 * h, 2 * w, _stream()), "depth_to_space")
    return dx


def prelu(x, slope):
    _chk(x, "x"); _chk(slope, "slope")
    if slope.numel() != 1:
        raise ValueError("prelu: one shared slope (nn.PReLU())")
    out = torch.empty_like(x)
    check(lib().bem_prelu_f32(_p(x), _p(slope), _p(out), x.numel(), _stream()), "prelu")
    return out


def prelu_bwd(x, slope, dout, dslope):
    _chk(x, "x"); _chk(slope, "slope"); _chk(dout, "dout"); _chk(dslope, "dslope")
    if slope.numel() != 1 or dslope.numel() != 1 or dout.shape != x.shape:
        raise ValueError("prelu_bwd: shapes")
    dx = torch.empty_like(x)
    check(lib().bem_prelu_bwd_f32(_p(x), _p(slope), _p(dout), _p(dx), _p(dslope), x.numel(), _stream()), "prelu_bwd")
    return dx


def bilinear_up_bwd(dout, s):
    _chk(dout, "dout")
    B, C, Ho, Wo = dout.shape
    if Ho % s or Wo % s:
        raise ValueError("bilinear_up_bwd: output size not a multiple of the scale")
    dx = torch.empty(B, C, Ho // s, Wo // s, device=dout.device, dtype=dout.dtype)
    check(lib().bem_bilinear_up_bwd_f32(_p(dout), _p(dx), B, C, Ho // s, Wo // s, int(s), _stream()), "bilinear_up_bwd")
    return dx


# --------------------------------------------------------------------------- Bayesian / MC ----
def bnn_sample(mu, rho, nsets, eps=None, seed=0, stream_id=0, stream_add=None):
    """w[s] = mu + log1p(exp(rho)) * eps[s];  eps None -> Philox N(0,1) keyed by (seed, stream_id [+ stream_add[0], a one-element int64
    device tensor read by the kernel: the per-iteration part of the id of a graph-captured step])."""
    _chk(mu, "mu"); _chk(rho, "rho"); _chk(eps, "eps", optional=True)
    n = mu.numel()
    if rho.numel() != n or (eps is not None and eps.numel() != nsets * n):
        raise ValueError("bnn_sample: shapes")
    out = torch.empty((nsets,) + tuple(mu.shape), device=mu.device, dtype=mu.dtype)
    check(lib().bem_bnn_sample_f32(_p(mu), _p(rho), _p(eps), _p(out), nsets, n, seed, stream_id, _p(stream_add), _stream()), "bnn_sample")
    return out


def bnn_sample_packed(mu, rho, nsets, M, K, eps=None, seed=0, stream_id=0, sigma_given=False, stream_add=None):
    """bnn_sample + pack_pw_weight(x6) in one kernel: (nsets, packed(M, K)) GEMM weights of a Bayesian 1x1 layer.
    sigma_given: ``rho`` already holds sigma = log1p(exp(rho)) (it does not depend on the sample)."""
    _chk(mu, "mu"); _chk(rho, "rho"); _chk(eps, "eps", optional=True)
    if mu.numel() != M * K or rho.numel() != M * K or (eps is not None and eps.numel() != nsets * M * K):
        raise ValueError("bnn_sample_packed: shapes")
    out = torch.empty(nsets, packed_elems(M, K, True), device=mu.device, dtype=mu.dtype)
    check(lib().bem_bnn_sample_pack_x6(_p(mu), _p(rho), _p(eps), _p(out), nsets, M, K, seed, stream_id, _p(stream_add), int(bool(sigma_given)), _stream()), "bnn_sample_pack_x6")
    out._bem_mk = (M, K)
    return out


def pad_reflect(x, Hp, Wp):
    """(B,C,H,W) -> (B,C,Hp,Wp), reflect-padded at the bottom / right (numpy 'reflect')."""
    _chk(x, "x")
    B, C, H, W = x.shape
    if Hp == H and Wp == W:
        return x
    if not (0 <= Hp - H < H and 0 <= Wp - W < W):
        raise ValueError(f"pad_reflect: the pad must be smaller than the image ({H}x{W} -> {Hp}x{Wp})")
    out = torch.empty(B, C, Hp, Wp, device=x.device, dtype=x.dtype)
    check(lib().bem_pad_reflect_f32(_p(x), _p(out), B * C, H, W, Hp, Wp, _stream()), "pad_reflect")
    return out


def resize_down(x, s):
    """cv2.resize(fx=fy=1/s, INTER_LINEAR) of (B,C,Hp,Wp) planes for even s dividing Hp, Wp."""
    _chk(x, "x")
    B, C, Hp, Wp = x.shape
    out = torch.empty(B, C, Hp // s, Wp // s, device=x.device, dtype=x.dtype)
    check(lib().bem_resize_down_f32(_p(x), _p(out), B * C, Hp, Wp, s, _stream()), "resize_down")
    return out


def batch_assemble(lq_arena, gt_arena, table, table_dev, plan, plan_dev, row0, B, Sh, Sw, s, noise_dev=None, noise_steps=0):
    """Rows [row0, row0 + B) of an epoch plan -> lq, gt (B,3,Sh,Sw), lq_down, gt_down (B,3,Sh/s,Sw/s) from the uint8 image store, one launch.
    ``table`` (n,3) int64 (offset, H, W) and ``plan`` (R,4) int32 (image, top, left, mode) are host tensors, ``table_dev`` / ``plan_dev``
    their device copies; ``noise_dev`` (R,3) float32 (t, b, c) with ``noise_steps`` (bit 0 temperature, 1 brightness, 2 contrast).
    ``s`` = 0 returns None for the two down planes (whole validation images whose size no scale_down divides)."""
    _chk(lq_arena, "lq_arena", torch.uint8); _chk(gt_arena, "gt_arena", torch.uint8)
    _chk(table_dev, "table_dev", torch.int64); _chk(plan_dev, "plan_dev", torch.int32)
    _chk(noise_dev, "noise_dev", optional=True)
    for n, t, dt, w in (("table", table, torch.int64, 3), ("plan", plan, torch.int32, 4)):
        if t.is_cuda or t.dtype != dt or t.dim() != 2 or t.shape[1] != w or not t.is_contiguous():
            raise ValueError(f"batch_assemble: {n} must be a contiguous host (rows,{w}) {dt} tensor")
    if lq_arena.dim() != 1 or lq_arena.shape != gt_arena.shape:
        raise ValueError("batch_assemble: the two arenas must be flat and of one size")
    if table_dev.shape != table.shape or plan_dev.shape != plan.shape:
        raise ValueError("batch_assemble: the device tables must mirror the host tables")
    if not (0 <= row0 and B > 0 and row0 + B <= plan.shape[0]):
        raise ValueError(f"batch_assemble: rows [{row0}, {row0 + B}) outside a plan of {plan.shape[0]} rows")
    if noise_dev is not None and tuple(noise_dev.shape) != (plan.shape[0], 3):
        raise ValueError("batch_assemble: noise_dev must be (rows,3)")
    if s < 0 or Sh <= 0 or Sw <= 0:
        raise ValueError("batch_assemble: crop and scale_down must be positive (scale_down 0: no down planes)")
    dev = lq_arena.device
    lq, gt = torch.empty(B, 3, Sh, Sw, device=dev), torch.empty(B, 3, Sh, Sw, device=dev)
    lqd, gtd = (torch.empty(B, 3, Sh // s, Sw // s, device=dev), torch.empty(B, 3, Sh // s, Sw // s, device=dev)) if s else (None, None)
    check(lib().bem_batch_assemble_u8(_p(lq_arena), _p(gt_arena), lq_arena.numel(), _p(table), _p(table_dev), table.shape[0],
                                      ctypes.c_void_p(plan.data_ptr() + 16 * row0), ctypes.c_void_p(plan_dev.data_ptr() + 16 * row0),
                                      ctypes.c_void_p(0 if noise_dev is None else noise_dev.data_ptr() + 12 * row0), int(noise_steps),
                                      B, Sh, Sw, s, _p(lq), _p(gt), _p(lqd), _p(gtd), _stream()), "batch_assemble")
    return lq, gt, lqd, gtd


def randn(shape, device, seed=0, stream_id=0, stream_add=None):
    out = torch.empty(shape, device=device, dtype=torch.float32)
    check(lib().bem_randn_f32(_p(out), out.numel(), seed, stream_id, _p(stream_add), _stream()), "randn")
    return out


def plane_mean(x, h=None, w=None):
    """Mean over the top-left (h,w) window of every (b,c) plane -> (B,C)."""
    _chk(x, "x")
    B, C, Hs, Ws = x.shape
    h, w = h or Hs, w or Ws
    out = torch.empty(B, C, device=x.device, dtype=x.dtype)
    check(lib().bem_plane_mean_f32(_p(x), _p(out), B * C, Hs, Ws, h, w, _stream()), "plane_mean")
    return out


# --------------------------------------------------------------------------- DecompDualBranch's bottleneck blocks ----
def row_scale(w, scale):
    """w (M, ...) * scale (M) along the first axis."""
    _chk(w, "w"); _chk(scale, "scale")
    M = w.shape[0]
    if scale.numel() != M:
        raise ValueError("row_scale: one factor per row")
    out = torch.empty_like(w)
    check(lib().bem_row_scale_f32(_p(w), _p(scale), _p(out), M, w.numel() // M, _stream()), "row_scale")
    return out


def _need4(op, x):
    if x.dim() != 4:
        raise ValueError(f"{op}: x must be (B, C, H, W), got {tuple(x.shape)}")
    return tuple(x.shape)


def _sa_kernel_size(op, w):
    k = w.shape[-1] if w.dim() == 4 else 0
    if k not in (3, 7) or tuple(w.shape) != (1, 2, k, k):
        raise ValueError(f"{op}: w must be (1, 2, k, k) with k 3 or 7, got {tuple(w.shape)}")
    return k


def se_gate(x, w1, w2, want_mean=False):
    """SEBlock's per-channel gate (B,C) = sigmoid(w2 relu(w1 mean_hw(x)))."""
    _chk(x, "x"); _chk(w1, "w1"); _chk(w2, "w2")
    B, C, _, _ = _need4("se_gate", x)
    Cr = w1.shape[0]
    if tuple(w1.shape) != (Cr, C) or tuple(w2.shape) != (C, Cr):
        raise ValueError("se_gate: weight shapes")
    mean = plane_mean(x)
    y = torch.empty(B, C, device=x.device, dtype=x.dtype)
    check(lib().bem_se_gate_f32(_p(mean), _p(w1), _p(w2), _p(y), B, C, Cr, _stream()), "se_gate")
    return (y, mean) if want_mean else y


def spatial_attention(x, w, chan_scale=None, want_map=False):
    """x * chan_scale * sigmoid(conv_kxk([mean_c, max_c](x * chan_scale))); w (1,2,k,k).  want_map: also the (B,2,H,W) map (for the backward)."""
    _chk(x, "x"); _chk(w, "w"); _chk(chan_scale, "chan_scale", optional=True)
    B, C, H, W = _need4("spatial_attention", x)
    k = _sa_kernel_size("spatial_attention", w)
    if chan_scale is not None and tuple(chan_scale.shape) != (B, C):
        raise ValueError("spatial_attention: the gate must be (B, C)")
    ws = torch.empty(B, 2, H, W, device=x.device, dtype=x.dtype)
    out = torch.empty_like(x)
    check(lib().bem_spatial_attention_f32(_p(x), _p(chan_scale), _p(w), _p(ws), _p(out), B, C, H, W, k, _stream()), "spatial_attention")
    return (out, ws) if want_map else out


def spatial_attention_bwd(x, dout, amap, w, dw):
    """Backward of spatial_attention(x, w): returns dx; dw (1,2,k,k) accumulated."""
    for t, n in ((x, "x"), (dout, "dout"), (amap, "map"), (w, "w"), (dw, "dw")):
        _chk(t, n)
    B, C, H, W = _need4("spatial_attention_bwd", x)
    k = _sa_kernel_size("spatial_attention_bwd", w)
    if dout.shape != x.shape:
        raise ValueError(f"spatial_attention_bwd: dout {tuple(dout.shape)} must have x's shape {tuple(x.shape)}")
    if tuple(amap.shape) != (B, 2, H, W):
        raise ValueError(f"spatial_attention_bwd: map must be {(B, 2, H, W)}, got {tuple(amap.shape)}")
    if dw.numel() != 2 * k * k:
        raise ValueError(f"spatial_attention_bwd: dw must hold {2 * k * k} elements, got {dw.numel()}")
    dpre = torch.empty(B, H, W, device=x.device, dtype=x.dtype)
    dx = torch.empty_like(x)
    check(lib().bem_spatial_attention_bwd_f32(_p(x), _p(dout), _p(amap), _p(w), _p(dpre), _p(dx), _p(dw), B, C, H, W, k, _stream()),
          "spatial_attention_bwd")
    return dx


def chan_scale(x, scale, add=None, add_bc=None, add_bc_scale=1.0):
    """scale[(b,) c] * x (+ add) (+ add_bc[b, c] * add_bc_scale); scale: one axis of C elements and otherwise axes of 1 ((C,), (1,C,1,1))
    for one factor per channel, or exactly (B, C) for one per image and channel (a flat vector of B*C elements with B > 1 is ambiguous
    and rejected)."""
    _chk(x, "x"); _chk(scale, "scale"); _chk(add, "add", optional=True); _chk(add_bc, "add_bc", optional=True)
    if x.dim() < 3:
        raise ValueError(f"chan_scale: x must be (B, C, ...), got {tuple(x.shape)}")
    B, C = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    if tuple(scale.shape) == (B, C):
        bstride = C
    elif scale.numel() == C and C in tuple(scale.shape):
        bstride = 0
    else:
        raise ValueError(f"chan_scale: scale must be one axis of {C} elements or {(B, C)}, got {tuple(scale.shape)}")
    if add is not None and add.shape != x.shape:
        raise ValueError(f"chan_scale: add {tuple(add.shape)} must have x's shape {tuple(x.shape)}")
    if add_bc is not None and tuple(add_bc.shape) != (B, C):
        raise ValueError(f"chan_scale: add_bc must be {(B, C)}, got {tuple(add_bc.shape)}")
    out = torch.empty_like(x)
    check(lib().bem_chan_scale_f32(_p(x), _p(scale), bstride, _p(add), _p(add_bc), float(add_bc_scale), _p(out), B, C, HW, _stream()), "chan_scale")
    return out


def chan_dot(a, b, out=None):
    """out is None: (B,C) = sum_p a b per image; out (C): += sum over images and pixels (a parameter's gradient)."""
    _chk(a, "a"); _chk(b, "b"); _chk(out, "out", optional=True)
    if a.dim() < 3:
        raise ValueError(f"chan_dot: a must be (B, C, ...), got {tuple(a.shape)}")
    B, C = a.shape[0], a.shape[1]
    HW = a[0, 0].numel()
    if b.shape != a.shape:
        raise ValueError(f"chan_dot: b {tuple(b.shape)} must have a's shape {tuple(a.shape)}")
    if out is not None and out.numel() != C:
        raise ValueError(f"chan_dot: out must hold {C} elements, got {out.numel()}")
    per = out is None
    if per:
        out = torch.empty(B, C, device=a.device, dtype=a.dtype)
    check(lib().bem_chan_dot_f32(_p(a), _p(b), _p(out), B, C, HW, int(per), _stream()), "chan_dot")
    return out


def se_gate_bwd(mean, w1, w2, y, dy, dw1, dw2):
    """Backward of se_gate's (B,C) gate from its plane means: returns dmean (B,C); dw1 (Cr,C) and dw2 (C,Cr) accumulated."""
    for t, n in ((mean, "mean"), (w1, "w1"), (w2, "w2"), (y, "y"), (dy, "dy"), (dw1, "dw1"), (dw2, "dw2")):
        _chk(t, n)
    if mean.dim() != 2 or w1.dim() != 2:
        raise ValueError(f"se_gate_bwd: mean must be (B, C) and w1 (Cr, C), got {tuple(mean.shape)}, {tuple(w1.shape)}")
    B, C = mean.shape
    Cr = w1.shape[0]
    for t, n, shape in ((y, "y", (B, C)), (dy, "dy", (B, C)), (w1, "w1", (Cr, C)), (w2, "w2", (C, Cr)), (dw1, "dw1", (Cr, C)), (dw2, "dw2", (C, Cr))):
        if tuple(t.shape) != shape:
            raise ValueError(f"se_gate_bwd: {n} must be {shape}, got {tuple(t.shape)}")
    dmean = torch.empty_like(mean)
    check(lib().bem_se_gate_bwd_f32(_p(mean), _p(w1), _p(w2), _p(y), _p(dy), _p(dmean), _p(dw1), _p(dw2), B, C, Cr, _stream()), "se_gate_bwd")
    return dmean


def _images(op, Bn, samples_per_image, what="images", limit=_GRID_MAX):
    """Bn candidates in groups of samples_per_image -> the number of images.  A call takes at most ``limit`` of ``what``: 'images' or
    'candidates', whichever the op's launch grids spread over y or z."""
    if samples_per_image < 1 or Bn % samples_per_image:
        raise ValueError(f"{op}: {Bn} candidates are not a multiple of samples_per_image = {samples_per_image}")
    B = Bn // samples_per_image
    n = B if what == "images" else Bn
    if n > limit:
        raise ValueError(f"{op}: at most {limit} {what} per call, got {n}")
    return B


# bem_select_scores_f32's rule numbers (csrc/selection.hip states the rules)
SELECT_RULES = {"weighted": 0, "max": 1, "min": 2, "relative": 3}


def cond_postproc(pred, target_mean, noise, samples_per_image, noise_level):
    _chk(pred, "pred"); _chk(target_mean, "target_mean", optional=True); _chk(noise, "noise", optional=True)
    Bn, C, h, w = pred.shape
    if C != 3 or Bn % samples_per_image:
        raise ValueError("cond_postproc: expects (Bn,3,h,w)")
    if target_mean is not None and tuple(target_mean.shape) != (Bn // samples_per_image, 3):
        raise ValueError("cond_postproc: target_mean shape")
    if noise is not None and noise.shape != pred.shape:
        raise ValueError("cond_postproc: noise shape")
    out = torch.empty_like(pred)
    check(lib().bem_cond_postproc_f32(_p(pred), _p(target_mean), _p(noise), _p(out), Bn, h, w, samples_per_image,
                                      float(noise_level), _stream()), "cond_postproc")
    return out


def candidate_finalize(pred, target, samples_per_image, h, w, gt_mean):
    """pred (Bn,3,Hp,Wp), target (n_img,3,h,w)|None -> (final (Bn,3,h,w), psnr (Bn)).  3 Bn <= 65535 (one grid row per candidate channel)."""
    _chk(pred, "pred"); _chk(target, "target", optional=True)
    Bn, C, Hp, Wp = pred.shape
    _images("candidate_finalize", Bn, samples_per_image, "candidates", _GRID_MAX // 3)
    if C != 3 or not (0 < h <= Hp and 0 < w <= Wp):
        raise ValueError("candidate_finalize: shapes")
    if gt_mean and target is None:
        raise ValueError("candidate_finalize: gt_mean needs a target")
    if target is not None and tuple(target.shape) != (Bn // samples_per_image, 3, h, w):
        raise ValueError("candidate_finalize: target shape")
    fin = torch.empty(Bn, 3, h, w, device=pred.device, dtype=pred.dtype)
    ps = torch.zeros(Bn, device=pred.device, dtype=pred.dtype)
    ws = torch.empty(7 * Bn, device=pred.device, dtype=torch.float64)
    check(lib().bem_candidate_finalize_f32(_p(pred), _p(target), _p(fin), _p(ps), _p(ws), Bn, samples_per_image, Hp, Wp, h, w,
                                           int(bool(gt_mean)), _stream()), "candidate_finalize")
    return fin, ps


def select_best(final, psnr, samples_per_image):
    """eval.py:284-285 on the device, select_scores' rule 'relative': (best (B) int32, best_psnr (B), best_images (B,3,h,w))."""
    best, bp, _, img = select_scores(final, psnr, samples_per_image, rule="relative")
    return best, bp, img


def ssim(final, target, samples_per_image):
    """Enhancement/utils.py calculate_ssim per candidate: final (Bn,3,h,w) in [0,1], target (Bn/N,3,h,w) -> (Bn) f32.  Bn <= 65535."""
    _chk(final, "final"); _chk(target, "target")
    Bn, C, h, w = final.shape
    _images("ssim", Bn, samples_per_image, "candidates")
    if C != 3 or tuple(target.shape) != (Bn // samples_per_image, 3, h, w) or h <= 10 or w <= 10:
        raise ValueError("ssim: shapes (3-channel images larger than the 11x11 window)")
    out = torch.empty(Bn, device=final.device, dtype=torch.float32)
    ws = torch.empty(Bn, device=final.device, dtype=torch.float64)
    check(lib().bem_ssim_f32(_p(final), _p(target), _p(out), _p(ws), Bn, samples_per_image, h, w, _stream()), "ssim")
    return out


def select_scores(final, s1, samples_per_image, s2=None, weight=1.0, rule="weighted"):
    """Per-image selection on the device (eval.py:268-297): rule 'weighted' (weight s1/max + (1-weight) s2/max), 'max', 'min', or
    'relative' (s1/max of one score, started like Python's max(): the default PSNR rule); first index on ties; row = image*N + sample.
    Returns (best (B) int32, best s1 (B), best s2 (B)|None, best images (B,3,h,w)|None).  B <= 65535."""
    _chk(s1, "s1"); _chk(s2, "s2", optional=True); _chk(final, "final", optional=True)
    N = samples_per_image
    Bn = s1.numel()
    if rule not in SELECT_RULES:
        raise ValueError(f"select_scores: unknown rule {rule!r}")
    B = _images("select_scores", Bn, N)
    if (s2 is not None and s2.numel() != Bn) or (final is not None and final.shape[0] != Bn):
        raise ValueError("select_scores: shapes")
    if s2 is not None and rule == "relative":
        raise ValueError("select_scores: the 'relative' rule takes one score")
    best = torch.empty(B, device=s1.device, dtype=torch.int32)
    b1 = torch.empty(B, device=s1.device, dtype=torch.float32)
    b2 = torch.empty(B, device=s1.device, dtype=torch.float32) if s2 is not None else None
    img = torch.empty((B,) + tuple(final.shape[1:]), device=s1.device, dtype=final.dtype) if final is not None else None
    check(lib().bem_select_scores_f32(_p(final), _p(s1), _p(s2), float(weight), SELECT_RULES[rule], _p(best), _p(b1), _p(b2), _p(img), B, N,
                                      (final[0].numel() if final is not None else 0), _stream()), "select_scores")
    return best, b1, b2, img


def mc_mean(raw, target, samples_per_image, h, w, gt_mean):
    """Monte-Carlo mean prediction (eval.py:224-225,308-314): raw (Bn,3,Hp,Wp) -> (B,3,h,w).  B <= 65535."""
    _chk(raw, "raw"); _chk(target, "target", optional=True)
    Bn, C, Hp, Wp = raw.shape
    N = samples_per_image
    B = _images("mc_mean", Bn, N)
    if C != 3 or not (0 < h <= Hp and 0 < w <= Wp) or (gt_mean and (target is None or tuple(target.shape) != (Bn // N, 3, h, w))):
        raise ValueError("mc_mean: shapes")
    out = torch.empty(B, 3, h, w, device=raw.device, dtype=raw.dtype)
    ws = torch.empty(2 * B, device=raw.device, dtype=torch.float64) if gt_mean else None
    check(lib().bem_mc_mean_f32(_p(raw), _p(target if gt_mean else None), _p(out), _p(ws), B, N, Hp, Wp, h, w, int(bool(gt_mean)), _stream()), "mc_mean")
    return out


class McState:
    """The state planes of the streamed Monte-Carlo statistics of one ``enhance`` call, all (B,3,h,w) f32 and zero before the first chunk:
    ``sum`` (of the clamped raw outputs; ``mean=True``) and / or ``mean`` and ``m2`` (Welford's running mean and sum of squared
    deviations of the finished candidates; ``spread=True``).  ``n`` counts the samples per image accumulated so far."""

    def __init__(self, B, h, w, device, mean=False, spread=False):
        _images("McState", B, 1)
        if B < 0 or h < 1 or w < 1:
            raise ValueError("McState: shapes")
        self.B, self.h, self.w, self.n = B, h, w, 0
        planes = torch.zeros((1 if mean else 0) + (2 if spread else 0), B, 3, h, w, device=device, dtype=torch.float32)
        self.sum = planes[0] if mean else None
        self.mean, self.m2 = (planes[-2], planes[-1]) if spread else (None, None)


def _mc_accum_cost(state, raw, final, samples_per_image, **_):
    per = 4.0 * state.B * 3 * state.h * state.w
    return ((samples_per_image + 2) * per if raw is not None else 0.0) + ((samples_per_image + 4) * per if final is not None else 0.0), 0.0


@_bracket(_mc_accum_cost)
def mc_accum(state, raw=None, final=None, samples_per_image=1):
    """One chunk of ``samples_per_image`` samples of every image into ``state``, in sample order: raw (B*Nc,3,Hp,Wp) into ``state.sum`` (the
    additions mc_mean performs), final (B*Nc,3,h,w) into ``state.mean`` / ``state.m2``.  Either may be None where the state has no plane for
    it.  Any split of the N samples into chunks leaves the same bits.  B <= 65535."""
    B, h, w, Nc = state.B, state.h, state.w, samples_per_image
    if raw is None and final is None:
        raise ValueError("mc_accum: neither raw outputs nor candidates")
    if (raw is not None and state.sum is None) or (final is not None and state.mean is None):
        raise ValueError("mc_accum: the state has no plane for this input")
    _chk(raw, "raw", optional=True); _chk(final, "final", optional=True)
    Hp, Wp = (h, w) if raw is None else tuple(raw.shape[2:])
    for t, shape, name in ((raw, (B * Nc, 3, Hp, Wp), "raw"), (final, (B * Nc, 3, h, w), "final")):
        if t is not None and (Nc < 1 or tuple(t.shape) != shape or not (h <= Hp and w <= Wp)):
            raise ValueError(f"mc_accum: {name} {tuple(t.shape)} is not {Nc} samples of {B} images of {h}x{w}")
    check(lib().bem_mc_accum_f32(_p(raw), _p(final), _p(state.sum), _p(state.mean), _p(state.m2), B, Nc, state.n, Hp, Wp, h, w, _stream()),
          "mc_accum")
    state.n += Nc


def _mc_finish_cost(state, mean, spread, **_):
    per = 4.0 * state.B * 3 * state.h * state.w
    return (2 * per if mean else 0.0) + (2 * per if spread else 0.0), 0.0


@_bracket(_mc_finish_cost)
def mc_finish(state, target=None, gt_mean=False, mean=True, spread=False):
    """What ``state`` holds after its ``state.n`` samples: ``mean`` -> mc (B,3,h,w), bit for bit mc_mean of the same raw outputs; ``spread`` ->
    the unbiased per-pixel std of the candidates (B,3,h,w), zeros for one sample, and its mean per image (B) f64 (fixed summation order).
    Returns (mc | None, std | None, std_mean | None)."""
    _chk(target, "target", optional=True)
    B, h, w = state.B, state.h, state.w
    if state.n < 1:
        raise ValueError("mc_finish: no samples accumulated")
    if (mean and state.sum is None) or (spread and state.m2 is None) or not (mean or spread):
        raise ValueError("mc_finish: the state has no plane for what is asked")
    gt_mean = bool(gt_mean and mean)
    if gt_mean and (target is None or tuple(target.shape) != (B, 3, h, w)):
        raise ValueError("mc_finish: shapes")
    dev = (state.sum if mean else state.m2).device
    mc = torch.empty(B, 3, h, w, device=dev, dtype=torch.float32) if mean else None
    sd = torch.empty(B, 3, h, w, device=dev, dtype=torch.float32) if spread else None
    sm = torch.empty(B, device=dev, dtype=torch.float64) if spread else None
    ws = torch.empty(258 * B, device=dev, dtype=torch.float64)
    check(lib().bem_mc_finish_f32(_p(state.sum if mean else None), _p(state.m2 if spread else None), _p(target if gt_mean else None), _p(mc),
                                  _p(sd), _p(sm), _p(ws), B, state.n, h, w, int(gt_mean), _stream()), "mc_finish")
    return mc, sd, sm


class BestState:
    """The running choice of a streamed single-score selection: best (B) int32, score (B), images (B,3,h,w) | None, over ``n`` samples."""

    def __init__(self, B, image_shape, device, rule):
        if rule not in ("max", "min"):
            raise ValueError(f"select_merge: rule {rule!r} cannot be decided chunk by chunk ('max' or 'min')")
        _images("select_merge", B, 1)
        self.B, self.rule, self.n = B, rule, 0
        self.best = torch.zeros(B, device=device, dtype=torch.int32)
        self.score = torch.zeros(B, device=device, dtype=torch.float32)
        self.images = torch.zeros((B,) + tuple(image_shape), device=device, dtype=torch.float32) if image_shape is not None else None
        self.pick = torch.empty(B, device=device, dtype=torch.int32)


def _select_merge_cost(state, final, **_):
    return (8.0 * state.images.numel() if state.images is not None else 0.0), 0.0


@_bracket(_select_merge_cost)
def select_merge(state, final, scores, samples_per_image):
    """Folds one chunk -- scores (B*Nc), final (B*Nc,3,h,w) | None, row = image*Nc + sample, chunks in sample order -- into the running
    choice: it changes only where the chunk holds a strictly better score (f64 comparison), so the result equals select_scores with
    the same rule over all samples at once, first index on ties."""
    _chk(scores, "scores"); _chk(final, "final", optional=True)
    B, Nc = state.B, samples_per_image
    if Nc < 1 or scores.numel() != B * Nc:
        raise ValueError(f"select_merge: {scores.numel()} scores are not {Nc} samples of {B} images")
    if (final is None) != (state.images is None) or (final is not None and tuple(final.shape) != (B * Nc,) + tuple(state.images.shape[1:])):
        raise ValueError("select_merge: shapes")
    check(lib().bem_select_merge_f32(_p(final), _p(scores), SELECT_RULES[state.rule], _p(state.best), _p(state.score), _p(state.images),
                                     _p(state.pick), B, Nc, state.n, (state.images[0].numel() if final is not None and B else 0), _stream()),
          "select_merge")
    state.n += Nc


# NIQE (basicsr/metrics/niqe.py as Enhancement/eval.py:248-254 calls it).  Its tables (bem.tables): the AGGD shape grid, and per cropped
# length the weights and source indices of the x0.5 resize.
NIQE_BLOCK = 96


def _niqe_tables(device, Hc, Wc):
    return (_tables("niqe_gamma", device, niqe_gamma_table),
            *(_tables(("niqe_resize", n), device, lambda: niqe_resize_table(n)) for n in (Hc, Wc)))


def niqe(final, params):
    """NIQE per candidate: final (Bn,3,h,w) f32 in [0,1] (RGB, clipped, GT-mean rescaled: BEMPipeline's ``final``), params a
    bem.scorers.NiqeParams (mu (36,), cov (36,36), window (7,7), f64 on the device) -> (Bn) f64 on the device, lower is better.
    A candidate with fewer than 2 NaN-free block rows (a flat image) scores NaN."""
    _chk(final, "final")
    _chk(params.mu, "mu_pris", torch.float64); _chk(params.cov, "cov_pris", torch.float64); _chk(params.window, "window", torch.float64)
    if final.dim() != 4 or final.shape[1] != 3:
        raise ValueError("niqe: final must be (Bn,3,h,w)")
    Bn, _, h, w = final.shape
    if h < NIQE_BLOCK or w < NIQE_BLOCK:
        raise ValueError(f"niqe: images must be at least {NIQE_BLOCK} x {NIQE_BLOCK}, got {h} x {w}")
    if params.mu.numel() != 36 or tuple(params.cov.shape) != (36, 36) or tuple(params.window.shape) != (7, 7):
        raise ValueError("niqe: pristine parameters must be mu (36), cov (36,36), window (7,7)")
    dev = final.device
    tab, (wh, ih), (ww, iw) = _niqe_tables(dev, h // NIQE_BLOCK * NIQE_BLOCK, w // NIQE_BLOCK * NIQE_BLOCK)
    out = torch.empty(Bn, device=dev, dtype=torch.float64)
    if Bn == 0:
        return out
    ws = _scratch("niqe", dev, int(lib().bem_niqe_ws_bytes(Bn, h, w)), torch.uint8)
    check(lib().bem_niqe_f32(_p(final), _p(params.mu), _p(params.cov), _p(params.window), _p(tab), tab.shape[1], _p(wh), _p(ih), wh.shape[1],
                             _p(ww), _p(iw), ww.shape[1], _p(out), _p(ws), ws.numel(), Bn, h, w, _stream()), "niqe")
    return out


# UIQM / UCIQE (basicsr/metrics/uciqe_uiqm.py as Enhancement/eval.py:255-260 calls them).  Their tables (bem.tables): per (source length,
# target length) Pillow's BICUBIC coefficients, and OpenCV's 8-bit RGB -> Lab tables.
UIQM_WINDOW = 10                    # UIQM_WIDTH (256) comes from bem.tables, whose builders read it


def _uiqm_tables(device, h, w, Hr):
    return (_tables("uiqm_lab", device, lab_tables),
            *(_tables(("uiqm_resize", n_in, n_out), device, lambda: pil_resize_table(n_in, n_out)) for n_in, n_out in ((w, UIQM_WIDTH), (h, Hr))))


def uiqm_uciqe(final, debug=False):
    """UIQM and UCIQE per candidate: final (Bn,3,h,w) f32 in [0,1] (RGB, clipped, GT-mean rescaled: BEMPipeline's ``final``) ->
    (uiqm (Bn) f64, uciqe (Bn) f64) on the device, higher is better.  UIQM is computed on the image resized to width 256 and needs
    int(256 / w * h) >= 10 rows; a candidate with a channel without Sobel edges (a flat plane) has NaN UIQM.
    debug=True also returns a dict of device views into the workspace, valid until the next call on this stream: ``parts`` (Bn, 8) f64
    (uicm, uism, uiconm, uiqm, var_chr, con_lum, aver_sat, uciqe), ``resized`` (Bn,3,Hr,256) u8 and ``lab`` (Bn,3,h,w) u8."""
    _chk(final, "final")
    if final.dim() != 4 or final.shape[1] != 3:
        raise ValueError("uiqm_uciqe: final must be (Bn,3,h,w)")
    Bn, _, h, w = final.shape
    if h < 1 or w < 1:
        raise ValueError("uiqm_uciqe: empty images")
    Hr = uiqm_resized_rows(h, w)
    if Hr < UIQM_WINDOW:
        raise ValueError(f"uiqm_uciqe: a {h} x {w} image resizes to {Hr} x {UIQM_WIDTH} (int(256 * h / w) rows); UIQM needs at least "
                         f"{UIQM_WINDOW} rows, i.e. h / w >= {UIQM_WINDOW / UIQM_WIDTH:.4f}")
    dev = final.device
    u1 = torch.empty(Bn, device=dev, dtype=torch.float64)
    u2 = torch.empty(Bn, device=dev, dtype=torch.float64)
    if Bn == 0:
        return (u1, u2, None) if debug else (u1, u2)
    tab, (bh, kh), (bv, kv) = _uiqm_tables(dev, h, w, Hr)
    ws = _scratch("uiqm", dev, int(lib().bem_uiqm_ws_bytes(Bn, h, w, Hr)), torch.uint8)
    check(lib().bem_uiqm_uciqe_f32(_p(final), _p(tab), _p(bh), _p(kh), kh.shape[1], _p(bv), _p(kv), kv.shape[1], _p(u1), _p(u2), _p(ws),
                                   ws.numel(), Bn, h, w, Hr, _stream()), "uiqm_uciqe")
    if not debug:
        return u1, u2
    up = lambda n: (n + 255) // 256 * 256
    o_rs = up(Bn * 64)
    o_lab = o_rs + up(Bn * 3 * Hr * UIQM_WIDTH)
    views = dict(parts=ws[:Bn * 64].view(torch.float64).reshape(Bn, 8),
                 resized=ws[o_rs:o_rs + Bn * 3 * Hr * UIQM_WIDTH].reshape(Bn, 3, Hr, UIQM_WIDTH),
                 lab=ws[o_lab:o_lab + Bn * 3 * h * w].reshape(Bn, 3, h, w))
    return u1, u2, views


# --------------------------------------------------------------------------- training step ----
# Backward kernels + optimizer.  Parameter-gradient outputs (dw, dbias, dgamma, ...) are
# ACCUMULATED INTO: they are views of the parameters' .grad buffers.
def l1_loss(pred, gt, weight=1.0):
    """loss (1,) = weight * mean |pred - gt|."""
    _chk(pred, "pred"); _chk(gt, "gt")
    if pred.shape != gt.shape:
        raise ValueError("l1_loss: shapes differ")
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    ws = torch.empty(1, device=pred.device, dtype=torch.float64)
    check(lib().bem_l1_loss_f32(_p(pred), _p(gt), _p(None), _p(loss), _p(ws), pred.numel(), float(weight), _p(None), _stream()), "l1_loss")
    return loss


def l1_loss_bwd(pred, gt, weight=1.0, gmul=None):
    """dpred = gmul * weight * sign(pred - gt) / numel  (gmul: device scalar dL/dloss, None = 1)."""
    _chk(pred, "pred"); _chk(gt, "gt"); _chk(gmul, "gmul", optional=True)
    dp = torch.empty_like(pred)
    ws = torch.empty(1, device=pred.device, dtype=torch.float64)
    check(lib().bem_l1_loss_f32(_p(pred), _p(gt), _p(dp), _p(None), _p(ws), pred.numel(), float(weight), _p(gmul), _stream()), "l1_loss_bwd")
    return dp


def mse_loss(pred, gt, weight=1.0):
    """loss (1,) = weight * mean (pred - gt)^2."""
    _chk(pred, "pred"); _chk(gt, "gt")
    if pred.shape != gt.shape:
        raise ValueError("mse_loss: shapes differ")
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    ws = torch.empty(1, device=pred.device, dtype=torch.float64)
    check(lib().bem_mse_loss_f32(_p(pred), _p(gt), _p(None), _p(loss), _p(ws), pred.numel(), float(weight), _p(None), _stream()), "mse_loss")
    return loss


def mse_loss_bwd(pred, gt, weight=1.0, gmul=None):
    """dpred = gmul * weight * 2 (pred - gt) / numel  (gmul: device scalar dL/dloss, None = 1)."""
    _chk(pred, "pred"); _chk(gt, "gt"); _chk(gmul, "gmul", optional=True)
    if pred.shape != gt.shape:
        raise ValueError("mse_loss_bwd: shapes differ")
    dp = torch.empty_like(pred)
    ws = torch.empty(1, device=pred.device, dtype=torch.float64)
    check(lib().bem_mse_loss_f32(_p(pred), _p(gt), _p(dp), _p(None), _p(ws), pred.numel(), float(weight), _p(gmul), _stream()), "mse_loss_bwd")
    return dp


def _charbonnier(what, pred, gt, dp, loss, weight, eps, gmul):
    if pred.shape != gt.shape:
        raise ValueError(f"{what}: shapes differ")
    if not eps >= 0:
        raise ValueError(f"{what}: eps {eps} must be >= 0")
    n = pred.numel()
    ws = torch.empty(int(lib().bem_charbonnier_loss_ws_elems(n)), device=pred.device, dtype=torch.float64)
    check(lib().bem_charbonnier_loss_f32(_p(pred), _p(gt), _p(dp), _p(loss), _p(ws), n, float(weight), float(eps), _p(gmul), _stream()), what)


def charbonnier_loss(pred, gt, weight=1.0, eps=1e-12):
    """loss (1,) = weight * mean sqrt((pred - gt)^2 + eps), the same bits from call to call."""
    _chk(pred, "pred"); _chk(gt, "gt")
    loss = torch.empty(1, device=pred.device, dtype=torch.float32)
    _charbonnier("charbonnier_loss", pred, gt, None, loss, weight, eps, None)
    return loss


def charbonnier_loss_bwd(pred, gt, weight=1.0, eps=1e-12, gmul=None):
    """dpred = gmul * weight * (pred - gt) / sqrt((pred - gt)^2 + eps) / numel  (gmul: device scalar dL/dloss, None = 1)."""
    _chk(pred, "pred"); _chk(gt, "gt"); _chk(gmul, "gmul", optional=True)
    dp = torch.empty_like(pred)
    _charbonnier("charbonnier_loss_bwd", pred, gt, dp, None, weight, eps, gmul)
    return dp


SSIM_WINDOW = 11          # the Gaussian window of the SSIM loss (sigma 1.5): the valid region of an H x W plane is (H - 10) x (W - 10)


def ssim_loss_tile():
    """Edge of the square tile one workgroup of the SSIM-loss kernels takes (csrc/ssim_loss.hip)."""
    return int(lib().bem_ssim_loss_tile())


def _ssim_loss_planes(op, pred, gt):
    """Operand check shared by the SSIM loss and its backward -> (planes, H, W)."""
    _chk(pred, "pred"); _chk(gt, "gt")
    if pred.dim() != 4 or pred.shape != gt.shape:
        raise ValueError(f"{op}: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must be one (B,C,H,W) shape")
    B, C, H, W = pred.shape
    if H < SSIM_WINDOW or W < SSIM_WINDOW:
        raise ValueError(f"{op}: {H} x {W} planes are smaller than the {SSIM_WINDOW}x{SSIM_WINDOW} window")
    if B * C == 0:
        raise ValueError(f"{op}: empty tensor")
    return B * C, H, W


def _ssim_valid(pred):
    return _prod(pred.shape[:2]) * (pred.shape[2] - SSIM_WINDOW + 1) * (pred.shape[3] - SSIM_WINDOW + 1)


def ssim_loss_cost(pred, want_grad=False, **_):
    """Algorithmic (bytes, flops) of the forward: pred and gt read once, the three coefficient maps written when a gradient is wanted;
    5 separable 11-tap filters (2 x 11 multiply-adds per position and map, at the valid region's size) and ~40 flops of map arithmetic."""
    nv = _ssim_valid(pred)
    return 8.0 * pred.numel() + (12.0 * nv if want_grad else 0.0), nv * (5 * 2 * 2 * SSIM_WINDOW + 40.0)


def ssim_loss_bwd_cost(pred, **_):
    """Algorithmic (bytes, flops) of the backward: the three maps, pred and gt read once, dpred written; 3 separable filters + 5 flops."""
    return 12.0 * _ssim_valid(pred) + 12.0 * pred.numel(), pred.numel() * (3 * 2 * 2 * SSIM_WINDOW + 5.0)


@_bracket(ssim_loss_cost)
def ssim_loss(pred, gt, weight=1.0, want_grad=False):
    """loss (1,) = weight * (1 - mean SSIM(pred, gt)) on (B,C,H,W) tensors in [0,1]: 11x11 Gaussian window (sigma 1.5), valid region,
    every (b,c) plane on its own (my_loss.py:37-38).  ``want_grad``: also the backward's coefficient maps (3,B,C,H-10,W-10), written by
    the same launch -> (loss, coef)."""
    P, H, W = _ssim_loss_planes("ssim_loss", pred, gt)
    dev = pred.device
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    coef = torch.empty((3,) + tuple(pred.shape[:2]) + (H - SSIM_WINDOW + 1, W - SSIM_WINDOW + 1), device=dev, dtype=torch.float32) if want_grad else None
    ws = _scratch("ssim_loss", dev, int(lib().bem_ssim_loss_ws_elems(P, H, W)), torch.float64)
    check(lib().bem_ssim_loss_f32(_p(pred), _p(gt), _p(loss), _p(coef), _p(ws), P, H, W, float(weight), _stream()), "ssim_loss")
    return (loss, coef) if want_grad else loss


@_bracket(ssim_loss_bwd_cost)
def ssim_loss_bwd(pred, gt, coef, weight=1.0, gmul=None):
    """dpred of ssim_loss from the coefficient maps its forward wrote (gmul: device scalar dL/dloss, None = 1)."""
    P, H, W = _ssim_loss_planes("ssim_loss_bwd", pred, gt)
    _chk(coef, "coef"); _chk(gmul, "gmul", optional=True)
    if tuple(coef.shape) != (3,) + tuple(pred.shape[:2]) + (H - SSIM_WINDOW + 1, W - SSIM_WINDOW + 1):
        raise ValueError(f"ssim_loss_bwd: coef {tuple(coef.shape)} is not the three valid-region maps of pred {tuple(pred.shape)}")
    dp = torch.empty_like(pred)
    check(lib().bem_ssim_loss_bwd_f32(_p(pred), _p(gt), _p(coef), _p(dp), P, H, W, float(weight), _p(gmul), _stream()), "ssim_loss_bwd")
    return dp


PIXSTAT_VALUES = ("loss", "smooth_l1", "mse", "psnr", "color", "hist")     # what pixstat_loss returns, in this order
PIXSTAT_BINS = 256


def pixstat_loss_chunk():
    """Elements one workgroup of the pixstat kernels takes of a sample (csrc/pixstat_loss.hip); samples of at most a quarter of it go to
    workgroups whole."""
    return int(lib().bem_pixstat_loss_chunk())


def _pixstat_samples(op, pred, gt):
    """Operand check shared by the pixstat loss and its backward -> (B, C*H*W)."""
    _chk(pred, "pred"); _chk(gt, "gt")
    if pred.dim() != 4 or pred.shape != gt.shape:
        raise ValueError(f"{op}: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must be one (B,C,H,W) shape")
    if pred.device != gt.device:
        raise ValueError(f"{op}: pred is on {pred.device}, gt on {gt.device}")
    if pred.numel() == 0:
        raise ValueError(f"{op}: empty tensor")
    return pred.shape[0], _prod(pred.shape[1:])


def _pixstat_alphas(op, alphas):
    a = tuple(float(v) for v in alphas)
    if len(a) != 4 or not all(v >= 0 for v in a):
        raise ValueError(f"{op}: alphas = (smooth_l1, hist, psnr, color) weights, each >= 0, got {alphas}")
    return a


def pixstat_loss_cost(pred, **_):
    """Algorithmic (bytes, flops) of the forward: pred and gt read once; ~12 flops and two bin indices per element."""
    return 8.0 * pred.numel(), 12.0 * pred.numel()


def pixstat_loss_bwd_cost(pred, **_):
    """Algorithmic (bytes, flops) of the backward: pred and gt read once, dpred written; 7 flops per element."""
    return 12.0 * pred.numel(), 7.0 * pred.numel()


@_bracket(pixstat_loss_cost)
def pixstat_loss(pred, gt, alphas, want_grad=False, return_hist=False):
    """The per-pixel statistics of CombinedLoss (my_loss.py:51-74) on (B,C,H,W) tensors, one pass: values (6,) f32 = PIXSTAT_VALUES, i.e.
    a1 smooth_l1 + a3 hist + a5 psnr + a6 color for ``alphas`` = (a1, a3, a5, a6) followed by the unweighted smooth_l1, mse, psnr =
    40 - 20 log10(1 / sqrt(mse)), color and hist.  ``want_grad``: also the backward's record (2 + B,) f64.  ``return_hist``: also the
    counts (2, 256) int64 of torch.histc(pred, 256, 0, 1) and of gt.  Returns the values, or a tuple values[, rec][, hist]."""
    B, n1 = _pixstat_samples("pixstat_loss", pred, gt)
    a = _pixstat_alphas("pixstat_loss", alphas)
    dev = pred.device
    vals = torch.empty(len(PIXSTAT_VALUES), device=dev, dtype=torch.float32)
    rec = torch.empty(2 + B, device=dev, dtype=torch.float64) if want_grad else None
    nb = int(lib().bem_pixstat_loss_ws_bytes(B, n1))               # 0: a size the call below refuses by name
    ws = _scratch("pixstat_loss", dev, max(nb, 8) // 8, torch.float64)
    check(lib().bem_pixstat_loss_f32(_p(pred), _p(gt), _p(vals), _p(rec), _p(ws), B, n1, *a, _stream()), "pixstat_loss")
    out = (vals,) + ((rec,) if want_grad else ())
    if return_hist:
        out += (ws[:PIXSTAT_BINS].view(torch.int32).reshape(2, PIXSTAT_BINS).to(torch.int64) & 0xFFFFFFFF,)
    return out if len(out) > 1 else vals


@_bracket(pixstat_loss_bwd_cost)
def pixstat_loss_bwd(pred, gt, rec, gmul=None):
    """dpred of pixstat_loss from the record its forward wrote (gmul: device scalar dL/dloss, None = 1)."""
    B, n1 = _pixstat_samples("pixstat_loss_bwd", pred, gt)
    _chk(rec, "rec", dtype=torch.float64); _chk(gmul, "gmul", optional=True)
    if tuple(rec.shape) != (2 + B,):
        raise ValueError(f"pixstat_loss_bwd: rec {tuple(rec.shape)} is not the record (2 + B,) of pred {tuple(pred.shape)}")
    dp = torch.empty_like(pred)
    check(lib().bem_pixstat_loss_bwd_f32(_p(pred), _p(gt), _p(rec), _p(dp), B, n1, _p(gmul), _stream()), "pixstat_loss_bwd")
    return dp


def iwt_hamilton_bwd(q1w, q2w, dout):
    _chk(q1w, "q1w"); _chk(q2w, "q2w"); _chk(dout, "dout")
    B, C, h, w = q1w.shape
    if C != 16 or q2w.shape != q1w.shape or tuple(dout.shape) != (B, 3, 2 * h, 2 * w):
        raise ValueError("iwt_hamilton_bwd: shapes")
    d1, d2 = torch.empty_like(q1w), torch.empty_like(q2w)
    check(lib().bem_iwt_hamilton_bwd_f32(_p(q1w), _p(q2w), _p(dout), _p(d1), _p(d2), B, h, w, _stream()), "iwt_hamilton_bwd")
    return d1, d2


def pixel_unshuffle2(x):
    """nn.PixelUnshuffle(2): (B,C,2H,2W) -> (B,4C,H,W)."""
    _chk(x, "x")
    B, C, H2, W2 = x.shape
    if H2 % 2 or W2 % 2:
        raise ValueError("pixel_unshuffle2: even H, W required")
    out = torch.empty(B, 4 * C, H2 // 2, W2 // 2, device=x.device, dtype=x.dtype)
    check(lib().bem_pixel_unshuffle2_f32(_p(x), _p(out), B, C, H2 // 2, W2 // 2, _stream()), "pixel_unshuffle2")
    return out


def channel_sum_(x, out):
    """out[c] += sum_{b,p} x[b][c][p]."""
    _chk(x, "x"); _chk(out, "out")
    B, C = x.shape[0], x.shape[1]
    if out.numel() != C:
        raise ValueError("channel_sum: out size")
    check(lib().bem_channel_sum_f32(_p(x), _p(out), B, C, x[0, 0].numel(), _stream()), "channel_sum")
    return out


def add(a, b, alpha=1.0):
    """a + alpha * b."""
    _chk(a, "a"); _chk(b, "b")
    if a.shape != b.shape:
        raise ValueError("add: shapes differ")
    out = torch.empty_like(a)
    check(lib().bem_add_f32(_p(a), _p(b), _p(out), a.numel(), float(alpha), _stream()), "add")
    return out


# --------------------------------------------------------------------------- perceptual loss --
# What runs between the convolutions of the VGG19 feature pass (percep.hip; bem.autograd.PerceptualFn is the caller).
def vgg_prep(pred, gt, input_norm=True, range_norm=False):
    """pred, gt (B,3,H,W) -> (2B,8,H,W): rows [0,B) pred, [B,2B) gt, channels 0..2 normalised (vgg_arch.py:150-153), 3..7 zero."""
    _chk(pred, "pred"); _chk(gt, "gt")
    if pred.dim() != 4 or pred.shape[1] != 3 or pred.shape != gt.shape:
        raise ValueError(f"vgg_prep: two (B,3,H,W) tensors of one shape required, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    B, _, H, W = pred.shape
    xn = torch.empty(2 * B, 8, H, W, device=pred.device, dtype=torch.float32)
    check(lib().bem_vgg_prep_f32(_p(pred), _p(gt), _p(xn), B, H, W, int(bool(input_norm)), int(bool(range_norm)), _stream()), "vgg_prep")
    return xn


def vgg_prep_bwd(dxn, B, input_norm=True, range_norm=False):
    """dpred (B,3,H,W) from channels 0..2 of the first B rows of dxn (rows >= B, C >= 3, H, W)."""
    _chk(dxn, "dxn")
    if dxn.dim() != 4 or dxn.shape[1] < 3 or not 0 <= B <= dxn.shape[0]:
        raise ValueError(f"vgg_prep_bwd: dxn {tuple(dxn.shape)} does not hold {B} rows of three planes")
    _, C, H, W = dxn.shape
    dpred = torch.empty(B, 3, H, W, device=dxn.device, dtype=torch.float32)
    check(lib().bem_vgg_prep_bwd_f32(_p(dxn), C * H * W, _p(dpred), B, H, W, int(bool(input_norm)), int(bool(range_norm)), _stream()),
          "vgg_prep_bwd")
    return dpred


def _pool_planes(op, x):
    if x.dim() < 2 or x.shape[-2] < 2 or x.shape[-1] < 2:
        raise ValueError(f"{op}: planes of at least 2 x 2 required, got {tuple(x.shape)}")
    return _prod(x.shape[:-2]), x.shape[-2], x.shape[-1]


def maxpool2(x):
    """nn.MaxPool2d(2, 2) over the last two dimensions (floor: an odd last row / column is dropped)."""
    _chk(x, "x")
    P, H, W = _pool_planes("maxpool2", x)
    out = torch.empty(tuple(x.shape[:-2]) + (H // 2, W // 2), device=x.device, dtype=torch.float32)
    check(lib().bem_maxpool2_f32(_p(x), _p(out), P, H, W, _stream()), "maxpool2")
    return out


def relu_pool_bwd(y, dpool):
    """Gradient of maxpool2(y) with respect to the input of the ReLU that made y: dpool at each window's first maximum where y > 0."""
    _chk(y, "y"); _chk(dpool, "dpool")
    P, H, W = _pool_planes("relu_pool_bwd", y)
    if tuple(dpool.shape) != tuple(y.shape[:-2]) + (H // 2, W // 2):
        raise ValueError(f"relu_pool_bwd: dpool {tuple(dpool.shape)} is not the pooled shape of y {tuple(y.shape)}")
    dy = torch.empty_like(y)
    check(lib().bem_relu_pool_bwd_f32(_p(y), _p(dpool), _p(dy), P, H, W, _stream()), "relu_pool_bwd")
    return dy


def relu_bwd(y, dy, inplace=False):
    """dy * (y > 0); ``inplace`` writes into dy."""
    _chk(y, "y"); _chk(dy, "dy")
    if y.shape != dy.shape:
        raise ValueError("relu_bwd: shapes differ")
    out = dy if inplace else torch.empty_like(dy)
    check(lib().bem_relu_bwd_f32(_p(y), _p(dy), _p(out), y.numel(), _stream()), "relu_bwd")
    return out


def relu(x):
    _chk(x, "x")
    out = torch.empty_like(x)
    check(lib().bem_relu_f32(_p(x), _p(out), x.numel(), _stream()), "relu")
    return out


# --------------------------------------------------------------------------- LPIPS -------------
# What runs around the five convolutions of LPIPS v0.1 / AlexNet (lpips.hip; bem.lpips.LPIPS is the caller).
LPIPS_MIN_HW = 31          # 31 -> 7 (conv1) -> 3 (pool) -> 1 (pool): below it the second pool has no output


def lpips_conv1_hw(H, W):
    """Output size of AlexNet's first convolution (11x11, stride 4, pad 2)."""
    return (H - 7) // 4 + 1, (W - 7) // 4 + 1


def lpips_prep(ref, pred, quantise=True, normalize=False):
    """ref, pred (B,3,H,W) -> (2B,48,Hb,Wb), rows [0,B) ref and [B,2B) pred: img_as_ubyte and im2tensor (``quantise``: inputs in [0,1]) or
    2 x - 1 (``normalize``: inputs in [0,1], not quantised) or neither (inputs in [-1,1] already), the scaling layer, and the 4x4 space-to-depth block layout conv1 reads (include/bem_hip.h: bem_lpips_prep_f32)."""
    _chk(ref, "ref"); _chk(pred, "pred")
    if ref.dim() != 4 or ref.shape[1] != 3 or ref.shape != pred.shape:
        raise ValueError(f"lpips_prep: two (B,3,H,W) tensors of one shape required, got {tuple(ref.shape)} and {tuple(pred.shape)}")
    B, _, H, W = ref.shape
    if H < LPIPS_MIN_HW or W < LPIPS_MIN_HW:
        raise ValueError(f"lpips_prep: images of at least {LPIPS_MIN_HW} x {LPIPS_MIN_HW} required, got {H} x {W}")
    Ho, Wo = lpips_conv1_hw(H, W)
    xs = torch.empty(2 * B, 48, Ho + 2, (Wo + 3) // 2 * 2, device=ref.device, dtype=torch.float32)
    check(lib().bem_lpips_prep_f32(_p(ref), _p(pred), _p(xs), B, H, W, 1 if quantise else 2 if normalize else 0, _stream()), "lpips_prep")
    return xs


def _plane_view(op, x, lead):
    """Checks a float32 device tensor whose last two dimensions may be a crop of a wider plane (unit stride along the last one) and whose
    ``lead`` dimensions before them are evenly strided; returns the strides of those dimensions and of the rows."""
    if not x.is_cuda:
        raise native.BemNativeError(f"{op}: x must be a CUDA/HIP tensor: the BEM hot path has no CPU implementation")
    if x.dtype != torch.float32:
        raise TypeError(f"{op}: x must be float32, got {x.dtype}")
    if x.dim() != lead + 2 or x.stride(-1) != 1 or min(x.shape) < 1:
        raise ValueError(f"{op}: a non-empty {lead + 2}-dimensional tensor with unit stride along the last dimension required, got "
                         f"{tuple(x.shape)} / {x.stride()}")
    return x.stride()[:-1]


def maxpool3s2(x):
    """nn.MaxPool2d(3, 2) over the last two dimensions of x (B,C,H,W), floor mode (leftover rows / columns are dropped); x may be a crop of
    a wider contiguous tensor (conv1's output inside its block grid)."""
    bs, cs, rs = _plane_view("maxpool3s2", x, 2)
    B, C, H, W = x.shape
    if H < 3 or W < 3:
        raise ValueError(f"maxpool3s2: planes of at least 3 x 3 required, got {tuple(x.shape)}")
    if B != 1 and bs != C * cs:
        raise ValueError(f"maxpool3s2: planes are not evenly strided ({x.stride()})")
    out = torch.empty(B, C, (H - 3) // 2 + 1, (W - 3) // 2 + 1, device=x.device, dtype=torch.float32)
    check(lib().bem_maxpool3s2_f32(_p(x), cs, rs, _p(out), B * C, H, W, _stream()), "maxpool3s2")
    return out


def lpips_layer(feat, lin, ws=None, out=None, first=True):
    """Distance head of one layer: feat (2B,C,h,w) (rows b and B + b are pair b; may be a crop of a wider tensor), lin (C) -> (out (B) f32,
    ws).  ``first`` starts the f64 running sum in ws from zero; later layers pass the returned ws and out back and add to it."""
    bs, cs, rs = _plane_view("lpips_layer", feat, 2)
    _chk(lin, "lin")
    B2, C, h, w = feat.shape
    if B2 % 2 or lin.numel() != C:
        raise ValueError(f"lpips_layer: feat {tuple(feat.shape)} needs an even number of rows and lin {tuple(lin.shape)} one weight per channel")
    B = B2 // 2
    need = lib().bem_lpips_layer_ws_elems(B, h, w)
    if ws is None or ws.numel() < need:
        if not first:
            raise ValueError("lpips_layer: a later layer needs the workspace of the first (it holds the running sum)")
        ws = torch.empty(need, device=feat.device, dtype=torch.float64)
    _chk(ws, "ws", dtype=torch.float64)
    if out is None:
        out = torch.empty(B, device=feat.device, dtype=torch.float32)
    _chk(out, "out")
    if out.numel() != B:
        raise ValueError("lpips_layer: out shape")
    check(lib().bem_lpips_layer_f32(_p(feat), bs, cs, rs, _p(lin), _p(ws), ws.numel(), _p(out), B, C, h, w, int(bool(first)), _stream()),
          "lpips_layer")
    return out, ws


def lpips_mean(ws, B, weight=1.0):
    """loss (1,) = weight * mean of the B distances whose f64 running sums the last lpips_layer call left in ws[:B]."""
    _chk(ws, "ws", dtype=torch.float64)
    if not 1 <= B <= ws.numel():
        raise ValueError(f"lpips_mean: {B} distances in a workspace of {ws.numel()}")
    loss = torch.empty(1, device=ws.device, dtype=torch.float32)
    check(lib().bem_lpips_mean_f32(_p(ws), _p(loss), B, float(weight), _stream()), "lpips_mean")
    return loss


def lpips_layer_bwd(feat, lin, gin=None, gmul=None, scale=1.0, out=None, origin=(0, 0)):
    """Head backward of one layer for the pred rows: feat (2B,C,h,w) and lin as lpips_layer takes them, ``gin`` (B,C,h,w) the gradient reaching
    the same post-ReLU feature from the layer above, ``gmul`` the device scalar dL/dloss (None = 1), ``scale`` = loss_weight / B.  Returns
    (y_pred > 0) ? gin + g : 0, the gradient at the convolution's output before its ReLU (include/bem_hip.h: bem_lpips_layer_bwd_f32).
    ``out`` (B,C,oh,ow), unit stride along its rows, is written as a whole: the result at rows / columns ``origin`` onwards, zero around it."""
    bs, cs, rs = _plane_view("lpips_layer_bwd", feat, 2)
    _chk(lin, "lin"); _chk(gin, "gin", optional=True); _chk(gmul, "gmul", optional=True)
    B2, C, h, w = feat.shape
    if B2 % 2 or B2 == 0 or lin.numel() != C:
        raise ValueError(f"lpips_layer_bwd: feat {tuple(feat.shape)} needs an even number of rows and lin {tuple(lin.shape)} one weight per channel")
    B = B2 // 2
    if gin is not None and tuple(gin.shape) != (B, C, h, w):
        raise ValueError(f"lpips_layer_bwd: gin {tuple(gin.shape)} is not the pred half {(B, C, h, w)} of feat")
    if gmul is not None and gmul.numel() != 1:
        raise ValueError("lpips_layer_bwd: gmul is one device scalar")
    if out is None:
        out = torch.empty(B, C, h + origin[0], w + origin[1], device=feat.device, dtype=torch.float32)
    obs, ocs, ors = _plane_view("lpips_layer_bwd", out, 2)
    oh, ow = out.shape[2:]
    if tuple(out.shape[:2]) != (B, C) or min(origin) < 0 or origin[0] + h > oh or origin[1] + w > ow:
        raise ValueError(f"lpips_layer_bwd: out {tuple(out.shape)} does not hold a {(B, C, h, w)} gradient at {tuple(origin)}")
    check(lib().bem_lpips_layer_bwd_f32(_p(feat), bs, cs, rs, _p(lin), _p(gin), _p(gmul), float(scale), _p(out), obs, ocs, ors, B, C, h, w,
                                        oh, ow, int(origin[0]), int(origin[1]), _stream()), "lpips_layer_bwd")
    return out


def relu_pool3s2_bwd(y, dpool):
    """Gradient of maxpool3s2(y) with respect to y (B,C,H,W), which may be a crop of a wider tensor: dpool at each window's first maximum
    in row-major order (torch's rule), summed where windows overlap, zero elsewhere -> (B,C,H,W) contiguous.  The mask of the ReLU that
    made y is left to lpips_layer_bwd, which takes the result as its ``gin``."""
    bs, cs, rs = _plane_view("relu_pool3s2_bwd", y, 2)
    _chk(dpool, "dpool")
    B, C, H, W = y.shape
    if H < 3 or W < 3:
        raise ValueError(f"relu_pool3s2_bwd: planes of at least 3 x 3 required, got {tuple(y.shape)}")
    if B != 1 and bs != C * cs:
        raise ValueError(f"relu_pool3s2_bwd: planes are not evenly strided ({y.stride()})")
    if tuple(dpool.shape) != (B, C, (H - 3) // 2 + 1, (W - 3) // 2 + 1):
        raise ValueError(f"relu_pool3s2_bwd: dpool {tuple(dpool.shape)} is not the pooled shape of y {tuple(y.shape)}")
    dy = torch.empty(B, C, H, W, device=y.device, dtype=torch.float32)
    check(lib().bem_relu_pool3s2_bwd_f32(_p(y), cs, rs, _p(dpool), _p(dy), B * C, H, W, _stream()), "relu_pool3s2_bwd")
    return dy


def lpips_prep_bwd(gxs, H, W, quantise=False, normalize=False):
    """dpred (B,3,H,W) from gxs (B,48,Hb,Wb), the gradient of the pred rows of lpips_prep's output; ``normalize`` as the forward took it.
    The quantising input stage has no gradient: ``quantise`` is refused by the library."""
    _chk(gxs, "gxs")
    if H < LPIPS_MIN_HW or W < LPIPS_MIN_HW:
        raise ValueError(f"lpips_prep_bwd: images of at least {LPIPS_MIN_HW} x {LPIPS_MIN_HW} required, got {H} x {W}")
    Ho, Wo = lpips_conv1_hw(H, W)
    if gxs.dim() != 4 or gxs.shape[0] < 1 or tuple(gxs.shape[1:]) != (48, Ho + 2, (Wo + 3) // 2 * 2):
        raise ValueError(f"lpips_prep_bwd: gxs {tuple(gxs.shape)} is not the block form (B, 48, {Ho + 2}, {(Wo + 3) // 2 * 2}) of {H} x {W} images")
    B = gxs.shape[0]
    dpred = torch.empty(B, 3, H, W, device=gxs.device, dtype=torch.float32)
    check(lib().bem_lpips_prep_bwd_f32(_p(gxs), _p(dpred), B, H, W, 1 if quantise else 2 if normalize else 0, _stream()), "lpips_prep_bwd")
    return dpred


def _ln_bwd_cost(x1, x2, dres, want_n, **_):
    return 4.0 * x1.numel() * (3 + (x2 is not None) + (dres is not None) + bool(want_n)), 0.0


@_bracket(_ln_bwd_cost)
def ln_bwd(x1, dn, gamma, beta, eps, dgamma, dbeta, x2=None, dres=None, want_n=True):
    """LayerNorm2d backward over channels of x = x1 (+ x2): returns (dx, n = LN(x) | None); dgamma / dbeta accumulated."""
    for n, t in (("x1", x1), ("dn", dn), ("gamma", gamma), ("beta", beta), ("dgamma", dgamma), ("dbeta", dbeta)):
        _chk(t, n)
    _chk(x2, "x2", optional=True); _chk(dres, "dres", optional=True)
    B, C = x1.shape[0], x1.shape[1]
    if dn.shape != x1.shape or (x2 is not None and x2.shape != x1.shape) or (dres is not None and dres.shape != x1.shape):
        raise ValueError("ln_bwd: activation shapes")
    if gamma.numel() != C or beta.numel() != C or dgamma.numel() != C or dbeta.numel() != C:
        raise ValueError("ln_bwd: parameter sizes")
    dx = torch.empty_like(x1)
    nn_ = torch.empty_like(x1) if want_n else None
    check(lib().bem_ln_bwd_f32(_p(x1), _p(x2), _p(dn), _p(gamma), _p(beta), float(eps), _p(dres), _p(dx), _p(nn_), _p(dgamma), _p(dbeta),
                               B, C, x1[0, 0].numel(), _stream()), "ln_bwd")
    return dx, nn_


def ln_fwd(x1, gamma, beta, eps, x2=None):
    _chk(x1, "x1"); _chk(gamma, "gamma"); _chk(beta, "beta"); _chk(x2, "x2", optional=True)
    B, C = x1.shape[0], x1.shape[1]
    if gamma.numel() != C or beta.numel() != C or (x2 is not None and x2.shape != x1.shape):
        raise ValueError("ln_fwd: shapes")
    out = torch.empty_like(x1)
    check(lib().bem_ln_fwd_f32(_p(x1), _p(x2), _p(gamma), _p(beta), float(eps), _p(out), B, C, x1[0, 0].numel(), _stream()), "ln_fwd")
    return out


@_bracket(lambda t, dout, **_: (4.0 * (2 * t.numel() + dout.numel()), 40.0 * t.numel()))
def dwact_bwd(t, w, bias, dout, dw, dbias, mode):
    """Backward of dwconv3x3(mode) through the activation: returns dpre (like t); dw (Cw,1,3,3) / dbias accumulated."""
    _chk(t, "t"); _chk(w, "w"); _chk(bias, "bias", optional=True); _chk(dout, "dout"); _chk(dw, "dw"); _chk(dbias, "dbias", optional=True)
    B, Cw, H, W = t.shape
    Cout = Cw // 2 if mode == 2 else Cw
    if tuple(dout.shape) != (B, Cout, H, W) or w.numel() != Cw * 9 or dw.numel() != Cw * 9 or (bias is None) != (dbias is None):
        raise ValueError("dwact_bwd: shapes")
    if bias is not None and (bias.numel() != Cw or dbias.numel() != Cw):
        raise ValueError("dwact_bwd: bias shapes")
    dpre = torch.empty_like(t)
    check(lib().bem_dwact_bwd_f32(_p(t), _p(w), _p(bias), _p(dout), _p(dpre), _p(dw), _p(dbias), B, Cout, H, W, mode, _stream()), "dwact_bwd")
    return dpre


WGRAD_X6 = os.environ.get("BEM_WGRAD_X6", "1") != "0"      # 1x1 weight gradients on the bf16 matrix cores (no LDS transposes) when L % 32 == 0
# below this many pixels per launch the x6 form's fixed costs (one wave per SIMD, second reduction launch) lose to the f32-MFMA kernel:
# Stage-I training (8 x 8 planes) 34.7 -> 23.8 ms per step
WGRAD_X6_MIN_PIXELS = 16384


def _pw_wgrad_cost(dy, x1, x2, M, **_):
    B, L = x1.shape[0], x1[0, 0].numel()
    M = dy.shape[1] if M is None else M
    K = x1.shape[1] + (0 if x2 is None else x2.shape[1])
    return 4.0 * B * L * (M + K) + 4.0 * M * K, 2.0 * M * K * B * L


@_bracket(_pw_wgrad_cost)
def pw_wgrad_(dy, x1, dw, x2=None, dbias=None, blk_rows=0, perm=(0, 1, 2, 3), dy_bstride=0, M=None):
    """dw (M, C1 + C2) += dy . cat(x1, x2)^T over batch and pixels; dbias (M) += row sums of dy.
    dy may be a channel slice of a wider tensor (pass M and dy_bstride)."""
    _chk(x1, "x1"); _chk(x2, "x2", optional=True); _chk(dw, "dw"); _chk(dbias, "dbias", optional=True)
    if not dy.is_cuda or dy.dtype != torch.float32:
        raise native.BemNativeError("pw_wgrad: dy must be a float32 CUDA/HIP tensor")
    B, C1 = x1.shape[0], x1.shape[1]
    L = x1[0, 0].numel()
    C2 = 0 if x2 is None else x2.shape[1]
    if M is None:
        _chk(dy, "dy")
        M = dy.shape[1]
    if dy.shape[0] != B or (x2 is not None and (x2.shape[0] != B or x2[0, 0].numel() != L)):
        raise ValueError("pw_wgrad: batch / pixel counts")
    if dw.numel() != M * (C1 + C2) or (dbias is not None and dbias.numel() != M):
        raise ValueError(f"pw_wgrad: dw has {dw.numel()} elements, expected {M} x {C1 + C2}")
    a = native.WgradArgs()
    a.dy, a.dy_bstride, a.M = dy.data_ptr(), dy_bstride, M
    a.x1, a.x1_bstride, a.C1 = x1.data_ptr(), 0, C1
    a.x2, a.x2_bstride, a.C2 = (x2.data_ptr() if x2 is not None else 0), 0, C2
    a.dw, a.ldw, a.blk_rows = dw.data_ptr(), C1 + C2, blk_rows
    for i in range(4):
        a.perm[i] = perm[i]
    a.dbias = dbias.data_ptr() if dbias is not None else 0
    a.B, a.L = B, L
    if WGRAD_X6 and L % 32 == 0 and B * L >= WGRAD_X6_MIN_PIXELS:
        ws = _scratch("wgrad_x6", dw.device, max(lib().bem_pw_wgrad_x6_ws_elems(M, C1 + C2, B, L), 1 << 20), torch.float32)
        check(lib().bem_pw_wgrad_x6_f32(ctypes.byref(a), _p(ws), ws.numel(), _stream()), "pw_wgrad_x6")
    else:
        check(lib().bem_pw_wgrad_f32(ctypes.byref(a), _stream()), "pw_wgrad")
    return dw


def _conv_wgrad_cost(dy, x, dw, **_):
    Cout, Cin, KH, KW = dw.shape
    return 4.0 * (dy.numel() + x.shape[0] * Cin * x.shape[2] * x.shape[3]) + 4.0 * dw.numel(), 2.0 * dy.numel() * Cin * KH * KW


@_bracket(_conv_wgrad_cost)
def conv_wgrad_(dy, x, dw, dbias=None, stride=1, pad=1, cin_slice=None):
    """dw (Cout,Cin,KH,KW) += weight gradient of conv2d(x, w, stride, pad); dbias (Cout) += sum dy."""
    _chk(dy, "dy"); _chk(x, "x"); _chk(dw, "dw"); _chk(dbias, "dbias", optional=True)
    B, Ct, H, W = x.shape
    Cout, Cin, KH, KW = dw.shape
    c0 = 0
    if cin_slice is not None:
        c0, cs = cin_slice
        if cs != Cin or c0 + Cin > Ct:
            raise ValueError("conv_wgrad: channel slice")
    elif Ct != Cin:
        raise ValueError("conv_wgrad: channels")
    if tuple(dy.shape) != (B, Cout) + _conv_out_hw(H, W, KH, KW, stride, pad) or (dbias is not None and dbias.numel() != Cout):
        raise ValueError("conv_wgrad: dy / dbias shapes")
    check(lib().bem_conv_wgrad_f32(_p(dy), *_pslice(x, c0), _p(dw), _p(dbias), B, Cin, H, W, Cout,
                                   KH, KW, stride, pad, _stream()), "conv_wgrad")
    return dw


def _head_operand(t, name, shape):
    """A (B,3,H,W) branch output whose planes are contiguous; the batch stride is free (a channel slice of a wider tensor is fine)."""
    if t is None:
        raise ValueError(f"{name} is required")
    if not t.is_cuda:
        raise native.BemNativeError(f"{name} must be a CUDA/HIP tensor: the BEM hot path has no CPU implementation")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    if t.dim() != 4 or (shape is not None and tuple(t.shape) != shape):
        raise ValueError(f"fusion_head: {name} must be {shape or '(B,3,H,W)'}, got {tuple(t.shape)}")
    B, C, H, W = t.shape
    if C != 3:
        raise ValueError(f"fusion_head: {name} has {C} channels; only out_channels 3 is supported")
    if t.stride()[1:] != (H * W, W, 1) and B * H * W > 0:
        raise ValueError(f"fusion_head: {name} planes must be contiguous (strides {t.stride()})")
    return t.stride(0)


def _head_weights(w1, b1, w2, b2):
    for n, t, shp in (("w1", w1, (3, 6, 3, 3)), ("b1", b1, (3,)), ("w2", w2, (3, 3, 3, 3)), ("b2", b2, (3,))):
        if t is None:
            continue
        _chk(t, n)
        if tuple(t.shape) != shp:
            raise ValueError(f"fusion_head: {n} must be {shp} (Conv2d(6,3,3) then Conv2d(3,3,3)), got {tuple(t.shape)}")


def fusion_head(o1, o2, w1=None, b1=None, w2=None, b2=None, mean=False):
    """The output head of the two-branch archs on two (B,3,H,W) branch outputs, without forming their concatenation:
    conv2(relu(conv1(cat(o1, o2)) + b1)) + b2 (w1 (3,6,3,3), w2 (3,3,3,3)), or (o1 + o2) / 2 with ``mean=True``."""
    bs1 = _head_operand(o1, "o1", None)
    B, _, H, W = o1.shape
    bs2 = _head_operand(o2, "o2", (B, 3, H, W))
    if not mean:
        if w1 is None or b1 is None or w2 is None or b2 is None:
            raise ValueError("fusion_head: w1, b1, w2, b2 are required")
        _head_weights(w1, b1, w2, b2)
    out = torch.empty(B, 3, H, W, device=o1.device, dtype=o1.dtype)
    check(lib().bem_fusion_head_f32(_p(o1), bs1, _p(o2), bs2, _p(w1), _p(b1), _p(w2), _p(b2), _p(out), B, 6, 3, H, W, int(bool(mean)),
                                    _stream()), "fusion_head")
    return out


def fusion_head_bwd_(o1, o2, dout, w1=None, b1=None, w2=None, dw1=None, db1=None, dw2=None, db2=None, mean=False):
    """Backward of fusion_head: returns (do1, do2) (B,3,H,W); dw1, db1, dw2, db2 += the weight gradients (``mean=False``)."""
    _chk(dout, "dout")
    if dout.dim() != 4 or dout.shape[1] != 3:
        raise ValueError(f"fusion_head_bwd: dout must be (B,3,H,W), got {tuple(dout.shape)}")
    B, _, H, W = dout.shape
    bs1 = bs2 = 0
    ws = None
    if not mean:
        bs1, bs2 = _head_operand(o1, "o1", (B, 3, H, W)), _head_operand(o2, "o2", (B, 3, H, W))
        if any(t is None for t in (w1, b1, w2, dw1, db1, dw2, db2)):
            raise ValueError("fusion_head_bwd: w1, b1, w2 and the gradient buffers dw1, db1, dw2, db2 are required")
        _head_weights(w1, b1, w2, None)
        _head_weights(dw1, db1, dw2, db2)
        ws = torch.empty(int(lib().bem_fusion_head_bwd_ws_elems(B, H, W)), device=dout.device, dtype=torch.float32)
    do1, do2 = torch.empty_like(dout), torch.empty_like(dout)
    check(lib().bem_fusion_head_bwd_f32(_p(o1), bs1, _p(o2), bs2, _p(dout), _p(w1), _p(b1), _p(w2), _p(do1), _p(do2), _p(dw1), _p(db1),
                                        _p(dw2), _p(db2), _p(ws), 0 if ws is None else ws.numel(), B, 6, 3, H, W, int(bool(mean)), _stream()),
          "fusion_head_bwd")
    return do1, do2


@_bracket(lambda x0, xd0, **_: (4.0 * (6 * x0.numel() + 4 * xd0.numel()), 0.0))
def ss2d_scan_bwd(x0, x1, xd0, xd1, dy0, dy1, dtw, dtb, A, Ds, dAlog, dDs, ddtw, ddtb):
    """Backward of ss2d_scan: returns (dx0, dx1, dxd0, dxd1); parameter gradients accumulated into dAlog (4C), dDs (4C),
    ddtw (4,C,R), ddtb (4,C)."""
    B, C, L, R, _, bs0, bs1 = _scan_operands("ss2d_scan_bwd", False, (("x0", x0), ("x1", x1), ("dy0", dy0), ("dy1", dy1)), xd0, xd1,
                                             dtw, dtb, A, Ds, (dAlog, dDs, ddtw, ddtb))
    dx0, dx1, dxd0, dxd1 = torch.empty_like(x0), torch.empty_like(x0), xd0.new_empty(xd0.shape), xd0.new_empty(xd0.shape)
    check(lib().bem_ss2d_scan_bwd_f32(_p(x0), _p(x1), _p(xd0), _p(xd1), _p(dy0), _p(dy1), _p(dtw), _p(dtb), _p(A), _p(Ds), _p(dx0), _p(dx1),
                                      _p(dxd0), _p(dxd1), _p(dAlog), _p(dDs), _p(ddtw), _p(ddtb), B, C, L, R, bs0, bs1, _stream()),
          "ss2d_scan_bwd")
    return dx0, dx1, dxd0, dxd1


def ss2d_scan_n_bwd(x0, x1, xd0, xd1, dy0, dy1, dtw, dtb, A, Ds, dAlog, dDs, ddtw, ddtb):
    """Backward of ss2d_scan_n: returns (dx0, dx1, dxd0, dxd1), dxd* (B,2,R+2N,L); parameter gradients accumulated into dAlog (4C, N),
    dDs (4C), ddtw (4,C,R), ddtb (4,C)."""
    B, C, L, R, N, bs0, bs1 = _scan_operands("ss2d_scan_n_bwd", True, (("x0", x0), ("x1", x1), ("dy0", dy0), ("dy1", dy1)), xd0, xd1,
                                             dtw, dtb, A, Ds, (dAlog, dDs, ddtw, ddtb))
    dx0, dx1, dxd0, dxd1 = torch.empty_like(x0), torch.empty_like(x0), xd0.new_empty(xd0.shape), xd0.new_empty(xd0.shape)
    ws = torch.empty(max(int(lib().bem_ss2d_scan_n_bwd_ws_elems(B, C, L, N)), 1), device=x0.device, dtype=torch.float32)
    check(lib().bem_ss2d_scan_n_bwd_f32(_p(x0), _p(x1), _p(xd0), _p(xd1), _p(dy0), _p(dy1), _p(dtw), _p(dtb), _p(A), _p(Ds), _p(dx0), _p(dx1),
                                        _p(dxd0), _p(dxd1), _p(dAlog), _p(dDs), _p(ddtw), _p(ddtb), _p(ws), ws.numel(), B, C, L, R, N,
                                        bs0, bs1, _stream()), "ss2d_scan_n_bwd")
    return dx0, dx1, dxd0, dxd1


def grad_sumsq(g, acc):
    """acc (1,) f64 = sum g^2 over the flat gradient buffer."""
    _chk(g, "g"); _chk(acc, "acc", dtype=torch.float64)
    check(lib().bem_grad_sumsq_f32(_p(g), g.numel(), _p(acc), _stream()), "grad_sumsq")
    return acc


def _adam_step(entry, what, p, g, m, v, lr, betas, eps, weight_decay, step, max_norm, sumsq, norm_out, hyper):
    _chk(hyper, "hyper", optional=True)
    for n, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _chk(t, n)
    _chk(sumsq, "sumsq", dtype=torch.float64, optional=True); _chk(norm_out, "norm_out", optional=True)
    n = p.numel()
    if g.numel() != n or m.numel() != n or v.numel() != n:
        raise ValueError(f"{what}: buffer sizes differ")
    check(entry(_p(p), _p(g), _p(m), _p(v), n, float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(step),
                float(max_norm), _p(sumsq), _p(norm_out), _p(hyper), _stream()), what)


def adamw_step_(p, g, m, v, lr, betas, eps, weight_decay, step, max_norm=0.0, sumsq=None, norm_out=None, hyper=None):
    """hyper: optional device tensor [lr, 1 - beta1^t, sqrt(1 - beta2^t)] read by the kernel in place of ``lr`` / ``step``."""
    _adam_step(lib().bem_adamw_step_f32, "adamw_step", p, g, m, v, lr, betas, eps, weight_decay, step, max_norm, sumsq, norm_out, hyper)


def adam_step_(p, g, m, v, lr, betas, eps, weight_decay, step, max_norm=0.0, sumsq=None, norm_out=None, hyper=None):
    """torch.optim.Adam's update (weight decay added to the gradient) with adamw_step_'s arguments."""
    _adam_step(lib().bem_adam_step_f32, "adam_step", p, g, m, v, lr, betas, eps, weight_decay, step, max_norm, sumsq, norm_out, hyper)


@_bracket(lambda ema, **_: (12.0 * ema.numel(), 3.0 * ema.numel()))
def ema_update_(ema, p, decay):
    """ema = decay * ema + (1 - decay) * p in place over two flat f32 buffers of equal length (base_model.py:77-84).  The kernel gets
    torch's two constants, (float)decay and (float)(1 - decay) with the difference taken in double; decay = 0 copies p bit for bit."""
    _chk(ema, "ema"); _chk(p, "p")
    if ema.device != p.device:
        raise ValueError(f"ema_update: ema on {ema.device}, p on {p.device}")
    if ema.numel() != p.numel():
        raise ValueError(f"ema_update: ema holds {ema.numel()} elements, p {p.numel()}")
    decay = float(decay)
    if not 0.0 <= decay <= 1.0:
        raise ValueError(f"ema_update: decay {decay} outside [0, 1]")
    if ema.numel() == 0:                   # nothing to launch, and torch's empty tensors carry the null pointer the library refuses
        return ema
    check(lib().bem_ema_update_f32(_p(ema), _p(p), ema.numel(), decay, 1.0 - decay, _stream()), "ema_update")
    return ema
