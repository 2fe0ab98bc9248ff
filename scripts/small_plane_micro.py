"""Micro-benchmark of every Stage-I pointwise GEMM and depthwise 3x3 shape of the bench (B = 64 samples, per-sample weights, planes 16x16 /
8x8 / 4x4 at C = 40 / 80 / 160), timed with HIP events.  The dispatch thresholds of the small-plane forms (pw_gemm_x6.hip, conv.hip) come
from this table; BEM_HIP_LIB=<other libbem_hip.so> runs the same table on another build."""
import math
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bayesian-enhancement-model_amd"))
import torch
from bem import ops

B, REPS = 64, 50
dev = "cuda"


def timed(f):
    for _ in range(5):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e30
    for _ in range(3):                               # best of three batches of REPS back-to-back launches
        e0.record()
        for _ in range(REPS):
            f()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / REPS)
    return best


def gemm(name, C1, M, H, ln=False, sum_=False, cat=0, bias=True, res=False, convT=False):
    K = C1 + cat
    x1 = torch.randn(B, C1, H, H, device=dev)
    x2 = torch.randn(B, cat or C1, H, H, device=dev) if (sum_ or cat) else None
    Wp = ops.pack_pw_weight(torch.randn(B, M, K, device=dev) * K ** -0.5)
    lnp = (torch.ones(K, device=dev), torch.zeros(K, device=dev)) if ln else None
    bb = torch.randn(B, M, device=dev) if bias else None
    rr = torch.randn(B, M, H, H, device=dev) if res else None
    us = timed(lambda: ops.pw_gemm(x1, Wp, M, x2=x2, in_mode=1 if sum_ else 2 if cat else 0, ln=lnp, bias=bb, res=rr, convT_Win=H if convT else 0))
    by = 4.0 * Wp.numel() + 4.0 * B * H * H * (K * (2 if sum_ else 1) + M * (2 if res else 1))
    print(f"gemm {name:12s} L={H * H:4d} K={K:4d} M={M:5d} kb={math.ceil(K / 16):3d} ln={int(ln)} sum={int(sum_)}: {us:7.1f} us  {by / us / 1e6:6.2f} TB/s")


def dw(name, C, H, mode):
    x = torch.randn(B, C, H, H, device=dev)
    w, b = torch.randn(B, C, 1, 3, 3, device=dev) / 3, torch.randn(B, C, device=dev)
    us = timed(lambda: ops.dwconv3x3(x, w, b, mode))
    print(f"dw   {name:12s} L={H * H:4d} C={C:5d} mode={mode}: {us:7.1f} us")


for C, H in ((40, 16), (80, 8), (160, 4)):
    R = math.ceil(C / 16)
    gemm("in_proj", C, C, H, ln=True)
    gemm("x_proj", C, 4 * (R + 2), H, bias=False)
    gemm("out_proj", C, C, H, ln=True, sum_=True, res=True)
    gemm("project_in", C, 8 * C, H, ln=True)
    gemm("project_out", 4 * C, C, H, res=True)
    if C > 40:
        gemm("up (convT)", C, 4 * (C // 2), H, convT=True)
    if C < 160:
        gemm("fuse (cat)", C, C, H, cat=C, bias=False)
    dw("ss2d conv", C, H, 1)
    dw("gate", 8 * C, H, 2)
