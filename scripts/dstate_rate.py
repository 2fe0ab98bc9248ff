"""GPU time of one VSSBlock (C = 40, 256x256, batch 8) at d_state N = 1, 2, 4, 8, 16: eval forward, and training forward + backward,
timed with HIP events.  Also the scan pair's time alone (bem_ss2d_scan_n_f32 for N > 1, the N = 1 dispatch otherwise) and its
algorithmic bytes: x read twice (one per orientation), x_dbl 2 (R + 2N) planes per orientation, y written once per orientation."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "bayesian-enhancement-model_amd"))
import torch
from bem.modules import VSSBlock

ap = argparse.ArgumentParser()
ap.add_argument("--n", default="1,2,4,8,16")
ap.add_argument("--b", type=int, default=8)
ap.add_argument("--c", type=int, default=40)
ap.add_argument("--hw", type=int, default=256)
ap.add_argument("--iters", type=int, default=10)
a = ap.parse_args()


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


B, C, H = a.b, a.c, a.hw
L = H * H
R = math.ceil(C / 16)
x = torch.randn(B, C, H, H, device="cuda")
for N in [int(v) for v in a.n.split(",")]:
    torch.manual_seed(0)
    blk = VSSBlock(hidden_dim=C, ssm_d_state=N, ssm_ratio=1, ssm_conv_bias=False, forward_type="v05_noz", mlp_ratio=4, mlp_type="gdmlp").cuda()
    blk.eval()
    with torch.no_grad():
        f = timed(lambda: blk(x), a.iters)
    blk.train()
    xg = x.clone().requires_grad_()
    dout = torch.randn_like(x)

    def fb():
        blk.zero_grad(set_to_none=False)
        blk(xg).backward(dout)
    fbm = timed(fb, a.iters)
    # the scan pair alone, on the operands forward_fused hands it
    from bem import ops
    op = blk.op
    wall, dtw, dtb, A, Ds, _ = op._scan_params()
    M = R + 2 * N
    xc = torch.randn(B, C, H, H, device="cuda")
    xd = ops.pw_gemm(xc, wall, 4 * M)
    xd1 = ops.transpose_plane_slice(xd, 2 * M, 2 * M)
    xcT = ops.transpose_planes(xc)
    if N > 1:
        sc = timed(lambda: ops.ss2d_scan_n(xc.view(B, C, L), xcT.view(B, C, L), xd.view(B, 4, M, L)[:, :2], xd1.view(B, 2, M, L), dtw, dtb, A, Ds), a.iters)
    else:
        sc = timed(lambda: ops.ss2d_scan(xc.view(B, C, L), xcT.view(B, C, L), xd.view(B, 4, M, L)[:, :2], xd1.view(B, 2, M, L), dtw, dtb, A, Ds), a.iters)
    nbytes = 4 * B * L * 2 * (2 * C + 2 * M + C)
    print(f"N={N:2d}  VSSBlock fwd {f:8.3f} ms  fwd+bwd {fbm:8.3f} ms  scan pair {sc:7.3f} ms  {nbytes / 1e6:7.1f} MB algorithmic "
          f"-> {nbytes / sc / 1e6:7.1f} GB/s", flush=True)
