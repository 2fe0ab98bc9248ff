"""GPU time of bem.ops.uiqm_uciqe for N candidates at h x w (default: 16 at 400x600, the config-5 geometry), timed with HIP events."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "bayesian-enhancement-model_amd"))
import torch
from bem import ops

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=16)
ap.add_argument("--h", type=int, default=400)
ap.add_argument("--w", type=int, default=600)
ap.add_argument("--iters", type=int, default=50)
a = ap.parse_args()
g = torch.Generator(device="cuda").manual_seed(0)
x = (torch.rand(a.n, 3, a.h, a.w, device="cuda", generator=g) * 0.6 + 0.2).contiguous()
for _ in range(3):
    u1, u2 = ops.uiqm_uciqe(x)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(a.iters):
    u1, u2 = ops.uiqm_uciqe(x)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / a.iters
print(f"uiqm_uciqe: {a.n} candidates at {a.h}x{a.w}: {ms:.3f} ms per call ({ms / a.n * 1e3:.1f} us per candidate), "
      f"uiqm[:3] {u1[:3].tolist()}, uciqe[:3] {u2[:3].tolist()}")
