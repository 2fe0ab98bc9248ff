#!/usr/bin/env python3
"""Rate of the two kernels of the train block beside their siblings (HIP events, warm-up, the two forms alternating in one process):

  1. bem_adam_step_f32 beside bem_adamw_step_f32 on a 2.8 M-parameter flat buffer with the clip folded in (seven words per parameter:
     p, g, m, v read, p, m, v written -- g is written back too when clipping, which both do alike);
  2. bem_charbonnier_loss_f32 beside bem_l1_loss_f32 at (16,3,256,256): the forward (two reads per element) and the backward (two reads,
     one write).

Each figure is the median of 5 timings; the pair is repeated three times and the spread of the sibling's three medians is printed beside
the difference, which is what "parity" is judged against.

  python scripts/train_block_rate.py [--iters 5] [--out profiles/train_block_rate.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bayesian-enhancement-model_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def timed(fn, iters, warmup=3):
    """Median ms of fn() over ``iters`` runs, each between its own pair of events."""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return sorted(ms)[len(ms) // 2]


def pair(name_new, new, name_old, old, iters, nbytes):
    """Three alternating repeats -> one report line."""
    a, b = [], []
    for _ in range(3):
        b.append(timed(old, iters))
        a.append(timed(new, iters))
    ma, mb = sorted(a)[1], sorted(b)[1]
    fmt = lambda v: ", ".join(f"{1e3 * x:.1f}" for x in v)
    return (f"  {name_new:24s} {1e3 * ma:7.1f} us ({fmt(a)})   {name_old:20s} {1e3 * mb:7.1f} us ({fmt(b)})   new - old {1e3 * (ma - mb):+.1f} us, "
            f"spread of old {1e3 * (max(b) - min(b)):.1f} us;  {nbytes / 1e6:.1f} MB -> {nbytes / ma / 1e9:.2f} vs {nbytes / mb / 1e9:.2f} TB/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_block_rate.txt"))
    a = ap.parse_args()
    from bem import ops
    dev = torch.device("cuda", 0)
    lines = [f"train_block_rate: {torch.cuda.get_device_name(0)}, median of {a.iters} HIP-event timings after warm-up, new and old forms "
             f"alternating in one process, 3 repeats (the three medians in brackets)"]

    n = 2_800_000
    g = torch.Generator().manual_seed(1)
    p, gr, m, v = (torch.randn(n, generator=g).to(dev) for _ in range(4))
    v.abs_()
    ss = torch.zeros(1, device=dev, dtype=torch.float64)
    ops.grad_sumsq(gr, ss)
    norm = torch.zeros(1, device=dev)
    args = (p, gr, m, v, 2e-4, (0.9, 0.999), 1e-8, 1e-4, 10)
    kw = dict(max_norm=1.0, sumsq=ss, norm_out=norm)
    lines.append(f"optimizer step, flat buffer of {n} parameters, clip at max_norm 1 folded in (8 words per parameter with g written back):")
    lines.append(pair("bem_adam_step_f32", lambda: ops.adam_step_(*args, **kw), "bem_adamw_step_f32", lambda: ops.adamw_step_(*args, **kw), a.iters, 32 * n))

    shape = (16, 3, 256, 256)
    gt = torch.rand(shape, generator=g)
    pred = (gt + 0.1 * torch.randn(shape, generator=g)).to(dev)
    gt = gt.to(dev)
    one = torch.ones(1, device=dev)
    ne = pred.numel()
    lines.append(f"pixel loss at {shape} ({ne} elements); each call also allocates its outputs and scratch through torch, as the training step does:")
    lines.append(pair("charbonnier_loss", lambda: ops.charbonnier_loss(pred, gt), "l1_loss", lambda: ops.l1_loss(pred, gt), a.iters, 8 * ne))
    lines.append(pair("charbonnier_loss_bwd", lambda: ops.charbonnier_loss_bwd(pred, gt, 1.0, 1e-12, one), "l1_loss_bwd",
                      lambda: ops.l1_loss_bwd(pred, gt, 1.0, one), a.iters, 12 * ne))
    lines.append(pair("mse_loss", lambda: ops.mse_loss(pred, gt), "l1_loss", lambda: ops.l1_loss(pred, gt), a.iters, 8 * ne))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
