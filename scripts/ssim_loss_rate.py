#!/usr/bin/env python3
"""Rate of the SSIM loss on the GPU (HIP events, warm-up), against a torch-on-GPU restatement of the same definition:

  1. ms of the forward (with the coefficient maps) and of the backward at (16,3,256,256) and (8,3,128,128): the HIP kernels
     (bem.ops.ssim_loss / ssim_loss_bwd) and the restatement below (grouped conv2d + autograd), the two forms alternating in one
     process, three repeats, the spread between the repeats quoted; the forward's fraction of the HBM roofline from its
     algorithmic traffic (20 bytes per pixel: pred and gt read once, three coefficient maps written);
  2. ms of a DecompDualBranchDDWavelet training step (Options/DecompDualBranch2DDWavelet_4.yml's net, batch 16, 256x256) with and
     without ``train.ssim_opt`` (loss_weight 0.5), the two alternating in one run.

  python scripts/ssim_loss_rate.py [--iters 10] [--hbm_tbs 8.0] [--out profiles/ssim_loss_rate.txt]
"""
import argparse
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bayesian-enhancement-model_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, iters, warmup=2):
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


def torch_ssim_loss(x, y, g, weight):
    """The definition in torch ops: separable grouped conv2d over the valid region, rows then columns."""
    C = x.shape[1]
    gr, gc = g.view(1, 1, 1, 11).expand(C, 1, 1, 11), g.view(1, 1, 11, 1).expand(C, 1, 11, 1)
    f = lambda t: F.conv2d(F.conv2d(t, gr, groups=C), gc, groups=C)
    m1, my, m2, my2, m12 = f(x), f(y), f(x * x), f(y * y), f(x * y)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    s = (2 * m1 * my + c1) * (2 * (m12 - m1 * my) + c2) / ((m1 * m1 + my * my + c1) * ((m2 - m1 * m1) + (my2 - my * my) + c2))
    return weight * (1 - s.mean())


def spread(v):
    return f"{sorted(v)[1]:.3f} ms (repeats {', '.join(f'{x:.3f}' for x in v)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--hbm_tbs", type=float, default=8.0, help="HBM peak in TB/s for the roofline fraction (MI355X: 8.0)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_loss_rate.txt"))
    a = ap.parse_args()
    from bem import ops
    dev = torch.device("cuda", 0)
    lines = [f"ssim_loss_rate: {torch.cuda.get_device_name(0)}, median of {a.iters} after warm-up, HIP events, HIP and torch forms alternating, 3 repeats"]
    i = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-i * i / 4.5)
    g = (g / g.sum()).float().to(dev)

    # ---- 1. forward and backward, HIP against the torch restatement ----
    for shape in ((16, 3, 256, 256), (8, 3, 128, 128)):
        gen = torch.Generator().manual_seed(1)
        gt = torch.rand(shape, generator=gen)
        pred = (gt + 0.1 * torch.randn(shape, generator=gen)).clamp(0, 1).to(dev)
        gt = gt.to(dev)
        one = torch.ones(1, device=dev)
        _, coef = ops.ssim_loss(pred, gt, 0.5, want_grad=True)
        xt = pred.clone().requires_grad_(True)
        state = {}

        def t_fwd():
            state["l"] = torch_ssim_loss(xt, gt, g, 0.5)

        def t_bwd():
            xt.grad = None
            state["l"].backward(retain_graph=True)
        t_fwd()
        hip_l, tor_l = float(ops.ssim_loss(pred, gt, 0.5)), float(state["l"].detach())
        hf, hb, tf, tb = [], [], [], []
        for _ in range(3):
            hf.append(timed(lambda: ops.ssim_loss(pred, gt, 0.5, want_grad=True), a.iters))
            tf.append(timed(t_fwd, a.iters))
            hb.append(timed(lambda: ops.ssim_loss_bwd(pred, gt, coef, 0.5, one), a.iters))
            tb.append(timed(t_bwd, a.iters))
        nb, _ = ops.ssim_loss_cost(pred, want_grad=True)
        nbb, _ = ops.ssim_loss_bwd_cost(pred)
        mhf, mhb, mtf, mtb = (sorted(v)[1] for v in (hf, hb, tf, tb))
        lines += [f"{shape}: loss HIP {hip_l:.6f}, torch {tor_l:.6f}",
                  f"  forward  HIP {spread(hf)}   torch {spread(tf)}   torch / HIP {mtf / mhf:.2f}",
                  f"  backward HIP {spread(hb)}   torch {spread(tb)}   torch / HIP {mtb / mhb:.2f}",
                  f"  forward: {nb / 1e6:.1f} MB algorithmic ({nb / pred.numel():.1f} B per pixel) -> {nb / mhf / 1e9:.3f} TB/s, "
                  f"{100 * nb / mhf / 1e9 / a.hbm_tbs:.1f} % of {a.hbm_tbs} TB/s; backward: {nbb / 1e6:.1f} MB -> {nbb / mhb / 1e9:.3f} TB/s, "
                  f"{100 * nbb / mhb / 1e9 / a.hbm_tbs:.1f} %"]
        del xt, state, coef

    # ---- 2. the training step with and without the term, alternating ----
    import yaml

    from basicsr.models import build_model
    from bem.pipeline import synthetic_pair
    with open(os.path.join(ROOT, "bayesian-enhancement-model_amd", "Options", "DecompDualBranch2DDWavelet_4.yml")) as f:
        opt = yaml.safe_load(f)
    opt.update(is_train=True, dist=False, rank=0, world_size=1)
    opt["path"] = dict(pretrain_network_g=None, strict_load_g=True, resume_state=None)
    opt_s = copy.deepcopy(opt)
    opt_s["train"]["ssim_opt"] = dict(type="SSIMLoss", loss_weight=0.5)
    torch.manual_seed(100)
    m0 = build_model(opt)
    torch.manual_seed(100)
    m1 = build_model(opt_s)
    B, S = 16, 256
    lq, gtt = synthetic_pair((B, 3, S, S), seed=9)
    data = dict(lq=lq.to(dev), gt=gtt.to(dev), gt_down=F.interpolate(gtt, scale_factor=1 / 16, mode="bilinear").to(dev))
    it = [0]

    def step(m):
        def run():
            it[0] += 1
            m.feed_train_data(data)
            m.optimize_parameters(it[0])
        return run
    n = max(3, a.iters // 2)
    t0, t1 = [], []
    for r in range(3):
        t0.append(timed(step(m0), n, warmup=2 if r == 0 else 1))
        t1.append(timed(step(m1), n, warmup=2 if r == 0 else 1))
    a0, a1 = sorted(t0)[1], sorted(t1)[1]
    lines.append(f"training step DecompDualBranchDDWavelet n_feat 40, batch {B}, {S}x{S}: L1 only {a0:.2f} ms, L1 + SSIM {a1:.2f} ms, the term adds "
                 f"{a1 - a0:.2f} ms = {100 * (a1 - a0) / a1:.2f} % of the step   (rounds: {', '.join(f'{x:.2f}/{y:.2f}' for x, y in zip(t0, t1))}; "
                 f"l_ssim {float(m1.log_dict['l_ssim']):.4f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
