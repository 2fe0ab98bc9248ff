#!/usr/bin/env python3
"""Rate and parity of the LPIPS loss term (train.lpips_opt) on the GPU (HIP events, warm-up, seeded weights):

  1. at batch 16 256x256 and batch 8 128x128: ms per layer of the forward (pool, convolution, head) and of the backward (head backward,
     the convolution's input gradient, pool backward), ms of one forward call and of forward + backward through the autograd node;
  2. ms of a DecompDualBranchDDWavelet training step (Options/DecompDualBranch2DDWavelet_4.yml's net, batch 16, 256x256) with and
     without ``train.lpips_opt`` (loss_weight 0.5), the two alternating in one process;
  3. parity on the shapes of tests/test_lpips_loss_gpu.py: loss and gradient of the HIP node and of the f32 torch-CPU evaluation of
     tests/lpips_loss_ref.py, each against float64 -- the asserted cases ``independent`` and ``near`` and the reported case ``close``
     (pred = gt + 0.02 noise), where cancellation in the normalised difference takes the f32 restatement itself past 1e-5.

  python scripts/lpips_loss_rate.py [--iters 10] [--out profiles/lpips_loss_rate.txt]
"""
import argparse
import copy
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bayesian-enhancement-model_amd"), os.path.join(ROOT, "tests")):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_loss_rate.txt"))
    a = ap.parse_args()
    import lpips_loss_ref as L
    import lpips_ref as R
    from basicsr.losses import build_loss
    from bem import ops
    from bem.lpips import WEIGHTS_ENV
    dev = torch.device("cuda", 0)
    sd, lin = R.seeded_state_dicts(0)
    wdir = tempfile.mkdtemp(prefix="lpips_seeded_")
    torch.save(sd, os.path.join(wdir, R.ALEXNET_FILE))
    torch.save(lin, os.path.join(wdir, R.LIN_FILE))
    os.environ[WEIGHTS_ENV] = wdir
    crit = build_loss(dict(type="LPIPSLoss", loss_weight=0.5)).to(dev)
    net = crit.lpips
    cw = net.conv_operands()
    cb = [c[0].input_grad() for c in cw]
    lines = [f"lpips_loss_rate: {torch.cuda.get_device_name(0)}, median of {a.iters} after 2 warm-up runs, HIP events, seeded weights",
             "command: python scripts/lpips_loss_rate.py"]

    # ---- 1. per layer and per call ----
    for B, S in ((16, 256), (8, 128)):
        g = torch.Generator().manual_seed(S)
        gt = torch.rand(B, 3, S, S, generator=g)
        pred = (gt + 0.1 * torch.randn(B, 3, S, S, generator=g)).to(dev)
        gt = gt.to(dev)
        xs = ops.lpips_prep(gt, pred, quantise=False, normalize=True)
        ys = net.features(xs, S, S)
        one = torch.ones(1, device=dev)
        lines.append(f"--- batch {B}, {S}x{S}: features " + ", ".join(f"{y.shape[1]}x{y.shape[2]}x{y.shape[3]}" for y in ys)
                     + f"; saved for the backward {sum(y.numel() for y in ys) * 4 / 1e6:.1f} MB (largest {ys[0].numel() * 4 / 1e6:.1f} MB)")
        fwd = [("prep", lambda: ops.lpips_prep(gt, pred, quantise=False, normalize=True)),
               ("layer 0: conv1 (block form)", lambda: ops.conv2d(xs, cw[0][0], cw[0][1], pad=1, relu=True)),
               ("layer 1: pool + conv2 5x5", lambda: ops.conv2d(ops.maxpool3s2(ys[0]), cw[1][0], cw[1][1], pad=2, relu=True)),
               ("layer 2: pool + conv3", lambda: ops.conv2d(ops.maxpool3s2(ys[1]), cw[2][0], cw[2][1], pad=1, relu=True)),
               ("layer 3: conv4", lambda: ops.conv2d(ys[2], cw[3][0], cw[3][1], pad=1, relu=True)),
               ("layer 4: conv5", lambda: ops.conv2d(ys[3], cw[4][0], cw[4][1], pad=1, relu=True))]
        for name, fn in fwd:
            lines.append(f"forward  {name:<34} {timed(fn, a.iters):7.3f} ms")

        def heads():
            out = ws = None
            for i, y in enumerate(ys):
                out, ws = ops.lpips_layer(y, getattr(net, f"lin{i}"), ws=ws, out=out, first=i == 0)
            return ops.lpips_mean(ws, B, 0.5)
        lines.append(f"forward  {'five heads + mean':<34} {timed(heads, a.iters):7.3f} ms")
        # the backward, layer by layer, on gradients of the right shapes (values from one real pass)
        scale, gins, ds = 0.5 / B, {}, {}
        gin = None
        for i in (4, 3, 2, 1):
            ds[i] = ops.lpips_layer_bwd(ys[i], getattr(net, f"lin{i}"), gin, one, scale)
            gins[i] = gin
            gin = ops.conv2d(ds[i], cb[i], None, pad=cw[i][2])
            if i <= 2:
                ds[("pool", i)] = gin
                gin = ops.relu_pool3s2_bwd(ys[i - 1][B:], gin)
        gins[0] = gin
        Ho, Wo = ops.lpips_conv1_hw(S, S)
        d0 = torch.empty(B, 64, Ho + 2, (Wo + 3) // 2 * 2, device=dev)
        ops.lpips_layer_bwd(ys[0], net.lin0, gin, one, scale, out=d0, origin=(1, 1))
        gxs = ops.conv2d(d0, cb[0], None, pad=1)
        for i in (4, 3, 2, 1):
            t_h = timed(lambda: ops.lpips_layer_bwd(ys[i], getattr(net, f"lin{i}"), gins[i], one, scale), a.iters)
            t_c = timed(lambda: ops.conv2d(ds[i], cb[i], None, pad=cw[i][2]), a.iters)
            t_p = timed(lambda: ops.relu_pool3s2_bwd(ys[i - 1][B:], ds[("pool", i)]), a.iters) if i <= 2 else 0.0
            lines.append(f"backward layer {i}: head {t_h:7.3f} ms, conv{i + 1} input gradient {t_c:7.3f} ms"
                         + (f", pool backward {t_p:7.3f} ms" if i <= 2 else ""))
        t_h = timed(lambda: ops.lpips_layer_bwd(ys[0], net.lin0, gins[0], one, scale, out=d0, origin=(1, 1)), a.iters)
        t_c = timed(lambda: ops.conv2d(d0, cb[0], None, pad=1), a.iters)
        t_p = timed(lambda: ops.lpips_prep_bwd(gxs, S, S, normalize=True), a.iters)
        lines.append(f"backward layer 0: head {t_h:7.3f} ms, conv1 input gradient {t_c:7.3f} ms, prep backward {t_p:7.3f} ms")
        del ds, gins, d0, gxs, gin

        def call_fwd():
            with torch.no_grad():
                crit(pred, gt)

        def call_both():
            p = pred.detach().requires_grad_(True)
            crit(p, gt).backward()
        tf, tb = [], []
        for r in range(3):
            tf.append(timed(call_fwd, a.iters, warmup=2 if r == 0 else 1))
            tb.append(timed(call_both, a.iters, warmup=2 if r == 0 else 1))
        lines.append(f"one call: forward {sorted(tf)[1]:.3f} ms, forward + backward {sorted(tb)[1]:.3f} ms   "
                     f"(rounds: {', '.join(f'{x:.3f}/{y:.3f}' for x, y in zip(tf, tb))})")
        del xs, ys

    # ---- 2. the training step with and without the term, alternating ----
    import yaml

    from basicsr.models import build_model
    from bem.pipeline import synthetic_pair
    with open(os.path.join(ROOT, "bayesian-enhancement-model_amd", "Options", "DecompDualBranch2DDWavelet_4.yml")) as f:
        opt = yaml.safe_load(f)
    opt.update(is_train=True, dist=False, rank=0, world_size=1)
    opt["path"] = dict(pretrain_network_g=None, strict_load_g=True, resume_state=None)
    opt_l = copy.deepcopy(opt)
    opt_l["train"]["lpips_opt"] = dict(type="LPIPSLoss", loss_weight=0.5)
    torch.manual_seed(100)
    m0 = build_model(opt)
    torch.manual_seed(100)
    m1 = build_model(opt_l)
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
    lines.append(f"training step DecompDualBranchDDWavelet n_feat 40, batch {B}, {S}x{S}: L1 only {a0:.2f} ms, L1 + LPIPS {a1:.2f} ms, the term adds "
                 f"{a1 - a0:.2f} ms = {100 * (a1 - a0) / a1:.2f} % of the step   (rounds: {', '.join(f'{x:.2f}/{y:.2f}' for x, y in zip(t0, t1))}; "
                 f"l_lpips {float(m1.log_dict['l_lpips']):.4f})")
    del m0, m1, data

    # ---- 3. parity ----
    lines.append("parity against float64 (seeded weights, B = 2, loss_weight 0.5): relative error of the loss, and the worst gradient error as a "
                 "fraction of the float64 gradient's maximum, over the whole tensor")
    lines.append("  case                      float64 loss    loss HIP  loss CPU f32   grad HIP  grad CPU f32")
    for H, W in ((31, 31), (37, 53), (64, 64), (100, 152)):
        g = torch.Generator().manual_seed(H * 1000 + W)
        gt = torch.rand(2, 3, H, W, generator=g)
        ind = torch.rand(2, 3, H, W, generator=g)
        noise = torch.randn(2, 3, H, W, generator=g)
        for kind, pred in (("independent", ind), ("near", gt + 0.1 * noise), ("close", gt + 0.02 * noise)):
            l64, g64 = L.loss_and_grad(sd, lin, pred, gt, 0.5, torch.float64)
            l32, g32 = L.loss_and_grad(sd, lin, pred, gt, 0.5, torch.float32)
            p = pred.to(dev).requires_grad_(True)
            lh = crit(p, gt.to(dev))
            lh.backward()
            top = float(g64.abs().max())
            lines.append(f"  {H:>3}x{W:<3} {kind:<12}  {float(l64):.6e}   {abs(float(lh.detach()) - float(l64)) / float(l64):.2e}    "
                         f"{abs(float(l32) - float(l64)) / float(l64):.2e}     {float((p.grad.cpu().double() - g64).abs().max()) / top:.2e}    "
                         f"{float((g32.double() - g64).abs().max()) / top:.2e}" + ("   (reported, not asserted)" if kind == "close" else ""))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
