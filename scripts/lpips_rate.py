#!/usr/bin/env python3
"""Rate and parity of LPIPS (v0.1, AlexNet) on the GPU (HIP events, warm-up, seeded weights, B = 1), at 400x600 and 384x384:

  1. ms per layer (its pool and convolution), ms of the five distance heads, ms of one ``distance01``;
  2. conv2 (5x5, 64 -> 192) as 25 shifted x6 taps beside the direct kernel on the same tensor, the two alternating in one process
     (conv1 has the block form only: the direct kernel's LDS patch for an 11x11 stride-4 window does not fit a workgroup);
  3. one ``BEMPipeline.enhance`` at 16 samples on a 400x600 image beside one ``distance01``, and their ratio;
  4. parity on the cases of tests/test_lpips_gpu.py: HIP and the f32 torch-CPU evaluation of tests/lpips_ref.py, each against float64.

  python scripts/lpips_rate.py [--iters 5] [--out profiles/lpips_rate.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "bayesian-enhancement-model_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_rate.txt"))
    a = ap.parse_args()
    import lpips_ref as R
    from bem import ops
    from bem.lpips import ALEX_CONVS, LPIPS
    dev = torch.device("cuda", 0)
    sd, lin = R.seeded_state_dicts(0)
    m = LPIPS(state_dict=sd, lin_state_dict=lin).to(dev)
    cw = m.conv_operands()
    lines = [f"lpips_rate: {torch.cuda.get_device_name(0)}, B = 1, median of {a.iters} after 2 warm-up runs, HIP events"]
    t_dist = {}
    for H, W in ((400, 600), (384, 384)):
        g = torch.Generator().manual_seed(H)
        ref, pred = torch.rand(1, 3, H, W, generator=g).to(dev), torch.rand(1, 3, H, W, generator=g).to(dev)
        xs = ops.lpips_prep(ref, pred)
        ys = m.features(xs, H, W)
        Ho, Wo = ops.lpips_conv1_hw(H, W)
        lines.append(f"--- {H}x{W}: features " + ", ".join(f"{y.shape[1]}x{y.shape[2]}x{y.shape[3]}" for y in ys))
        lines.append(f"prep (quantise, scale, block layout)          {timed(lambda: ops.lpips_prep(ref, pred), a.iters):7.3f} ms")
        steps = [("conv1 11x11 s4 as 3x3 over 48 block channels", lambda: ops.conv2d(xs, cw[0][0], cw[0][1], pad=1, relu=True)),
                 ("pool + conv2 5x5", lambda: ops.conv2d(ops.maxpool3s2(ys[0]), cw[1][0], cw[1][1], pad=2, relu=True)),
                 ("pool + conv3 3x3", lambda: ops.conv2d(ops.maxpool3s2(ys[1]), cw[2][0], cw[2][1], pad=1, relu=True)),
                 ("conv4 3x3", lambda: ops.conv2d(ys[2], cw[3][0], cw[3][1], pad=1, relu=True)),
                 ("conv5 3x3", lambda: ops.conv2d(ys[3], cw[4][0], cw[4][1], pad=1, relu=True))]
        for i, (name, fn) in enumerate(steps):
            co, ci, k = ALEX_CONVS[i][2], ALEX_CONVS[i][1], ALEX_CONVS[i][3]
            t = timed(fn, a.iters)
            fl = 2.0 * 2 * co * ci * k * k * ys[i].shape[2] * ys[i].shape[3]
            lines.append(f"layer {i}: {name:<44} {t:7.3f} ms  ({fl / 1e9:5.2f} GFLOP, {fl / t / 1e9:6.1f} TF/s f32-equivalent; "
                         f"width {ys[i].shape[3]}: {'block grid, x6' if i == 0 else 'even, x6' if ys[i].shape[3] % 2 == 0 else 'odd, direct kernel'})")

        def heads():
            out = ws = None
            for i, y in enumerate(ys):
                out, ws = ops.lpips_layer(y, getattr(m, f"lin{i}"), ws=ws, out=out, first=i == 0)
        lines.append(f"five distance heads                            {timed(heads, a.iters):7.3f} ms")
        t_dist[(H, W)] = timed(lambda: m.distance01(ref, pred), a.iters)
        lines.append(f"distance01 (everything above)                  {t_dist[(H, W)]:7.3f} ms")
        # conv2: the tap form and the direct kernel on the same tensor, alternating.  At an odd width the tap form does not apply: the
        # plane is then timed with one column dropped for the taps and as it is for the direct kernel.
        x2 = ops.maxpool3s2(ys[0])
        x2e = x2 if x2.shape[3] % 2 == 0 else x2[:, :, :, :-1].contiguous()
        tt, td = [], []
        for r in range(3):
            ops.USE_CONV_X6 = True
            tt.append(timed(lambda: ops.conv2d(x2e, cw[1][0], cw[1][1], pad=2, relu=True), a.iters, warmup=2 if r == 0 else 1))
            ops.USE_CONV_X6 = False
            td.append(timed(lambda: ops.conv2d(x2e, cw[1][0].w, cw[1][1], pad=2, relu=True), a.iters, warmup=2 if r == 0 else 1))
        ops.USE_CONV_X6 = True
        lines.append(f"conv2 on {x2e.shape[2]}x{x2e.shape[3]}: 25 x6 taps {sorted(tt)[1]:.3f} ms, direct kernel {sorted(td)[1]:.3f} ms "
                     f"(rounds: {', '.join(f'{x:.3f}/{y:.3f}' for x, y in zip(tt, td))})")

    # ---- 3. beside the enhancement it scores ----
    from bem.pipeline import BEMPipeline, build_nets, synthetic_pair
    net1, net2 = build_nets(device="cuda")
    lq, gt = synthetic_pair((1, 3, 400, 600))
    lq, gt = lq.to(dev), gt.to(dev)
    pipe = BEMPipeline(net1, net2)
    with torch.inference_mode():
        t_enh = timed(lambda: pipe.enhance(lq, gt, 16, gt_mean=True), a.iters)
    lines.append(f"enhance (16 samples, 400x600, shipped widths) {t_enh:.2f} ms; distance01 at 400x600 {t_dist[(400, 600)]:.3f} ms = "
                 f"{t_dist[(400, 600)] / t_enh:.4f} of it")

    # ---- 4. parity ----
    lines.append("parity, max relative error against float64 over the two pairs of a case (seeded weights, B = 2):")
    lines.append("  case                      float64 value      HIP       torch CPU f32")
    for H, W in ((31, 31), (37, 53), (64, 64), (100, 152)):
        g = torch.Generator().manual_seed(H * 1000 + W)
        x = torch.rand(2, 3, H, W, generator=g)
        for kind, y in (("independent", torch.rand(2, 3, H, W, generator=g)), ("close", x + 0.02 * torch.randn(2, 3, H, W, generator=g))):
            want = R.lpips01(sd, lin, x, y)
            hip = m.distance01(x.to(dev), y.to(dev)).cpu().double()
            f32 = R.lpips01(sd, lin, x, y, torch.float32).double()
            lines.append(f"  {H:>3}x{W:<3} {kind:<12}  {float(want[0]):.6e}  {float(((hip - want).abs() / want).max()):.2e}  "
                         f"{float(((f32 - want).abs() / want).max()):.2e}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
