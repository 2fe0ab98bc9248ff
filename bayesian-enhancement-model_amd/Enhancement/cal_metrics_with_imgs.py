#!/usr/bin/env python3
"""Metrics of a folder of finished images against a folder of targets -- Enhancement/cal_metrics_with_imgs.py with the reference's command
line on the device metrics of bem.ops:

  python Enhancement/cal_metrics_with_imgs.py --pred_dir results/LOLv1 --target_dir data/LOLv1/Test/target --psnr --ssim --lpips \
      [--lpips_weights DIR] [--niqe --niqe_params niqe_pris_params.npz]

Files (.png, .jpg, .bmp) are sorted by name and paired by position, one pair at a time, so sizes may differ between pairs.  PSNR is
bem.ops.candidate_finalize, SSIM bem.ops.ssim, LPIPS bem.lpips (its two weight files as for eval.py --lpips), NIQE bem.ops.niqe with the
pristine-model file of a BasicSR install.  Prints the reference's ``Best_*`` lines (:58-69) and returns the per-image values."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
if PKG not in sys.path:
    sys.path.insert(0, PKG)

EXTS = (".png", ".jpg", ".bmp")


def get_parser():
    p = argparse.ArgumentParser(description="Image Enhancement")
    p.add_argument("--pred_dir", type=str, help="Dir of predited images")
    p.add_argument("--target_dir", type=str, default="", help="Dir of targets")
    p.add_argument("--psnr", action="store_true", help="True to compute PSNR")
    p.add_argument("--ssim", action="store_true", help="True to compute SSIM")
    p.add_argument("--lpips", action="store_true", help="True to compute LPIPS")
    p.add_argument("--niqe", action="store_true", help="True to compute NIQE")
    p.add_argument("--lpips_weights", default="", type=str, help="directory holding alexnet-owt-7be5be79.pth and alex.pth, for --lpips")
    p.add_argument("--niqe_params", default="", type=str, help="niqe_pris_params.npz of a BasicSR install (basicsr/metrics/), for --niqe")
    return p


def load_rgb(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.float32) / 255.0          # utils.load_img + /255 (:44)


def _images(d):
    return sorted(os.path.join(d, f) for f in os.listdir(d) if f.lower().endswith(EXTS))


def main(argv=None):
    args = get_parser().parse_args(argv)
    # every argument is checked before any device work
    if not args.pred_dir or not os.path.isdir(args.pred_dir):
        raise SystemExit(f"--pred_dir {args.pred_dir!r} is not a directory")
    for flag in ("psnr", "ssim", "lpips"):
        if getattr(args, flag) and not args.target_dir:
            raise SystemExit(f"--{flag} is a full-reference metric: it needs --target_dir")
    if args.target_dir and not os.path.isdir(args.target_dir):
        raise SystemExit(f"--target_dir {args.target_dir!r} is not a directory")
    if args.niqe and not args.niqe_params:
        raise SystemExit("--niqe needs --niqe_params PATH: the NIQE pristine-model file niqe_pris_params.npz "
                         "(basicsr/metrics/niqe_pris_params.npz in a BasicSR install)")
    if args.lpips:
        from bem.lpips import find_weight_files
        try:
            find_weight_files(args.lpips_weights or None)
        except FileNotFoundError as e:
            raise SystemExit(f"--lpips: {e} (--lpips_weights DIR)")
    preds = _images(args.pred_dir)
    targets = _images(args.target_dir) if args.target_dir else []
    if args.target_dir and len(targets) < len(preds):
        raise SystemExit(f"--target_dir holds {len(targets)} images, --pred_dir {len(preds)}: they are paired by position")
    from bem import ops
    loss_fn = params = None
    if args.lpips:
        from bem.lpips import LPIPS
        loss_fn = LPIPS(net="alex", verbose=False, weights_dir=args.lpips_weights or None).cuda()
    if args.niqe:
        from bem.scorers import NiqeParams
        params = NiqeParams.load(args.niqe_params)
    psnr, ssim, lpips_, niqe = [], [], [], []
    dev = lambda path: torch.from_numpy(load_rgb(path)).permute(2, 0, 1)[None].contiguous().cuda()
    with torch.inference_mode():
        for i, path in enumerate(preds):
            pred = dev(path)
            target = dev(targets[i]) if args.target_dir else None
            if target is not None and target.shape != pred.shape:
                raise SystemExit(f"{path} is {tuple(pred.shape[2:])}, its target {targets[i]} {tuple(target.shape[2:])}")
            if args.psnr:
                psnr.append(float(ops.candidate_finalize(pred, target, 1, pred.shape[2], pred.shape[3], False)[1][0]))
            if args.ssim:
                ssim.append(float(ops.ssim(pred, target, 1)[0]))
            if args.lpips:
                lpips_.append(float(loss_fn.distance01(target, pred)[0]))
            if args.niqe:
                niqe.append(float(ops.niqe(pred, params)[0]))
    if args.psnr:
        print("Best_PSNR: {:.4f} dB".format(np.mean(psnr)))
    if args.ssim:
        print("Best_SSIM: {:.4f}".format(np.mean(ssim)))
    if args.lpips:
        print("Best_lpips: {:.4f}".format(np.mean(lpips_)))
    if args.niqe:
        print("Best_NIQE: {:.4f}".format(np.mean(niqe)))
    return dict(psnr=psnr, ssim=ssim, lpips=lpips_, niqe=niqe)


if __name__ == "__main__":
    main()
