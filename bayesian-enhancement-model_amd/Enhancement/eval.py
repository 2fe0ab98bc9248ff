#!/usr/bin/env python3
"""Two-stage N-sample Bayesian enhancement of a folder of images -- the driver of Enhancement/eval.py with the reference's command
line (eval.py:30-60) on the device-resident pipeline (bem.pipeline.BEMPipeline):

  python Enhancement/eval.py --opt Options/CG_UNet_LOLv1.yml --cond_opt Options/DecompDualBranch2DDWavelet_4.yml \
      --weights cg.pth --cond_weights stage2.pth --input_dir data/LOLv1/Test/input --target_dir data/LOLv1/Test/target \
      --dataset LOLv1 --GT_mean --num_samples 16 [--no_ref clip | --no_ref niqe --niqe_params niqe_pris_params.npz |
      --no_ref uiqm_uciqe [--uiqm_weight 0.5]] [--psnr_weight 0.5] [--Monte_Carlo] [--deterministic]

What differs from the reference script, none of it in the results: all N samples of an image go through Stage I and Stage II as one
batch (``--parallel_num`` is accepted and ignored), conditions never leave the GPU, selection metrics run on the device, and images
are read / written with PIL (cv2, skimage, natsort, lpips, torchmetrics are not dependencies).  ``--no_ref clip`` uses the scorer
returned by ``make_clip_scorer`` -- the deterministic stand-in of bem.scorers unless a CLIP-IQA module is importable.  ``--no_ref niqe``
scores every candidate with NIQE on the device (bem.ops.niqe) and keeps the first minimum; it needs ``--niqe_params``, the pristine-model
file ``niqe_pris_params.npz`` of a BasicSR install (basicsr/metrics/), which is data and not shipped here.  ``--no_ref uiqm_uciqe``
scores every candidate with UIQM and UCIQE on the device (bem.ops.uiqm_uciqe) and keeps the first maximum of ``w * uiqm / max(uiqm) +
(1 - w) * uciqe / max(uciqe)``, w = ``--uiqm_weight`` (eval.py:277-278); images must resize to at least 10 rows at width 256.  ``--lpips``
(with ``--target_dir``) adds LPIPS v0.1 / AlexNet of the selected image against the target on the device (bem.lpips); its two weight files,
``alexnet-owt-7be5be79.pth`` of torchvision and ``alex.pth`` of the lpips package, are data and not shipped here: ``--lpips_weights DIR``, the
environment variable BEM_LPIPS_WEIGHTS or experiments/pretrained_models/ names the directory holding them.  Scoring happens after the
candidates are gathered, so every mode works on the sample-sharded ``torchrun`` path.
``--weights_key`` / ``--cond_weights_key`` (default ``params``) name the state dict of each checkpoint to load: ``params_ema`` evaluates the
averaged weights of a run trained with ``train.ema_decay``; a key the file lacks stops the driver with the keys it has.
``--sample_chunk K`` runs the samples of an image K at a time (BEMPipeline.enhance(sample_chunk=K): the memory knob for many samples of
large images; every chunk draws under a fresh Philox epoch, so the N samples differ from the single batch's with the same seed);
``--sample_chunk auto`` measures one one-sample forward per image size and picks the largest K whose estimate stays under half the free
memory.  ``--uncertainty`` writes ``<result_dir>/<dataset>/std/<image>.png``, the per-pixel standard deviation of the N candidates as
8-bit grey (``rint(255 min(1, mean_c(std) / --std_white))``; the std of a [0,1] variable is at most 0.5 and a fixed scale keeps images
comparable), and ``Mean_pred_std``.  ``--keep_best`` keeps only the running best candidate of an image (single-score rules: PSNR at
``--psnr_weight 1``, ``--no_ref clip`` / ``niqe``).  ``--sample_chunk`` and ``--keep_best`` do not run on the sample-sharded path.
Output: ``<result_dir>/<dataset>/<image>.png`` (the selected candidate) and ``result.txt`` with the reference's summary lines
(``Best_lpips`` after the PSNR / SSIM lines, then ``Best_NIQE``, then ``Best_UIQM`` and ``Best_UCIQE``, eval.py:339-355; ``Mean_pred_std``
last)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
if PKG not in sys.path:
    sys.path.insert(0, PKG)


def get_parser():
    p = argparse.ArgumentParser(description="Image Enhancement")
    p.add_argument("--result_dir", default="./results/", type=str, help="Directory for results")
    p.add_argument("--input_dir", default="", type=str, help="Directory for inputs")
    p.add_argument("--target_dir", default="", type=str, help="Directory for targets")
    p.add_argument("--opt", type=str, default="youryaml.yaml", help="Path to option YAML file.")
    p.add_argument("--cond_opt", type=str, default="your condition_yaml.yaml", help="Path to option YAML file.")
    p.add_argument("--weights", default="yourweight.pth", type=str, help="Path to weights")
    p.add_argument("--cond_weights", default="yourweight.pth", type=str, help="Path to weights")
    p.add_argument("--weights_key", default="params", type=str, help="state dict of --weights to load: params, or params_ema (averaged weights)")
    p.add_argument("--cond_weights_key", default="params", type=str, help="state dict of --cond_weights to load: params, or params_ema")
    p.add_argument("--dataset", default="yourdataset", type=str, help="Name of dataset")
    p.add_argument("--GT_mean", action="store_true", help="Use the mean of GT to rectify the output of the model")
    p.add_argument("--num_samples", default=200, type=int, help="Number of random samples")
    p.add_argument("--Monte_Carlo", action="store_true", help="also report the average of the random samples")
    p.add_argument("--psnr_weight", default=1.0, type=float, help="Balance between PSNR and SSIM")
    p.add_argument("--no_ref", default="", type=str, choices=["", "clip", "niqe", "uiqm_uciqe"], help="no reference image quality evaluator")
    p.add_argument("--niqe_params", default="", type=str, help="niqe_pris_params.npz of a BasicSR install (basicsr/metrics/), for --no_ref niqe")
    p.add_argument("--uiqm_weight", default=1.0, type=float, help="Balance between UIQM and UICIQE")
    p.add_argument("--lpips", action="store_true", help="True to compute LPIPS")
    p.add_argument("--lpips_weights", default="", type=str, help="directory holding alexnet-owt-7be5be79.pth and alex.pth, for --lpips")
    p.add_argument("--deterministic", action="store_true", help="Use deterministic mode")
    p.add_argument("--parallel_num", default=1, type=int, help="accepted for compatibility and ignored: all samples of an image run as one "
                   "batch unless --sample_chunk says otherwise")
    p.add_argument("--sample_chunk", default="", type=str, metavar="K|auto", help="run the samples of an image K at a time (the memory knob); "
                   "'auto' measures one sample and picks K; default: all samples as one batch")
    p.add_argument("--uncertainty", action="store_true", help="write the per-pixel std of the samples to <result_dir>/<dataset>/std/ and report its mean")
    p.add_argument("--std_white", default=0.25, type=float, help="the std that --uncertainty's grey images show as white")
    p.add_argument("--keep_best", action="store_true", help="keep only the running best candidate of an image (single-score selection rules)")
    p.add_argument("--seed", default=287128, type=int, help="fix random seed to reproduce consistent results")
    p.add_argument("--clip_prompts", nargs="+", default=["brightness", "noisiness", "quality"])
    return p


def make_clip_scorer(prompts):
    from bem.scorers import ClipStandIn
    return ClipStandIn(prompts)


def load_rgb(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.float32) / 255.0          # utils.load_img + /255 (eval.py:166-170)


def save_rgb(path, img01_hw3):
    from PIL import Image
    Image.fromarray(np.rint(np.clip(img01_hw3, 0, 1) * 255.0).astype(np.uint8)).save(path)   # img_as_ubyte


def load_params(net, path, key="params"):
    """``key``: which state dict of the checkpoint to load -- ``params``, or ``params_ema`` for the averaged weights of a run trained with
    ``train.ema_decay``.  A file that is a bare state dict serves as ``params``; any other missing key is an error."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if key in ck:
        sd = ck[key]
    elif key == "params" and not any(isinstance(v, dict) for v in ck.values()):
        sd = ck
    else:
        keys = sorted(map(str, ck))
        raise KeyError(f"{path}: no '{key}' in the checkpoint; keys present: {keys[:8] + (['...'] if len(keys) > 8 else [])}")
    net.load_state_dict({(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()})      # eval.py:98-100 (strict)


def save_std(path, std_3hw, white):
    """--uncertainty's picture of one image: 8-bit grey, rint(255 min(1, mean_c(std) / white))."""
    from PIL import Image
    g = np.minimum(1.0, std_3hw.mean(axis=0) / white)
    Image.fromarray(np.rint(255.0 * g).astype(np.uint8), mode="L").save(path)


def auto_sample_chunk(pipe, img, tgt, num_samples, **kw):
    """--sample_chunk auto: one extra forward of ONE sample of this image (its draws are not used), the peak of allocated memory around it
    and the memory that is free now.  That forward's whole peak is counted once per sample of a chunk -- the per-image part with it, so
    the estimate K x peak is on the high side -- and K is the largest chunk whose estimate stays under HALF the free memory (a safety cap, not
    a tuned number).  A second cap keeps K x peak under 2^34 bytes: no tensor of the one-sample forward is larger than its peak, so no
    tensor of a chunk then holds 2^32 elements or more -- the range tests/test_large_tensors_gpu.py covers: it runs the kernels of the eval
    forward, the selection tail and the no-reference scorers on tensors that cross 2^29, 2^30, 2^31 and 2^32 elements (DESIGN.md section
    4.9).  Units of float4 can still wrap at 2^33 and 2^34 elements, which nothing tests; an explicit ``--sample_chunk K`` is the way past
    the cap.  Returns (K, bytes per sample)."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    pipe.enhance(img, tgt, 1, sync=False, keep="best", **kw)
    torch.cuda.synchronize()
    per = max(torch.cuda.max_memory_allocated() - before, 1)
    free = torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()     # the allocator's cache is free too
    return max(1, min(num_samples, int(free // 2 // per), (2**34 - 1) // per)), per


def main(argv=None):
    args = get_parser().parse_args(argv)
    # --sample_chunk / --keep_best / --uncertainty: checked before any option-file, model or device work
    chunk = None
    if args.sample_chunk not in ("", "auto"):
        try:
            chunk = int(args.sample_chunk)
        except ValueError:
            raise SystemExit(f"--sample_chunk: expected a number of samples or 'auto', got {args.sample_chunk!r}")
        if chunk < 1:
            raise SystemExit(f"--sample_chunk: a chunk holds at least 1 sample, got {chunk}")
    if (args.sample_chunk or args.keep_best) and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(("--sample_chunk" if args.sample_chunk else "--keep_best") + ": not available on the sample-sharded multi-GPU path")
    if args.keep_best and (args.no_ref == "uiqm_uciqe" or (not args.no_ref and args.target_dir and args.psnr_weight != 1.0)):
        raise SystemExit("--keep_best: a two-score weighted rule (" + ("--no_ref uiqm_uciqe" if args.no_ref else f"--psnr_weight {args.psnr_weight}")
                         + ") normalises by the maximum over all samples and cannot be decided chunk by chunk")
    if args.uncertainty and not (np.isfinite(args.std_white) and args.std_white > 0):
        raise SystemExit(f"--std_white: must be a positive std, got {args.std_white}")
    if args.lpips:
        # checked before any option-file, model or device work
        if not args.target_dir:
            raise SystemExit("--lpips is a full-reference metric: it needs --target_dir")
        from bem.lpips import find_weight_files
        try:
            find_weight_files(args.lpips_weights or None)
        except FileNotFoundError as e:
            raise SystemExit(f"--lpips: {e} (--lpips_weights DIR)")
    if args.no_ref == "uiqm_uciqe":
        # checked before any model or device work
        if not os.path.isdir(args.input_dir):
            raise SystemExit(f"--no_ref uiqm_uciqe: --input_dir {args.input_dir!r} is not a directory")
        if not np.isfinite(args.uiqm_weight):
            raise SystemExit(f"--no_ref uiqm_uciqe: --uiqm_weight must be finite, got {args.uiqm_weight}")
    if args.no_ref == "niqe" and not args.niqe_params:
        raise SystemExit("--no_ref niqe needs --niqe_params PATH: the NIQE pristine-model file niqe_pris_params.npz "
                         "(basicsr/metrics/niqe_pris_params.npz in a BasicSR install)")
    from basicsr.bayesian import set_prediction_type
    from basicsr.models import build_model
    from basicsr.utils.options import parse
    from bem.pipeline import BEMPipeline
    from bem.scorers import FullReference, Niqe, NiqeParams, UiqmUciqe
    # one process per GPU under `python -m torch.distributed.run --nproc-per-node N Enhancement/eval.py ...`: the driver feeds ONE image at a
    # time (eval.py:160-222), so the N Bayesian samples of that image are what gets sharded (sample-major, bem.dist); every rank holds the
    # gathered candidates, rank 0 writes the files
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if not dist.is_initialized():
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", torch.cuda.current_device()))
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    opt, cond_opt = parse(args.opt, is_train=False), parse(args.cond_opt, is_train=False)
    net = build_model(opt).net_g
    set_prediction_type(net, deterministic=args.deterministic)
    cond_net = build_model(cond_opt).net_g
    try:
        load_params(net, args.weights, args.weights_key)
        load_params(cond_net, args.cond_weights, args.cond_weights_key)
    except KeyError as e:
        raise SystemExit(f"--weights_key / --cond_weights_key: {e.args[0]}")
    net, cond_net = net.cuda().eval(), cond_net.cuda().eval()
    # scale from the Stage-I option file, noise level from the Stage-II one, default 0 (eval.py:174-176,207)
    pipe = BEMPipeline(net, cond_net, opt.get("condition", {}).get("scale_down", 16), cond_opt.get("condition", {}).get("noise_level", 0))
    result_dir = os.path.join(args.result_dir, args.dataset)
    os.makedirs(os.path.join(result_dir, "std") if args.uncertainty else result_dir, exist_ok=True)
    names = sorted(f for f in os.listdir(args.input_dir) if f.lower().endswith((".png", ".jpg", ".jpeg", ".bmp")))
    if args.no_ref == "clip":
        scorer = make_clip_scorer(args.clip_prompts)
    elif args.no_ref == "niqe":
        scorer = Niqe(NiqeParams.load(args.niqe_params))
    elif args.no_ref == "uiqm_uciqe":
        scorer = UiqmUciqe(args.uiqm_weight)
    else:
        scorer = FullReference(args.psnr_weight) if args.target_dir else None
    psnr, ssim, mc_psnr, mc_ssim, niqe, uiqm, uciqe, lpips_ = [], [], [], [], [], [], [], []
    pred_std, auto_chunks = [], {}          # --uncertainty: mean std per image; --sample_chunk auto: image size -> chunk
    loss_fn = None
    if args.lpips and rank == 0:          # every rank holds the gathered best image: one computes the metric
        from bem.lpips import LPIPS
        loss_fn = LPIPS(net="alex", verbose=False, weights_dir=args.lpips_weights or None).cuda()
    t0 = time.perf_counter()
    with torch.inference_mode():
        for i, name in enumerate(names):
            img = torch.from_numpy(load_rgb(os.path.join(args.input_dir, name))).permute(2, 0, 1)[None].cuda()
            tgt = None
            if args.target_dir:
                tgt = torch.from_numpy(load_rgb(os.path.join(args.target_dir, name))).permute(2, 0, 1)[None].cuda()
            if args.sample_chunk == "auto" and not args.deterministic and tuple(img.shape[2:]) not in auto_chunks:
                K, per = auto_sample_chunk(pipe, img, tgt, args.num_samples, gt_mean=args.GT_mean, seed=args.seed + i)
                auto_chunks[tuple(img.shape[2:])] = K
                print(f"--sample_chunk auto: {img.shape[2]}x{img.shape[3]}: {per / 2**20:.1f} MiB per sample, {K} samples per chunk")
            r = pipe.enhance(img, tgt, args.num_samples, gt_mean=args.GT_mean, deterministic=args.deterministic, scorer=scorer,
                             monte_carlo=args.Monte_Carlo, seed=args.seed + i, shard=(rank, world) if world > 1 else None,
                             sample_chunk=auto_chunks.get(tuple(img.shape[2:]), chunk), uncertainty=args.uncertainty,
                             keep="best" if args.keep_best else "all")
            best = r["best_images"]
            if args.uncertainty:
                pred_std.append(float(r["std_mean"][0]))
                if rank == 0:
                    save_std(os.path.join(result_dir, "std", os.path.splitext(name)[0] + ".png"), r["std"][0].cpu().numpy(), args.std_white)
            if args.no_ref == "niqe":
                niqe.append(float(r["scores"][r["best"][0]]))          # the chosen sample's score (eval.py:273-275)
            elif args.no_ref == "uiqm_uciqe":
                k = int(r["best"][0])                                     # the chosen sample's pair (eval.py:279-280)
                uiqm.append(float(r["scores"][k])); uciqe.append(float(r["scores2"][k]))
            if tgt is not None:
                from bem import ops
                _, p = ops.candidate_finalize(best.contiguous(), tgt.contiguous(), 1, best.shape[2], best.shape[3], False)
                psnr.append(float(p[0]))
                ssim.append(float(ops.ssim(best.contiguous(), tgt.contiguous(), 1)[0]))
                if args.Monte_Carlo:
                    mc_psnr.append(float(r["mc_psnr"][0])); mc_ssim.append(float(r["mc_ssim"][0]))
                if loss_fn is not None:
                    lpips_.append(float(loss_fn.distance01(tgt, best)[0]))      # eval.py:301-306, the quantisation of save_rgb below
            if rank == 0:
                save_rgb(os.path.join(result_dir, os.path.splitext(name)[0] + ".png"), best[0].permute(1, 2, 0).cpu().numpy())
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    if rank != 0:
        return dict(psnr=psnr, ssim=ssim, mc_psnr=mc_psnr, mc_ssim=mc_ssim, niqe=niqe, uiqm=uiqm, uciqe=uciqe, lpips=lpips_, result_dir=result_dir,
                    **(dict(pred_std=pred_std) if args.uncertainty else {}))
    print(f"running time: {time.perf_counter() - t0:.4f} sec")
    with open(os.path.join(result_dir, "result.txt"), "w") as f:
        if args.target_dir:
            for label, vals, unit in (("Best_PSNR", psnr, " dB"), ("Best_SSIM", ssim, "")):
                line = f"{label}: {np.mean(vals):.4f}{unit}"
                print(line); f.write(line + " \n")
            if args.lpips:
                line = f"Best_lpips: {np.mean(lpips_):.4f}"
                print(line); f.write(line + " \n")
            if args.Monte_Carlo:
                for label, vals, unit in (("MC_PSNR", mc_psnr, " dB"), ("MC_SSIM", mc_ssim, "")):
                    line = f"{label}: {np.mean(vals):.4f}{unit}"
                    print(line); f.write(line + " \n")
        if args.no_ref == "niqe":
            line = f"Best_NIQE: {np.mean(niqe):.4f}"
            print(line); f.write(line + " \n")
        if args.no_ref == "uiqm_uciqe":
            for label, vals in (("Best_UIQM", uiqm), ("Best_UCIQE", uciqe)):
                line = f"{label}: {np.mean(vals):.4f}"
                print(line); f.write(line + " \n")
        if args.uncertainty:
            line = f"Mean_pred_std: {np.mean(pred_std):.4f}"
            print(line); f.write(line + " \n")
    return dict(psnr=psnr, ssim=ssim, mc_psnr=mc_psnr, mc_ssim=mc_ssim, niqe=niqe, uiqm=uiqm, uciqe=uciqe, lpips=lpips_, result_dir=result_dir,
                    **(dict(pred_std=pred_std) if args.uncertainty else {}))


if __name__ == "__main__":
    main()
