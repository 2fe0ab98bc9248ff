"""The two-stage N-sample Bayesian enhancement loop of Enhancement/eval.py:146-297, kept on the device.

Differences from the reference driver that do not change results:
  * all (image, sample) pairs of a call go through Stage-I and Stage-II as ONE batch -- every pair has
    its own Bayesian weight sample (per-batch-element weights in the GEMM / depthwise kernels), which is
    what the reference's B=1 loop draws (eval.py:199-211); ``enhance(sample_chunk=K)`` cuts that batch into forwards of K samples per
    image where memory asks for it, with the mean and the spread of the N predictions streamed over the chunks;
  * Stage-I outputs never leave the GPU (the reference copies every sample D2H and back, eval.py:211,219);
  * decomp(image) is evaluated once per image and shared by its N samples (it does not depend on the sample) -- and, depending on nothing
    Stage I produces, on a second HIP stream beside it: Stage I is ~160 kernels on H/16 x W/16 planes that occupy a few CUs each, the
    decomposition's full-resolution kernels fill the rest of the chip meanwhile (BEM_DECOMP_OVERLAP=0: one stream).
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Dict, List, Optional

import torch

from . import ops
from .modules import SampleCtx, sampling
from .scorers import first_index


class BEMPipeline:
    """net1: Stage-I Bayesian ``Network`` (after convert2bnn), net2: Stage-II ``DecompDualBranchDDWavelet``."""

    def __init__(self, net1, net2, scale_down: int = 16, noise_level: float = 0.1):
        self.net1, self.net2 = net1, net2
        self.scale, self.noise_level = scale_down, noise_level
        self._side = None          # second stream for decomp(image), created on first use

    @torch.no_grad()
    def per_image(self, imgs, targets, gt_mean: bool, img_down: Optional[torch.Tensor] = None):
        """What a call computes from the images alone, once however many sample forwards follow: the reflect-padded image, its 1/scale
        resize (Stage I's input), decomp(image) with the image half of Stage II's first convs (on the side stream where there is one;
        the first sample forward joins it) and the targets' channel means."""
        h, w = imgs.shape[-2:]
        f = 4 * self.scale
        Hp = (((h + f) // f) * f) if h % f else h                                # _padimg_np, eval.py:146-153
        Wp = (((w + f) // f) * f) if w % f else w
        pi = SimpleNamespace(hoist=hasattr(self.net2, "forward_decomposed"), d_img=None, p_img=None, side=None)
        pi.pad = pad = ops.pad_reflect(imgs.contiguous(), Hp, Wp)
        pi.img_down = ops.resize_down(pad, self.scale) if img_down is None else img_down
        if pi.hoist and os.environ.get("BEM_DECOMP_OVERLAP", "1") != "0":
            if self._side is None or self._side.device != pad.device:
                self._side = torch.cuda.Stream(device=pad.device)
            pi.side = self._side
            pi.side.wait_stream(torch.cuda.current_stream())                     # pad is ready
            with torch.cuda.stream(pi.side):
                pi.d_img = self.net2.decompose(pad, 0)                           # once per image, beside Stage I
                pi.p_img = self.net2.first_conv_image(pi.d_img)                  # the image half of the two first convs likewise
            pad.record_stream(pi.side)
        elif pi.hoist:
            pi.d_img = self.net2.decompose(pad, 0)                               # once per image
            pi.p_img = self.net2.first_conv_image(pi.d_img)
        pi.tmean = ops.plane_mean(targets.contiguous()) if (gt_mean and targets is not None) else None
        return pi

    @torch.no_grad()
    def candidates(self, imgs, targets, num_samples: int, gt_mean: bool, deterministic: bool = False,
                   eps: Optional[Dict[str, torch.Tensor]] = None, noise: Optional[torch.Tensor] = None,
                   img_down: Optional[torch.Tensor] = None, seed: int = 0, rank: int = 0, sample_offset: int = 0,
                   total_samples: Optional[int] = None, per_image=None):
        """imgs (B,3,h,w) in [0,1] on the GPU, targets (B,3,h,w) or None.
        Returns dict(conds (B*N,3,hd,wd), raw (B*N,3,Hp,Wp), final (B*N,3,h,w), psnr (B*N)); row = image*N + sample.
        ``sample_offset`` / ``total_samples``: this call draws samples [offset, offset + num_samples) of ``total_samples`` per image
        (sample-major multi-GPU sharding, bem.dist; the chunks of ``enhance(sample_chunk=...)``): injected ``eps`` / ``noise`` are given for
        ALL (image, sample) rows and sliced here.  ``per_image``: ``self.per_image(imgs, targets, gt_mean)`` where the caller has it already
        (one call per image batch serves every chunk)."""
        from basicsr.bayesian import set_prediction_type
        B, _, h, w = imgs.shape
        N = 1 if deterministic else num_samples
        NT = total_samples or N
        if not deterministic and (eps is not None or noise is not None) and NT != N:
            rows = (torch.arange(B)[:, None] * NT + sample_offset + torch.arange(N)[None, :]).reshape(-1).to(imgs.device)
            if eps is not None:
                eps = {k_: v.index_select(0, rows) for k_, v in eps.items()}
            if noise is not None:
                noise = noise.index_select(0, rows)
        pi = per_image if per_image is not None else self.per_image(imgs, targets, gt_mean, img_down)
        pad, Hp, Wp = pi.pad, pi.pad.shape[-2], pi.pad.shape[-1]
        hd, wd = pi.img_down.shape[-2:]
        x1 = pi.img_down[:, None].expand(B, N, 3, hd, wd).reshape(B * N, 3, hd, wd)  # (B*N,3,hd,wd): row = image*N + sample
        set_prediction_type(self.net1, deterministic)
        with sampling(None if deterministic else SampleCtx(B * N, eps, seed, rank=rank)) as ctx:
            pred = self.net1(x1)[-1]
        if noise is None and self.noise_level:
            # torch.randn_like of eval.py:209: its own key space (bit 62 of the stream id), per rank and per forward
            noise = ops.randn(tuple(pred.shape), pred.device, seed, (1 << 62) | (rank << 44) | SampleCtx._epoch)
        conds = ops.cond_postproc(pred, pi.tmean, noise if self.noise_level else None, N, self.noise_level)
        if pi.hoist:
            if pi.side is not None:                                              # first sample forward of this image batch
                main = torch.cuda.current_stream()
                main.wait_stream(pi.side)
                for t in [pi.d_img] + pi.p_img:
                    t.record_stream(main)                                        # allocated on the side stream, consumed (and freed) on this one
                pi.side = None
            d_cond = self.net2.decompose_cond(conds, self.scale)                 # decomp of the enlarged condition, which is never formed
            raw = self.net2.forward_decomposed(pi.d_img, d_cond, None if N == 1 else N, p_img=pi.p_img)
        else:
            cond_up = ops.bilinear_up(conds, self.scale)                         # (B*N,3,Hp,Wp)
            # Stage-II archs without a separable decomposition stage (DecompDualBranch, the *2 / *DD / SingleBranch siblings): the
            # reference's own call per candidate, net(cat(img, cond)) (eval.py:211-213), as one batch of B*N rows
            x2 = torch.empty(B * N, 6, Hp, Wp, device=pad.device, dtype=pad.dtype)
            ops.copy_channels(pad[:, None].expand(B, N, 3, Hp, Wp).reshape(B * N, 3, Hp, Wp).contiguous(), x2, 0)
            ops.copy_channels(cond_up, x2, 3)
            raw = self.net2(x2)[-1]
        final, psnr = ops.candidate_finalize(raw, None if targets is None else targets.contiguous(), N, h, w,
                                             bool(gt_mean and targets is not None))
        return dict(conds=conds, raw=raw, final=final, psnr=psnr, N=N)

    @staticmethod
    def select(psnr_rows: List[float]) -> int:
        """eval.py:284-285 with psnr_weight = 1: index of the first maximum of psnr / max(psnr)."""
        return first_index(psnr_rows)

    @torch.no_grad()
    def enhance(self, imgs, targets, num_samples, gt_mean=True, deterministic=False, sync=True, scorer=None, monte_carlo=False, shard=None,
                sample_chunk=None, uncertainty=False, keep="all", **kw):
        """candidates + per-image selection.  Default selection = the full-reference PSNR rule (first maximum of psnr / max(psnr),
        eval.py:284-285) on the device; ``scorer`` (bem.scorers) switches to the PSNR/SSIM-weighted rule or a no-reference
        scorer (eval.py:268-281).  ``monte_carlo``: also returns the Monte-Carlo mean prediction (eval.py:224-225,308-314) with its
        PSNR / SSIM.  With ``sync=False`` nothing is copied to the host.

        ``sample_chunk=K``: the N samples of every image run as ceil(N / K) forwards of at most K samples (the memory knob; None or
        K >= N is the single batch).  The image-only work runs once, ``final`` / ``psnr`` / ``conds`` are assembled in the single batch's row
        order (image*N + sample) and scored once; the raw outputs are never all resident (``raw`` is not returned, the Monte-Carlo mean is
        streamed: ops.mc_accum / mc_finish, the same bits as ops.mc_mean).  Every chunk is a forward of its own with a fresh Philox epoch
        for the weights and the condition noise, as two successive calls have: a chunked run draws a different, equally distributed set
        of N samples than the single batch with the same seed.  Injected ``eps`` / ``noise`` rows are consumed exactly as by the single batch.
        ``uncertainty``: adds ``std`` (B,3,h,w), the unbiased per-pixel standard deviation of the N candidates (zeros for N = 1, so in
        deterministic mode), and ``std_mean`` (B) f64, its mean per image; chunked or not.
        ``keep='best'``: every chunk's candidates are dropped once scored; no ``final`` / ``conds`` / ``raw``, only ``best``, ``best_images``,
        ``best_psnr`` and the score vectors.  The choice is merged chunk by chunk (ops.select_merge), which a single-score rule allows: the
        default PSNR rule, FullReference(1.0) (PSNR >= 0, so dividing by the maximum changes no comparison) and the 'max' / 'min' rules.
        The two-score weighted rules normalise by maxima over all N and raise ValueError; so does UiqmUciqe at weight 1.0 or 0.0, which
        is not a single-score rule here: it divides by max(s1), whose sign (UIQM may be negative) turns the order round, and the other
        score still enters as 0 * s2 / max(s2), NaN where that is -- cases select_scores defines and a running maximum would not follow.
        ``shard`` together with ``sample_chunk`` or ``keep='best'`` raises ValueError: chunking a rank's block is not built."""
        N = 1 if deterministic else num_samples
        if keep not in ("all", "best"):
            raise ValueError(f"enhance: keep must be 'all' or 'best', got {keep!r}")
        if sample_chunk is not None and (sample_chunk != int(sample_chunk) or sample_chunk < 1):
            raise ValueError(f"enhance: sample_chunk must be None or a number of samples >= 1, got {sample_chunk!r}")
        if shard is not None and shard[1] > 1 and (sample_chunk is not None or keep == "best"):
            raise ValueError("enhance: shard together with sample_chunk" + (" / keep='best'" if keep == "best" else "") + " is not supported")
        K = N if sample_chunk is None else min(int(sample_chunk), N)
        streamed = K < N or keep == "best"
        tg = None if targets is None else targets.contiguous()
        r, stats, run = self._collect(imgs, targets, N, K, streamed, gt_mean, deterministic, scorer, monte_carlo, uncertainty, keep, shard, kw)
        best, img, bp = self._choose(r, run, scorer, targets, N)
        r.update(best=best, best_images=img, best_psnr=bp)
        self._statistics(r, stats, streamed, tg, N, imgs.shape[-2:], gt_mean, monte_carlo, uncertainty)
        if sync:
            r["best"], r["best_psnr"] = best.cpu().tolist(), bp.cpu().tolist()
        return r

    def _collect(self, imgs, targets, N, K, streamed, gt_mean, deterministic, scorer, monte_carlo, uncertainty, keep, shard, kw):
        """Step 1 of ``enhance``: the candidates of all N samples, as streamed chunks of K, as this rank's block of a sample-sharded run, or
        as the single batch.  Returns (r, stats, run): the candidates dict with ``N``; the McState that the Monte-Carlo mean (streamed
        only) and the spread accumulate in, or None; the BestState of ``keep='best'`` with every chunk merged, or None."""
        B, _, h, w = imgs.shape
        stats = ops.McState(B, h, w, imgs.device, mean=monte_carlo and streamed, spread=uncertainty) if (uncertainty or (monte_carlo and streamed)) else None
        run = ops.BestState(B, (3, h, w), imgs.device, _online_rule(scorer)) if keep == "best" else None
        if streamed:
            pi = self.per_image(imgs, targets, gt_mean, kw.pop("img_down", None))
            r = {}
            for lo in range(0, N, K):
                n = min(K, N - lo)
                c = self.candidates(imgs, targets, n, gt_mean, deterministic, sample_offset=lo, total_samples=N, per_image=pi, **kw)
                if stats is not None:
                    ops.mc_accum(stats, c["raw"] if monte_carlo else None, c["final"] if uncertainty else None, n)
                if run is not None:
                    s1 = c["psnr"] if scorer is None else scorer.scores(c["final"], targets, n, psnr=c["psnr"])[0].contiguous()
                    ops.select_merge(run, c["final"], s1, n)
                    c = dict(psnr=c["psnr"]) if scorer is None else dict(psnr=c["psnr"], scores=s1)
                else:
                    c = {k_: c[k_] for k_ in ("final", "psnr", "conds")}
                for k_, t in c.items():                                          # into the single batch's row order, chunk by chunk
                    if k_ not in r:
                        r[k_] = t.new_empty((B, N) + tuple(t.shape[1:]))
                    r[k_][:, lo:lo + n] = t.view((B, n) + tuple(t.shape[1:]))
                del c
            r = {k_: t.flatten(0, 1) for k_, t in r.items()}
            r["N"] = N
        elif shard is not None and shard[1] > 1 and not deterministic:
            # sample-major multi-GPU form (bem.dist): this rank draws its block of the N samples of every image, one RCCL all-gather per
            # tensor brings candidates, scores (and raw outputs for the Monte-Carlo mean) back into the unsharded (image, sample) order
            from . import dist as bdist
            rank, world = shard
            kw.pop("rank", None)
            lo, hi = bdist.shard_samples(N, rank, world)
            r = self.candidates(imgs, targets, max(hi - lo, 1), gt_mean, False, rank=rank, sample_offset=lo, total_samples=N, **kw)
            for k_ in ("final", "psnr", "conds") + (("raw",) if monte_carlo else ()):
                t = r[k_] if hi > lo else r[k_][:0]
                r[k_] = bdist.gather_samples(t.contiguous(), B, N, rank, world)
            if not monte_carlo:
                r.pop("raw")
            r["N"] = N
        else:
            r = self.candidates(imgs, targets, N, gt_mean, deterministic, **kw)
        return r, stats, run

    @staticmethod
    def _choose(r, run, scorer, targets, N):
        """Step 2 of ``enhance``: (best (B) int32, best images, best PSNR (B)) by the running merge, the scorer or the default PSNR rule;
        a scorer's score vectors go into ``r`` as ``scores`` / ``scores2``."""
        if run is not None:                            # chosen chunk by chunk already; its one score vector was assembled with the chunks
            best, img = run.best, run.images
            if scorer is None:
                return best, img, run.score            # the default rule's running score is the PSNR
            r["scores2"] = None
        elif scorer is not None:
            sel = scorer.select(r["final"], targets, N, psnr=r["psnr"])
            best, img = sel["best"], sel["best_images"]
            r.update(scores=sel["s1"], scores2=sel["s2"])
        else:
            best, bp, img = ops.select_best(r["final"], r["psnr"], N)
            if targets is None:
                best = torch.zeros_like(best)          # no reference: the reference keeps the first sample (eval.py:291-293)
                img = r["final"][::N].contiguous()
            return best, img, bp
        # a scorer chose: the PSNR of its choice, or without targets (every PSNR is 0) what the 'max' rule makes of them
        bp = ops.select_scores(None, r["psnr"], N, rule="max")[1] if targets is None else _gather(r["psnr"], best, N)
        return best, img, bp

    @staticmethod
    def _statistics(r, stats, streamed, tg, N, hw, gt_mean, monte_carlo, uncertainty):
        """Step 3 of ``enhance``: the Monte-Carlo mean with its PSNR / SSIM and the spread of the candidates, into ``r``.  A streamed run
        has both in ``stats`` already; the single batch takes the mean in one pass (ops.mc_mean) and accumulates the spread here."""
        h, w = hw
        if monte_carlo:
            gm = bool(gt_mean and tg is not None)
            r["mc"] = mc = ops.mc_finish(stats, tg, gm, mean=True)[0] if streamed else ops.mc_mean(r["raw"], tg, N, h, w, gm)
            if tg is not None:
                _, r["mc_psnr"] = ops.candidate_finalize(mc, tg, 1, h, w, False)
                r["mc_ssim"] = ops.ssim(mc, tg, 1) if min(h, w) > 10 else None
        if uncertainty:
            if not streamed:
                ops.mc_accum(stats, None, r["final"], N)
            _, r["std"], r["std_mean"] = ops.mc_finish(stats, mean=False, spread=True)


def _online_rule(scorer):
    """The 'max' / 'min' rule by which ``enhance(keep='best')`` can merge the scorer's choice chunk by chunk, or ValueError."""
    from .scorers import FullReference
    if scorer is None or (type(scorer) is FullReference and scorer.weight == 1.0):
        return "max"                       # PSNR >= 0: psnr / max(psnr) orders the candidates as psnr does
    if scorer.rule in ("max", "min"):
        return scorer.rule
    raise ValueError(f"enhance: keep='best' cannot follow the {scorer.rule!r} rule of {type(scorer).__name__} (weight {scorer.weight}): it "
                     f"normalises by maxima over all N samples; use keep='all'")


def _gather(v, best, N):
    """v (B*N), best (B) -> v[b*N + best[b]] on the device (index arithmetic only)."""
    B = best.numel()
    return v.view(B, N).gather(1, best.long().view(B, 1)).view(B)


# ------------------------------------------------------------------------------------------------
# small shared helpers (bench.py, smoke(), tests)
# ------------------------------------------------------------------------------------------------
def synthetic_pair(shape, seed=287128, device="cpu"):
    """LOL-like dark input and bright target: lq = 0.25 U[0,1), gt = clamp(3.5 lq + 0.05 N)."""
    g = torch.Generator().manual_seed(seed)
    lq = 0.25 * torch.rand(shape, generator=g)
    gt = (3.5 * lq + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)
    return lq.to(device), gt.to(device)


def build_nets(n_feat=40, num_blocks=(2, 2, 2), seed=100, device="cuda", stage2="DecompDualBranchDDWavelet", decomp="model4"):
    """Seeded random-init Stage-I (Bayesian) and Stage-II nets through the registry, like eval.py:84-85."""
    import inspect
    from basicsr.archs import build_network
    from basicsr.bayesian import convert2bnn_selective
    from basicsr.utils.registry import ARCH_REGISTRY
    torch.manual_seed(seed)
    common = dict(n_feat=n_feat, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4, mlp_type="gdmlp", use_pixelshuffle=True,
                  drop_path=0.0, sam=False, stage=1, num_blocks=list(num_blocks))
    net1 = build_network(dict(type="Network", in_channels=3, out_channels=3, **common))
    convert2bnn_selective(net1, {"sigma_init": 0.05, "decay": 0.998, "pretrain": False})
    opt2 = dict(type=stage2, in_channels=6, out_channels=3, **common)
    if "decomp_model" in inspect.signature(ARCH_REGISTRY.get(stage2)).parameters:      # the image-domain archs take no decomposition
        opt2["decomp_model"] = decomp
    net2 = build_network(opt2)
    return net1.to(device).eval(), net2.to(device).eval()
