"""Candidate scoring and selection of Enhancement/eval.py:229-297 as a pluggable interface.

A scorer maps the finished candidates of a batch -- ``final`` (B*N,3,h,w) in [0,1], row = image*N + sample, and the targets
(B,3,h,w) or None -- to one or two score vectors plus the selection rule the reference applies to them:

  FullReference(psnr_weight)   PSNR (Enhancement/utils.py:5-9) and, for psnr_weight < 1, SSIM (utils.py:12-57), rule
                               ``index(max(w * psnr / max(psnr) + (1 - w) * ssim / max(ssim)))``            (eval.py:284-285)
  NoReference(fn, 'max'|'min') any image-quality function returning one score per candidate; ``index(max)`` for CLIP-IQA
                               (eval.py:271), ``index(min)`` for NIQE (eval.py:273-274)
  ClipStandIn()                a deterministic stand-in for torchmetrics' CLIPImageQualityAssessment, whose weights cannot be
                               fetched here.  It follows eval.py:229-243's post-processing (prompt scores
                               'brightness' x 0.7, 'noisiness' x 1, 'quality', averaged) on closed-form per-image statistics;
                               its VALUES are parity-unpinned, the ordering logic applied to them is the reference's.
  Niqe(params)                 NIQE (basicsr/metrics/niqe.py, eval.py:253), rule ``index(min)``; ops.niqe on the device with the
                               pristine-model statistics of a NiqeParams (niqe_pris_params.npz from a BasicSR install).
  UiqmUciqe(uiqm_weight)       UIQM and UCIQE (basicsr/metrics/uciqe_uiqm.py, eval.py:255-260), rule ``index(max(w * uiqm / max(uiqm)
                               + (1 - w) * uciqe / max(uciqe)))`` (eval.py:277-278); ops.uiqm_uciqe on the device.
All scores stay on the device; ``select`` runs bem_select_scores_f32 (first index on ties, float64 comparisons).  The selection rules
are stated twice, once per side: ``first_index`` below for the host and the comment above ``first_better`` in csrc/selection.hip."""
from __future__ import annotations

from typing import Callable, Optional

import torch

from . import ops


def first_index(s1_row, s2_row=None, weight=1.0, rule="relative"):
    """The reference's choice among one image's samples with its Python list semantics (eval.py:268-285): the FIRST index of the best
    score.  'max' / 'min': of s1.  'relative' / 'weighted': of s1 / max(s1), or weight * s1 / max(s1) + (1 - weight) * s2 / max(s2) with
    s2.  max() keeps a leading NaN and passes any other over, so a leading NaN wins; the device's 'weighted' rule alone passes that one
    over too.  A zero maximum (no usable score: PSNR without targets) gives the first sample, where the division would give NaN or -inf
    for every one."""
    rel = [float(v) for v in s1_row]
    if rule not in ("max", "min"):
        s2 = None if s2_row is None else [float(v) for v in s2_row]
        m1, m2 = max(rel), (1.0 if s2 is None else max(s2))
        if m1 == 0 or m2 == 0:
            return 0
        rel = [p / m1 for p in rel] if s2 is None else [weight * p / m1 + (1 - weight) * q / m2 for p, q in zip(rel, s2)]
    return rel.index(min(rel)) if rule == "min" else rel.index(max(rel))


class Scorer:
    rule = "weighted"      # 'weighted' | 'max' | 'min'
    weight = 1.0

    def scores(self, final, targets, samples_per_image, psnr=None):
        """-> (s1 (Bn), s2 (Bn) | None)"""
        raise NotImplementedError

    def select(self, final, targets, samples_per_image, psnr=None):
        """-> dict(best (B) int32, best_images (B,3,h,w), s1, s2, best_s1, best_s2)"""
        s1, s2 = self.scores(final, targets, samples_per_image, psnr)
        best, b1, b2, img = ops.select_scores(final, s1.contiguous(), samples_per_image, None if s2 is None else s2.contiguous(), self.weight, self.rule)
        return dict(best=best, best_images=img, s1=s1, s2=s2, best_s1=b1, best_s2=b2)


class FullReference(Scorer):
    def __init__(self, psnr_weight: float = 1.0):
        self.weight = float(psnr_weight)

    def scores(self, final, targets, samples_per_image, psnr=None):
        if targets is None:
            raise ValueError("FullReference scorer needs targets")
        if psnr is None:
            raise ValueError("FullReference scorer: pass the PSNR vector computed by candidate_finalize")
        # the reference always evaluates both metrics (eval.py:263-264); SSIM is skipped here only when it cannot change the choice
        s2 = ops.ssim(final, targets.contiguous(), samples_per_image) if self.weight != 1.0 else None
        return psnr, s2


class NoReference(Scorer):
    def __init__(self, fn: Callable[[torch.Tensor], torch.Tensor], rule: str = "max"):
        if rule not in ("max", "min"):
            raise ValueError("NoReference: rule must be 'max' or 'min'")
        self.fn, self.rule = fn, rule

    def scores(self, final, targets, samples_per_image, psnr=None):
        s = self.fn(final)
        if s.shape != (final.shape[0],):
            raise ValueError("NoReference scorer function must return one score per candidate")
        return s.float().contiguous(), None


class ClipStandIn(NoReference):
    """eval.py:229-243 with closed-form 'prompt' scores in [0,1] instead of CLIP similarities (deterministic, weights-free)."""

    def __init__(self, prompts=("brightness", "noisiness", "quality")):
        self.prompts = tuple(prompts)
        super().__init__(self._score, "max")

    def _score(self, final):
        Bn = final.shape[0]
        m = ops.plane_mean(final.contiguous())                              # (Bn,3) channel means, HIP reduction
        lum = 0.299 * m[:, 0] + 0.587 * m[:, 1] + 0.114 * m[:, 2]
        sq = ops.plane_mean((final * final).contiguous())
        var = (sq - m * m).clamp_min(0).mean(dim=1)
        vals = {"brightness": lum.clamp(0, 1) * 0.7,                         # eval.py:236-238: brightness scaled down by 0.7
                "noisiness": (1.0 - 4.0 * var).clamp(0, 1) * 1.0,
                "quality": (1.0 - (lum - 0.45).abs() * 2.0).clamp(0, 1)}
        unknown = [p for p in self.prompts if p not in vals]
        if unknown:
            raise ValueError(f"ClipStandIn: unknown prompts {unknown}")
        return torch.stack([vals[p] for p in self.prompts]).mean(dim=0).reshape(Bn)


class NiqeParams:
    """NIQE's pristine multivariate-Gaussian model and smoothing window (basicsr/metrics/niqe_pris_params.npz), f64 on the device."""

    def __init__(self, mu, cov, window, device="cuda"):
        t = lambda a: torch.as_tensor(a, dtype=torch.float64).to(device).contiguous()
        self.mu, self.cov, self.window = t(mu).reshape(-1), t(cov), t(window)
        if self.mu.numel() != 36 or tuple(self.cov.shape) != (36, 36) or tuple(self.window.shape) != (7, 7):
            raise ValueError("NiqeParams: expected mu_pris_param (36), cov_pris_param (36,36), gaussian_window (7,7)")

    @classmethod
    def load(cls, path, device="cuda"):
        import numpy as np
        with np.load(path) as z:
            missing = [k for k in ("mu_pris_param", "cov_pris_param", "gaussian_window") if k not in z]
            if missing:
                raise ValueError(f"{path}: missing {missing} (expected BasicSR's niqe_pris_params.npz)")
            return cls(z["mu_pris_param"], z["cov_pris_param"], z["gaussian_window"], device)


class Niqe(NoReference):
    """eval.py:253,272-274: NIQE of every candidate, the first minimum wins (bem_select_scores_f32 rule 2).  The selection compares the
    scores as float32, like every scorer here; ``ops.niqe`` gives the float64 values."""

    def __init__(self, params: NiqeParams):
        self.params = params
        super().__init__(lambda final: ops.niqe(final.contiguous(), params), "min")


class UiqmUciqe(Scorer):
    """eval.py:255-260,276-280: UIQM (s1) and UCIQE (s2) of every candidate, the first maximum of w * s1 / max(s1) + (1 - w) * s2 / max(s2)
    wins (bem_select_scores_f32 rule 0).  Both are always computed: the driver reports the chosen sample's pair.  The selection compares
    the scores as float32, like every scorer here; ``ops.uiqm_uciqe`` gives the float64 values.
    NaN (UIQM of a candidate with a flat channel): max() skips NaN scores and a NaN weighted score never wins, so such a candidate is
    chosen only when every candidate's score is NaN (then the first).  The reference's Python max() differs when the FIRST candidate is
    NaN: it then keeps index 0."""

    rule = "weighted"

    def __init__(self, uiqm_weight: float = 1.0):
        self.weight = float(uiqm_weight)

    def scores(self, final, targets, samples_per_image, psnr=None):
        u1, u2 = ops.uiqm_uciqe(final.contiguous())
        return u1.float().contiguous(), u2.float().contiguous()
