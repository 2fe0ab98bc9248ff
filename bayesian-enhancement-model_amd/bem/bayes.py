"""Bayesian weight sampling of the Stage-I net (basicsr/bayesian/conv.py:10-128, linear.py:8-104, tools.py:76-84): the scope of a
forward (``scope``, opened by ``sampling`` / ``train_sampling`` / ``eval_sampling`` / ``capturing``), the leaves with their current sample
(``leaf.sample``) and recorded streams (``leaf.draws``), the banks that serve all leaves of a net by one launch, and the autograd nodes
of a training forward.  Imports ``ops`` and ``autograd`` only; ``modules``, ``archs`` and the models import this module.
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import Dict, Optional

import torch
import torch.nn as nn
from torch.autograd import Function

from . import ops
from .autograd import grad_of
from .native import BemNativeError


# ------------------------------------------------------------ the scope of a forward
class SampleCtx:
    """Per-forward Bayesian sampling context.

    nsets: number of independent weight samples (= batch size: one per batch element) or 1 (shared);
    eps:   optional {'<module path>.weight'|'.bias': tensor (nsets, *shape)} injected N(0,1) draws
           (parity runs); when None the draws come from the in-kernel Philox stream (seed, counter).
    """

    _epoch = 0      # process-wide forward counter: successive forwards never reuse a Philox stream

    def __init__(self, nsets: int, eps: Optional[Dict[str, torch.Tensor]] = None, seed: int = 0, rank: int = 0, epoch: Optional[int] = None,
                 epoch_dev: Optional[torch.Tensor] = None):
        self.nsets, self.eps, self.seed, self.rank = nsets, eps, seed, rank
        self.counter = 0
        # epoch_dev: one int64 on the device holding ``epoch << 20``, added to the stream ids by the sampling kernels; the ids handed out
        # here then carry epoch 0.  A captured step (HIP graph) replays with whatever epoch the host wrote there last.
        self.epoch_dev = epoch_dev
        self.bank = None                     # EvalSampleBank whose one launch made this forward's draws (set by eval_sampling)
        self.counter0 = 0                    # value of ``counter`` when the forward began (the leaves record relative stream numbers)
        if epoch_dev is not None:
            epoch = 0
        if epoch is None:
            SampleCtx._epoch += 1
            epoch = SampleCtx._epoch
        self.epoch = int(epoch)              # a caller-chosen epoch (the training iteration) makes the draws a function of (seed, rank, iteration)

    def next_stream(self):
        """A fresh Philox stream id per sampled tensor: [rank : 16 bits | forward epoch : 24 bits | tensor counter : 20 bits].
        Ranks of a multi-GPU run that share ``seed`` therefore draw different weight sets; bit 62 is reserved for the
        condition-noise draws (BEMPipeline.candidates)."""
        self.counter += 1
        if self.counter >= (1 << 20) or self.epoch >= (1 << 24):
            raise RuntimeError("SampleCtx: Philox stream id space exhausted (2^20 tensors per forward, 2^24 forwards per process)")
        return (self.rank << 44) | (self.epoch << 20) | self.counter


class BayesStep:
    """One training forward's Bayesian bookkeeping: the leaves that drew a weight sample, to be folded back into mu / rho once the
    whole backward pass has run (the sampled weight's gradient is complete only then)."""

    def __init__(self):
        self.leaves, self.done = [], False
        self.bank = None                 # BayesBank when the samples of this forward were drawn by its one launch
        self.counter0 = 0                # the context's stream counter when the leaf-by-leaf draws of this forward began

    def finish(self):
        if self.done:
            return
        self.done = True
        if self.bank is not None:        # dmu += dw, drho += dw eps sigmoid(rho) for every tensor of the net in one launch
            ops.bnn_bank_reparam_bwd_(self.bank)
        for m in self.leaves:
            m.clear_sample() if self.bank is not None else m.fold_sample_grads()


class _Scope:
    """Which forward is running, to be read as ``scope.ctx`` (its SampleCtx), ``scope.step`` (the BayesStep of a training forward) and
    ``scope.state`` (the bem.train.StepState of a step under HIP-graph capture: per-iteration scalars come from it); the openers write."""
    ctx = step = state = None


scope = _Scope()


@contextlib.contextmanager
def _entered(field, value):
    prev = getattr(scope, field)
    setattr(scope, field, value)
    try:
        yield value
    finally:
        setattr(scope, field, prev)


def sampling(ctx: Optional[SampleCtx]):
    """``with sampling(SampleCtx(...)):`` scopes the Bayesian draws of the enclosed forwards."""
    return _entered("ctx", ctx)


def capturing(state):
    """``with capturing(StepState(...)):`` the enclosed training step is being recorded into a HIP graph."""
    return _entered("state", state)


def set_module_paths(root: nn.Module):
    """Record each leaf's dotted path (used as the key of injected epsilon draws)."""
    for name, m in root.named_modules():
        if hasattr(m, "module_path"):
            m.module_path = name


@contextlib.contextmanager
def train_sampling(net, ctx: SampleCtx):
    """The sampling scope of one training forward of ``net``; yields its BayesStep.  Every such forward draws new weights (derived copies of
    the last draw are stale): by the one launch of the net's BayesBank when that is ready, else leaf by leaf, recording the draw order the
    bank is built from once the forward has run.  BEM_BAYES_BANK=0 keeps the per-leaf form."""
    step = BayesStep()
    ops.bump_weight_epoch()
    with _entered("step", step), sampling(ctx):
        set_module_paths(net)
        if os.environ.get("BEM_BAYES_BANK", "1") != "0":
            bank = BayesBank.of(net, create=True)
            if bank.ready() and bank.usable(ctx):
                bank.sample(ctx, step, scope.state)
        step.counter0 = ctx.counter if step.bank is None else 0
        yield step
        bank = BayesBank.of(net)
        if bank is not None and not bank.ready() and ctx.eps is None:
            bank.try_build()


@contextlib.contextmanager
def eval_sampling(net, ctx: SampleCtx):
    """The sampling scope of one stochastic or deterministic eval forward of ``net``.  With Philox draws of more than one set, all leaves'
    weight sets come from one launch of the net's EvalSampleBank; the first such forward goes leaf by leaf and records the streams."""
    with sampling(ctx):
        set_module_paths(net)
        if ctx.eps is None and ctx.nsets > 1:
            bank = EvalSampleBank.of(net, create=True)
            ctx.counter0 = ctx.counter
            if bank.usable(ctx):
                bank.sample(ctx)
        yield ctx
        ctx.bank = None


# ------------------------------------------------------------ leaves
class Sample:
    """A leaf's weight sample of one training forward.  w / b: the sampled weight and bias (b None without a bias), which the kernels see
    as the leaf's parameters (bem.autograd.wb; their .grad is folded into mu / rho after the backward pass); eps_w / eps_b: the N(0,1) draws
    behind them; owner: the BayesStep of that forward; packed: w as forward x6 GEMM operand where the BayesBank packed it, else None."""
    __slots__ = ("w", "b", "eps_w", "eps_b", "owner", "packed")

    def __init__(self, owner=None):
        self.w = self.b = self.eps_w = self.eps_b = self.packed = None
        self.owner = owner

    def put(self, kind, w, eps):
        if kind == "weight":
            self.w, self.eps_w = w, eps
        else:
            self.b, self.eps_b = w, eps


class _BayesBase(nn.Module):
    def _setup(self, shape, init_mu, sigma_init, decay, bias):
        """mu / rho of the weight (+ bias); the prior_* buffers (non-persistent, as conv.py:57-70): copies of the fresh mu / rho, which the
        training forward moves towards the parameters (threshold EMA) and a loaded checkpoint does not touch -- the reference's behaviour;
        the sampling state: no ``sample``, no ``draws`` = {'weight' | 'bias': stream in training, 'eval': (mk, weight stream, bias stream)},
        the Philox streams of a forward (1, 2, ...) the leaf drew from when it went leaf by leaf, which the banks then give its tensors;
        mk = (M, K) where it asked for its weights as x6 GEMM operand, None for natural order."""
        self.deterministic, self.module_path = False, ""
        self.decay, self.sigma_init, self.step, self.bias = decay, sigma_init, 0, bias
        for kind in self._kinds():
            shp = shape if kind == "weight" else shape[:1]
            setattr(self, f"mu_{kind}", nn.Parameter(torch.zeros(shp)))
            setattr(self, f"rho_{kind}", nn.Parameter(torch.full(shp, math.log(math.expm1(abs(sigma_init)) + 1e-20))))
        init_mu(self.mu_weight)
        for kind in self._kinds():
            self.register_buffer(f"prior_mu_{kind}", getattr(self, f"mu_{kind}").detach().clone(), persistent=False)
            self.register_buffer(f"prior_rho_{kind}", getattr(self, f"rho_{kind}").detach().clone(), persistent=False)
        self.sample: Optional[Sample] = None
        self.draws = {}

    def _kinds(self):
        return ("weight", "bias") if self.bias else ("weight",)

    def clear_sample(self):
        self.sample = None

    def ema_decay(self):
        """The prior's EMA decay of this iteration (threshold EMA, conv.py:84-98)."""
        return min(self.decay, (1 + self.step) / (10 + self.step))

    def _train_sample(self):
        """Once per training forward (conv.py:84-104): move the prior, draw eps, form w = mu + softplus(rho) eps.  The sampled tensors
        are what the forward / backward kernels see as this leaf's weight and bias (bem.autograd.wb)."""
        step = scope.step
        if step is None:
            raise BemNativeError("Bayesian leaves: a training-mode forward runs under Network.forward, which scopes the weight sample")
        if self.sample is not None and self.sample.owner is step:
            return
        ctx, st = scope.ctx, scope.state
        d, d_dev = self.ema_decay(), (st.slot(self.ema_decay) if st is not None else None)   # a captured step reads the iteration's decay from HBM
        s = Sample(step)
        for kind in self._kinds():
            mu, rho = getattr(self, f"mu_{kind}"), getattr(self, f"rho_{kind}")
            ops.bnn_prior_ema_(getattr(self, f"prior_mu_{kind}"), getattr(self, f"prior_rho_{kind}"), mu.detach(), rho.detach(), d, d_dev)
            if ctx.eps is not None:
                e = ctx.eps[f"{self.module_path}.{kind}"].reshape((1,) + tuple(mu.shape)).contiguous()
            else:
                e = ops.randn((1,) + tuple(mu.shape), mu.device, ctx.seed, ctx.next_stream(), ctx.epoch_dev)
                self.draws[kind] = ctx.counter - step.counter0             # for BayesBank: same streams
            s.put(kind, ops.bnn_sample(mu.detach(), rho.detach(), 1, e)[0], e)
        if st is None:
            self.step += 1
        else:
            st.on_advance(self._count_step)           # recorded, not run: the counter moves when the captured step is replayed
        self.sample = s
        step.leaves.append(self)

    def _count_step(self):
        self.step += 1

    def fold_sample_grads(self):
        """dmu += dw, drho += dw eps sigmoid(rho) for the sampled weight and bias of the finished backward pass, then drop the sample."""
        s = self.sample or Sample()
        for w, e, kind in ((s.w, s.eps_w, "weight"), (s.b, s.eps_b, "bias")):
            if w is not None and w.grad is not None:
                mu, rho = getattr(self, f"mu_{kind}"), getattr(self, f"rho_{kind}")
                ops.bnn_reparam_bwd_(w.grad, e, rho.detach(), grad_of(mu), grad_of(rho))
        self.clear_sample()

    def kl_terms(self):
        return [tuple(getattr(self, f"{p}_{kind}") for p in ("mu", "rho", "prior_mu", "prior_rho")) for kind in self._kinds()]

    def _sigma(self):
        rho = self.rho_weight
        return ops.derived(self).get("sigma", [rho], lambda: ops.bnn_sample(torch.zeros_like(rho), rho.detach(), 1, torch.ones_like(rho))[0])

    def _sampled(self, B, packed_mk=None):
        """(weights (nsets,*shape), bias (nsets,C)|None, nsets) for this forward; with ``packed_mk = (M, K)`` the sampled
        weights come back already packed for the x6 GEMM (stochastic mode only)."""
        if self.deterministic:
            return self.mu_weight.detach()[None], (self.mu_bias.detach()[None] if self.bias else None), 1
        if self.training:
            self._train_sample()             # raises outside Network's training forward (e.g. train() mode under no_grad: call eval())
            s = self.sample
            return s.w[None], (s.b[None] if self.bias else None), 1
        ctx = scope.ctx or SampleCtx(B, None, seed=torch.initial_seed() & 0xFFFFFFFF)      # outside a Network forward: one-off context (fresh epoch)
        ns = ctx.nsets
        if ctx.bank is not None:                     # this forward's draws were all made by one launch (EvalSampleBank)
            return ctx.bank.take(self, packed_mk, ns)
        ew = eb = None
        if ctx.eps is not None:
            ew = ctx.eps[self.module_path + ".weight"].contiguous()
            if self.bias:
                eb = ctx.eps[self.module_path + ".bias"].contiguous()
        if packed_mk is not None:
            # GEMM weights go straight into operand order (same Philox stream ids, same values as sample-then-pack)
            # sigma = log1p(exp(rho)) once per weight version (one launch of the sampler with mu = 0, eps = 1), not once per sample
            w = ops.bnn_sample_packed(self.mu_weight.detach(), self._sigma(), ns, packed_mk[0], packed_mk[1], ew, ctx.seed, ctx.next_stream(), sigma_given=True, stream_add=ctx.epoch_dev)
        else:
            w = ops.bnn_sample(self.mu_weight.detach(), self.rho_weight.detach(), ns, ew, ctx.seed, ctx.next_stream(), ctx.epoch_dev)
        tw, tb, b = ctx.counter - ctx.counter0, None, None
        if self.bias:
            b = ops.bnn_sample(self.mu_bias.detach(), self.rho_bias.detach(), ns, eb, ctx.seed, ctx.next_stream(), ctx.epoch_dev)
            tb = ctx.counter - ctx.counter0
        self.draws["eval"] = (packed_mk, tw, tb)       # which streams of the forward this leaf drew from, and in which form (EvalSampleBank)
        return w, b, ns

    def gemm_weights(self, B):
        """Pointwise interface of a 1x1 conv / Linear2d leaf: (x6-packed weights (nsets, packed(M, K)), bias); (M, K) = self._mk."""
        if self.deterministic or self.training:
            w, b, ns = self._sampled(B)
            if not self.deterministic and self.sample.packed is not None:
                return self.sample.packed, b         # packed by the bank's one launch for this forward
            return ops.pack_pw_weight(w.reshape((ns,) + self._mk).contiguous()), b
        Wp, b, _ = self._sampled(B, self._mk)
        return Wp, b


class Conv2dReparameterization(_BayesBase):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 sigma_init=0.05, decay=0.9998):
        super().__init__()
        ks = tuple(kernel_size) if isinstance(kernel_size, (tuple, list)) else (kernel_size, kernel_size)
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.stride, self.padding, self.dilation, self.groups = stride, padding, dilation, groups
        self._setup((out_channels, in_channels // groups) + ks, lambda w: nn.init.kaiming_normal_(w, mode="fan_in", nonlinearity="leaky_relu"), sigma_init, decay, bias)
        self._mk = (out_channels, in_channels)
        self._is_dw = groups == in_channels and groups == out_channels and ks == (3, 3)
        self._is_pw = groups == 1 and ks == (1, 1)
        if not (self._is_dw or self._is_pw):
            raise NotImplementedError("Bayesian conv: only 1x1 dense and 3x3 depthwise occur on the BEM path")

    # depthwise interface (the pointwise one, gemm_weights, is _BayesBase's)
    def dw_weights(self, B):
        w, b, ns = self._sampled(B)
        return (w if ns > 1 else w[0]), (b if (b is None or ns > 1) else b[0])


class Linear2dReparameterization(_BayesBase):
    def __init__(self, in_features, out_features, bias=True, sigma_init=0.05, decay=0.9998):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self._mk = (out_features, in_features)
        self._setup((out_features, in_features), nn.init.xavier_uniform_, sigma_init, decay, bias)


# ------------------------------------------------------------ banks: all Bayesian tensors of a net in one launch
def _tables(rows, blks, dev):
    """(int64 row table, int32 (row, block) list, number of blocks) of a bank kernel, on the device."""
    return torch.tensor(rows, dtype=torch.int64).to(dev), torch.tensor(blks, dtype=torch.int32).to(dev), len(blks)


class _Bank:
    def __init__(self, net):
        self.leaves = [m for m in net.modules() if isinstance(m, _BayesBase)]
        self.sig = None

    @classmethod
    def of(cls, net, create=False):
        """The bank of this kind that ``net`` holds; None when it has not been created (``create`` makes it)."""
        bank = net.__dict__.get("_" + cls.__name__)
        if bank is None and create:
            bank = net.__dict__["_" + cls.__name__] = cls(net)
        return bank


class BayesBank(_Bank):
    """All Bayesian tensors of a net as segments of flat arenas, so that the per-tensor steps of a training iteration -- prior EMA + eps
    draw + weight sample, KL, KL backward, reparameterisation backward (conv.py:84-112, tools.py:76-84) -- are ONE launch each over the
    whole net (bem_bnn_bank_*) instead of one per tensor (60 leaves / 90 tensors in the shipped Stage-I net: ~630 launches per step).

    The prior buffers of the leaves become views of the bank's prior arenas; the sampled weights, their eps and their gradient buffers
    are persistent views of the w / eps / gw arenas (the sampling launch zeroes gw), held by one persistent ``Sample`` per leaf.  Parameters
    and their .grad buffers are addressed by pointer (they usually live in BemAdamW's flat buffers); the tables are rebuilt when any of
    those pointers changes.  Used for Philox draws only -- injected eps (parity runs) take the per-leaf path."""

    def ready(self):
        return self.sig is not None

    def try_build(self):
        """After a per-leaf Philox forward: every tensor has recorded which stream of the forward it drew from (1 .. S in execution
        order); the bank gives each segment that same stream, so its draws are the per-leaf path's draws."""
        order = sorted(m.draws.get(kind, -1) for m, kind, _, _ in self._tensors())
        if order == list(range(1, len(order) + 1)) and not torch.cuda.is_current_stream_capturing():
            self._build()

    def _tensors(self):
        for m in self.leaves:
            for kind in m._kinds():
                yield m, kind, getattr(m, f"mu_{kind}"), getattr(m, f"rho_{kind}")

    def usable(self, ctx):
        if ctx is None or ctx.eps is not None or ctx.nsets != 1 or not self.leaves:
            return False
        m0 = self.leaves[0]
        return all(m.training and not m.deterministic and m.decay == m0.decay and m.step == m0.step for m in self.leaves)

    def _signature(self):
        sig = []
        for m, kind, mu, rho in self._tensors():
            sig += [mu.data_ptr(), rho.data_ptr(), grad_of(mu).data_ptr(), grad_of(rho).data_ptr(),
                    getattr(m, f"prior_mu_{kind}").data_ptr(), getattr(m, f"prior_rho_{kind}").data_ptr()]
        return tuple(sig)

    def _build(self):
        if torch.cuda.is_current_stream_capturing():
            raise BemNativeError("BayesBank: its tables cannot be (re)built while a HIP graph is being captured")
        dev = self.leaves[0].mu_weight.device
        rows, blks, off = [], [], 0
        items = list(self._tensors())
        for s_, (m, kind, mu, rho) in enumerate(items):
            n = mu.numel()
            inv_n = int.from_bytes(torch.tensor(1.0 / n, dtype=torch.float32).numpy().tobytes(), "little")
            rows.append([mu.data_ptr(), rho.data_ptr(), grad_of(mu).data_ptr(), grad_of(rho).data_ptr(), off, n, m.draws[kind], inv_n])
            blks += [[s_, b] for b in range(0, n, 1024)]
            off += (n + 3) // 4 * 4
        self.total = off
        pm, pr = torch.empty(off, device=dev), torch.empty(off, device=dev)
        self.w, self.eps, self.gw = torch.zeros(off, device=dev), torch.zeros(off, device=dev), torch.zeros(off, device=dev)
        self.views, samples = [], {id(m): Sample() for m in self.leaves}
        for (m, kind, mu, rho), r in zip(items, rows):
            o, n = r[4], r[5]
            with torch.no_grad():
                pm[o:o + n].copy_(getattr(m, f"prior_mu_{kind}").reshape(-1))
                pr[o:o + n].copy_(getattr(m, f"prior_rho_{kind}").reshape(-1))
            setattr(m, f"prior_mu_{kind}", pm[o:o + n].view(mu.shape))
            setattr(m, f"prior_rho_{kind}", pr[o:o + n].view(mu.shape))
            wv = self.w[o:o + n].view(mu.shape)
            wv.grad = self.gw[o:o + n].view(mu.shape)
            ev = self.eps[o:o + n].view((1,) + tuple(mu.shape))
            self.views.append((m, kind, wv, ev))
            samples[id(m)].put(kind, wv, ev)
        self.samples = [(m, samples[id(m)]) for m in self.leaves]         # handed to the leaves by every sample()
        self.pm, self.pr = pm, pr
        self.segs, self.blks, self.nblk = _tables(rows, blks, dev)
        # the x6 operand forms of every 1x1 weight sample -- forward (M, K) and transposed (K, M, for the input-gradient GEMM) -- by ONE more
        # launch (bem_pack_pw_weight_x6_jobs) instead of two small packing launches per layer and iteration
        pw = [(m, s) for m, s in self.samples if getattr(m, "_is_pw", False) or isinstance(m, Linear2dReparameterization)]
        jobs, jblk, spans, poff = [], [], [], 0
        for m, s in pw:
            M, K = m._mk
            for (Mj, Kj, rs, cs) in ((M, K, K, 1), (K, M, 1, K)):
                it = ((Mj + 31) // 32) * ((Kj + 15) // 16) * 64
                jobs.append([s.w.data_ptr(), poff, Mj | (Kj << 32), rs, cs, it, 0, 0])
                jblk += [[len(jobs) - 1, b] for b in range((it + 255) // 256)]
                spans.append((poff, ops.packed_elems(Mj, Kj, True), (Mj, Kj)))
                poff += spans[-1][1]
        self.packs = []                  # (leaf, forward operand, transposed operand, the sampled weight they are packed from)
        if jobs:
            self.parena = torch.empty(poff, device=dev, dtype=torch.float32)
            self.jobs, self.jblks, self.njblk = _tables(jobs, jblk, dev)
            vs = [self.parena[o:o + pe].view(1, pe) for o, pe, _ in spans]
            for v, (_, _, mk) in zip(vs, spans):
                v._bem_mk = mk
            for (m, s), fwd, tr in zip(pw, vs[0::2], vs[1::2]):
                s.packed = fwd                                               # gemm_weights of a training forward
                self.packs.append((m, fwd, tr, s.w))
        self.sig = self._signature()

    def sample(self, ctx, step, state=None):
        """One launch: every leaf's prior EMA, eps and weight sample for this forward.  The leaves are handed their samples, marked as
        drawn for ``step``; their own _train_sample() then has nothing left to do."""
        if self.sig != self._signature():
            self._build()                                # a parameter, gradient or prior buffer moved (optimizer created, net.to(...))
        m0 = self.leaves[0]
        d_dev = state.slot(m0.ema_decay) if state is not None else None
        base = (ctx.rank << 44) | (ctx.epoch << 20) | ctx.counter
        ops.bnn_bank_sample(self, m0.ema_decay(), d_dev, ctx.seed, base, ctx.epoch_dev)
        ctx.counter += len(self.views)
        if self.packs:
            ops.pack_pw_weight_jobs(self.jobs, self.jblks, self.njblk, self.parena)
            for m, _, tr, wv in self.packs:
                ops.derived(m).put("T", [wv], tr)                                           # autograd._pack(m, "T", [w], ...) hits
        for m, s in self.samples:
            s.owner, m.sample = step, s
            step.leaves.append(m)
            if state is None:
                m.step += 1
            else:
                state.on_advance(m._count_step)
        step.bank = self


class EvalSampleBank(_Bank):
    """The N weight sets of every Bayesian tensor of a net, for one stochastic (eval) forward, drawn by ONE launch (bem_bnn_ebank_sample_f32)
    into a flat arena; the leaves then take views of it.  Leaf by leaf the Stage-I net of the Monte-Carlo loop issues 90 sampling launches
    per forward between its layers' kernels, on planes of H/16 x W/16 pixels where every dependent launch costs >= 5 us.

    Built after a leaf-by-leaf Philox forward, which records for every leaf the form it asked for (x6-packed GEMM operand or natural
    order) and the streams it drew from: the bank gives each tensor that same stream, so its values are the per-leaf path's values.
    Rebuilt when the number of sets, a parameter, a cached sigma or a leaf's form changes.  Injected eps take the per-leaf path."""

    def usable(self, ctx):
        return (ctx is not None and ctx.eps is None and ctx.epoch_dev is None and bool(self.leaves)
                and all(not m.training and not m.deterministic and "eval" in m.draws for m in self.leaves))

    def _signature(self, ns):
        sig = [ns]
        for m in self.leaves:
            mk, tw, tb = m.draws["eval"]
            sig += [mk, tw, tb, m.mu_weight.data_ptr(), (m._sigma() if mk else m.rho_weight).data_ptr()]
            if m.bias:
                sig += [m.mu_bias.data_ptr(), m.rho_bias.data_ptr()]
        return tuple(sig)

    def _build(self, ns):
        dev = self.leaves[0].mu_weight.device
        rows, spans, off = [], [], 0                     # spans: (leaf, mk, (arena offset, shape) of the weight sets, of the bias sets | None)

        def natural(mu, rho, t):
            nonlocal off
            n = mu.numel()
            rows.append([mu.data_ptr(), rho.data_ptr(), off, n, 0, t, (ns * n + 3) // 4, ns * n])
            off += (ns * n + 3) // 4 * 4
            return rows[-1][2], (ns,) + tuple(mu.shape)
        for m in self.leaves:
            mk, tw, tb = m.draws["eval"]
            if mk is not None:
                M, K = mk
                rows.append([m.mu_weight.data_ptr(), m._sigma().data_ptr(), off, M * K, M | (K << 32), tw, ns * ((M + 31) // 32) * ((K + 15) // 16) * 64, ns * M * K])
                wv = off, (ns, ops.packed_elems(M, K, True))
                off += ns * wv[1][1]
            else:
                wv = natural(m.mu_weight, m.rho_weight, tw)
            spans.append((m, mk, wv, natural(m.mu_bias, m.rho_bias, tb) if m.bias else None))
        if sorted(r[5] for r in rows) != list(range(1, len(rows) + 1)):
            return False                                 # the recorded forward did not draw every Bayesian tensor exactly once: stay leaf by leaf
        self.arena = torch.empty(off, device=dev, dtype=torch.float32)
        view = lambda o, shape: self.arena[o:o + math.prod(shape)].view(shape)
        self.views = {}
        for m, mk, wv, bv in spans:
            w = view(*wv)
            if mk is not None:
                w._bem_mk = mk
            self.views[id(m)] = (mk, w, None if bv is None else view(*bv))
        self.nrows = len(rows)
        self.segs, self.blks, self.nblk = _tables(rows, [[s_, b] for s_, r in enumerate(rows) for b in range((r[6] + 255) // 256)], dev)
        self.sig = self._signature(ns)
        return True

    def sample(self, ctx):
        ns = ctx.nsets
        if self.sig != self._signature(ns) and not self._build(ns):
            self.sig = None
            return
        base = (ctx.rank << 44) | (ctx.epoch << 20) | ctx.counter
        ops.bnn_ebank_sample(self, ctx.seed, base)
        ctx.counter += self.nrows
        ctx.bank = self

    def take(self, leaf, packed_mk, ns):
        mk, w, b = self.views[id(leaf)]
        if mk != packed_mk:
            raise BemNativeError("EvalSampleBank: a leaf asked for its weights in another form than in the recorded forward")
        return w, b, ns


# ------------------------------------------------------------ autograd nodes of a training forward (basicsr/bayesian/conv.py:84-114, linear.py:61-90, tools.py:76-84)
class BayesAnchorFn(Function):
    """Identity on the network output; its backward (the first node of the pass) queues BayesStep.finish to run after the pass."""

    @staticmethod
    def forward(ctx, out, step):
        ctx.step = step
        return out.view_as(out)

    @staticmethod
    def backward(ctx, g):
        torch.autograd.Variable._execution_engine.queue_callback(ctx.step.finish)
        return g, None


class KLFn(Function):
    """sum over the Bayesian leaves of kl_div(q || EMA prior).mean() for weight (+ bias)  (get_kl_loss, tools.py:76-84)."""

    @staticmethod
    def forward(ctx, leaves, *params):
        out = torch.zeros(1, device=params[0].device, dtype=torch.float32)
        st = getattr(leaves[0].sample, "owner", None)
        bank = getattr(st, "bank", None)
        if bank is not None and len(bank.leaves) == len(leaves) and all(a is b and getattr(a.sample, "owner", None) is st for a, b in zip(bank.leaves, leaves)):
            ops.bnn_bank_kl_(bank, out)              # the forward that has just run drew its samples through the bank: same tensors, one launch
            ctx.bank = bank
            return out.reshape(())
        ctx.bank = None
        for m in leaves:
            for mu, rho, pmu, prho in m.kl_terms():
                ops.bnn_kl_(mu.detach(), rho.detach(), pmu, prho, out)
        ctx.leaves = leaves
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        g = g.reshape(1).contiguous().float()
        if ctx.bank is not None:
            ops.bnn_bank_kl_bwd_(ctx.bank, g)
        else:
            for m in ctx.leaves:
                for mu, rho, pmu, prho in m.kl_terms():
                    ops.bnn_kl_bwd_(mu.detach(), rho.detach(), pmu, prho, g, grad_of(mu), grad_of(rho))
        return (None,) * len(ctx.needs_input_grad)
