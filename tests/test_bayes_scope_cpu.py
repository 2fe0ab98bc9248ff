"""The host side of bem.bayes on leaves built on the CPU: a leaf's declared sampling state, and the scope of a forward (the SampleCtx, the
BayesStep of a training forward, the StepState of a step under capture) as its openers enter, nest and unwind it.  No GPU, no kernel."""
import pytest
import torch
import torch.nn as nn

from bem import bayes
from bem.native import BemNativeError


class Leaves(nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = bayes.Linear2dReparameterization(3, 4, bias=True)
        self.dw = bayes.Conv2dReparameterization(4, 4, 3, padding=1, groups=4, bias=False)


def scope():
    return bayes.scope.ctx, bayes.scope.step, bayes.scope.state


def test_a_fresh_leaf_has_no_sample_and_no_draws():
    for m in Leaves().children():
        assert m.sample is None and m.draws == {}
        assert sorted(m.state_dict()) == sorted(n for n, _ in m.named_parameters())          # priors and sampling state stay out of it


def test_deterministic_returns_mu_without_a_scope():
    net = Leaves()
    assert scope() == (None, None, None)
    for m in net.children():
        m.deterministic = True
        for mode in (m.train, m.eval):
            mode()
            w, b, ns = m._sampled(2)
            assert ns == 1 and w.data_ptr() == m.mu_weight.data_ptr() and tuple(w.shape) == (1,) + tuple(m.mu_weight.shape)
            assert (b is None) == (not m.bias) and (b is None or torch.equal(b[0], m.mu_bias))
        assert m.sample is None


def test_a_training_leaf_outside_train_sampling_raises():
    net = Leaves().train()
    with pytest.raises(BemNativeError, match="runs under Network.forward"):
        net.lin._sampled(1)
    with bayes.sampling(bayes.SampleCtx(1, None, seed=1, epoch=1)):                          # a context alone is not a training forward
        with pytest.raises(BemNativeError, match="runs under Network.forward"):
            net.dw._sampled(1)
    assert net.lin.sample is None and net.dw.sample is None


def test_the_scope_unwinds_after_an_exception():
    net = Leaves().train()
    outer, inner, state = bayes.SampleCtx(1, None, seed=1, epoch=1), bayes.SampleCtx(1, None, seed=2, epoch=2), object()
    with bayes.sampling(outer):
        before = scope()
        assert before == (outer, None, None)
        with pytest.raises(KeyError):
            with bayes.sampling(inner), bayes.capturing(state), bayes.train_sampling(net, inner) as step:
                assert scope() == (inner, step, state) and isinstance(step, bayes.BayesStep)
                raise KeyError("inside")
        assert scope() == before
        bank = bayes.BayesBank.of(net)
        assert bank is not None and not bank.ready()                                         # the failed forward built nothing
    assert scope() == (None, None, None)
    assert bayes.EvalSampleBank.of(net) is None


def test_clear_sample_drops_the_sample_and_keeps_the_draws():
    m = Leaves().lin
    m.sample = bayes.Sample(bayes.BayesStep())
    m.sample.put("weight", torch.zeros(4, 3), torch.zeros(1, 4, 3))
    m.draws.update(weight=3, eval=((4, 3), 3, 4))
    m.clear_sample()
    assert m.sample is None and m.draws == {"weight": 3, "eval": ((4, 3), 3, 4)}


def test_ema_decay_is_the_threshold_ema():
    m = Leaves().lin
    assert m.decay == 0.9998
    for step, want in ((0, 0.1), (8, 0.5), (10 ** 6, 0.9998)):
        m.step = step
        assert m.ema_decay() == min(0.9998, (1 + step) / (10 + step)) == pytest.approx(want)
