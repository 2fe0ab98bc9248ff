"""GPU: derived weights (packed / transposed / flipped copies) are made once per weight epoch, by their owner's one ops.Derived cache.

Launches are counted by wrapping the packing and sampling wrappers of bem.ops, not by profiling: steady-state eval packs nothing, a
training step packs what the step before it packed and leaves no more entries or device memory behind, and the Stage-I bank's one packing
launch serves every Bayesian 1x1 leaf forward and backward."""
import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTED = ("pack_pw_weight", "pack_pw_weight_jobs", "bnn_sample")
# the Bayesian steps of a Stage-I forward / training iteration: one launch over the whole net (a bank), or one per tensor
BANKED = ("bnn_bank_sample", "bnn_bank_kl_", "bnn_bank_kl_bwd_", "bnn_bank_reparam_bwd_", "bnn_ebank_sample")
PER_TENSOR = ("randn", "bnn_prior_ema_", "bnn_kl_", "bnn_kl_bwd_", "bnn_reparam_bwd_", "bnn_sample_packed")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bem import ops as _ops
    return _ops


@pytest.fixture
def calls(ops, monkeypatch):
    """{name: [first argument of each call]} for the wrappers in COUNTED, BANKED and PER_TENSOR; ``calls.mark()`` starts a new count.
    ops.attn_fold packs the per-image matrix it has just folded from the features -- an activation, which no cache could hold: those
    calls of pack_pw_weight are counted apart, under "attn_fold", and every test states how many it expects."""
    class Calls(dict):
        def mark(self):
            for v in self.values():
                v.clear()

        def n(self, name):
            return len(self[name])
    rec = Calls({n: [] for n in COUNTED + BANKED + PER_TENSOR + ("attn_fold",)})
    inside = []
    for name in COUNTED + BANKED + PER_TENSOR:
        def wrapped(*a, _orig=getattr(ops, name), _name=name, **k):
            rec["attn_fold" if inside and _name == "pack_pw_weight" else _name].append(a[0])
            return _orig(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)

    def attn_fold(*a, _orig=ops.attn_fold, **k):
        inside.append(1)
        try:
            return _orig(*a, **k)
        finally:
            inside.pop()
    monkeypatch.setattr(ops, "attn_fold", attn_fold)
    return rec


def caches(ops, net):
    """Every module's Derived cache; a holder has one at the most, under one name."""
    out = []
    for m in net.modules():
        own = [k for k, v in m.__dict__.items() if isinstance(v, ops.Derived)]
        assert own in ([], ["_derived"]) and "_cache" not in m.__dict__ and "_bem_derived" not in m.__dict__, (type(m).__name__, own)
        out += [m.__dict__[k] for k in own]
    return out


def small_stage2():
    from bem import archs
    torch.manual_seed(3)
    return archs.DecompDualBranchDDWavelet(n_feat=8, num_blocks=[1, 1, 1], decomp_model="model4").cuda()


def test_eval_steady_state_packs_nothing(ops, calls):
    net = small_stage2().eval()
    x = torch.rand(1, 6, 32, 32, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        calls.mark()
        y1 = net(x)[-1]
        first = calls.n("pack_pw_weight")
        entries = sum(len(c.d) for c in caches(ops, net))
        calls.mark()
        y2 = net(x)[-1]
        assert first > 0 and all(calls.n(n) == 0 for n in COUNTED), {n: calls.n(n) for n in COUNTED}
        assert calls.n("attn_fold") == 2                                     # the decomposition of the image and of the condition
        assert torch.equal(y1, y2)
        ops.bump_weight_epoch()
        calls.mark()
        y3 = net(x)[-1]
        assert calls.n("pack_pw_weight") == first and torch.equal(y1, y3)
        assert sum(len(c.d) for c in caches(ops, net)) == entries            # every entry was replaced, none added


def test_training_steps_leave_nothing_behind(ops, calls):
    """ImageEnhancer-style steps (forward, L1, backward, clip, BemAdamW): every step starts a weight epoch, so every derived weight is
    remade once per step -- and the one of the step before is dropped, in the caches and on the device."""
    from bem import autograd as ag
    from bem.train import BemAdamW
    net = small_stage2().train()
    g = torch.Generator().manual_seed(5)
    x, gt = torch.rand(2, 6, 32, 32, generator=g).cuda(), torch.rand(2, 3, 32, 32, generator=g).cuda()
    opt = BemAdamW([p for p in net.parameters() if p.requires_grad], lr=2e-4, betas=(0.9, 0.999), weight_decay=1e-4)
    seen = []
    for it in range(3):
        calls.mark()
        opt.zero_grad()
        loss = ag.l1_loss(net(x)[-1], gt)
        loss.backward()
        opt.clip_grad_norm_(1.0)
        opt.step()
        del loss
        opt.zero_grad()                                   # gradients zeroed in place: the flat buffer stays
        torch.cuda.synchronize()
        seen.append((calls.n("pack_pw_weight"), sum(len(c.d) for c in caches(ops, net)), torch.cuda.memory_allocated()))
    print("per step (packs, cache entries, bytes allocated):", seen)
    assert seen[1][0] > 0 and seen[2][0] == seen[1][0]
    assert seen[2][1] == seen[1][1]
    assert seen[2][2] == seen[1][2]


def test_bank_preseed_serves_forward_and_backward(ops, calls, monkeypatch):
    """Stage-I training with Philox draws: iteration 1 goes leaf by leaf and builds the BayesBank, iteration 2 takes every Bayesian 1x1
    leaf's operands -- forward (M, K) and transposed, for the input-gradient GEMM -- from the bank's one packing launch.  The launch budget
    of iteration 2 follows from the code: every Bayesian step of the iteration is one launch over the whole net, none is per tensor."""
    from basicsr.bayesian import get_kl_loss
    from bem import autograd as ag
    from bem.modules import BayesBank, SampleCtx, sampling
    from bem.pipeline import build_nets, synthetic_pair
    from bem.train import BemAdamW
    monkeypatch.setenv("BEM_BAYES_BANK", "1")
    net = build_nets(n_feat=16, num_blocks=(1, 1, 1), seed=100, device="cuda")[0].train()
    lq, gt = synthetic_pair((2, 3, 16, 16), seed=6, device="cuda")
    opt = BemAdamW([p for p in net.parameters() if p.requires_grad], lr=2e-4, betas=(0.9, 0.999), weight_decay=1e-4)
    for it in range(2):
        calls.mark()
        opt.zero_grad()
        with sampling(SampleCtx(1, None, seed=7, epoch=it + 1)):
            pred = net(lq)[-1]
        ag.ScaledSumFn.apply(ag.l1_loss(pred, gt), get_kl_loss(net), 0.01 / 2).backward()
        opt.clip_grad_norm_(1.0)
        opt.step()
        torch.cuda.synchronize()
        bank = BayesBank.of(net)
        assert bank.ready() and len(bank.packs) >= 10
        if it == 0:
            assert calls.n("pack_pw_weight_jobs") == 0 and calls.n("bnn_sample") > 0 and calls.n("pack_pw_weight") >= 2 * len(bank.packs)
    lo, hi = bank.w.data_ptr(), bank.w.data_ptr() + 4 * bank.total

    def sampled(t):             # a view (natural or transposed) of a weight the bank sampled
        return lo <= t.data_ptr() < hi
    assert all(sampled(wv) for _, _, _, wv in bank.packs)
    assert calls.n("pack_pw_weight_jobs") == 1 and calls.n("bnn_sample") == 0
    budget = {n: calls.n(n) for n in BANKED + PER_TENSOR}
    assert budget == {**{n: 1 for n in BANKED}, **{n: 0 for n in PER_TENSOR}, "bnn_ebank_sample": 0}, budget
    assert [tuple(t.shape) for t in calls["pack_pw_weight"] if sampled(t)] == []
    for m, _, tr, _ in bank.packs:                                              # what the backward read is the bank's transposed pack
        assert ops.derived(m).d["T"][1] is tr


def test_second_stochastic_eval_forward_is_one_sampling_launch(ops, calls):
    """Stage-I eval with Philox draws of 4 weight sets (2 images x 2 samples: one set per batch row): the first forward goes leaf by leaf
    and records its streams, the second takes every leaf's sets from the EvalSampleBank's one launch."""
    from bem.modules import EvalSampleBank, SampleCtx, sampling
    from bem.pipeline import build_nets, synthetic_pair
    net = build_nets(n_feat=16, num_blocks=(1, 1, 1), seed=100, device="cuda")[0].eval()
    lq = synthetic_pair((2, 3, 16, 16), seed=6, device="cuda")[0].repeat_interleave(2, 0).contiguous()
    for it in range(2):
        calls.mark()
        with sampling(SampleCtx(4, None, seed=7, epoch=it + 1)):
            out = net(lq)[-1]
        if it == 0:
            assert calls.n("bnn_ebank_sample") == 0 and calls.n("bnn_sample") > 0 and calls.n("bnn_sample_packed") > 0
    bank = EvalSampleBank.of(net)
    assert bank is not None and bank.sig is not None and bool(torch.isfinite(out).all())
    assert calls.n("bnn_ebank_sample") == 1 and calls.n("bnn_sample") == 0 and calls.n("bnn_sample_packed") == 0


def test_raw_tensor_conv_keeps_nothing(ops):
    """conv2d on plain tensors (tests, scripts) packs for the call only: once the caller drops its tensors the device memory is back."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    g = torch.Generator().manual_seed(8)
    for shape, kw in (((16, 8, 3, 3), dict(stride=1, pad=1)), ((16, 6, 3, 3), dict(stride=1, pad=1)), ((16, 8, 4, 4), dict(stride=2, pad=1))):
        x, w = torch.randn(1, shape[1], 12, 10, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
        y = ops.conv2d(x, w, None, **kw)
        cw = ops.ConvWeight(w)
        assert torch.equal(ops.conv2d(x, cw, None, **kw), y) and torch.equal(ops.conv2d(x, cw, None, **kw), y)
        del x, w, y, cw
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base


def test_profiled_conv_takes_a_prepared_weight(ops):
    """bench.py brackets one op's launches with events (ops.profile_start): the conv2d bracket reads the weight's shape, prepared or plain."""
    from bem.modules import Conv2dK
    torch.manual_seed(9)
    conv = Conv2dK(8, 16, 3, padding=1).cuda().eval()
    x = torch.randn(1, 8, 12, 10, generator=torch.Generator().manual_seed(9)).cuda()
    with torch.no_grad():
        y = conv(x)
        ops.profile_start("conv2d")
        try:
            y1, y2 = conv(x), ops.conv2d(x, conv.weight.detach(), conv.bias.detach(), pad=1)
        finally:
            rec = ops.profile_stop()
    assert rec["launches"] == 2 and rec["flops"] == 2 * 2.0 * 16 * 8 * 9 * 12 * 10 and torch.equal(y, y1) and torch.equal(y, y2)
