"""Every consumer of the device Philox / Box-Muller draw (csrc/bem_common.h) against the float64 CPU model tests/philox_ref.py, element
for element: a wrong element -> (counter block, component, stream) mapping shows on nearly every element, a right one on none, so the
only tolerance is that of the float32 evaluation.

Tolerance of a draw:   |z_gpu - z_model| <= 1e-6 r + 1e-9,   r = sqrt(-2 ln u1) the Box-Muller radius of the element's pair.
  The uniforms u1, u2 are exact in float32 (24-bit integers times 2^-24).  Angle theta = fl(2 pi) u2 < 8: |fl(2 pi) - 2 pi| = 1.75e-7
  and half an ulp of the product (2.4e-7) give <= 4.2e-7 absolute on the angle, i.e. on sin / cos; sincosf <= 2 ulp of a value <= 1
  = 2.4e-7; logf and sqrtf <= 1 ulp each, together <= 1.8e-7 relative on r; the final product r * cs rounds once more, 6e-8.  Sum:
  about 9e-7 r.  The library is built with -fno-fast-math, so the device math functions keep these documented bounds.  The float32
  Box-Muller emulated on the CPU stays within 4.4e-7 r of the float64 value, a factor of two inside the bound.
Tolerance of a sampled weight w = mu + softplus(rho) z:
  |w_gpu - (mu + softplus64(rho) z_model)| <= sigma (1e-6 r + 5e-7 |z|) + 2^-23 |w| + 1e-9
  sigma times the z bound, plus log1pf(expf(.)) <= 3 ulp on sigma and one rounding of sigma * z (together < 5e-7 sigma |z|), plus one
  rounding of the sum (2^-24 |w|, doubled for the binade edge).

The largest observed |dz| / r and |dw| / bound per consumer are printed; with BEM_PHILOX_PARITY_OUT=<file> they are written there too
(profiles/philox_parity.txt is one such run)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import philox_ref as P

pytestmark = pytest.mark.gpu

RHO0 = float(np.log(np.expm1(0.05)))           # sigma_init = 0.05 of the shipped nets
FIG = {}                                       # consumer -> {"dz/r": worst, "dw/bound": worst}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bem import ops as _ops
    yield _ops
    lines = [f"{k:<34s} {d['elements']:>9d} elements  " + "  ".join(f"max {m} = {v:.3e}" for m, v in sorted(d.items()) if m != "elements")
             for k, d in sorted(FIG.items())]
    text = ("Philox / Box-Muller draws on the GPU vs the float64 CPU model (tests/test_philox_gpu.py), all elements compared\n"
            "bounds: |dz| <= 1e-6 r + 1e-9  (dz/r column: 1e-6 allowed);  |dw| <= bound (dw/bound column: 1 allowed)\n" + "\n".join(lines) + "\n")
    print("\n" + text)
    out = os.environ.get("BEM_PHILOX_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            f.write(text)


def note(consumer, metric, value, count):
    d = FIG.setdefault(consumer, {})
    d[metric] = max(d.get(metric, 0.0), float(value))
    d["elements"] = d.get("elements", 0) + int(count)


def f64(t):
    return t.detach().cpu().double().numpy().reshape(-1)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_z(consumer, got, n, seed, sid, what=""):
    """All n draws of (seed, sid) against the model."""
    z, r = P.normals(n, seed, sid)
    g = f64(got)
    assert g.shape == z.shape and np.isfinite(g).all(), (consumer, what)
    d = np.abs(g - z)
    note(consumer, "dz/r", (d / np.maximum(r, 1e-3)).max(), d.size)
    bad = d > 1e-6 * r + 1e-9
    assert not bad.any(), f"{consumer} {what}: {int(bad.sum())} of {n} draws off, first at {int(np.argmax(bad))}: got {g[np.argmax(bad)]!r} model {z[np.argmax(bad)]!r}"


def check_w(consumer, got, mu, rho, nsets, seed, sid, what="", prefix=None):
    """got (nsets, n) natural-order samples: set s, element e takes draw s * n + e of (seed, sid)."""
    mu, rho = f64(mu), f64(rho)
    n = mu.size
    if prefix is not None:                                            # the first elements of set 0 only
        n0, n, nsets = n, min(prefix, n), 1
        got, mu, rho = got.reshape(-1, n0)[:1, :n], mu[:n], rho[:n]
    z, r = P.normals(nsets * n, seed, sid)
    z, r = z.reshape(nsets, n), r.reshape(nsets, n)
    g = f64(got).reshape(nsets, n)
    sigma = P.softplus64(rho)
    ref = mu + sigma * z
    bound = sigma * (1e-6 * r + 5e-7 * np.abs(z)) + 2.0 ** -23 * np.abs(ref) + 1e-9
    d = np.abs(g - ref)
    assert np.isfinite(g).all(), (consumer, what)
    note(consumer, "dw/bound", (d / bound).max(), d.size)
    bad = d > bound
    assert not bad.any(), f"{consumer} {what}: {int(bad.sum())} of {g.size} weights off, first at {np.argwhere(bad)[0].tolist()} (set, element)"


def rand_mu_rho(shape, seed):
    g = torch.Generator().manual_seed(seed)
    mu = torch.randn(shape, generator=g)
    rho = RHO0 + 4 * torch.rand(shape, generator=g) - 2              # the shipped nets' initial rho, +- 2
    return mu.cuda(), rho.cuda()


def i64(v):
    return torch.tensor([v], dtype=torch.int64, device="cuda")


# ------------------------------------------------------------------------------------------------ bem_randn_f32
SEED_A, SEED_B = 0xDEADBEEF00000007, 0x0BADF00D00000007             # differ in the high word only
STREAMS = (7, P.stream_id(3, 5, 9), P.noise_stream_id(65535, 123), (1 << 62) | (1 << 61) | (9 << 44) | 0xFFFFFFFF)


def test_randn_every_element(ops):
    for n in (1, 2, 3, 4, 5, 255, 1023, 1025, (1 << 20) + 3):
        for sid in STREAMS:
            a, b = ops.randn((n,), "cuda", SEED_A, sid), ops.randn((n,), "cuda", SEED_B, sid)
            check_z("randn", a, n, SEED_A, sid, f"n={n} stream={sid:#x}")
            check_z("randn", b, n, SEED_B, sid, f"n={n} stream={sid:#x} seed B")
            assert not torch.equal(a, b)                              # the high word of the seed reaches the key
    n = 4099
    outs = [ops.randn((n,), "cuda", SEED_A, s) for s in STREAMS] + [ops.randn((n,), "cuda", SEED_A, STREAMS[1] + (1 << 44))]
    for i in range(len(outs)):
        for j in range(i):
            assert not torch.equal(outs[i][:8], outs[j][:8]), (i, j)   # the high word of the stream id reaches the counter


def test_randn_stream_add_is_part_of_the_id(ops):
    n = 1025
    for sid, add in ((P.stream_id(2, 0, 17), 5 << 20), (0xFFFFFFFF, 1), (P.noise_stream_id(1, 0), 5 << 20)):
        a = ops.randn((n,), "cuda", SEED_A, sid, i64(add))
        b = ops.randn((n,), "cuda", SEED_A, sid + add)
        assert bits_equal(a, b), hex(sid)
        assert not torch.equal(a, ops.randn((n,), "cuda", SEED_A, sid))
        check_z("randn (stream_add)", a, n, SEED_A, sid + add, hex(sid))


# ------------------------------------------------------------------------------------------------ bem_bnn_sample_f32
@pytest.mark.parametrize("nsets", [1, 3, 16])
def test_bnn_sample_every_element(ops, nsets):
    """The flat index runs across sets: with n % 4 != 0 a counter block straddles two sets."""
    for n in (1, 3, 5, 40, 1600, 1601):
        mu, rho = rand_mu_rho((n,), 100 + n)
        sid = P.stream_id(1, 2, n)
        w = ops.bnn_sample(mu, rho, nsets, None, seed=SEED_A, stream_id=sid)
        assert w.shape == (nsets, n)
        check_w("bnn_sample", w, mu, rho, nsets, SEED_A, sid, f"n={n} nsets={nsets}")
        wa = ops.bnn_sample(mu, rho, nsets, None, seed=SEED_A, stream_id=sid - (5 << 20), stream_add=i64(5 << 20))
        assert bits_equal(w, wa), (n, nsets)
        if nsets > 1 and n > 1:
            assert not torch.equal(w[0] - mu, w[1] - mu)


# ------------------------------------------------------------------------------------------------ bem_bnn_sample_pack_x6
def unpack_x6(Wp, M, K):
    """(nsets, packed(M, K)) x6 operand -> natural (nsets, M, K) float32, exactly: 16-byte vector ((set MT + mt) KB + kb) 3 64 + limb 64
    + lane holds, for row mt 32 + (lane & 31), the eight k = kb 16 + (lane >> 5) 8 + e as bf16 pairs (even e in the low half); the
    three limbs of a value add up to it without rounding (csrc/x6_common.h split8, csrc/pack.hip pack_x6_item)."""
    ns, MT, KB = Wp.shape[0], (M + 31) // 32, (K + 15) // 16
    u = Wp.contiguous().view(torch.int32).view(ns, MT, KB, 3, 2, 32, 4)
    v = torch.stack([(u << 16).view(torch.float32), (u & -65536).view(torch.float32)], -1).double().sum(3)     # (ns, MT, KB, kh, row, q, j)
    v = v.permute(0, 1, 4, 2, 3, 5, 6).reshape(ns, MT * 32, KB * 16)
    assert float(v[:, M:].abs().max() if M < MT * 32 else 0) == 0 and float(v[:, :, K:].abs().max() if K < KB * 16 else 0) == 0
    return v[:, :M, :K].float().contiguous()


def gemm_unpack(ops, Wp, M, K):
    """The weight sets as the GEMM sees them: an identity plane through ops.pw_gemm with one weight set per batch element."""
    ns = Wp.shape[0]
    L = max(K, 4)
    x = torch.zeros(ns, K, L, 1, device="cuda")
    x[:, :, :K, 0] = torch.eye(K, device="cuda")
    return ops.pw_gemm(x, Wp, M).reshape(ns, M, L)[:, :, :K].contiguous()


PACK_M, PACK_K, PACK_NS = (1, 31, 32, 33, 40, 160), (1, 3, 7, 8, 9, 15, 16, 17, 23, 40, 160), (1, 3, 8)


def first_block_offsets(M, K, ns):
    """g0 & 3 of every work item of the packing kernel that holds an element: g0 = set M K + row K + k0, k0 = 0, 8, 16, ..."""
    s, row, k0 = np.meshgrid(np.arange(ns), np.arange(M), np.arange(0, K, 8), indexing="ij")
    return set(((s * M * K + row * K + k0) & 3).reshape(-1).tolist())


def test_packed_shapes_reach_all_four_select_branches():
    seen = {}
    for M in PACK_M:
        for K in PACK_K:
            for ns in PACK_NS:
                offs = first_block_offsets(M, K, ns)
                for o in offs:
                    seen[o] = seen.get(o, 0) + 1
                if K % 2 and K > 1 and M >= 4:
                    assert offs == {0, 1, 2, 3}, (M, K, ns)             # an odd K walks g0 & 3 through all four values along the rows
    assert set(seen) == {0, 1, 2, 3} and min(seen.values()) >= 50, seen


def test_bnn_sample_packed_every_shape(ops):
    """bem_bnn_sample_pack_x6 = bem_bnn_sample_f32 (pinned to the model above) followed by the packing kernel, bit for bit; with rho
    and with a precomputed sigma, with and without the device-resident part of the stream id."""
    add = i64(5 << 20)
    for M in PACK_M:
        for K in PACK_K:
            mu, rho = rand_mu_rho((M, K), 1000 * M + K)
            sigma = ops.bnn_sample(torch.zeros_like(mu), rho, 1, torch.ones_like(mu))[0]       # log1p(exp(rho)) by the sampler itself
            for ns in PACK_NS:
                sid = P.stream_id(7, 300 + ns, M * K)
                nat = ops.bnn_sample(mu, rho, ns, None, seed=SEED_B, stream_id=sid)
                ref = ops.pack_pw_weight(nat, x6=True)
                what = f"M={M} K={K} nsets={ns}"
                for sig in (False, True):
                    a = ops.bnn_sample_packed(mu, sigma if sig else rho, ns, M, K, None, seed=SEED_B, stream_id=sid, sigma_given=sig)
                    b = ops.bnn_sample_packed(mu, sigma if sig else rho, ns, M, K, None, seed=SEED_B, stream_id=sid - (5 << 20), sigma_given=sig, stream_add=add)
                    assert bits_equal(a, ref), f"{what} sigma_given={sig}: packed sample != pack(sample)"
                    assert bits_equal(b, ref), f"{what} sigma_given={sig}: stream_add"
                assert bits_equal(unpack_x6(ref, M, K), nat), what
            if (M, K) in ((33, 23), (160, 17), (1, 1)):
                check_w("bnn_sample_packed (decoded)", unpack_x6(a, M, K), mu, rho, ns, SEED_B, sid, what)


# ------------------------------------------------------------------------------------------------ recording the sampling calls
class Recorder:
    """Wraps the sampling entry points of bem.ops and notes every Philox draw: (stream id with the device addend, kind, tensors)."""

    def __init__(self, ops, monkeypatch):
        self.calls = []
        o_s, o_p, o_e, o_b, o_r = ops.bnn_sample, ops.bnn_sample_packed, ops.bnn_ebank_sample, ops.bnn_bank_sample, ops.randn

        def addend(t):
            return 0 if t is None else int(t.cpu()[0])

        def sample(mu, rho, nsets, eps=None, seed=0, stream_id=0, stream_add=None):
            out = o_s(mu, rho, nsets, eps, seed, stream_id, stream_add)
            if eps is None:
                self.calls.append(dict(kind="natural", sid=stream_id + addend(stream_add), seed=seed, mu=mu, rho=rho, ns=nsets, out=out))
            return out

        def packed(mu, rho, nsets, M, K, eps=None, seed=0, stream_id=0, sigma_given=False, stream_add=None):
            out = o_p(mu, rho, nsets, M, K, eps, seed, stream_id, sigma_given, stream_add)
            if eps is None:
                self.calls.append(dict(kind="packed", sid=stream_id + addend(stream_add), seed=seed, mu=mu, sig=rho, sigma_given=sigma_given, ns=nsets, mk=(M, K), out=out))
            return out

        def ebank(bank, seed, stream_base):
            o_e(bank, seed, stream_base)
            self.calls.append(dict(kind="ebank", bank=bank, seed=seed, sids=[stream_base + int(c) for c in bank.segs[:, 5].cpu()]))

        def bbank(bank, decay, decay_dev, seed, stream_base, stream_add):
            o_b(bank, decay, decay_dev, seed, stream_base, stream_add)
            self.calls.append(dict(kind="bbank", bank=bank, seed=seed, decay=decay, sids=[stream_base + addend(stream_add) + int(c) for c in bank.segs[:, 6].cpu()]))

        def randn(shape, device, seed=0, stream_id=0, stream_add=None):
            out = o_r(shape, device, seed, stream_id, stream_add)
            self.calls.append(dict(kind="randn", sid=stream_id + addend(stream_add), seed=seed, out=out))
            return out

        for name, fn in (("bnn_sample", sample), ("bnn_sample_packed", packed), ("bnn_ebank_sample", ebank), ("bnn_bank_sample", bbank), ("randn", randn)):
            monkeypatch.setattr(ops, name, fn)

    def take(self):
        c, self.calls = self.calls, []
        return c

    @staticmethod
    def weight_ids(calls):
        ids = []
        for c in calls:
            if c["kind"] in ("natural", "packed"):
                ids.append(c["sid"])
            elif c["kind"] in ("ebank", "bbank"):
                ids += c["sids"]
        return ids


# ------------------------------------------------------------------------------------------------ bem_bnn_ebank_sample_f32
class EvalLeaves(nn.Module):
    """1x1 weights (x6-packed), a depthwise 3x3 weight (natural order), biases of odd length; with 8 sets the depthwise weight is 594 and
    the 160 x 33 weight 7680 work items, i.e. segments of 3 and 30 workgroups."""

    def __init__(self):
        super().__init__()
        from bem.modules import Conv2dReparameterization as C, Linear2dReparameterization as L
        self.pw = C(23, 33, 1, bias=True)
        self.dw = C(33, 33, 3, padding=1, groups=33, bias=True)
        self.lin = L(33, 160, bias=False)
        self.out = L(160, 7, bias=True)
        self.one = C(1, 1, 1, bias=True)

    def draw(self, B):
        """What the layers' forwards ask their leaves for, in execution order: [(leaf, weights, bias)]."""
        return [(m, *(m.dw_weights(B) if m is self.dw else m.gemm_weights(B))) for m in (self.pw, self.dw, self.lin, self.out, self.one)]


def randomize(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            v = torch.randn(p.shape, generator=g) if "mu_" in name else RHO0 + 4 * torch.rand(p.shape, generator=g) - 2
            p.copy_(v.to(p.device))


def test_eval_bank_equals_the_leaves_and_the_model(ops, monkeypatch):
    from bem.modules import EvalSampleBank, SampleCtx, sampling
    net = EvalLeaves().cuda().eval()
    randomize(net, 5)
    rec = Recorder(ops, monkeypatch)
    ns, seed, rank, epoch = 8, SEED_A, 513, 70001
    ctx = SampleCtx(ns, None, seed=seed, rank=rank, epoch=epoch)
    with sampling(ctx):
        leafwise = net.draw(ns)
    calls = rec.take()
    T = 9
    want = [P.stream_id(rank, epoch, t) for t in range(1, T + 1)]
    assert Recorder.weight_ids(calls) == want
    for c in calls:
        if c["kind"] == "natural":
            check_w("bnn_sample (leaf)", c["out"], c["mu"], c["rho"], ns, seed, c["sid"], "eval leaf")
    bank = EvalSampleBank(net)
    ctx2 = SampleCtx(ns, None, seed=seed, rank=rank, epoch=epoch)
    ctx2.counter0 = ctx2.counter
    assert bank.usable(ctx2)
    bank.sample(ctx2)
    assert ctx2.bank is bank and bank.nrows == T and ctx2.counter == T
    segs = bank.segs.cpu()
    assert int((segs[:, 6] + 255).div(256, rounding_mode="floor").max()) >= 30 and bank.nblk == int((segs[:, 6] + 255).div(256, rounding_mode="floor").sum())
    with sampling(ctx2):
        banked = net.draw(ns)
    calls = rec.take()
    assert [c["kind"] for c in calls] == ["ebank"]
    ids = calls[0]["sids"]
    assert len(set(ids)) == T and sorted(ids) == want
    for (m, w0, b0), (m1, w1, b1) in zip(leafwise, banked):
        assert m is m1 and bits_equal(w0, w1), type(m).__name__
        assert (b0 is None) == (b1 is None) and (b0 is None or bits_equal(b0, b1))
    # natural-order views, and the packed ones decoded, against the model
    t = 0
    for m, w, b in banked:
        t += 1
        if m is net.dw:
            check_w("ebank_sample (natural)", w, m.mu_weight, m.rho_weight, ns, seed, P.stream_id(rank, epoch, t), "depthwise weight")
        else:
            M, K = m._mk
            nat = unpack_x6(w, M, K)
            assert bits_equal(nat, gemm_unpack(ops, w, M, K)), (M, K)
            check_w("ebank_sample (packed, decoded)", nat, m.mu_weight, m.rho_weight, ns, seed, P.stream_id(rank, epoch, t), f"1x1 weight {M}x{K}")
        if b is not None:
            t += 1
            check_w("ebank_sample (natural)", b, m.mu_bias, m.rho_bias, ns, seed, P.stream_id(rank, epoch, t), "bias")
    assert t == T


# ------------------------------------------------------------------------------------------------ bem_bnn_bank_sample_f32
class TrainLeaves(nn.Module):
    """Tensors of 1, 3, 1023, 1024, 1025 and 4100 elements (plus odd biases and a depthwise weight): a workgroup of the bank kernel takes
    1024 consecutive elements of one segment, element bk.first + q 256 + tid."""

    def __init__(self):
        super().__init__()
        from bem.modules import Conv2dReparameterization as C, Linear2dReparameterization as L
        self.a = L(1, 1, bias=True)          # 1, 1
        self.b = L(1, 3, bias=True)          # 3, 3
        self.c = L(31, 33, bias=True)        # 1023, 33
        self.d = L(32, 32, bias=False)       # 1024
        self.e = L(25, 41, bias=True)        # 1025, 41
        self.f = L(100, 41, bias=False)      # 4100
        self.g = C(5, 5, 3, padding=1, groups=5, bias=True)     # 45, 5

    def leaves(self):
        return [self.a, self.b, self.c, self.d, self.e, self.f, self.g]


def train_forward(net, ctx):
    """The sampling part of Network._forward_train (bayes.train_sampling): the bank's one launch when it is ready, otherwise leaf by leaf
    (which records the draw order the bank is then built from)."""
    from bem.bayes import train_sampling
    with train_sampling(net, ctx) as step:
        for m in net.leaves():
            m._sampled(1)
    return step


STEP0, DECAY = 10 ** 6, 0.9998


def ulp_ok(got, ref, ulps=1):
    got, ref = f64(got), np.asarray(ref, dtype=np.float64).reshape(-1)
    return np.abs(got - ref) <= ulps * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("dev_epoch", [False, True])
def test_train_bank_against_the_model(ops, monkeypatch, dev_epoch):
    """One iteration leaf by leaf (which the bank is built from), the next by the bank's one launch; host epoch or device epoch word.

    Prior EMA: pm' = d pm + (1 - d) mu in float64, d the float32 decay the C ABI takes, to 1 ulp of the result.  The kernels evaluate the
    reference's expression operation by operation in float32 -- two products and a sum, each rounded (v_pk_mul_f32 + v_add_f32, no fma):
    |error| <= ulp(d pm) / 2 + ulp((1 - d) mu) / 2 + ulp(result) / 2.  The priors are set to the parameters times U(0.5, 1.5), so the terms
    do not cancel and ulp(d pm) <= ulp(result); the leaves' step counter is set to 10^6, where d = min(decay, (1 + step) / (10 + step)) is
    the leaves' decay 0.9998 -- every iteration after the first 45 000 of a run -- so that 1 - d is exact and the second term is below
    2^-12 of the result: the bound is 1 ulp.  (At d = 0.7, iteration 20, the same three roundings reach 1.25 ulp in a float32 emulation on
    the CPU: 1 ulp is not a property of this expression there.)"""
    from bem.modules import BayesBank, SampleCtx
    monkeypatch.setenv("BEM_BAYES_BANK", "1")
    net = TrainLeaves().cuda().train()
    randomize(net, 11)
    g = torch.Generator().manual_seed(12)
    kinds = [(m, k) for m in net.leaves() for k in (("weight", "bias") if m.bias else ("weight",))]
    for m, k in kinds:
        m.step = STEP0
        for pn in ("mu", "rho"):
            p = getattr(m, f"{pn}_{k}").detach()
            getattr(m, f"prior_{pn}_{k}").copy_(p * (0.5 + torch.rand(p.shape, generator=g).cuda()))
    T = len(kinds)
    assert all(m.decay == DECAY and (1 + STEP0) / (10 + STEP0) > DECAY for m in net.leaves())
    assert {1, 3, 1023, 1024, 1025, 4100} <= {getattr(m, f"mu_{k}").numel() for m, k in kinds}
    rec = Recorder(ops, monkeypatch)
    seed, rank, E1, E2 = SEED_B, 9, 4000, 4001
    word = i64(0)

    def context(epoch):
        if dev_epoch:
            word.fill_(epoch << 20)
            return SampleCtx(1, None, seed=seed, rank=rank, epoch_dev=word)
        return SampleCtx(1, None, seed=seed, rank=rank, epoch=epoch)

    def ema(prior, param, d):
        d = float(np.float32(d))
        return d * f64(prior) + (1.0 - d) * f64(param)

    bank = BayesBank.of(net, create=True)
    # ---- iteration 1, leaf by leaf
    before = {(id(m), k, pn): getattr(m, f"prior_{pn}_{k}").clone() for m, k in kinds for pn in ("mu", "rho")}
    train_forward(net, context(E1))
    calls = rec.take()
    assert [c["kind"] for c in calls] == ["randn"] * T          # (the leaf forms w from that eps through the injected-eps path)
    assert [c["sid"] for c in calls] == [P.stream_id(rank, E1, t) for t in range(1, T + 1)]
    d1 = DECAY
    for m, k in kinds:
        t = m.draws[k]
        e, w = (m.sample.eps_w, m.sample.w) if k == "weight" else (m.sample.eps_b, m.sample.b)
        mu, rho = getattr(m, f"mu_{k}"), getattr(m, f"rho_{k}")
        check_z("randn (training leaf)", e, mu.numel(), seed, P.stream_id(rank, E1, t), f"{type(m).__name__}.{k}")
        check_w("bnn_sample (training leaf)", w, mu, rho, 1, seed, P.stream_id(rank, E1, t), f"{type(m).__name__}.{k}")
        for pn, p in (("mu", mu), ("rho", rho)):
            ok = ulp_ok(getattr(m, f"prior_{pn}_{k}"), ema(before[(id(m), k, pn)], p, d1))
            assert ok.all(), f"prior_{pn}_{k} (leaf): {int((~ok).sum())} of {ok.size} beyond 1 ulp"
    assert bank.ready() and all(m.step == STEP0 + 1 for m in net.leaves())
    # ---- iteration 2, the bank's one launch
    segs = bank.segs.cpu()
    off, n, ctr = segs[:, 4].tolist(), segs[:, 5].tolist(), segs[:, 6].tolist()
    assert sorted(ctr) == list(range(1, T + 1)) and all(o % 4 == 0 for o in off)
    pad = torch.ones(bank.total, dtype=torch.bool)
    for o, k_ in zip(off, n):
        pad[o:o + k_] = False
    assert int(pad.sum()) >= 10                                       # segments of 1, 3, 1023, 1025, 33, 41, 45, 5 elements leave gaps
    pad = pad.cuda()
    SENT = 12345.0
    for arena in (bank.eps, bank.w, bank.pm, bank.pr):
        arena[pad] = SENT
    bank.gw.fill_(SENT)                                               # the sampling launch zeroes the samples' gradients, and only them
    pm0, pr0 = bank.pm.clone(), bank.pr.clone()
    train_forward(net, context(E2))
    calls = rec.take()
    assert [c["kind"] for c in calls] == ["bbank"]
    ids = calls[0]["sids"]
    assert len(set(ids)) == T and sorted(ids) == [P.stream_id(rank, E2, t) for t in range(1, T + 1)]
    d2 = DECAY
    assert calls[0]["decay"] == d2
    for arena in (bank.eps, bank.w, bank.pm, bank.pr, bank.gw):
        assert bool((arena[pad] == SENT).all()), "arena padding written"
    for (m, k), o, k_, c in zip(kinds, off, n, ctr):
        mu, rho = getattr(m, f"mu_{k}"), getattr(m, f"rho_{k}")
        sid = P.stream_id(rank, E2, c)
        what = f"{type(m).__name__}.{k} n={k_}"
        assert k_ == mu.numel() and c == m.draws[k]
        e = bank.eps[o:o + k_]
        check_z("bank_sample eps", e, k_, seed, sid, what)
        assert bits_equal(e, ops.randn((k_,), "cuda", seed, sid)), what
        check_w("bank_sample w", bank.w[o:o + k_], mu, rho, 1, seed, sid, what)
        assert float(bank.gw[o:o + k_].abs().max()) == 0, what
        assert ulp_ok(bank.pm[o:o + k_], ema(pm0[o:o + k_], mu, d2)).all(), what
        assert ulp_ok(bank.pr[o:o + k_], ema(pr0[o:o + k_], rho, d2)).all(), what
        wv, ev = (m.sample.w, m.sample.eps_w) if k == "weight" else (m.sample.b, m.sample.eps_b)
        assert wv.data_ptr() == bank.w.data_ptr() + 4 * o and ev.data_ptr() == bank.eps.data_ptr() + 4 * o
        assert getattr(m, f"prior_mu_{k}").data_ptr() == bank.pm.data_ptr() + 4 * o
    rec.take()


# ------------------------------------------------------------------------------------------------ the shipped Stage-I net
def tensors_of_forward(ops, net, calls):
    """{stream id: (natural-order weight sets (ns, n), mu, rho or None, sigma or None)} of one recorded stochastic forward, whichever form
    drew them.  Packed 1x1 weights are recovered through the GEMM (identity plane) and must equal the decoded operand."""
    by_mu = {}
    for m in net.modules():
        if hasattr(m, "mu_weight"):
            by_mu[m.mu_weight.data_ptr()] = (m.mu_weight, m.rho_weight)
            if m.bias:
                by_mu[m.mu_bias.data_ptr()] = (m.mu_bias, m.rho_bias)
    out = {}

    def put(sid, w, mk, mu_ptr, ns):
        mu, rho = by_mu[mu_ptr]
        if mk is not None:
            nat = gemm_unpack(ops, w, *mk)
            assert bits_equal(nat, unpack_x6(w, *mk)), mk
            w = nat
        assert sid not in out
        out[sid] = (w.reshape(ns, -1), mu, rho)

    for c in calls:
        if c["kind"] == "natural":
            put(c["sid"], c["out"], None, c["mu"].data_ptr(), c["ns"])
        elif c["kind"] == "packed":
            put(c["sid"], c["out"], c["mk"], c["mu"].data_ptr(), c["ns"])
        elif c["kind"] == "ebank":
            bank, segs = c["bank"], c["bank"].segs.cpu()
            for row, sid in zip(segs.tolist(), c["sids"]):
                mu_ptr, o, n_, mk_word, total = row[0], row[2], row[3], row[4], row[7]
                ns = total // n_
                if mk_word:
                    M, K = mk_word & 0xFFFFFFFF, mk_word >> 32
                    pe = ops.packed_elems(M, K, True)
                    put(sid, bank.arena[o:o + ns * pe].view(ns, pe), (M, K), mu_ptr, ns)
                else:
                    put(sid, bank.arena[o:o + total].view(ns, n_), None, mu_ptr, ns)
    return out


def test_gemm_recovery_of_packed_weights_is_exact(ops):
    """Injected eps: an identity plane through ops.pw_gemm with per-sample weight sets returns the natural weights bit for bit."""
    g = torch.Generator().manual_seed(4)
    for M, K, ns in ((40, 23, 3), (160, 640, 8), (640, 160, 2), (33, 1, 1)):
        mu, rho = rand_mu_rho((M, K), M + K)
        eps = torch.randn(ns, M, K, generator=g).cuda()
        nat = ops.bnn_sample(mu, rho, ns, eps)
        Wp = ops.bnn_sample_packed(mu, rho, ns, M, K, eps)
        assert bits_equal(gemm_unpack(ops, Wp, M, K), nat), (M, K, ns)
        assert bits_equal(unpack_x6(Wp, M, K), nat), (M, K, ns)


def test_shipped_stage1_net_draws(ops, monkeypatch):
    """build_nets(): 60 Bayesian leaves / 90 tensors.  One stochastic eval forward with N = 8 under (seed, rank 3, epoch), every weight set
    of every tensor against the model; then rank 4 and the next epoch: new draws everywhere, a 64-element prefix against the model."""
    from bem.modules import SampleCtx, sampling
    from bem.pipeline import build_nets
    from basicsr.bayesian import set_prediction_type
    net1, _ = build_nets(device="cuda")
    set_prediction_type(net1, False)
    rec = Recorder(ops, monkeypatch)
    N, seed, E = 8, 0x5EED00000000ABCD, 123456
    x = torch.rand(N, 3, 16, 16, generator=torch.Generator().manual_seed(1)).cuda()

    def forward(rank, epoch):
        with sampling(SampleCtx(N, None, seed=seed, rank=rank, epoch=epoch)):
            net1(x)
        calls = rec.take()
        ids = Recorder.weight_ids(calls)
        assert len(ids) == 90 and len(set(ids)) == 90
        assert sorted(ids) == [P.stream_id(rank, epoch, t) for t in range(1, 91)]
        assert all(s >> 44 == rank and (s >> 20) & 0xFFFFFF == epoch for s in ids)
        return calls, tensors_of_forward(ops, net1, calls)

    calls, first = forward(3, E)
    assert {c["kind"] for c in calls} == {"natural", "packed"}                     # the first Philox forward goes leaf by leaf
    assert sum(c["kind"] == "packed" for c in calls) >= 30
    for sid, (w, mu, rho) in first.items():
        check_w("Stage-I net, leaf by leaf", w, mu, rho, N, seed, sid, f"stream {sid:#x} n={mu.numel()}")
    n_bayes = sum(p.numel() for name, p in net1.named_parameters() if "mu_" in name)
    assert FIG["Stage-I net, leaf by leaf"]["elements"] == N * n_bayes == 8 * 1243200        # every weight of every set was compared
    first = {sid & 0xFFFFF: (w.clone(), mu) for sid, (w, mu, rho) in first.items()}
    for rank, epoch in ((3, E), (4, E), (3, E + 1)):
        calls, again = forward(rank, epoch)
        assert [c["kind"] for c in calls] == ["ebank"]                             # from the second forward on: one launch
        for sid, (w, mu, rho) in again.items():
            w0, mu0 = first[sid & 0xFFFFF]
            assert mu0 is mu
            if (rank, epoch) == (3, E):
                assert bits_equal(w, w0), hex(sid)                                 # the bank draws what the leaves drew
                continue
            assert not torch.equal(w[:, :64], w0[:, :64]), hex(sid)
            check_w("Stage-I net, one launch", w, mu, rho, N, seed, sid, f"stream {sid:#x}", prefix=64)


# ------------------------------------------------------------------------------------------------ condition noise
def test_condition_noise_stream(ops, monkeypatch):
    """BEMPipeline.candidates draws the condition noise from stream bit 62 | rank << 44 | epoch (the epoch in the low bits), the epoch being
    that of the SampleCtx of the same forward."""
    from bem.modules import SampleCtx
    from bem.pipeline import BEMPipeline, build_nets, synthetic_pair
    net1, net2 = build_nets(device="cuda")
    pipe = BEMPipeline(net1, net2, 16, 0.1)
    lq, gt = synthetic_pair((1, 3, 64, 64), seed=3, device="cuda")
    rec = Recorder(ops, monkeypatch)
    N, seed = 4, 0xC0FFEE0000000011

    def run(rank):
        pipe.candidates(lq, gt, N, True, seed=seed, rank=rank)
        calls = rec.take()
        epoch = SampleCtx._epoch
        wid = Recorder.weight_ids(calls)
        assert len(set(wid)) == 90 and sorted(wid) == [P.stream_id(rank, epoch, t) for t in range(1, 91)]
        noise = [c for c in calls if c["kind"] == "randn"]
        assert len(noise) == 1 and noise[0]["seed"] == seed
        assert noise[0]["sid"] == P.noise_stream_id(rank, epoch) == (1 << 62) | (rank << 44) | epoch
        assert tuple(noise[0]["out"].shape) == (N, 3, 4, 4)
        check_z("condition noise", noise[0]["out"], N * 3 * 4 * 4, seed, noise[0]["sid"], f"rank {rank} epoch {epoch}")
        assert noise[0]["sid"] not in wid
        return noise[0]["sid"], wid, noise[0]["out"].clone()

    monkeypatch.setattr(SampleCtx, "_epoch", 90000)
    a, wa, na = run(5)
    b, wb, nb = run(5)                      # the next forward
    c, wc, nc = run(6)                      # another rank
    assert len({a, b, c}) == 3 and not ({a, b, c} & set(wa + wb + wc))
    assert a == P.noise_stream_id(5, 90001) and b == P.noise_stream_id(5, 90002) and c == P.noise_stream_id(6, 90003)
    assert a != P.noise_stream_id(6, 90001)
    assert not torch.equal(na, nb) and not torch.equal(nb, nc) and not torch.equal(na, nc)
