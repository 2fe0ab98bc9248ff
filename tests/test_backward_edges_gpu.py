"""GPU: the backward kernels of the training step against float64 at the smallest shapes that reach every branch of their host
dispatch -- template instantiations, tile edges, workgroup ranges that cross an image, operand strides.

References and the two error rules live in tests/backward_ref.py (checked on the CPU by tests/test_backward_ref_cpu.py): element-wise
outputs within 2 x the float32 restatement's own error + 1e-6 of the output scale, reduced outputs within n 2^-24 S + 2 x that error.
Because n 2^-24 S is loose for long sums, every reduced output is also run on PROBE inputs: the upstream gradient is zero except on one
tile -- the first, the last (ragged) one, the pair on both sides of an image boundary; for the small kernels one block, one split or the
second pass of the stride loop -- where the same formula is tight and a dropped or doubled tile is a 100 % error.

Harness: accumulators start from a non-zero fill inside guard floats; outputs the wrappers allocate (the ones a call zeroes included) sit
in the middle of canary buffers (large_rows.canaries), so they start from garbage, must be written everywhere and nowhere outside;
inputs are compared with their host copies afterwards.  Each check prints one PARITY line (error, f32 restatement's error, ratios)."""
import contextlib
import math

import numpy as np
import pytest
import torch

import backward_ref as R
from large_rows import canaries

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
GUARD, FILL = -7.25, 0.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs a GPU"
    from bem import native
    native.lib()
    return torch.device("cuda", 0)


def G(seed):
    return torch.Generator().manual_seed(seed)


class Acc:
    """A caller-owned accumulator of ``shape`` holding ``fill``, between four guard floats on either side (16-byte aligned)."""

    def __init__(self, shape, dev, fill=FILL):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 8,), GUARD, device=dev)
        self.t = self.buf[4:4 + self.n].view(*shape)
        self.t.fill_(fill)

    def guards(self):
        got = self.buf.cpu()
        assert bool((got[:4] == GUARD).all()) and bool((got[4 + self.n:] == GUARD).all()), "a store landed next to the accumulator"


class Inputs:
    """Host float32 operands and their device copies; unchanged(): the op wrote into none of them."""

    def __init__(self, dev, **host):
        self.host = host
        for k, v in host.items():
            setattr(self, k, None if v is None else v.to(dev))

    def unchanged(self):
        for k, v in self.host.items():
            assert v is None or torch.equal(getattr(self, k).cpu(), v), f"the op changed its input {k}"


@contextlib.contextmanager
def watched(monkeypatch, returned):
    """large_rows.canaries around one op call, with Tensor.new_empty (the scan wrappers' dxd) routed through it as well."""
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "new_empty", lambda self, shape, **_: torch.empty(*shape, device=self.device, dtype=self.dtype))
        with canaries(monkeypatch, returned):
            yield


def both(fn, *a, **kw):
    return fn(*a, dtype=F64, **kw), fn(*a, dtype=F32, **kw)


def tile_probes(B, L, tile):
    """(name, (B, L) mask) of the probe gradients: the first tile, the last (ragged when L % tile) one, and the last tile of image 0
    together with the first of image 1 -- the pair a workgroup that walks consecutive (image, tile) chunks takes in one range."""
    tiles = -(-L // tile)
    first = torch.zeros(B, L); first[0, :tile] = 1
    last = torch.zeros(B, L); last[B - 1, (tiles - 1) * tile:] = 1
    out = [("first tile", first), ("last tile", last)]
    if B > 1:
        cross = torch.zeros(B, L); cross[0, (tiles - 1) * tile:] = 1; cross[1, :tile] = 1
        out.append(("tiles across the image boundary", cross))
    return out


# ================================================================================================ (a) weight gradients, f32 form
def _pw(dev, dy, x, case):
    from bem import ops
    inp = Inputs(dev, dy=dy, x=x)
    dw, db = Acc((dy.shape[1], x.shape[1]), dev), Acc((dy.shape[1],), dev)
    ops.pw_wgrad_(inp.dy, inp.x, dw.t, dbias=db.t)
    o64, o32 = both(R.pw_wgrad_ref, dy, x, fill=FILL)
    R.check(dw.t, o64["dw"], o32["dw"], "dw", case); R.check(db.t, o64["dbias"], o32["dbias"], "dbias", case)
    dw.guards(); db.guards(); inp.unchanged()


PW_CASES = [((2, 20, 16, 64), "<1,1>: one M-tile group, one N-tile"), ((1, 160, 32, 64), "<2,1>: M = 160 is five 32-row tiles, two per wave"),
            ((1, 288, 24, 32), "<3,1>: nine M-tiles, three per wave"), ((1, 160, 40, 64), "<2,2>: K = 40 is two N-tiles"),
            ((2, 80, 80, 64), "<1,3>: K = 80, the shipped level-1 width, M <= 128"), ((1, 640, 80, 64), "<2,3>: K = 80 under M = 640"),
            ((5, 40, 40, 1700), "<1,2>: 5 x 54 = 270 chunks, 8 per workgroup, the last workgroup has 6, ranges cross images, tile 53 holds 4 pixels")]


@pytest.mark.parametrize("shape", [c[0] for c in PW_CASES], ids=["-".join(map(str, c[0])) for c in PW_CASES])
def test_pw_wgrad_f32_every_instantiation(dev, shape, monkeypatch):
    """bem_pw_wgrad_f32 (forced with WGRAD_X6_MIN_PIXELS): dispatch_wgrad picks wgrad_kernel<MTW,NTW,false,true> from ceil(M/32) and
    ceil(K/32); each case is the smallest (B, M, K, L) that selects the instantiation named in PW_CASES.  Full random dy, then the three
    probes on 32-pixel tiles (the kernel's chunk)."""
    from bem import ops
    monkeypatch.setattr(ops, "WGRAD_X6_MIN_PIXELS", 1 << 62)
    B, M, K, L = shape
    g = G(100 + M + K)
    dy, x = torch.randn(B, M, L, generator=g), torch.randn(B, K, L, generator=g)
    case = f"pw_wgrad {shape}"
    _pw(dev, dy, x, case)
    for name, mask in tile_probes(B, L, 32):
        _pw(dev, dy * mask[:, None], x, f"{case} probe {name}")


def _conv(dev, dy, x, wshape, s, p, case, cin_slice=None, bias=True):
    from bem import ops
    inp = Inputs(dev, dy=dy, x=x)
    dw, db = Acc(wshape, dev), Acc((wshape[0],), dev)
    ops.conv_wgrad_(inp.dy, inp.x, dw.t, db.t if bias else None, stride=s, pad=p, cin_slice=cin_slice)
    xs = x if cin_slice is None else x[:, cin_slice[0]:cin_slice[0] + cin_slice[1]]
    o64, o32 = both(R.conv_wgrad_ref, dy, xs, wshape, s, p, fill=FILL)
    R.check(dw.t, o64["dw"], o32["dw"], "dw", case)
    if bias:
        R.check(db.t, o64["dbias"], o32["dbias"], "dbias", case)
    else:
        assert bool((db.t == FILL).all()), "dbias written although none was passed"
    dw.guards(); db.guards(); inp.unchanged()


CONV_CASES = [((2, 3, 8, 8, 16, 3, 1, 1), "<1,1,true,true>: N = 27, Stage I's 3-channel first conv"),
              ((2, 6, 8, 12, 40, 3, 1, 1), "<1,2,true,true>: N = 54, the 6-channel first conv of every Stage-II net"),
              ((1, 3, 8, 8, 160, 3, 1, 1), "<2,1>"), ((1, 6, 8, 8, 160, 3, 1, 1), "<2,2>"), ((1, 10, 8, 8, 160, 3, 1, 1), "<2,3>: N = 90"),
              ((1, 3, 8, 8, 300, 3, 1, 1), "<3,1>: ten M-tiles"), ((1, 6, 8, 8, 300, 3, 1, 1), "<3,2>"),
              ((2, 16, 10, 14, 32, 4, 2, 1), "<1,2,true,false>: 5 x 7 outputs, L = 35, the ragged dense form at stride 2")]


@pytest.mark.parametrize("shape", [c[0] for c in CONV_CASES], ids=["-".join(map(str, c[0])) for c in CONV_CASES])
def test_conv_wgrad_f32_every_instantiation(dev, shape):
    """bem_conv_wgrad_f32: the gathered (ci, ky, kx) rows make N = Cin k k; the cases select the dense instantiations named in CONV_CASES.
    Probes on 32-output-pixel tiles."""
    B, Cin, H, W, Cout, k, s, p = shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    g = G(200 + Cin + Cout)
    x, dy = torch.randn(B, Cin, H, W, generator=g), torch.randn(B, Cout, Ho, Wo, generator=g)
    case = f"conv_wgrad {shape}"
    _conv(dev, dy, x, (Cout, Cin, k, k), s, p, case)
    for name, mask in tile_probes(B, Ho * Wo, 32):
        _conv(dev, dy * mask.view(B, 1, Ho, Wo), x, (Cout, Cin, k, k), s, p, f"{case} probe {name}")


def test_conv_wgrad_channel_slice_and_no_bias(dev):
    """cin_slice=(2, Cin): x is a channel slice of a wider tensor, so x_bstride is (Cin + 3) H W and the base pointer sits two planes in
    (Stage II's split first conv); then dbias=None, the rowsum pointer the epilogue tests."""
    B, Cin, H, W, Cout = 2, 6, 8, 12, 40
    g = G(250)
    wide, dy = torch.randn(B, Cin + 3, H, W, generator=g), torch.randn(B, Cout, H, W, generator=g)
    _conv(dev, dy, wide, (Cout, Cin, 3, 3), 1, 1, "conv_wgrad cin_slice=(2,6) of 9 channels", cin_slice=(2, Cin))
    for name, mask in tile_probes(B, H * W, 32):
        _conv(dev, dy * mask.view(B, 1, H, W), wide, (Cout, Cin, 3, 3), 1, 1, f"conv_wgrad cin_slice probe {name}", cin_slice=(2, Cin))
    _conv(dev, dy, wide[:, :Cin].contiguous(), (Cout, Cin, 3, 3), 1, 1, "conv_wgrad dbias=None", bias=False)


# ================================================================================================ (b) LayerNorm2d backward / forward
def _ln_x(g, shape):
    """x = m + s z per pixel: z has zero mean and unit variance over the channels, s in [0.5, 2], m ~ N(0.5, 1).  Among tens of thousands
    of pixels of iid numbers some have a channel variance of 1e-4 under a mean of 2; there LayerNorm's gradient is the rounding of the mean
    times 1 / sigma ~ 100, any two float32 evaluations differ by their own size (first run: the kernel 9.0e-3, torch's float32 3.1e-3 on
    dx of scale 270; a numpy replay of the kernel's formulas with an exact 1 / sqrt and another summation order gives 4.8e-3 at that pixel:
    the same order, not the same figure), and rule 1 would compare noise.  With sigma >= 0.5 the yardstick measures rounding, and the bound
    is tighter in absolute terms; test_ln_bwd_iid_inputs_with_near_zero_channel_variance keeps the iid draw."""
    B, C, H, W = shape
    r = torch.randn(shape, generator=g, dtype=F64)
    z = (r - r.mean(1, keepdim=True)) / r.std(1, unbiased=False, keepdim=True) if C > 1 else torch.zeros(shape, dtype=F64)
    s, m = 0.5 + 1.5 * torch.rand(B, 1, H, W, generator=g, dtype=F64), 0.5 + torch.randn(B, 1, H, W, generator=g, dtype=F64)
    return (m + s * z).float()


def _ln(dev, monkeypatch, shape, two, res, want_n, case, tile=None, seed=0, iid=False):
    from bem import ops
    B, C, H, W = shape
    g = G(300 + seed + C)
    x2 = torch.randn(shape, generator=g) if two else None
    x1 = torch.randn(shape, generator=g) * 2 + 0.5 if iid else _ln_x(g, shape) - (x2 if two else 0)
    # iid: the element-wise outputs are judged on the pixels whose channel sigma is at least _ln_x's lower edge, 0.5; all must be finite
    keep = None
    if iid:
        keep = ((x1 + x2 if two else x1).double().std(1, unbiased=False, keepdim=True) >= 0.5).expand(shape)
        assert 0.5 < float(keep.double().mean()) < 1.0, "the case needs pixels on both sides of the threshold"
    pick = (lambda t: t) if keep is None else (lambda t: R.Out(t.value[keep]) if isinstance(t, R.Out) else t.cpu()[keep])
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dn0 = torch.randn(shape, generator=g)
    dres = torch.randn(shape, generator=g) if res else None
    masks = [("", None)] + ([] if tile is None else [(" probe " + n, m) for n, m in tile_probes(B, H * W, tile)])
    for tag, mask in masks:
        dn = dn0 if mask is None else dn0 * mask.view(B, 1, H, W)
        inp = Inputs(dev, x1=x1, x2=x2, dn=dn, gam=gam, bet=bet, dres=dres)
        dg, db = Acc((C,), dev, 1.0), Acc((C,), dev)
        ret = []
        with watched(monkeypatch, ret):
            dx, nn_ = ops.ln_bwd(inp.x1, inp.dn, inp.gam, inp.bet, 1e-5, dg.t, db.t, x2=inp.x2, dres=inp.dres, want_n=want_n)
            ret += [dx] + ([nn_] if want_n else [])
        assert (nn_ is not None) == want_n
        o64, o32 = both(R.ln_ref, x1, x2, gam, bet, 1e-5, dn, dres, fill=0.0)
        assert bool(torch.isfinite(dx).all())
        R.check(pick(dx), pick(o64["dx"]), pick(o32["dx"]), "dx", case + tag)
        if want_n:
            assert bool(torch.isfinite(nn_).all())
            R.check(pick(nn_), pick(o64["n"]), pick(o32["n"]), "n", case + tag)
        for acc, fill, nm in ((dg, 1.0, "dgamma"), (db, FILL, "dbeta")):
            f64, f32 = (R.Out(o[nm].value + fill, o[nm].S + fill, o[nm].n + 1) for o in (o64, o32))
            R.check(acc.t, f64, f32, nm, case + tag)
            acc.guards()
        inp.unchanged()
    fwd = Inputs(dev, x1=x1, x2=x2, gam=gam, bet=bet)
    ret = []
    with watched(monkeypatch, ret):
        ret.append(ops.ln_fwd(fwd.x1, fwd.gam, fwd.bet, 1e-5, x2=fwd.x2))
    n64, n32 = both(R.ln_ref, x1, x2, gam, bet, 1e-5, dn0, None)
    assert bool(torch.isfinite(ret[0]).all())
    R.check(pick(ret[0]), pick(n64["n"]), pick(n32["n"]), "ln_fwd", case)
    fwd.unchanged()


@pytest.mark.parametrize("C", [1, 3, 16, 17, 40, 41, 80, 81, 160])
def test_ln_bwd_width_classes_two_tiles(dev, monkeypatch, C):
    """ln_bwd_split_kernel<CPT,NWV>: C <= 16 -> <4,4>, <= 40 -> <10,4>, <= 80 -> <10,8>, <= 160 -> <20,8>; each class at its upper edge and
    one channel above the class below (dead channel slots in the last wave), and C = 1, 3 (most waves idle).  7 x 10 planes are two
    64-pixel tiles, the second holding 6 pixels.  Probes on 64-pixel tiles."""
    _ln(dev, monkeypatch, (2, C, 7, 10), True, True, True, f"ln C={C} (2,{C},7,10) x2 dres n", tile=64)


@pytest.mark.parametrize("C", [40, 160])
@pytest.mark.parametrize("two,res,want_n", [(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)])
def test_ln_bwd_all_eight_variants(dev, monkeypatch, C, two, res, want_n):
    """The eight <X2, DRES, NOUT> instantiations at the two shipped widths; the two without dres are what every VSSBlock's LN + 1x1
    backward runs."""
    _ln(dev, monkeypatch, (2, C, 7, 10), two, res, want_n, f"ln C={C} x2={int(two)} dres={int(res)} n={int(want_n)}", tile=64, seed=1)


@pytest.mark.parametrize("C", [16, 80])
@pytest.mark.parametrize("two,res", [(False, False), (False, True), (True, False), (True, True)])
def test_ln_bwd_want_n_variants_other_width_classes(dev, monkeypatch, C, two, res):
    """The four variants that write n at the <4,4> and <10,8> width classes (C = 40 and 160 run all eight above)."""
    _ln(dev, monkeypatch, (2, C, 7, 10), two, res, True, f"ln C={C} x2={int(two)} dres={int(res)} n=1", tile=64, seed=2)


def test_ln_bwd_iid_inputs_with_near_zero_channel_variance(dev, monkeypatch):
    """(3, 3, 1, 21893) on iid normal inputs, as the other cases were first drawn: among 65679 pixels of three numbers some have a channel
    sigma of 1e-2 under a mean of 2, where dx and n are the rounding of the mean times 1 / sigma and two float32 evaluations differ by
    their own size (first run: kernel 9.0e-3, torch float32 3.1e-3, dx scale 270).  The kernel still runs every such pixel here.  The claim
    is reduced where it has to be and nowhere else: dx, n and ln_fwd are finite everywhere and hold rule 1 on the pixels with a channel
    sigma >= 0.5; dgamma and dbeta hold rule 2 over all pixels."""
    _ln(dev, monkeypatch, (3, 3, 1, 21893), True, False, True, "ln iid (3,3,1,21893), element-wise on sigma >= 0.5", seed=5, iid=True)


@pytest.mark.parametrize("C", [3, 40])
def test_ln_bwd_two_tiles_per_workgroup_across_images(dev, monkeypatch, C):
    """(3, C, 1, 21893): 343 tiles per image, 1029 in all, above the 1024 workgroups of the grid, so tiles_per_wg = 2.  Workgroup 171 takes
    tile 342 of image 0 (5 pixels) and tile 0 of image 1: the probe across the image boundary is exactly its range."""
    _ln(dev, monkeypatch, (3, C, 1, 21893), True, False, True, f"ln (3,{C},1,21893) tiles_per_wg=2", tile=64, seed=3)


LN_WIDE = [((2, 161, 4, 4), 1, "one workgroup per pixel, 161 channels under 256 threads"),
           ((1, 600, 1, 3), 1, "one workgroup per pixel, three channels per thread in the strided channel loop"),
           ((2, 161, 1, 17), 256, "L = 17 > 16: the pixel-per-thread form, one partial 256-pixel tile per image"),
           ((2, 168, 1, 257), 256, "two 256-pixel tiles per image, the second holding one pixel"),
           ((1, 1100, 1, 40), 256, "2 C = 2200 floats of LDS: the zeroing and flushing loops over C run five times per thread")]


@pytest.mark.parametrize("shape,tile", [c[:2] for c in LN_WIDE], ids=["-".join(map(str, c[0])) for c in LN_WIDE])
def test_ln_bwd_wide(dev, monkeypatch, shape, tile):
    """C > 160: ln_bwd_chan_kernel (L <= 16) and ln_bwd_kernel (256-pixel tiles, dgamma / dbeta through 2 C floats of LDS); LN_WIDE says what
    each shape is for.  Probes on the kernel's own tile (one pixel, or 256)."""
    _ln(dev, monkeypatch, shape, True, True, True, f"ln wide {shape}", tile=tile, seed=4)


# ================================================================================================ (c) depthwise 3x3 + activation backward
def _dwact(dev, monkeypatch, shape, mode, bias, case, misaligned=False, row_probes=False):
    from bem import ops
    B, Cw, H, W = shape
    Cout = Cw // 2 if mode == 2 else Cw
    g = G(400 + H + W + mode)
    t = torch.randn(shape, generator=g)
    w, b = torch.randn(Cw, 1, 3, 3, generator=g) * 0.4, (torch.randn(Cw, generator=g) * 0.3 if bias else None)
    do0 = torch.randn(B, Cout, H, W, generator=g)
    masks = [("", None)]
    if row_probes:
        first, last = torch.zeros(H, W), torch.zeros(H, W)
        first[:2] = 1; last[2 * ((H - 1) // 2):] = 1
        masks += [(" probe first row pair (x-block 0)", first), (" probe last row pair (x-block 1)", last)]
    for tag, mask in masks:
        do = do0 if mask is None else do0 * mask
        inp = Inputs(dev, t=t, w=w, b=b, do=do)
        td = inp.t
        if misaligned:
            big = torch.full((t.numel() + 4,), GUARD, device=dev)
            td = big[1:1 + t.numel()].view(shape)
            td.copy_(inp.t)
            assert td.data_ptr() % 16 == 4 and td.is_contiguous()
        dw, db = Acc((Cw, 1, 3, 3), dev), Acc((Cw,), dev)
        ret = []
        with watched(monkeypatch, ret):
            ret.append(ops.dwact_bwd(td, inp.w, inp.b, inp.do, dw.t, db.t if bias else None, mode))
        o64, o32 = both(R.dwact_ref, t, w, b, do, mode, fill=FILL)
        R.check(ret[0], o64["dpre"], o32["dpre"], "dpre", case + tag)
        R.check(dw.t, o64["dw"], o32["dw"], "dw", case + tag)
        if bias:
            R.check(db.t, o64["dbias"], o32["dbias"], "dbias", case + tag)
        else:
            assert bool((db.t == FILL).all())
        dw.guards(); db.guards(); inp.unchanged()
        if misaligned:
            assert torch.equal(td.cpu(), t) and float(big[0]) == GUARD and bool((big[1 + t.numel():] == GUARD).all())


DW_SHAPES = [((1, 2, 34, 64), "17 x 16 = 272 threads: two x-blocks, vector form (W % 4 == 0, aligned)"),
             ((1, 2, 33, 61), "17 x 16 = 272 threads: two x-blocks, scalar form, ragged last row pair and last column group"),
             ((2, 4, 1, 1), "one pixel: every neighbour of the window is outside"), ((1, 4, 3, 2), "3 x 2: half a row pair, half a column group")]


@pytest.mark.parametrize("mode,bias", [(m, b) for m in (0, 1, 2) for b in (False, True)])
@pytest.mark.parametrize("shape", [c[0] for c in DW_SHAPES], ids=["-".join(map(str, c[0])) for c in DW_SHAPES])
def test_dwact_bwd_blocks_and_forms(dev, monkeypatch, shape, mode, bias):
    """dwact_bwd_kernel<MODE,VEC>: grid.x = ceil(ceil(H/2) ceil(W/4) / 256) is 2 at 34 x 64 and 33 x 61 (thread 256.. own the last row
    pair); the probes light the first and the last row pair only."""
    _dwact(dev, monkeypatch, shape, mode, bias, f"dwact {shape} mode {mode} bias {int(bias)}", row_probes=shape[2] > 30)


@pytest.mark.parametrize("mode,bias", [(m, b) for m in (0, 1, 2) for b in (False, True)])
def test_dwact_bwd_unaligned_t_takes_the_scalar_form(dev, monkeypatch, mode, bias):
    """(2, 6, 5, 8) with t one float into a larger buffer: W % 4 == 0 but the pointer is not 16-byte aligned, so the host picks
    <MODE,false> -- the scalar loads on a plane whose width would allow the vector ones."""
    _dwact(dev, monkeypatch, (2, 6, 5, 8), mode, bias, f"dwact (2,6,5,8) unaligned t mode {mode} bias {int(bias)}", misaligned=True)


# ================================================================================================ (e) N-state fused scan backward
def _scan_operands(B, C, L, Rk, N, seed):
    g = G(seed)
    x0, x1 = torch.randn(B, C, L, generator=g), torch.randn(B, C, L, generator=g)
    xd0, xd1 = torch.randn(B, 2, Rk + 2 * N, L, generator=g) * 0.7, torch.randn(B, 2, Rk + 2 * N, L, generator=g) * 0.7
    dtw = 0.2 * torch.randn(4, C, Rk, generator=g)
    dt = 0.05 + 0.95 * torch.rand(4, C, generator=g)
    dtb = dt + torch.log(-torch.expm1(-dt))
    A = -torch.exp(torch.log(torch.arange(1, N + 1, dtype=F32)).repeat(4 * C, 1) + 0.1 * torch.randn(4 * C, N, generator=g))
    Ds = 0.1 * torch.randn(4 * C, generator=g)
    return x0, x1, xd0, xd1, dtw, dtb, A, Ds, torch.randn(B, C, L, generator=g), torch.randn(B, C, L, generator=g)


def _strided(xd, dev):
    """xd (B,2,rows,L) as the [:, :2] view of a (B,4,rows,L) buffer (bem/autograd.py hands x_dbl over like this): twice the batch stride."""
    B, _, rows, L = xd.shape
    wide = torch.full((B, 4, rows, L), GUARD, device=dev)
    v = wide[:, :2]
    v.copy_(xd.to(dev))
    assert not v.is_contiguous() or B == 1
    return wide, v


def _scan_n(dev, monkeypatch, B, C, L, Rk, N, case, strided=False, probes=("first", "middle", "last")):
    from bem import ops
    x0, x1, xd0, xd1, dtw, dtb, A, Ds, dy0f, dy1f = _scan_operands(B, C, L, Rk, N, 500 + L + N)
    masks, seen, tiles = [("", None)], [], -(-L // 256)
    for key, nm, tl in (("first", "first tile", 0), ("middle", "a middle tile (state and adjoint carry both enter)", tiles // 2),
                        ("last", "last tile", tiles - 1)):
        if key in probes and tl not in seen:
            seen.append(tl)
            m = torch.zeros(L); m[tl * 256:(tl + 1) * 256] = 1
            masks.append((" probe " + nm, m))
    for tag, mask in masks:
        dy0, dy1 = (dy0f, dy1f) if mask is None else (dy0f * mask, dy1f * mask)
        inp = Inputs(dev, x0=x0, x1=x1, xd0=xd0, xd1=xd1, dtw=dtw, dtb=dtb, A=A, Ds=Ds, dy0=dy0, dy1=dy1)
        a0, a1 = inp.xd0, inp.xd1
        if strided:
            (w0, a0), (w1, a1) = _strided(xd0, dev), _strided(xd1, dev)
        dA, dD, dW, db = Acc((4 * C, N), dev), Acc((4 * C,), dev), Acc((4, C, Rk), dev), Acc((4, C), dev)
        ret = []
        with watched(monkeypatch, ret):
            outs = ops.ss2d_scan_n_bwd(inp.x0, inp.x1, a0, a1, inp.dy0, inp.dy1, inp.dtw, inp.dtb, inp.A, inp.Ds, dA.t, dD.t, dW.t, db.t)
            ret += list(outs)
        o64, o32 = both(R.ss2d_bwd_ref, x0, x1, xd0, xd1, dtw, dtb, A, Ds, dy0, dy1, fill=FILL)
        for got, nm in zip(outs + (dA.t, dD.t, dW.t, db.t), ("dx0", "dx1", "dxd0", "dxd1", "dA_logs", "dDs", "ddtw", "ddtb")):
            R.check(got, o64[nm], o32[nm], nm, case + tag)
        for acc in (dA, dD, dW, db):
            acc.guards()
        inp.unchanged()
        if strided:
            for wide, src in ((w0, xd0), (w1, xd1)):
                assert torch.equal(wide[:, :2].cpu(), src) and bool((wide[:, 2:] == GUARD).all()), "the strided x_dbl buffer was written"


@pytest.mark.parametrize("B,C,L,Rk,N", [(2, 12, 600, 3, 4), (1, 9, 1023, 2, 3), (1, 8, 1024, 16, 16)])
def test_ss2d_scan_n_bwd_three_and_more_tiles(dev, monkeypatch, B, C, L, Rk, N):
    """bem_ss2d_scan_n_bwd_f32 beyond two 256-position tiles (tests/test_dstate_gpu.py stops at L = 391).  L = 600: three tiles, the middle
    one has an entering state AND an entering adjoint carry (this case also runs the tile probes).  L = 1023: L % 4 == 3, four tiles, the
    last one position short, C = 9 a partial channel group.  (1, 8, 1024, 16, 16): the largest d_state and dt_rank on four full tiles.
    Probe gradients on the first, a middle and the last tile; the N = 16 case, whose references take two seconds a run, keeps to the last."""
    _scan_n(dev, monkeypatch, B, C, L, Rk, N, f"ss2d_scan_n_bwd ({B},{C},{L},{Rk},{N})", probes=("last",) if N == 16 else ("first", "middle", "last"))


def test_ss2d_scan_n_bwd_strided_x_dbl(dev, monkeypatch):
    """xd0 / xd1 as [:, :2] views of (B,4,R+2N,L) buffers, B = 2: the batch stride the training path passes; L = 300 is two tiles, each probed."""
    _scan_n(dev, monkeypatch, 2, 5, 300, 2, 4, "ss2d_scan_n_bwd strided xd (2,5,300,2,4)", strided=True, probes=("first", "last"))


# ================================================================================================ (f) the operator seam
def _seam(dev, monkeypatch, Bt, KC, L, N, K, case, with_D, with_bias, softplus, big_bias=False, probes=False):
    from bem import ops
    g = G(600 + L + N)
    u = torch.randn(Bt, KC, L, generator=g)
    delta = torch.randn(Bt, KC, L, generator=g) * 0.5 if softplus else 0.05 + 0.5 * torch.rand(Bt, KC, L, generator=g)
    A = -torch.exp(torch.log(torch.arange(1, N + 1, dtype=F32)).repeat(KC, 1) + 0.1 * torch.randn(KC, N, generator=g))
    Bm, Cm = torch.randn(Bt, K, N, L, generator=g), torch.randn(Bt, K, N, L, generator=g)
    Dv = torch.randn(KC, generator=g) if with_D else None
    # softplus off: z = delta + bias is the step size itself and has to stay positive (a negative one makes the recurrence grow)
    bias = ((torch.randn(KC, generator=g) * 0.5 - 1.0) if softplus else 0.3 * torch.rand(KC, generator=g)) if with_bias else None
    if big_bias:
        bias[1] = 25.0                                     # z = delta + 25 > 20: softplus(z) = z, its derivative 1
    do0 = torch.randn(Bt, KC, L, generator=g)
    masks = [("", None)]
    if probes:
        chunks = -(-L // 1024)
        seen = []
        for nm, c in (("first chunk", 0), ("middle chunk", chunks // 2), ("last chunk", chunks - 1)):
            if c not in seen:
                seen.append(c)
                m = torch.zeros(L); m[c * 1024:(c + 1) * 1024] = 1
                masks.append((" probe " + nm, m))
    for tag, mask in masks:
        dout = do0 if mask is None else do0 * mask
        inp = Inputs(dev, u=u, delta=delta, A=A, Bm=Bm, Cm=Cm, Dv=Dv, bias=bias, dout=dout)
        ret = []
        with watched(monkeypatch, ret):
            outs = ops.selective_scan_bwd(inp.u, inp.delta, inp.A, inp.Bm, inp.Cm, inp.Dv, inp.bias, inp.dout, softplus)
            ret += [o for o in outs if o is not None]
        assert (outs[5] is None) == (not with_D) and (outs[6] is None) == (not with_bias)
        o64, o32 = both(R.selective_scan_bwd_ref, u, delta, A, Bm, Cm, Dv, bias, dout, softplus)
        for got, nm in zip(outs, ("du", "ddelta", "dA", "dB", "dC", "dD", "ddelta_bias")):
            if got is not None:
                R.check(got, o64[nm], o32[nm], nm, case + tag)
        inp.unchanged()


def test_seam_bwd_three_chunks_three_states_d_only(dev, monkeypatch):
    """(2, 6, 2051, 3, 2): d_state 3 over three 1024-position chunks (the last holds 3 positions), two groups of three channels, D
    without delta_bias; probe gradients on the first, middle and last chunk."""
    _seam(dev, monkeypatch, 2, 6, 2051, 3, 2, "seam (2,6,2051,3,2) D only", True, False, True, probes=True)


def test_seam_bwd_bias_only_and_z_above_20(dev, monkeypatch):
    """(1, 4, 3072, 2, 1): three full chunks, delta_bias without D, channel 1 with bias 25 so that z > 20 takes softplus' linear branch;
    probe gradients per chunk."""
    _seam(dev, monkeypatch, 1, 4, 3072, 2, 1, "seam (1,4,3072,2,1) bias only, z > 20", False, True, True, big_bias=True, probes=True)


def test_seam_bwd_softplus_off_sixteen_states(dev, monkeypatch):
    """(1, 4, 1025, 16, 4): d_state 16 over two chunks (the second one position long), one channel per group, neither D nor bias,
    delta_softplus = 0 (delta is the step size itself); probe gradients on the full chunk and on the one-position chunk."""
    _seam(dev, monkeypatch, 1, 4, 1025, 16, 4, "seam (1,4,1025,16,4) no D, no bias, softplus off", False, False, False, probes=True)


@pytest.mark.parametrize("softplus", [True, False])
def test_seam_bwd_seven_positions(dev, monkeypatch, softplus):
    """(2, 4, 7, 2, 2): L = 7, less than one thread's four positions in most lanes; D and delta_bias both given."""
    _seam(dev, monkeypatch, 2, 4, 7, 2, 2, f"seam (2,4,7,2,2) D + bias softplus {int(softplus)}", True, True, softplus)


# ================================================================================================ (g) small kernels
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (1, 16, 24)])
def test_hamilton_bwd(dev, monkeypatch, B, H, W):
    """bem_hamilton_bwd_f32 on its own (so far only reached through HamiltonFn), against autograd of oracle.hamilton_ref(p, q)[:, 1:]:
    70 pixels is one partial 256-thread block with b = i / HW crossing images inside it, 384 pixels is two blocks."""
    from bem import ops
    from oracle import bem_oracle as O
    g = G(700 + H)
    inp = Inputs(dev, q8=torch.randn(B, 8, H, W, generator=g), do=torch.randn(B, 3, H, W, generator=g))
    ret = []
    with watched(monkeypatch, ret):
        ret.append(ops.hamilton_bwd(inp.q8, inp.do))
    o64, o32 = both(R.hamilton_bwd_ref, inp.host["q8"], inp.host["do"], product=lambda p, q: O.hamilton_ref(p, q)[:, 1:])
    R.check(ret[0], o64["dq8"], o32["dq8"], "dq8", f"hamilton_bwd ({B},{H},{W})")
    inp.unchanged()


@pytest.mark.parametrize("gmul", [None, 2.5])
def test_l1_loss_grid_stride(dev, monkeypatch, gmul):
    """n = 2048 x 256 + 3: the grid is capped at 2048 workgroups, so three threads take a second element in the stride loop.  The loss
    is a reduced output whose n backward_ref.l1_ref states (the kernel sums in float64)."""
    from bem import ops
    n = 2048 * 256 + 3
    g = G(710)
    p, t = torch.rand(n, generator=g), torch.rand(n, generator=g)
    p[5], p[n - 1] = t[5], t[n - 1] + 0.5                         # sign(0) = 0; the last element is one of the three
    inp = Inputs(dev, p=p, t=t)
    ret = []
    with watched(monkeypatch, ret):
        loss = ops.l1_loss(inp.p, inp.t, 0.7)
        ret.append(loss)
    ret2 = []
    with watched(monkeypatch, ret2):
        dp = ops.l1_loss_bwd(inp.p, inp.t, 0.7, None if gmul is None else torch.tensor([gmul], device=dev))
        ret2.append(dp)
    o64, o32 = both(R.l1_ref, p, t, 0.7, gmul)
    R.check(loss, o64["loss"], o32["loss"], "loss", f"l1 n={n} gmul={gmul}")
    R.check(dp, o64["dpred"], o32["dpred"], "dpred", f"l1 n={n} gmul={gmul}")
    inp.unchanged()


def span_probes(n, passes, tail_from):
    """(name, flat 0/1 mask over n elements) for a kernel whose threads walk n elements in passes of ``passes`` (grid size x block size):
    the first block of 256, the whole second pass (or what there is of it), and the last, partial pass from ``tail_from`` on."""
    out = []
    for nm, lo, hi in (("first block", 0, 256), ("second pass of the stride loop", passes, 2 * passes), ("last pass", tail_from, n)):
        if lo < n and (lo, min(hi, n)) not in [(a, b) for _, a, b in out]:
            out.append((nm, lo, min(hi, n)))
    masks = []
    for nm, lo, hi in out:
        m = torch.zeros(n); m[lo:hi] = 1
        masks.append((" probe " + nm, m))
    return masks


@pytest.mark.parametrize("shape", [(2, 3000, 1, 5), (2, 5, 1, 35000)], ids=["2-3000-1-5", "2-5-1-35000"])
def test_channel_sum_splits(dev, shape):
    """(2, 3000, 1, 5): 3000 channels in grid.y, one split, ten elements under 256 threads; probes: the first and the last element.
    (2, 5, 1, 35000): 70000 (image, pixel) positions over 18 splits of 256 threads, passes of 4608 -- the stride loop, with b = i / L
    changing inside it.  Probes, x zero elsewhere: split 0's first pass, split 17's first pass (one split alone), the whole second pass
    (positions 4608..9215), the sixteenth, partial pass (69120..69999, in image 1)."""
    from bem import ops
    B, C, _, L = shape
    x0 = torch.randn(shape, generator=G(720))
    n = B * L
    if L == 5:
        spans = [("first element", 0, 1), ("last element", n - 1, n)]
    else:
        spans = [("split 0, first pass", 0, 256), ("split 17, first pass", 17 * 256, 18 * 256), ("second pass", 4608, 9216), ("last pass", 69120, n)]
    masks = [("", None)]
    for nm, lo, hi in spans:
        m = torch.zeros(n); m[lo:hi] = 1
        masks.append((" probe " + nm, m.view(B, 1, 1, L)))
    for tag, mask in masks:
        x = x0 if mask is None else x0 * mask
        inp = Inputs(dev, x=x)
        acc = Acc((C,), dev)
        ops.channel_sum_(inp.x, acc.t)
        o64, o32 = both(R.channel_sum_ref, x, fill=FILL)
        R.check(acc.t, o64["sum"], o32["sum"], "sum", f"channel_sum {shape}" + tag)
        acc.guards(); inp.unchanged()


def test_prelu_bwd_and_kl_grid_stride(dev, monkeypatch):
    """n = 65536 + 37: prelu_bwd, bnn_kl_ run at most 256 workgroups of 256 threads, so 37 threads loop once more; bnn_kl_bwd_ is one thread
    per element with a partial last block.  dslope, the KL value, dmu and drho are accumulated onto a fill.  Probes: dout (prelu) is zero,
    posterior = prior (KL: a term of exactly 0) except on the first block, and except on the 37 elements of the second pass."""
    from bem import ops
    n = 65536 + 37
    g = G(730)
    x, dy0, a = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.tensor([0.25])
    x[n - 37:n - 20] = -x[n - 37:n - 20].abs() - 0.1             # the second pass holds terms of dslope for certain
    probes = span_probes(n, 65536, 65536)
    assert [m.sum().item() for _, m in probes] == [256, 37]
    for tag, mask in [("", None)] + probes:
        dy = dy0 if mask is None else dy0 * mask
        inp = Inputs(dev, x=x, dy=dy, a=a)
        da = Acc((1,), dev)
        ret = []
        with watched(monkeypatch, ret):
            ret.append(ops.prelu_bwd(inp.x, inp.a, inp.dy, da.t))
        o64, o32 = both(R.prelu_bwd_ref, x, a, dy, fill=FILL)
        R.check(ret[0], o64["dx"], o32["dx"], "dx", f"prelu_bwd n={n}" + tag); R.check(da.t, o64["dslope"], o32["dslope"], "dslope", f"prelu_bwd n={n}" + tag)
        da.guards(); inp.unchanged()
    mu, rho = torch.randn(n, generator=g), torch.randn(n, generator=g) - 3
    pmu0, prho0 = mu + 0.1 * torch.randn(n, generator=g), rho + 0.2 * torch.randn(n, generator=g)
    for tag, mask in [("", None)] + probes:
        pmu, prho = (pmu0, prho0) if mask is None else (torch.where(mask > 0, pmu0, mu), torch.where(mask > 0, prho0, rho))
        inp = Inputs(dev, mu=mu, rho=rho, pmu=pmu, prho=prho)
        kl, dmu, drho = Acc((1,), dev), Acc((n,), dev), Acc((n,), dev)
        ops.bnn_kl_(inp.mu, inp.rho, inp.pmu, inp.prho, kl.t)
        ops.bnn_kl_bwd_(inp.mu, inp.rho, inp.pmu, inp.prho, torch.tensor([0.37], device=dev), dmu.t, drho.t)
        o64, o32 = both(R.kl_ref, mu, rho, pmu, prho, 0.37, fill=FILL)
        assert mask is None or o64["kl"].n == int(mask.sum()) + 1
        for acc, nm in ((kl, "kl"), (dmu, "dmu"), (drho, "drho")):
            R.check(acc.t, o64[nm], o32[nm], nm, f"bnn_kl n={n}" + tag)
            acc.guards()
        inp.unchanged()


def test_mask_token_bwd_grid_stride(dev, monkeypatch):
    """B L = 13 x 1261 = 16384 + 9: grid.x is capped at 64 workgroups of 256 threads, nine threads take a second (image, pixel).  Probes:
    dout zero except on the first block of positions, and except on the nine positions of the second pass."""
    from bem import ops
    B, C, H, W = 13, 3, 13, 97
    g = G(740)
    dout0, mask = torch.randn(B, C, H, W, generator=g), (torch.rand(B, H, W, generator=g) < 0.5).float()
    mask[B - 1, H - 1, W - 9:] = 1                               # the nine positions of the second pass all carry a term
    probes = span_probes(B * H * W, 16384, 16384)
    assert [m.sum().item() for _, m in probes] == [256, 9]
    for tag, pm in [("", None)] + probes:
        dout = dout0 if pm is None else dout0 * pm.view(B, 1, H, W)
        inp = Inputs(dev, dout=dout, mask=mask)
        dt = Acc((C,), dev)
        ret = []
        with watched(monkeypatch, ret):
            ret.append(ops.mask_token_bwd(inp.dout, inp.mask, dt.t))
        o64, o32 = both(R.mask_token_bwd_ref, dout, mask, fill=FILL)
        R.check(ret[0], o64["dfea"], o32["dfea"], "dfea", "mask_token_bwd BL=16393" + tag)
        R.check(dt.t, o64["dtoken"], o32["dtoken"], "dtoken", "mask_token_bwd BL=16393" + tag)
        dt.guards(); inp.unchanged()


def test_grad_sumsq_stride_and_tail(dev):
    """n = 2^20 + 3: ceil(n / 1024) = 1025 workgroups are capped at 1024, whose 262144 threads take the 262144 float4s; the n & 3 = 3 tail
    floats go to the first threads of workgroup 0.  The kernel squares and sums in float64 (the squares are exact there), so the bound is
    rule 2 with the float64 unit: n 2^-53 S, S the sum itself."""
    from bem import ops
    n = (1 << 20) + 3
    gcpu = torch.randn(n, generator=G(750)) * 3
    gcpu[n - 3:] = torch.tensor([100.0, -200.0, 300.0])          # a dropped tail element is 1 % of the sum
    inp = Inputs(dev, g=gcpu)
    acc = torch.full((3,), -7.0, device=dev, dtype=F64)
    ops.grad_sumsq(inp.g, acc[1:2])
    ref = float(R.sumsq_ref(gcpu, F64))
    got = acc.cpu()
    assert float(got[0]) == -7.0 and float(got[2]) == -7.0
    err = abs(float(got[1]) - ref)
    print(f"PARITY grad_sumsq n={n} | sumsq | rule 2 (f64) | err {err:.3e} | bound {n * 2.0 ** -53 * ref:.3e}")
    assert err <= n * 2.0 ** -53 * ref, (err, ref)
    inp.unchanged()


def _adam_buffers(dev, n, seed):
    g = G(seed)
    host = dict(p=torch.randn(n, generator=g), g=torch.randn(n, generator=g) * 3, m=torch.randn(n, generator=g) * 0.1, v=torch.rand(n, generator=g) * 0.01)
    accs = {k: Acc((n,), dev) for k in host}
    for k, a in accs.items():
        a.t.copy_(host[k].to(dev))
    return host, accs


def test_adamw_step_direct(dev):
    """bem_adamw_step_f32 called directly at n = 1000 (three full blocks and a partial one): the update against a float64 evaluation of the
    documented formula with and without the clip; max_norm = 0 leaves g bit-identical; the device-resident ``hyper`` triple gives the
    same bits as the host values; norm_out is the float32 rounding of sqrt(sumsq)."""
    from bem import ops
    # the C ABI takes lr, the betas, eps and the weight decay as float: the formula is evaluated at exactly those values (1 - 0.999f is
    # 1.3e-5 away from 0.001, which v would show)
    n, step = 1000, 3
    lr, b1, b2, eps, wd = (float(np.float32(h)) for h in (2e-3, 0.9, 0.999, 1e-8, 1e-2))
    betas = (b1, b2)
    # (1) no clipping
    host, acc = _adam_buffers(dev, n, 760)
    ops.adamw_step_(acc["p"].t, acc["g"].t, acc["m"].t, acc["v"].t, lr, betas, eps, wd, step, max_norm=0.0)
    assert torch.equal(acc["g"].t.cpu().view(torch.int32), host["g"].view(torch.int32)), "max_norm = 0 changed the gradient"
    o64, o32 = both(R.adamw_ref, host["p"], host["g"], host["m"], host["v"], lr, betas, eps, wd, step, 1.0)
    for k in ("p", "m", "v"):
        R.check(acc[k].t, o64[k], o32[k], k, "adamw n=1000 no clip")
    for a in acc.values():
        a.guards()
    plain = {k: a.t.clone() for k, a in acc.items()}
    # (2) the same step with lr and the bias corrections read from device memory
    host2, acc2 = _adam_buffers(dev, n, 760)
    hyper = torch.tensor([np.float32(lr), np.float32(1.0 - b1 ** step), np.float32(math.sqrt(1.0 - b2 ** step))], dtype=F32, device=dev)
    ops.adamw_step_(acc2["p"].t, acc2["g"].t, acc2["m"].t, acc2["v"].t, 123.0, betas, eps, wd, 0, max_norm=0.0, hyper=hyper)
    for k in plain:
        assert torch.equal(acc2[k].t.view(torch.int32), plain[k].view(torch.int32)), f"hyper: {k} differs from the host-value call"
    # (3) clipping at max_norm = 1 with the norm written out
    host3, acc3 = _adam_buffers(dev, n, 761)
    ss = torch.zeros(1, device=dev, dtype=F64)
    ops.grad_sumsq(acc3["g"].t, ss)
    norm = Acc((1,), dev)
    ops.adamw_step_(acc3["p"].t, acc3["g"].t, acc3["m"].t, acc3["v"].t, lr, betas, eps, wd, step, max_norm=1.0, sumsq=ss, norm_out=norm.t)
    tn = float(host3["g"].double().pow(2).sum().sqrt())
    assert tn > 1.0 and abs(float(norm.t) - tn) <= 2.0 ** -23 * tn, (float(norm.t), tn)       # one float32 rounding of a float64 value
    coef = min(1.0, 1.0 / (tn + 1e-6))
    o64, o32 = both(R.adamw_ref, host3["p"], host3["g"], host3["m"], host3["v"], lr, betas, eps, wd, step, coef)
    for k in ("g", "p", "m", "v"):
        R.check(acc3[k].t, o64[k], o32[k], k, "adamw n=1000 clip 1.0")
    norm.guards()
    for a in acc3.values():
        a.guards()
