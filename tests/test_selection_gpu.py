"""The eval step's entry and exit kernels of csrc/layout.hip and csrc/selection.hip (pad_reflect, resize_down, bilinear_up, plane_mean, cond_postproc; the
three candidate_finalize grids, select_best / select_scores with both gathers, ssim, mc_mean + mc_rescale) at op level against the float64
references of tests/selection_ref.py, on the shape tables there: the smallest shapes at which each chunked, capped or strided loop makes a
second, ragged pass, and N = 64.

Bounds.
  * copies, clamps, crops, indices, gathers: bit-equal.
  * per-pixel float outputs (ratio-scaled finals, cond_postproc with a target mean, resize_down, bilinear_up, mc_mean): mean and max |err|
    against float64 <= 2x those of the float32 CPU evaluation of the same reference, floor one float32 ulp of the output's magnitude.
  * reductions returned as float32 (plane_mean, PSNR, SSIM): the kernels accumulate in float64 and round once, so they are held to the
    float64 reference within one float32 ulp of its value.  The PSNR under gt_mean also carries the rounding of the final image to float32
    pixels and of its ratio to a float32 number: that term is measured as the error of the oracle's float32 numpy path on the same case
    (R.psnr_f32_term) and admitted R.MARGIN = 4 times, because the float64 atomics of several workgroups and the ratio are order-dependent.
  * selection: the float64 reference's index; tests/test_selection_cpu.py shows for every case that its lead is R.GAP = 100 x what those
    bounds admit, or a bit-equal tie written in on purpose.
Every measured ratio is printed on a PARITY line.  No run on an MI355X has been recorded yet: the ratios are unmeasured."""
import ctypes

import numpy as np
import pytest
import torch

import selection_cases as C
import selection_ref as R

pytestmark = pytest.mark.gpu

ULP = R.ULP


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bem import native
    native.lib()


def dev(t):
    return t.cuda().contiguous()


def _err(a, r64):
    e = (a.detach().cpu().double() - r64).abs()
    return float(e.mean()), float(e.max())


def per_pixel(got, r32, r64, what):
    """got no further from float64 than 2x the f32 reference, mean and max; floor one f32 ulp of the output's magnitude."""
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite"
    (rm, rM), (hm, hM) = _err(r32, r64), _err(got, r64)
    fm, fM = ULP * float(r64.abs().mean()), ULP * float(r64.abs().max())
    print(f"PARITY pixel {what}: f32 ref mean {rm:.3e} max {rM:.3e} | HIP mean {hm:.3e} max {hM:.3e} | ratio {hm / max(rm, fm, 1e-300):.2f} {hM / max(rM, fM, 1e-300):.2f}")
    assert hm <= max(2 * rm, fm) and hM <= max(2 * rM, fM), (what, hm, rm, hM, rM, fm, fM)


def rounded_once(got, r64, what, extra=0.0):
    """A float32 figure that was accumulated in float64: within one float32 ulp of the float64 reference (+ extra, where a term is stated)."""
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite"
    err = (got.detach().cpu().double() - r64).abs()
    bound = R.ulp32(r64) + extra
    i = int(torch.argmax(err / bound))
    print(f"PARITY once {what}: worst |err| {float(err.flatten()[i]):.3e} at bound {float(bound.flatten()[i]):.3e} (ulp {float(R.ulp32(r64).flatten()[i]):.3e}, "
          f"f32 term x{R.MARGIN:g} {extra:.3e}) | ratio {float((err / bound).max()):.2f}")
    assert bool((err <= bound).all()), (what, float(err.flatten()[i]), float(bound.flatten()[i]))


def bit_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got.detach().cpu(), want), f"{what}: not bit-equal ({int((got.detach().cpu() != want).sum())} elements differ)"


def both(fn, *args, **kw):
    """fn on the float32 values and on their float64 copies."""
    cast = lambda t, d: t.to(d) if torch.is_tensor(t) and t.is_floating_point() else t
    return tuple(fn(*[cast(a, d) for a in args], **{k: cast(v, d) for k, v in kw.items()}) for d in (torch.float32, torch.float64))


def offset_by_one_float(t):
    """The same values in device memory that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device="cuda", dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ------------------------------------------------------------------------------------------------------------------ candidate_finalize
@pytest.mark.parametrize("name", list(R.FINALIZE))
def test_candidate_finalize(name):
    from bem import ops
    h, w, Hp, Wp, B, N = R.FINALIZE[name]
    tag = f"{name} {R.FINALIZE[name]}"
    # ---- gt_mean on.  A channel whose clamped sum is 0 stays 0 (zero_sum='zero'); numpy would make it NaN.
    pred, target = R.finalize_inputs(name)
    (f32, _, _), (f64, _, p64) = both(R.candidate_finalize, pred, target, N, h, w, True, zero_sum="zero")
    chain = h * w > 1
    if chain:
        extra = R.MARGIN * R.psnr_f32_term(pred, target, N, h, w, True)
    else:
        # One pixel per channel: clamp(q (t / q)) is t to the last bit or not, so the PSNR is 100, or 150 dB, or 300 dB by rounding alone
        # and the chain's figure bounds nothing.  The zero-sum edge is in this case: the reference is NaN there.
        assert bool(torch.isnan(R.candidate_finalize(pred.double(), target.double(), N, h, w, True)[0]).any())
    pred_d, target_d = dev(pred), dev(target)
    t64 = target.double().repeat_interleave(N, 0)
    for call in (1, 2):                                                                # the second call gets a used workspace back
        fin, ps = ops.candidate_finalize(pred_d, target_d, N, h, w, True)
        per_pixel(fin, f32, f64, f"finalize gt_mean final, call {call} {tag}")
        if chain:
            rounded_once(ps, p64, f"finalize gt_mean PSNR, call {call} {tag}", extra)
        # whatever the final image, the PSNR is that image's: float64 over the returned pixels, rounded once
        rounded_once(ps, R.psnr(t64, fin.cpu().double()), f"finalize gt_mean PSNR of the returned final, call {call} {tag}")
    # ---- gt_mean off, with a target: the final is the clamped crop, the PSNR has no float32 term, an exact candidate scores 100
    k = B * N - 1
    pred, target = R.finalize_inputs(name, exact_candidate=k)
    _, _, p64 = R.candidate_finalize(pred.double(), target.double(), N, h, w, False)
    assert float(p64[k]) == 100.0
    pred_d, target_d = dev(pred), dev(target)
    crop = pred[:, :, :h, :w].clamp(0, 1)
    for call in (1, 2):
        fin, ps = ops.candidate_finalize(pred_d, target_d, N, h, w, False)
        bit_equal(fin, crop, f"finalize clamp-only final {tag}")
        rounded_once(ps, p64, f"finalize clamp-only PSNR, call {call} {tag}")
        rounded_once(ps, R.psnr(target.double().repeat_interleave(N, 0), fin.cpu().double()), f"finalize clamp-only PSNR of the returned final {tag}")
        assert float(ps[k]) == 100.0
    # ---- no target
    for call in (1, 2):
        fin, ps = ops.candidate_finalize(pred_d, None, N, h, w, False)
        bit_equal(fin, crop, f"finalize without a target {tag}")
        assert float(ps.abs().max()) == 0.0


def test_composite_finalize_then_selection():
    """candidate_finalize -> select_best and -> ssim -> select_scores(0.5) at 61x203, N = 64: the float64 chain's index for both images."""
    from bem import ops
    h, w, Hp, Wp, B, N = R.FINALIZE[R.COMPOSITE]
    pred, target = R.finalize_inputs(R.COMPOSITE)
    c = R.composite_reference(pred, target, N, h, w)
    want_p = [R.select_best(c["psnr"][b * N:(b + 1) * N]) for b in range(B)]
    want_w = [R.select_scores(c["psnr"][b * N:(b + 1) * N], c["ssim"][b * N:(b + 1) * N], 0.5) for b in range(B)]
    assert want_p != want_w                                                            # the SSIM term does move the choice
    fin, ps = ops.candidate_finalize(dev(pred), dev(target), N, h, w, True)
    best, bp, img = ops.select_best(fin, ps, N)
    assert best.cpu().tolist() == want_p
    bit_equal(img, torch.stack([fin[b * N + want_p[b]].cpu() for b in range(B)]), "composite gather")
    bit_equal(bp, torch.stack([ps[b * N + want_p[b]].cpu() for b in range(B)]), "composite best PSNR")
    ss = ops.ssim(fin, dev(target), N)
    err = (ss.cpu().double() - c["ssim"]).abs()
    print(f"PARITY once composite SSIM of the GPU finals: worst |err| {float(err.max()):.3e} | ratio {float((err / c['ssim_bound']).max()):.2f}")
    assert bool((err <= c["ssim_bound"]).all())
    best, b1, b2, img = ops.select_scores(fin, ps, N, ss, 0.5, "weighted")
    assert best.cpu().tolist() == want_w
    bit_equal(img, torch.stack([fin[b * N + want_w[b]].cpu() for b in range(B)]), "composite gather, weighted")
    bit_equal(b2, torch.stack([ss[b * N + want_w[b]].cpu() for b in range(B)]), "composite best SSIM")


# ------------------------------------------------------------------------------------------------------------------ cond_postproc, plane_mean
@pytest.mark.parametrize("bn", R.COND_BN)
@pytest.mark.parametrize("plane", R.COND_PLANES)
def test_cond_postproc(plane, bn):
    from bem import ops
    (h, w), (B, N) = plane, bn
    g = R.gen(500 + h * w + B)
    tag = f"hw={h * w} B={B} N={N}"
    mixed = 0.4 * torch.randn(B * N, 3, h, w, generator=g) + 0.5                        # negatives and values above 1
    above = 1.0 + torch.rand(B * N, 3, h, w, generator=g)                               # every input >= 1: the clamped plane is all ones
    tm = 0.1 + 0.8 * torch.rand(B, 3, generator=g)
    noise = torch.randn(B * N, 3, h, w, generator=g)
    for pname, pred in (("mixed", mixed), ("all >= 1", above)):
        pred_d = dev(pred)
        bit_equal(ops.cond_postproc(pred_d, None, None, N, 0.1), pred.clamp(0, 1), f"cond_postproc clamp only, {pname} {tag}")
        for nz in (None, noise):
            r32, r64 = both(R.cond_postproc, pred, tm, nz, N, 0.1, zero_sum="zero")
            got = ops.cond_postproc(pred_d, dev(tm), None if nz is None else dev(nz), N, 0.1)
            per_pixel(got, r32, r64, f"cond_postproc target mean, noise={nz is not None}, {pname} {tag}")
        r32, r64 = both(R.cond_postproc, pred, None, noise, N, 0.1)
        per_pixel(ops.cond_postproc(pred_d, None, dev(noise), N, 0.1), r32, r64, f"cond_postproc noise only, {pname} {tag}")
    if (h * w, B) == (20, 1):                                                           # a plane without a positive value: stays 0, no NaN
        dead = mixed.clone()
        dead[0, 1] = -dead[0, 1].abs()
        assert bool(torch.isnan(R.cond_postproc(dead.double(), tm.double(), None, N, 0.1)[0, 1]).all())
        got = ops.cond_postproc(dev(dead), dev(tm), None, N, 0.1)
        assert float(got[0, 1].abs().max()) == 0.0
        per_pixel(got, *both(R.cond_postproc, dead, tm, None, N, 0.1, zero_sum="zero"), f"cond_postproc zero-sum channel {tag}")


def test_plane_mean():
    from bem import ops
    g = R.gen(600)
    wide = R.gen(601)

    def run(x_d, x, h, w, what):
        rounded_once(ops.plane_mean(x_d, h, w), R.plane_mean(x.double(), h, w), f"plane_mean {what}")

    x = torch.randn(2, 3, 33, 64, generator=g) + 0.5
    run(dev(x), x, None, None, "33x64: three float4 passes, ragged end")
    run(dev(x), x, 21, 64, "rows 0..20 of 33x64: 16-byte path with a row crop")
    y = torch.randn(2, 3, 37, 29, generator=g) + 0.5
    run(dev(y), y, None, None, "37x29: scalar path")
    z = torch.randn(2, 3, 16, 24, generator=g) + 0.5
    run(dev(z), z, 13, 21, "13x21 inside 16x24")
    for hw in ((1, 4), (1, 1)):
        t = torch.randn(2, 3, *hw, generator=g)
        run(dev(t), t, None, None, f"{hw[0]}x{hw[1]}")
    m = torch.randn(2, 3, 32, 64, generator=g) + 0.5
    run(offset_by_one_float(m), m, None, None, "32x64 from a base 4 bytes past a 16-byte boundary: scalar fallback")
    near_one = 1.0 + 1e-4 * torch.randn(2, 3, 33, 64, generator=wide)                   # a float32 accumulation loses these digits
    run(dev(near_one), near_one, None, None, "33x64 of 1 + 1e-4 N(0,1)")
    f32_sum = near_one.reshape(6, -1).cumsum(1)[:, -1] / (33 * 64)
    print(f"PARITY note plane_mean: a sequential float32 sum of the last case errs by {float((f32_sum.double() - near_one.double().mean((2, 3)).reshape(-1)).abs().max()):.3e}")


# ------------------------------------------------------------------------------------------------------------------ mc_mean
@pytest.mark.parametrize("name", list(R.MC_MEAN))
def test_mc_mean(name):
    from bem import ops
    h, w, Hp, Wp, B, N = R.MC_MEAN[name]
    raw, target = R.mc_inputs(name)
    raw_d, target_d = dev(raw), dev(target)
    for gm in (False, True):
        r32, r64 = both(R.mc_mean, raw, target, N, h, w, gm)
        for call in (1, 2):
            per_pixel(ops.mc_mean(raw_d, target_d, N, h, w, gm), r32, r64, f"mc_mean gt_mean={gm}, call {call} {name} {R.MC_MEAN[name]}")
    bit_equal(ops.mc_mean(raw_d, None, N, h, w, False), ops.mc_mean(raw_d, target_d, N, h, w, False).cpu(), "mc_mean without a target")


# ------------------------------------------------------------------------------------------------------------------ ssim
@pytest.mark.parametrize("name", list(R.SSIM))
def test_ssim(name):
    from bem import ops
    B, N, h, w = R.SSIM[name]
    fin, tg = R.ssim_inputs(name)
    rounded_once(ops.ssim(dev(fin), dev(tg), N), R.ssim(fin.double(), tg.double(), N), f"ssim {name} {R.SSIM[name]}")


def test_ssim_identical_and_constant_images():
    from bem import ops
    fin, tg = R.ssim_inputs("1x2-tiles")
    same = tg.repeat_interleave(2, 0)
    got = ops.ssim(dev(same), dev(tg), 2)
    assert got.cpu().tolist() == [1.0, 1.0]
    a, b = torch.full((1, 3, 26, 42), 100 / 255.0), torch.full((2, 3, 26, 42), 140 / 255.0)
    b[1] = 100 / 255.0
    want = R.ssim(b.double(), a.double(), 2)
    C1 = (0.01 * 255) ** 2
    assert abs(float(want[0]) - (2 * 100 * 140 + C1) / (100 ** 2 + 140 ** 2 + C1)) < 1e-12 and abs(float(want[1]) - 1.0) < 1e-12
    rounded_once(ops.ssim(dev(b), dev(a), 2), want, "ssim of two constant images (zero variance: C1 and C2 only)")


# ------------------------------------------------------------------------------------------------------------------ selection and gathers
@pytest.mark.parametrize("name", R.SELECT_CASES)
def test_selection_rules(name):
    from bem import ops
    ps, ss, _ = R.select_rows(name)
    B, N = ps.shape
    fin = torch.rand(B * N, 3, 3, 5, generator=R.gen(700))
    fin_d, ps_d, ss_d = dev(fin), dev(ps.reshape(-1)), dev(ss.reshape(-1))
    pick = lambda t, idx: torch.stack([t.reshape(B, N, *t.shape[1:])[b, idx[b]] for b in range(B)])
    want = [R.select_best(ps[b]) for b in range(B)]
    best, bp, img = ops.select_best(fin_d, ps_d, N)
    assert best.cpu().tolist() == want, (name, "select_best")
    bit_equal(bp, pick(ps.reshape(-1), want), "select_best score")
    bit_equal(img, pick(fin, want), "select_best image")
    for rule, wgt in R.SELECT_RULES:
        want = [R.select_scores(ps[b], ss[b] if rule == "weighted" else None, wgt, rule) for b in range(B)]
        best, b1, b2, img = ops.select_scores(fin_d, ps_d, N, ss_d if rule == "weighted" else None, wgt, rule)
        assert best.cpu().tolist() == want, (name, rule, wgt)
        bit_equal(b1, pick(ps.reshape(-1), want), f"select_scores {rule} {wgt} s1")
        bit_equal(img, pick(fin, want), f"select_scores {rule} {wgt} image")
        if rule == "weighted":
            bit_equal(b2, pick(ss.reshape(-1), want), f"select_scores {rule} {wgt} s2")
    w1 = [R.select_scores(ps[b], None, 1.0, "weighted") for b in range(B)]
    assert ops.select_scores(None, ps_d, N)[0].cpu().tolist() == w1 == [R.select_best(ps[b]) for b in range(B)]


def test_selection_with_nan_scores():
    """select_best and the max / min rules follow Python's list semantics for NaN (a leading NaN is kept, any other is passed over).  The
    weighted rule never chooses a NaN score unless every score is NaN: the reference's max() would keep a leading one."""
    from bem import ops
    nan = float("nan")
    rows = [[nan, 20.0, 30.0, 25.0], [20.0, nan, 30.0, 25.0], [30.0, 20.0, 25.0, nan], [nan, nan, nan, nan], [20.0, 30.0, nan, 30.0]]
    ps = dev(torch.tensor(rows).reshape(-1))
    fin = dev(torch.rand(len(rows) * 4, 3, 2, 2, generator=R.gen(701)))
    want = [R.select_best(r) for r in rows]
    assert want == [0, 2, 0, 0, 1]
    assert ops.select_best(fin, ps, 4)[0].cpu().tolist() == want
    assert ops.select_scores(None, ps, 4, rule="max")[0].cpu().tolist() == [R.select_scores(r, rule="max") for r in rows] == want
    assert ops.select_scores(None, ps, 4, rule="min")[0].cpu().tolist() == [R.select_scores(r, rule="min") for r in rows] == [0, 0, 1, 0, 0]
    assert ops.select_scores(None, ps, 4)[0].cpu().tolist() == [2, 2, 0, 0, 1]                      # row 0: Python's rule gives 0
    ss = dev(torch.tensor([[0.5, 0.6, 0.7, 0.8]] * len(rows)).reshape(-1))
    assert ops.select_scores(None, ps, 4, ss, 0.5)[0].cpu().tolist() == [2, 2, 2, 0, 3]


def relative(ops, fin, ps, N):
    """The default PSNR rule under its select_scores spelling, in select_scores' result order."""
    return ops.select_scores(fin, ps, N, rule="relative")


def same_bits(got, want, what):
    """Equal as bit patterns: NaN where NaN is, and the same one."""
    assert torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)), what


@pytest.mark.parametrize("rule", ["max", "min"])
def test_chunked_merge_is_the_one_shot_selection(rule):
    """select_merge over every split of N = 4 into ordered chunks leaves what one select_scores call over the four samples gives: index,
    score (NaN included) and image; on the NaN rows of test_selection_with_nan_scores, an all-equal and a strictly decreasing row."""
    from bem import ops
    rows, N = C.MERGE_ROWS, 4
    B = len(rows)
    ps = dev(torch.tensor(rows))
    fin = dev(torch.rand(B, N, 3, 2, 2, generator=R.gen(703)))
    want = [R.select_scores(r, rule=rule) for r in rows]
    best, b1, _, img = ops.select_scores(fin.flatten(0, 1), ps.reshape(-1), N, rule=rule)
    assert best.cpu().tolist() == want
    splits = list(C.compositions(N))
    assert len(splits) == 8 and (4,) in splits and (1, 1, 1, 1) in splits
    for split in splits:
        st, lo = ops.BestState(B, (3, 2, 2), "cuda", rule), 0
        for k in split:
            ops.select_merge(st, fin[:, lo:lo + k].contiguous().flatten(0, 1), ps[:, lo:lo + k].contiguous().reshape(-1), k)
            lo += k
        assert st.n == N and st.best.cpu().tolist() == want, (rule, split, st.best.cpu().tolist())
        same_bits(st.score, b1, f"select_merge {rule} {split} score")
        bit_equal(st.images, img.cpu(), f"select_merge {rule} {split} image")


@pytest.mark.parametrize("N", [1, 64])
def test_selection_at_the_workgroup_edge(N):
    """65 images: the second workgroup holds one thread with work.  Every rule against the float64 reference row by row;
    test_edge_tables_have_a_clear_winner_or_a_written_tie holds the tables to a clear winner or a written tie."""
    from bem import ops
    s1, s2, _ = C.edge_tables(N)
    B = C.EDGE_B
    fin = torch.rand(B * N, 1, 1, 1, generator=R.gen(704))
    fin_d, s1_d, s2_d = dev(fin), dev(s1.reshape(-1)), dev(s2.reshape(-1))
    rows = torch.arange(B) * N
    for rule, two, wgt in C.EDGE_RULES:
        want = torch.tensor([C.edge_reference(rule, s1[b], s2[b] if two else None, wgt) for b in range(B)])
        if rule == "relative":
            best, b1, b2, img = relative(ops, fin_d, s1_d, N)
        else:
            best, b1, b2, img = ops.select_scores(fin_d, s1_d, N, s2_d if two else None, wgt, rule)
        assert best.cpu().tolist() == want.tolist(), (N, rule, two)
        bit_equal(b1, s1.reshape(-1)[rows + want], f"edge {rule} s1")
        bit_equal(img, fin[rows + want], f"edge {rule} image")
        assert (b2 is None) == (not two)
        if two:
            bit_equal(b2, s2.reshape(-1)[rows + want], f"edge {rule} s2")


def test_relative_rule_is_select_best():
    """select_scores(rule='relative') and select_best return the same tensors: the tables of test_selection_rules and a negative maximum."""
    from bem import ops
    tables = [R.select_rows(name)[0] for name in R.SELECT_CASES] + [torch.tensor([[-3.0, -1.0, -2.0]])]
    for ps in tables:
        B, N = ps.shape
        fin_d, ps_d = dev(torch.rand(B * N, 3, 3, 5, generator=R.gen(705))), dev(ps.reshape(-1))
        best, b1, b2, img = relative(ops, fin_d, ps_d, N)
        best0, bp0, img0 = ops.select_best(fin_d, ps_d, N)
        assert b2 is None and torch.equal(best, best0) and torch.equal(img, img0)
        same_bits(b1, bp0, "relative score")
    assert best.cpu().tolist() == [0]                                     # [-3, -1, -2] / -1: the order turns round


@pytest.mark.parametrize("side,aligned", [(296, True), (296, False), (592, True)])
def test_gathers_past_their_grid_caps(side, aligned):
    """3 x 296 x 296 = 262848 elements per image: 704 past the scalar form's 1024 x 256 threads; 3 x 592 x 592 / 4 = 262848 float4.
    From a base 4 bytes past a 16-byte boundary the scalar form runs."""
    from bem import ops
    B, N = 2, 2
    fin = torch.rand(B * N, 3, side, side, generator=R.gen(702 + side))
    fin_d = dev(fin) if aligned else offset_by_one_float(fin)
    ps = dev(torch.tensor([1.0, 2.0, 4.0, 3.0]))
    best, _, img = ops.select_best(fin_d, ps, N)
    assert best.cpu().tolist() == [1, 0]
    bit_equal(img, fin[[1, 2]], f"gather_best{'' if aligned else '_scalar'} {side}")
    best, _, _, img = ops.select_scores(fin_d, ps, N, rule="min")
    assert best.cpu().tolist() == [0, 1]
    bit_equal(img, fin[[0, 3]], f"select_scores gather{'' if aligned else ', scalar'} {side}")


# ------------------------------------------------------------------------------------------------------------------ entry kernels
@pytest.mark.parametrize("planes", [(1, 1), (2, 3)])
@pytest.mark.parametrize("H,W,Hp,Wp", R.PADS)
def test_pad_reflect(H, W, Hp, Wp, planes):
    from bem import ops
    x = torch.rand(*planes, H, W, generator=R.gen(800 + H))
    want = np.pad(x.numpy(), ((0, 0), (0, 0), (0, Hp - H), (0, Wp - W)), "reflect")
    bit_equal(ops.pad_reflect(dev(x), Hp, Wp), torch.from_numpy(want), f"pad_reflect {H}x{W} -> {Hp}x{Wp}")
    x_d = dev(x)
    assert ops.pad_reflect(x_d, H, W) is x_d


@pytest.mark.parametrize("H,W,s", R.RESIZE)
def test_resize_down(H, W, s):
    from bem import ops
    x = torch.rand(2, 3, H, W, generator=R.gen(810 + s))
    per_pixel(ops.resize_down(dev(x), s), *both(R.resize_down, x, s), f"resize_down {H}x{W} / {s}")


@pytest.mark.parametrize("s", [2, 16])
@pytest.mark.parametrize("H,W", R.BILINEAR)
def test_bilinear_up(H, W, s):
    from bem import ops
    x = torch.rand(2, 3, H, W, generator=R.gen(820 + H * W))
    r32, r64 = both(R.bilinear_up, x, s)
    per_pixel(ops.bilinear_up(dev(x), s), r32, r64, f"bilinear_up {H}x{W} x{s}")
    fill = torch.randn(2, 7, H * s, W * s, generator=R.gen(821))
    dst = dev(fill.clone())
    assert ops.bilinear_up(dev(x), s, dst, 2) is dst
    per_pixel(dst[:, 2:5], r32, r64, f"bilinear_up {H}x{W} x{s} into channels 2..4 of 7")
    bit_equal(dst[:, :2], fill[:, :2], "channels below the slice")
    bit_equal(dst[:, 5:], fill[:, 5:], "channels above the slice")


# ------------------------------------------------------------------------------------------------------------------ host checks
class _NoLaunch:
    """Stands in for the library while malformed calls are made: reaching it means a host check is missing."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached: the wrapper would have launched")


def _bad_calls():
    z = lambda *s: torch.zeros(*s, device="cuda")
    return {
        "pad_reflect: pad equal to the height": lambda ops: ops.pad_reflect(z(1, 1, 4, 8), 8, 8),
        "pad_reflect: pad larger than the width": lambda ops: ops.pad_reflect(z(1, 1, 8, 3), 8, 7),
        "pad_reflect: smaller than the image": lambda ops: ops.pad_reflect(z(1, 1, 8, 8), 7, 8),
        "candidate_finalize: 4 candidates in groups of 3": lambda ops: ops.candidate_finalize(z(4, 3, 2, 2), z(1, 3, 2, 2), 3, 2, 2, True),
        "candidate_finalize: groups of 0": lambda ops: ops.candidate_finalize(z(4, 3, 2, 2), None, 0, 2, 2, False),
        "candidate_finalize: 21846 candidates, 3 Bn = 65538": lambda ops: ops.candidate_finalize(z(21846, 3, 1, 1), None, 1, 1, 1, False),
        "candidate_finalize: gt_mean without a target": lambda ops: ops.candidate_finalize(z(2, 3, 2, 2), None, 1, 2, 2, True),
        "candidate_finalize: crop wider than the plane": lambda ops: ops.candidate_finalize(z(2, 3, 2, 2), None, 1, 2, 3, False),
        "select_best: 5 candidates in groups of 2": lambda ops: ops.select_best(z(5, 3, 1, 1), z(5), 2),
        "select_best: 65536 images": lambda ops: ops.select_best(z(65536, 1, 1, 1), z(65536), 1),
        "select_scores: 5 candidates in groups of 2": lambda ops: ops.select_scores(None, z(5), 2),
        "select_scores: 65536 images": lambda ops: ops.select_scores(None, z(65536), 1, rule="max"),
        "select_scores: unknown rule": lambda ops: ops.select_scores(None, z(4), 2, rule="median"),
        "ssim: 3 candidates in groups of 2": lambda ops: ops.ssim(z(3, 3, 11, 11), z(1, 3, 11, 11), 2),
        "ssim: image of the window's size less one": lambda ops: ops.ssim(z(2, 3, 10, 11), z(1, 3, 10, 11), 2),
        "mc_mean: 3 candidates in groups of 2": lambda ops: ops.mc_mean(z(3, 3, 2, 2), None, 2, 2, 2, False),
        "mc_mean: 65536 images": lambda ops: ops.mc_mean(z(65536, 3, 1, 1), None, 1, 1, 1, False),
        "mc_mean: gt_mean without a target": lambda ops: ops.mc_mean(z(2, 3, 2, 2), None, 2, 2, 2, True),
    }


@pytest.mark.parametrize("what", list(_bad_calls()))
def test_malformed_calls_are_rejected_before_any_launch(what, monkeypatch):
    from bem import ops
    monkeypatch.setattr(ops, "lib", lambda: _NoLaunch())
    with pytest.raises(ValueError):
        _bad_calls()[what](ops)


def test_limits_hold_at_their_last_admitted_value_and_on_the_c_side(monkeypatch):
    """65535 images pass the wrappers and run; the library itself refuses 65536 candidates for ssim (whose wrapper's limit would cost
    95 MB of images to reach) before it reads anything."""
    from bem import native, ops
    B = 65535
    ps = torch.arange(2 * B, device="cuda", dtype=torch.float32)
    best = ops.select_scores(None, ps, 2, rule="max")[0]
    assert int(best.min()) == 1 and int(best.max()) == 1
    best, bp, _ = ops.select_best(torch.zeros(2 * B, 1, 1, 1, device="cuda"), ps, 2)
    assert int(best.min()) == 1 and torch.equal(bp, ps[1::2])
    fin, _ = ops.candidate_finalize(torch.full((21845, 3, 1, 1), 2.0, device="cuda"), None, 1, 1, 1, False)
    assert float(fin.min()) == 1.0 and float(fin.max()) == 1.0
    t = torch.zeros(3 * 11 * 11, device="cuda")
    ws = torch.zeros(1, device="cuda", dtype=torch.float64)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    rc = native.lib().bem_ssim_f32(p(t), p(t), p(t), p(ws), 65536, 1, 11, 11, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc != 0 and b"ssim: bad shape" in native.lib().bem_last_error()
    with pytest.raises(native.BemNativeError, match="ssim: bad shape"):
        native.check(rc, "ssim")


def test_no_launch_stub_is_what_a_missing_check_would_hit(monkeypatch):
    from bem import ops
    monkeypatch.setattr(ops, "lib", lambda: _NoLaunch())
    with pytest.raises(AssertionError, match="was reached"):
        ops.mc_mean(torch.zeros(2, 3, 2, 2, device="cuda"), None, 2, 2, 2, False)
