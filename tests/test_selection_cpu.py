"""The float64 references of tests/selection_ref.py pinned without a GPU: against the oracle's restatements (oracle/bem_oracle.py), against
what the reference nets' own run recorded (tests/golden/g8_eval.npz: preds -> finals -> psnr -> best) and against F.interpolate.  Also the
conditions the GPU tests rely on, for every case of the shape tables: best and runner-up of each selection case differ by more than
R.GAP x the score error the GPU bounds admit (or are bit-equal where a tie is written in), and the SSIM inputs sit on integer levels."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import selection_cases as C
import selection_ref as R
from conftest import load_golden
from oracle import bem_oracle as O


def hwc(t):
    return t.permute(1, 2, 0).numpy()


# ------------------------------------------------------------------------------------------------------------------ oracle
@pytest.mark.parametrize("H,W,Hp,Wp", R.PADS)
def test_pad_reflect_is_numpy_reflect_and_the_oracle(H, W, Hp, Wp):
    x = torch.rand(2, 3, H, W, generator=R.gen(1))
    got = R.pad_reflect(x, Hp, Wp)
    assert np.array_equal(got.numpy(), np.pad(x.numpy(), ((0, 0), (0, 0), (0, Hp - H), (0, Wp - W)), "reflect"))
    if (H, W, Hp, Wp) == (100, 150, 128, 192):                      # the pipeline's ((h + f) // f) * f rule, f = 64
        assert np.array_equal(hwc(got[1]), O.pad_reflect_ref(hwc(x[1]), 64))
    if (H, W, Hp, Wp) == (5, 9, 8, 16):
        assert np.array_equal(hwc(got[0]), O.pad_reflect_ref(hwc(x[0]), 8))


@pytest.mark.parametrize("H,W,s", R.RESIZE)
def test_resize_down_is_the_oracle(H, W, s):
    x = torch.rand(2, 3, H, W, generator=R.gen(2)).double()
    assert torch.allclose(R.resize_down(x, s), O.cv2_resize_down(x, s), rtol=0, atol=2e-16)
    assert R.resize_down(x, s).shape == (2, 3, H // s, W // s)


@pytest.mark.parametrize("H,W", R.BILINEAR)
@pytest.mark.parametrize("s", [2, 16])
def test_bilinear_up_is_interpolate_in_float64(H, W, s):
    x = torch.rand(2, 3, H, W, generator=R.gen(3)).double()
    want = F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=False)
    assert torch.allclose(R.bilinear_up(x, s), want, rtol=0, atol=4e-16)


def test_cond_postproc_is_the_eval_loops_expression():
    g = R.gen(4)
    pred, tm, nz = 0.4 * torch.randn(6, 3, 7, 5, generator=g).double() + 0.5, torch.rand(2, 3, generator=g).double(), torch.randn(6, 3, 7, 5, generator=g).double()
    c = pred.clamp(0, 1)
    want = (c * (tm.repeat_interleave(3, 0)[:, :, None, None] / c.mean(dim=(2, 3), keepdim=True))).clamp(0, 1) + nz * 0.1    # bem_oracle.eval_mc_ref
    assert torch.equal(R.cond_postproc(pred, tm, nz, 3, 0.1), want)
    assert torch.equal(R.cond_postproc(pred, None, None, 3, 0.1), c)
    assert torch.equal(R.plane_mean(pred, 4, 3), pred[:, :, :4, :3].mean((2, 3)))


@pytest.mark.parametrize("name", ["4097", "sub-wave", "degenerate"])
def test_candidate_finalize_is_the_oracles_numpy_path(name):
    h, w, Hp, Wp, B, N = R.FINALIZE[name]
    pred, target = R.finalize_inputs(name)
    for gt_mean in (True, False):
        fin, ratio, ps = R.candidate_finalize(pred.double(), target.double(), N, h, w, gt_mean)
        for i in range(0, B * N, max(1, B * N // 6)):
            q = np.clip(hwc(pred[i, :, :h, :w].double()), 0, 1)
            t = hwc(target[i // N].double())
            if gt_mean:
                with np.errstate(all="ignore"):
                    r = t.mean(axis=(0, 1), keepdims=True) / q.mean(axis=(0, 1), keepdims=True)
                    assert np.allclose(ratio[i].numpy(), r.reshape(3), rtol=1e-13, atol=0)
                    q = np.clip(q * r, 0, 1)
            assert np.allclose(hwc(fin[i]), q, rtol=0, atol=1e-15, equal_nan=True)
            want = O.psnr_ref(t, q)
            assert abs(float(ps[i]) - want) < 1e-11 or (np.isnan(want) and bool(torch.isnan(ps[i])))
    pred, target = R.finalize_inputs(name, exact_candidate=B * N - 1)
    ps = R.candidate_finalize(pred.double(), target.double(), N, h, w, False)[2]
    assert float(ps[-1]) == 100.0 and O.psnr_ref(hwc(target[-1]), hwc(pred[-1, :, :h, :w])) == 100.0
    fin, _, ps = R.candidate_finalize(pred.double(), None, N, h, w, False)
    assert torch.equal(fin, pred[:, :, :h, :w].double().clamp(0, 1)) and float(ps.abs().max()) == 0


@pytest.mark.parametrize("name", ["1x2-tiles", "one-pixel", "one-wide"])
def test_ssim_is_the_oracle(name):
    B, N, h, w = R.SSIM[name]
    fin, tg = R.ssim_inputs(name)
    got = R.ssim(fin.double(), tg.double(), N)
    for bn in range(B * N):
        want = O.ssim_ref(O.img_as_ubyte_ref(hwc(tg[bn // N])), O.img_as_ubyte_ref(hwc(fin[bn])))
        assert abs(float(got[bn]) - want) < 1e-12, (bn, float(got[bn]), want)
    # float images off the levels quantise like img_as_ubyte
    x = torch.rand(1, 3, 12, 13, generator=R.gen(5))
    assert np.array_equal(R.to_levels(x).numpy().astype(np.uint8), O.img_as_ubyte_ref(x.numpy()))


@pytest.mark.parametrize("name", ["second-pass", "n64", "degenerate"])
def test_mc_mean_is_the_oracle(name):
    h, w, Hp, Wp, B, N = R.MC_MEAN[name]
    raw, tg = R.mc_inputs(name)
    for gm in (False, True):
        got = R.mc_mean(raw.double(), tg.double(), N, h, w, gm)
        for b in range(B):
            pr = raw[b * N:(b + 1) * N, :, :h, :w].permute(0, 2, 3, 1).numpy()
            want = O.mc_mean_ref(pr, hwc(tg[b]), gm)                  # float32 arrays, as eval.py holds them
            assert np.abs(hwc(got[b]) - want).max() < 2e-6, (name, gm)


@pytest.mark.parametrize("name", R.SELECT_CASES)
def test_selection_rules_are_the_oracle(name):
    ps, ss, _ = R.select_rows(name)
    for b in range(ps.shape[0]):
        p, s = ps[b].double().tolist(), ss[b].double().tolist()
        with np.errstate(all="ignore"):
            assert R.select_best(ps[b]) == O.select_ref(p, s, 1.0)
            for wgt in (1.0, 0.5, 0.0):
                assert R.select_scores(ps[b], ss[b], wgt) == O.select_ref(p, s, wgt)
        assert R.select_scores(ps[b], rule="max") == O.select_ref(no_ref_list=p, no_ref="clip")
        assert R.select_scores(ps[b], rule="min") == O.select_ref(no_ref_list=p, no_ref="niqe")


def test_selection_rules_keep_pythons_nan_semantics():
    nan = float("nan")
    assert R.select_best([nan, 20.0, 30.0]) == 0                      # max() keeps a leading NaN: every score NaN, the first is "the" maximum
    assert R.select_best([20.0, nan, 30.0]) == 2 and R.select_best([30.0, nan, 20.0]) == 0
    assert R.select_best([0.0, 0.0]) == 0 and R.select_best([nan, nan]) == 0
    assert R.select_scores([nan, 1.0, 2.0], rule="max") == 0 and R.select_scores([1.0, nan, 0.5], rule="min") == 2


def test_zero_sum_channel_is_nan_in_the_reference_and_zero_under_the_projects_rule():
    """The 1x1 case of the finalize grid has candidates whose single pixel clamps to 0: numpy keeps NaN through np.clip, and the NaN
    reaches the PSNR; zero_sum='zero' is the kernels' stated behaviour: the channel stays 0 and the PSNR is finite."""
    h, w, Hp, Wp, B, N = R.FINALIZE["degenerate"]
    pred, target = R.finalize_inputs("degenerate")
    fin, _, ps = R.candidate_finalize(pred.double(), target.double(), N, h, w, True)
    dead = pred[:, :, 0, 0] <= 0
    assert bool(dead.any()) and not bool(dead.all(1).any())
    assert torch.equal(torch.isnan(fin[:, :, 0, 0]), dead) and torch.equal(torch.isnan(ps), dead.any(1))
    finz, _, psz = R.candidate_finalize(pred.double(), target.double(), N, h, w, True, zero_sum="zero")
    assert torch.isfinite(psz).all() and float(finz[:, :, 0, 0][dead].abs().max()) == 0 and torch.equal(finz[:, :, 0, 0][~dead], fin[:, :, 0, 0][~dead])
    x = torch.tensor([[[[-1.0, 0.0]], [[0.25, 0.75]], [[0.5, 2.0]]]], dtype=torch.float64)
    tm = torch.tensor([[0.3, 0.25, 0.0]], dtype=torch.float64)
    assert torch.isnan(R.cond_postproc(x, tm, None, 1, 0.0)[0, 0]).all()
    assert torch.equal(R.cond_postproc(x, tm, None, 1, 0.0, zero_sum="zero"), torch.tensor([[[[0.0, 0.0]], [[0.125, 0.375]], [[0.0, 0.0]]]], dtype=torch.float64))


# ------------------------------------------------------------------------------------------------------------------ recorded run
def test_references_reproduce_the_recorded_eval_tail():
    """g8: the reference nets' own run.  From its recorded preds and gt alone: finals, PSNRs and the chosen index."""
    g = load_golden("g8_eval")
    preds, gt = g["preds"], g["gt"]
    N, _, h, w = preds.shape
    fin, _, ps = R.candidate_finalize(preds.double(), gt.double(), N, h, w, True)
    assert float((fin.permute(0, 2, 3, 1) - g["finals"].double()).abs().max()) < 2e-7          # the recorded finals are float32
    assert float((ps - torch.as_tensor(g["psnr"]).double()).abs().max()) < 2e-6
    assert R.select_best(ps) == int(g["best"]) == R.select_best(g["psnr"])
    assert R.gap(R.ranked(ps)) > 1e-2


# ------------------------------------------------------------------------------------------------------------------ GPU-test conditions
@pytest.mark.parametrize("name", list(R.SSIM))
def test_ssim_inputs_sit_on_integer_levels(name):
    for x in R.ssim_inputs(name):
        for v in (x * 255.0, x.double() * 255.0):
            assert float((v - v.round()).abs().max()) < 1e-4
        assert torch.equal(R.to_levels(x).double(), R.to_levels(x.double())) and 0 <= float(x.min()) and float(x.max()) <= 1
    fin, tg = R.ssim_inputs(name)
    assert fin.shape[0] == R.SSIM[name][0] * R.SSIM[name][1] and not torch.equal(fin[0], tg[0])


@pytest.mark.parametrize("name", R.SELECT_CASES)
def test_score_tables_have_a_clear_winner_or_a_written_tie(name):
    """The tables reach the kernels exactly and are compared in float64 there: the admitted score error is a few float64 roundings."""
    ps, ss, ties = R.select_rows(name)
    assert torch.equal(ps, ps.double().float())
    for rule, wgt in R.SELECT_RULES:
        for b in range(ps.shape[0]):
            sc = R.ranked(ps[b], ss[b] if rule == "weighted" else None, wgt, rule)
            if torch.isnan(sc).any():
                assert ties.get(b) == "tie" and torch.isnan(sc).all()
                continue
            gp = R.gap(sc)
            if gp == 0:
                assert ties.get(b) == "tie", (name, rule, wgt, b)
            else:
                assert gp > R.GAP * 8 * 2.0 ** -52 * float(sc.abs().max()), (name, rule, wgt, b, gp)
    if name == "edges":
        assert float(ps[0].abs().max()) == 0 and float(ps[1].max()) == 100.0 and float(ps[4].max()) < 0
        assert R.select_best(ps[2]) == 0 and R.select_best(ps[3]) == 1 and int(torch.argmax(ps[3].flip(0))) == 0


def test_composite_case_has_a_clear_winner_for_both_images():
    """candidate_finalize -> select_best, and -> ssim -> select_scores(0.5), at 61x203 / N = 64: the float64 winner leads by more than
    R.GAP x what the PSNR bound (one ulp + MARGIN x the float32 term) and the same rule for the SSIM of float32 finals admit."""
    h, w, Hp, Wp, B, N = R.FINALIZE[R.COMPOSITE]
    pred, target = R.finalize_inputs(R.COMPOSITE)
    c = R.composite_reference(pred, target, N, h, w)
    for b in range(B):
        p, s = c["psnr"][b * N:(b + 1) * N], c["ssim"][b * N:(b + 1) * N]
        ep, es = float(c["psnr_bound"][b * N:(b + 1) * N].max()), float(c["ssim_bound"][b * N:(b + 1) * N].max())
        assert R.gap(R.ranked(p)) > R.GAP * R.weighted_score_error(p, ep), (b, R.gap(R.ranked(p)))
        assert R.gap(R.ranked(p, s, 0.5)) > R.GAP * R.weighted_score_error(p, ep, s, es, 0.5), (b, R.gap(R.ranked(p, s, 0.5)))
    assert float((target[0] - target[1]).abs().mean()) > 0.4


@pytest.mark.parametrize("name", list(R.FINALIZE))
def test_finalize_inputs_reach_both_clamps_and_distinct_targets(name):
    h, w, Hp, Wp, B, N = R.FINALIZE[name]
    pred, target = R.finalize_inputs(name)
    assert pred.shape == (B * N, 3, Hp, Wp) and target.shape == (B, 3, h, w)
    if h * w > 64:
        crop = pred[:, :, :h, :w]
        assert float((crop < 0).double().mean()) > 0.05 and float((crop > 1).double().mean()) > 0.05
    if B == 2:
        assert float((target[0] - target[1]).abs().min()) > 0.15


@pytest.mark.parametrize("N", [1, 64])
def test_edge_tables_have_a_clear_winner_or_a_written_tie(N):
    """The tables of test_selection_at_the_workgroup_edge: for every rule the float64 winner of every row leads the runner-up by
    C.EDGE_GAP relative, or the best score stands twice, bit-equal, in a row marked 'tie'."""
    s1, s2, ties = C.edge_tables(N)
    assert s1.shape == s2.shape == (C.EDGE_B, N) and s1.dtype == s2.dtype == torch.float32
    assert sorted(ties) == ([] if N == 1 else [0, C.EDGE_B - 1])
    for rule, two, wgt in C.EDGE_RULES if N > 1 else []:
        for b in range(C.EDGE_B):
            sc = C.edge_scores(rule, s1[b], s2[b] if two else None, wgt)
            gp = R.gap(sc)
            if gp == 0:
                assert ties.get(b) == "tie", (rule, two, b)
            else:
                assert b not in ties and gp >= C.EDGE_GAP * float(sc.abs().max()), (rule, two, b, gp)
        want = [C.edge_reference(rule, s1[b], s2[b] if two else None, wgt) for b in ties]
        assert want == ([7, 7] if rule == "min" else [3, 3])


# ------------------------------------------------------------------------------------------------------------------ the host's statement
def test_first_index_is_the_reference_on_every_table_and_rule():
    from bem.scorers import first_index
    for name in R.SELECT_CASES:
        ps, ss, _ = R.select_rows(name)
        for b in range(ps.shape[0]):
            assert first_index(ps[b]) == R.select_best(ps[b]), (name, b)
            for rule, wgt in R.SELECT_RULES:
                two = ss[b] if rule == "weighted" else None
                assert first_index(ps[b], two, wgt, rule) == R.select_scores(ps[b], two, wgt, rule), (name, b, rule, wgt)
    s2 = [0.5, 0.6, 0.7, 0.8]
    for row in C.NAN_ROWS + [[0.0, 0.0]]:
        assert first_index(row) == first_index(row, rule="relative") == R.select_best(row), row
        for rule in ("weighted", "max", "min"):
            assert first_index(row, rule=rule) == R.select_scores(row, rule=rule), (row, rule)
        assert first_index(row, s2[:len(row)], 0.5, "weighted") == R.select_scores(row, s2[:len(row)], 0.5), row
    assert [first_index(r) for r in C.NAN_ROWS] == [0, 2, 0, 0, 1] and first_index([0.0, 0.0]) == 0 and first_index([-3.0, -1.0, -2.0]) == 0


def test_host_selection_functions_are_first_index():
    from bem import dist
    from bem.pipeline import BEMPipeline
    from bem.scorers import first_index
    rows = C.MERGE_ROWS + [[0.0, 0.0, 0.0, 0.0], [-3.0, -1.0, -2.0, -1.0]]
    want = [first_index(r) for r in rows]
    assert [BEMPipeline.select(r) for r in rows] == want
    assert dist.select_best(torch.tensor(rows).reshape(-1), 4) == want
    for rule in ("max", "min"):
        assert dist.first_best(rows, rule) == [first_index(r, rule=rule) for r in rows]


def test_select_scores_entry_knows_four_rules():
    """The C entry's checks run before any HIP call (B = 0 returns after them): rules 0..3 pass, rule 3 with a second score and rule 4 do not;
    bem_select_best_f32 is gone from the library."""
    import os
    from bem import native, ops
    if not os.path.exists(native.LIB_PATH):
        native.build()
    lib, p = ops.lib(), 16                      # any non-null value: no pointer is touched
    call = lambda rule, s2=None, B=0: lib.bem_select_scores_f32(None, p, s2, 1.0, rule, p, p, None, None, B, 4, 0, None)
    assert [call(r) for r in sorted(ops.SELECT_RULES.values())] == [0, 0, 0, 0] and sorted(ops.SELECT_RULES.values()) == [0, 1, 2, 3]
    assert call(0, s2=p) == 0
    for bad, word in ((dict(rule=4), "select_scores: unknown rule 4"), (dict(rule=3, s2=p), "rule 3 with a second score"),
                      (dict(rule=1, B=65536), "select_scores: bad arguments B=65536")):
        with pytest.raises(native.BemNativeError, match=word):
            native.check(call(**bad), "select_scores")
    assert not hasattr(lib, "bem_select_best_f32")
