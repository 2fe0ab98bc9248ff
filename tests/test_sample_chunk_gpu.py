"""GPU: sample-chunked N-sample evaluation -- the streamed Monte-Carlo mean / std kernels (ops.mc_accum, ops.mc_finish) and the selection
merge (ops.select_merge) against ops.mc_mean, ops.select_scores and float64; BEMPipeline.enhance(sample_chunk=, uncertainty=, keep=)
against the single batch; the memory the chunking saves; the eval driver's --sample_chunk / --uncertainty."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import mc_stream_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

# name -> (B, N, Hp, Wp, h, w): a cropped odd width (scalar accesses), whole 260x260 planes (more than mc_mean's 256-workgroup grid cap
# covers at one element per thread, so its threads stride) and 16x16 (16-byte accesses)
SHAPES = {"odd": (2, 5, 20, 24, 17, 21), "stride": (1, 3, 260, 260, 260, 260), "vec": (2, 5, 16, 16, 16, 16)}


def _splits(N):
    return [(N,), tuple([2] * (N // 2) + [1] * (N % 2)), (1,) * N]


def _rows(t, B, N, lo, n):
    return t.view((B, N) + tuple(t.shape[1:]))[:, lo:lo + n].reshape((B * n,) + tuple(t.shape[1:])).contiguous()


def _accumulate(raw, fin, B, N, h, w, splits):
    """raw (B*N,3,Hp,Wp) | None, fin (B*N,3,h,w) | None on the device, in chunks of the sizes ``splits`` -> ops.McState"""
    from bem import ops
    st, lo = ops.McState(B, h, w, "cuda", mean=raw is not None, spread=fin is not None), 0
    for n in splits:
        ops.mc_accum(st, None if raw is None else _rows(raw, B, N, lo, n), None if fin is None else _rows(fin, B, N, lo, n), n)
        lo += n
    assert st.n == N
    return st


@pytest.fixture(scope="module", params=list(SHAPES))
def kcase(request):
    B, N, Hp, Wp, h, w = SHAPES[request.param]
    raw, fin = R.kernel_inputs(3, B, N, Hp, Wp, h, w)
    tgt = np.random.default_rng(9).random((B, 3, h, w), dtype=np.float32)
    dev = lambda a: torch.from_numpy(a).reshape((B * N,) + a.shape[2:]).cuda()
    return dict(name=request.param, B=B, N=N, h=h, w=w, raw=dev(raw), fin=dev(fin), fin_np=fin, tgt=torch.from_numpy(tgt).cuda())


def test_streamed_mean_is_mc_mean_bit_for_bit(kcase):
    from bem import ops
    c = kcase
    assert float(c["raw"].min()) < 0 and float(c["raw"].max()) > 1                # the clamp matters
    for gt_mean in (False, True):
        ref = ops.mc_mean(c["raw"], c["tgt"], c["N"], c["h"], c["w"], gt_mean)
        for sp in _splits(c["N"]):
            st = _accumulate(c["raw"], None, c["B"], c["N"], c["h"], c["w"], sp)
            mc = ops.mc_finish(st, c["tgt"], gt_mean, mean=True)[0]
            assert torch.equal(mc, ref), (c["name"], gt_mean, sp, float((mc - ref).abs().max()))


def test_std_map_same_bits_for_any_split_and_close_to_float64(kcase):
    """Against numpy float64 (ddof = 1) on the same f32 inputs.  The bound is 4 x R.REF_STD_DEV = 4 x 5.7e-8: the worst deviation of the
    numpy-float32 restatement of the same recurrence from float64 on these inputs, measured on the CPU (tests/test_sample_chunk_cpu.py),
    with a factor for differences in how the compiler rounds.  (The bound was measured on the 'odd' inputs; the other two shapes draw
    from the same distribution.)  Measured on the MI355X: odd 5.69e-8, stride 8.55e-8, vec 5.18e-8, and every element of the three maps
    has the bits of the numpy-float32 restatement."""
    from bem import ops
    c = kcase
    outs = []
    for sp in _splits(c["N"]):
        st = _accumulate(c["raw"], c["fin"], c["B"], c["N"], c["h"], c["w"], sp)          # both inputs in one launch
        outs.append(ops.mc_finish(st, mean=False, spread=True)[1:])
    for sd, sm in outs[1:]:
        assert torch.equal(sd, outs[0][0]) and torch.equal(sm, outs[0][1]), c["name"]
    sd, sm = outs[0]
    ref = R.std64(c["fin_np"])
    dev = float(np.abs(sd.cpu().numpy().astype(np.float64) - ref).max())
    same = int((sd.cpu().numpy() == R.run(c["fin_np"], (c["N"],)).std()).sum())
    print(f"{c['name']}: std map vs float64 max|d| {dev:.3e} (bound {4 * R.REF_STD_DEV:.1e}); {same} of {sd.numel()} elements equal the numpy-f32 restatement's bits")
    assert dev <= 4 * R.REF_STD_DEV
    assert sm.dtype == torch.float64 and tuple(sm.shape) == (c["B"],)
    assert np.abs(sm.cpu().numpy() - sd.cpu().numpy().astype(np.float64).mean(axis=(1, 2, 3))).max() < 1e-12


def test_std_survives_cancellation():
    """final = 0.9 + 1e-4 randn, N = 8: Welford in f32 sits near 6e-4 relative (one ulp of 0.9 against a deviation of 1e-4, twice for the
    square); a sum-of-squares accumulator misses by more than 1 (13 on these inputs, tests/test_sample_chunk_cpu.py).  Measured on the
    MI355X: 5.17e-4, the numpy-float32 restatement's own figure."""
    from bem import ops
    c = R.cancellation_inputs()
    fin = torch.from_numpy(c).reshape(8, 3, 16, 16).cuda()
    sd = ops.mc_finish(_accumulate(None, fin, 1, 8, 16, 16, (3, 3, 2)), mean=False, spread=True)[1]
    ref = R.std64(c)
    rel = float((np.abs(sd.cpu().numpy() - ref) / ref).max())
    print(f"cancellation case: relative error of the std map {rel:.2e}")
    assert rel <= 1e-2


def test_one_sample_has_zero_std_and_std_mean_repeats():
    from bem import ops
    _, fin = R.kernel_inputs(4, 2, 5, 17, 21, 17, 21)
    f1 = torch.from_numpy(fin[:, :1]).reshape(2, 3, 17, 21).cuda()
    _, sd, sm = ops.mc_finish(_accumulate(None, f1, 2, 1, 17, 21, (1,)), mean=False, spread=True)
    assert torch.equal(sd, torch.zeros_like(sd)) and torch.equal(sm, torch.zeros_like(sm))
    f5 = torch.from_numpy(fin).reshape(10, 3, 17, 21).cuda()
    a, b = (ops.mc_finish(_accumulate(None, f5, 2, 5, 17, 21, (5,)), mean=False, spread=True)[2] for _ in range(2))
    assert torch.equal(a, b) and float(a.min()) > 0


@pytest.mark.parametrize("hw", [(17, 21), (16, 16)])
@pytest.mark.parametrize("rule", ["max", "min"])
def test_merge_equals_select_scores(rule, hw):
    """Chunks (2,2,1); ties across chunks: candidates 0 and 3 of image 0 are identical (the maximum), candidates 2 and 4 of image 1 share
    the minimum.  The first index wins, as in one select_scores call over all five."""
    from bem import ops
    B, N = 2, 5
    final = torch.rand(B * N, 3, *hw, generator=torch.Generator().manual_seed(1)).cuda()
    final[3] = final[0]
    scores = torch.tensor([0.7, 0.2, 0.5, 0.7, 0.3, 0.3, 0.9, 0.1, 0.3, 0.1]).cuda()
    best, b1, _, img = ops.select_scores(final, scores, N, rule=rule)
    assert best.tolist() == ([0, 1] if rule == "max" else [1, 2])
    run, lo = ops.BestState(B, (3,) + hw, "cuda", rule), 0
    for n in (2, 2, 1):
        ops.select_merge(run, _rows(final, B, N, lo, n), _rows(scores, B, N, lo, n), n)
        lo += n
    assert torch.equal(run.best, best) and torch.equal(run.score, b1) and torch.equal(run.images, img)


# ------------------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def pcase():
    """Reduced-width nets, two 40x52 images (padded to 64x64), N = 5 with injected eps and noise, GT-mean; the single batch, computed once."""
    from bem.pipeline import BEMPipeline, build_nets, synthetic_pair
    net1, net2 = build_nets(n_feat=8, num_blocks=(1, 1, 1), device="cuda")
    B, N = 2, 5
    lq, gt = synthetic_pair((B, 3, 40, 52), seed=13)
    g = torch.Generator().manual_seed(17)
    eps = {(k[:-len("mu_weight")] + "weight" if k.endswith("mu_weight") else k[:-len("mu_bias")] + "bias"): torch.randn((B * N,) + tuple(v.shape), generator=g).cuda()
           for k, v in net1.state_dict().items() if k.endswith(("mu_weight", "mu_bias"))}
    noise = torch.randn(B * N, 3, 4, 4, generator=g).cuda()
    pipe = BEMPipeline(net1, net2, 16, 0.1)
    kw = dict(gt_mean=True, eps=eps, noise=noise)
    ref = pipe.enhance(lq.cuda(), gt.cuda(), N, monte_carlo=True, uncertainty=True, **kw)
    return dict(pipe=pipe, lq=lq.cuda(), gt=gt.cuda(), N=N, B=B, kw=kw, ref=ref)


def _std64(final, B, N):
    return final.double().view(B, N, *final.shape[1:]).std(dim=1, unbiased=True)


def test_chunked_enhance_matches_the_single_batch(pcase):
    """Tolerances of test_full_width_stochastic_mc_vs_oracle (3e-4 on images, 1e-3 dB): the batch size may change which kernel form a row
    takes.  Measured on the MI355X at these shapes: max|d| = 0 for final, conds, psnr, mc and std (the rows took the same kernel forms),
    and the std map 6.05e-8 from float64 of the returned candidates (bound 2.3e-7)."""
    p, ref = pcase, pcase["ref"]
    r = p["pipe"].enhance(p["lq"], p["gt"], p["N"], monte_carlo=True, uncertainty=True, sample_chunk=2, **p["kw"])
    assert "raw" not in r and r["N"] == p["N"] and tuple(r["final"].shape) == tuple(ref["final"].shape) and tuple(r["conds"].shape) == tuple(ref["conds"].shape)
    d = {k: float((r[k] - ref[k]).abs().max()) for k in ("final", "mc", "psnr", "conds", "std")}
    print("sample_chunk=2 vs the single batch, max|d|:", {k: f"{v:.2e}" for k, v in d.items()})
    assert r["best"] == ref["best"]
    assert d["final"] < 3e-4 and d["mc"] < 3e-4 and d["psnr"] < 1e-3
    assert abs(r["mc_psnr"][0] - ref["mc_psnr"][0]) < 1e-3
    if torch.equal(r["final"], ref["final"]):
        assert torch.equal(r["std"], ref["std"]) and torch.equal(r["std_mean"], ref["std_mean"])
    for x in (r, ref):
        dev = float((x["std"].double() - _std64(x["final"], p["B"], p["N"])).abs().max())
        print(f"std vs float64 of the returned candidates: max|d| {dev:.2e}")
        assert dev <= 4 * R.REF_STD_DEV
        assert tuple(x["std"].shape) == (p["B"], 3, 40, 52) and tuple(x["std_mean"].shape) == (p["B"],)


def test_uncertainty_of_fixed_candidates_is_split_invariant(pcase):
    """The single batch's std is one accumulation of its N candidates; the same candidates streamed as (2,2,1) give the same bits."""
    from bem import ops
    p, ref = pcase, pcase["ref"]
    st = _accumulate(None, ref["final"], p["B"], p["N"], 40, 52, (2, 2, 1))
    _, sd, sm = ops.mc_finish(st, mean=False, spread=True)
    assert torch.equal(sd, ref["std"]) and torch.equal(sm, ref["std_mean"])
    st = _accumulate(ref["raw"], None, p["B"], p["N"], 40, 52, (2, 2, 1))
    assert torch.equal(ops.mc_finish(st, p["gt"], True, mean=True)[0], ref["mc"])


def test_chunk_of_all_samples_is_the_single_batch(pcase):
    p, ref = pcase, pcase["ref"]
    for chunk in (5, 7):
        r = p["pipe"].enhance(p["lq"], p["gt"], p["N"], monte_carlo=True, uncertainty=True, sample_chunk=chunk, **p["kw"])
        assert "raw" in r and r["best"] == ref["best"]
        for k in ("final", "psnr", "conds", "mc", "std", "std_mean", "best_images"):
            assert torch.equal(r[k], ref[k]), (chunk, k)


@pytest.mark.parametrize("which", ["psnr", "noref_min"])
def test_keep_best_equals_gathering_from_keep_all(pcase, which):
    from bem import ops
    from bem.scorers import NoReference
    p = pcase
    scorer = None if which == "psnr" else NoReference(lambda f: ops.plane_mean(f.contiguous()).sum(dim=1), "min")
    a = p["pipe"].enhance(p["lq"], p["gt"], p["N"], sample_chunk=2, scorer=scorer, **p["kw"])
    b = p["pipe"].enhance(p["lq"], p["gt"], p["N"], sample_chunk=2, scorer=scorer, keep="best", monte_carlo=True, uncertainty=True, **p["kw"])
    assert not {"final", "conds", "raw"} & set(b) and b["best"] == a["best"]
    rows = torch.tensor(a["best"]) + p["N"] * torch.arange(p["B"])
    assert torch.equal(b["best_images"], a["final"][rows.cuda()]) and torch.equal(b["best_images"], a["best_images"])
    assert torch.equal(b["psnr"], a["psnr"]) and b["best_psnr"] == a["best_psnr"]
    if scorer is not None:
        assert torch.equal(b["scores"], a["scores"]) and b["scores2"] is None
    assert tuple(b["std"].shape) == (p["B"], 3, 40, 52) and tuple(b["mc"].shape) == (p["B"], 3, 40, 52)


def test_deterministic_mode_ignores_the_chunk(pcase):
    p = pcase
    r = p["pipe"].enhance(p["lq"], p["gt"], p["N"], deterministic=True, sample_chunk=2, uncertainty=True)
    assert r["N"] == 1 and torch.equal(r["std"], torch.zeros_like(r["std"])) and torch.equal(r["std_mean"], torch.zeros_like(r["std_mean"]))


def test_refusals_by_name(pcase):
    from bem.scorers import FullReference, UiqmUciqe
    p = pcase
    call = lambda **kw: p["pipe"].enhance(p["lq"], p["gt"], p["N"], **kw)
    for sc in (FullReference(0.5), UiqmUciqe(0.5), UiqmUciqe(1.0)):
        with pytest.raises(ValueError, match=f"keep='best'.*weighted.*{type(sc).__name__}"):
            call(keep="best", scorer=sc, sample_chunk=2)
    with pytest.raises(ValueError, match="shard together with sample_chunk"):
        call(shard=(0, 2), sample_chunk=2)
    with pytest.raises(ValueError, match="sample_chunk must be"):
        call(sample_chunk=0)
    with pytest.raises(ValueError, match="keep must be"):
        call(keep="some")


def test_chunking_saves_memory():
    """128x128, n_feat 16, N = 8, one image; the chunked call first (scratch caches stay grown).  Activations and per-row weight sets scale
    with the rows of a forward, so about a quarter plus the fixed part is expected; less than half is the condition.  Measured on the
    MI355X: 12.7 MiB against 34.9 MiB."""
    from bem.pipeline import BEMPipeline, build_nets, synthetic_pair
    net1, net2 = build_nets(n_feat=16, num_blocks=(1, 1, 1), device="cuda")
    pipe = BEMPipeline(net1, net2, 16, 0.1)
    lq, gt = (t.cuda() for t in synthetic_pair((1, 3, 128, 128), seed=3))
    peaks = []
    for kw in (dict(sample_chunk=2, keep="best"), {}):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        r = pipe.enhance(lq, gt, 8, seed=5, **kw)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - before)
        del r
    print(f"peak allocated above the resident state: sample_chunk=2 keep='best' {peaks[0] / 2**20:.1f} MiB, single batch {peaks[1] / 2**20:.1f} MiB")
    assert peaks[0] < 0.5 * peaks[1]


def test_driver_sample_chunk_and_uncertainty(tmp_path, monkeypatch):
    """Enhancement/eval.py on three 40x52 PNG pairs with reduced-width nets (the option files' widths overridden here): --sample_chunk 2
    --uncertainty writes std/<image>.png of the images' size, Mean_pred_std and pred_std; the same call without the flags has neither."""
    from PIL import Image
    import basicsr.utils.options as bopt
    from bem.pipeline import build_nets, synthetic_pair
    spec = importlib.util.spec_from_file_location("bem_eval_driver_chunk_gpu", os.path.join(PKG, "Enhancement", "eval.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    parse = bopt.parse

    def small(path, is_train=True):
        opt = parse(path, is_train=is_train)
        opt["network_g"].update(n_feat=8, num_blocks=[1, 1, 1])
        return opt
    monkeypatch.setattr(bopt, "parse", small)
    net1, net2 = build_nets(n_feat=8, num_blocks=(1, 1, 1), device="cpu")
    torch.save({"params": net1.state_dict()}, tmp_path / "cg.pth")
    torch.save({"params": net2.state_dict()}, tmp_path / "s2.pth")
    (tmp_path / "in").mkdir(); (tmp_path / "gt").mkdir()
    lq, gt = synthetic_pair((3, 3, 40, 52))
    for i in range(3):
        for d, t in (("in", lq), ("gt", gt)):
            Image.fromarray(np.rint(t[i].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(tmp_path / d / f"{i}.png")
    argv = lambda res: ["--opt", os.path.join(PKG, "Options", "CG_UNet_LOLv1.yml"), "--cond_opt", os.path.join(PKG, "Options", "DecompDualBranch2DDWavelet_4.yml"),
                        "--weights", str(tmp_path / "cg.pth"), "--cond_weights", str(tmp_path / "s2.pth"), "--input_dir", str(tmp_path / "in"),
                        "--target_dir", str(tmp_path / "gt"), "--result_dir", str(tmp_path / res), "--dataset", "synthetic", "--GT_mean",
                        "--num_samples", "4", "--Monte_Carlo", "--seed", "11"]
    out = drv.main(argv("res") + ["--sample_chunk", "2", "--uncertainty"])
    assert sorted(os.listdir(out["result_dir"])) == ["0.png", "1.png", "2.png", "result.txt", "std"]
    assert "Mean_pred_std: " in open(os.path.join(out["result_dir"], "result.txt")).read()
    assert len(out["pred_std"]) == 3 and all(0 < s < 0.5 for s in out["pred_std"]) and len(out["mc_psnr"]) == 3
    for i in range(3):
        im = Image.open(os.path.join(out["result_dir"], "std", f"{i}.png"))
        assert im.size == (52, 40) and im.mode == "L"
    plain = drv.main(argv("res0"))
    assert "pred_std" not in plain and sorted(os.listdir(plain["result_dir"])) == ["0.png", "1.png", "2.png", "result.txt"]
    assert "Mean_pred_std" not in open(os.path.join(plain["result_dir"], "result.txt")).read()
