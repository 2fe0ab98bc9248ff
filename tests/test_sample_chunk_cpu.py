"""CPU: sample-chunked evaluation without a GPU -- the C ABI of the streamed Monte-Carlo statistics and of the selection merge rejects bad
arguments before any HIP call, the eval driver refuses bad --sample_chunk / --keep_best combinations before any model work, and the numpy
restatement the GPU test measures against (tests/mc_stream_ref.py) is chunk-invariant and within its stated distance of float64."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import mc_stream_ref as R
from conftest import PKG


def _ops():
    from bem import native, ops
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return ops, native.BemNativeError


def test_abi_rejects_before_any_hip_call():
    ops, Err = _ops()
    lib, check = ops.lib(), ops.check
    p, B, Nc, h, w = 16, 2, 3, 5, 7         # any non-null value: the checks reject before a pointer is touched

    def accum(raw=p, fin=p, s=p, m=p, q=p, B=B, Nc=Nc, n_done=0, Hp=8, Wp=8, h=h, w=w):
        check(lib.bem_mc_accum_f32(raw, fin, s, m, q, B, Nc, n_done, Hp, Wp, h, w, None), "mc_accum")
    for bad, word in ((dict(raw=None, fin=None), "null"), (dict(s=None), "null sum"), (dict(q=None), "null mean / m2"), (dict(h=9), "bad shape"),
                      (dict(Nc=0), "Nc=0"), (dict(n_done=-1), "n_done=-1"), (dict(B=65536), "B=65536")):
        with pytest.raises(Err, match=word):
            accum(**bad)

    def finish(s=p, q=p, t=p, mc=p, sd=p, sm=p, ws=p, B=B, N=4, h=h, w=w, gm=1):
        check(lib.bem_mc_finish_f32(s, q, t, mc, sd, sm, ws, B, N, h, w, gm, None), "mc_finish")
    for bad, word in ((dict(mc=None, sd=None), "null outputs"), (dict(s=None), "sum plane"), (dict(q=None), "m2 plane"),
                      (dict(s=None, q=None), "plane"), (dict(ws=None), "workspace"), (dict(N=0), "N=0"), (dict(B=65536), "B=65536"),
                      (dict(t=None), "GT-mean")):
        with pytest.raises(Err, match=word):
            finish(**bad)

    def merge(c=p, sc=p, rule=1, best=p, bs=p, img=p, pick=p, B=B, Nc=Nc, n_done=0):
        check(lib.bem_select_merge_f32(c, sc, rule, best, bs, img, pick, B, Nc, n_done, 3 * h * w, None), "select_merge")
    for bad, word in ((dict(sc=None), "null"), (dict(pick=None), "null"), (dict(rule=0), "rule 0"), (dict(Nc=0), "Nc=0"),
                      (dict(n_done=-2), "n_done=-2"), (dict(B=65536), "B=65536"), (dict(img=None), "go together")):
        with pytest.raises(Err, match=word):
            merge(**bad)


def test_ops_refuse_cpu_tensors_and_bad_states():
    ops, Err = _ops()
    st = ops.McState(1, 4, 4, "cpu", mean=True, spread=True)
    with pytest.raises(Err):
        ops.mc_accum(st, torch.zeros(2, 3, 4, 4), None, 2)
    with pytest.raises(ValueError, match="no samples"):
        ops.mc_finish(st, mean=True)
    with pytest.raises(ValueError, match="no plane"):
        ops.mc_accum(ops.McState(1, 4, 4, "cpu", mean=True), None, torch.zeros(1, 3, 4, 4), 1)
    with pytest.raises(ValueError, match="65535"):
        ops.McState(65536, 1, 1, "meta", mean=True)
    with pytest.raises(ValueError, match="weighted"):
        ops.BestState(1, (3, 4, 4), "cpu", "weighted")


def test_keep_best_rule_table():
    """Which selection rules keep='best' follows, and that the others are refused by name."""
    from bem.pipeline import _online_rule
    from bem.scorers import FullReference, NoReference, UiqmUciqe
    assert _online_rule(None) == "max" and _online_rule(FullReference(1.0)) == "max"
    assert _online_rule(NoReference(lambda f: f, "min")) == "min" and _online_rule(NoReference(lambda f: f, "max")) == "max"
    for sc in (FullReference(0.5), UiqmUciqe(0.5), UiqmUciqe(1.0), UiqmUciqe(0.0)):
        with pytest.raises(ValueError, match=f"keep='best'.*'weighted'.*{type(sc).__name__}"):
            _online_rule(sc)


def _driver():
    spec = importlib.util.spec_from_file_location("bem_eval_driver_chunk", os.path.join(PKG, "Enhancement", "eval.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    return drv


@pytest.mark.parametrize("argv,flag", [(["--sample_chunk", "0"], "--sample_chunk"), (["--sample_chunk", "x"], "--sample_chunk"),
                                       (["--keep_best", "--psnr_weight", "0.5", "--target_dir", "gt"], "--keep_best"),
                                       (["--keep_best", "--no_ref", "uiqm_uciqe"], "--keep_best"),
                                       (["--uncertainty", "--std_white", "0"], "--std_white")])
def test_driver_refuses_by_flag(argv, flag):
    """Checked before any option file is read: the default --opt does not exist, so getting past the check would fail differently."""
    with pytest.raises(SystemExit) as e:
        _driver().main(argv)
    assert isinstance(e.value.code, str) and e.value.code.startswith(flag), e.value.code


def test_driver_new_flags_default_off():
    a = _driver().get_parser().parse_args([])
    assert a.sample_chunk == "" and a.uncertainty is False and a.keep_best is False and a.std_white == 0.25 and a.parallel_num == 1


def test_restatement_chunk_invariant_and_close_to_float64():
    raw, fin = R.kernel_inputs()
    runs = [R.run(fin, sp, raw) for sp in ((5,), (2, 2, 1), (1, 1, 1, 1, 1))]
    for r in runs[1:]:
        assert np.array_equal(r.std(), runs[0].std()) and np.array_equal(r.mc(), runs[0].mc()) and np.array_equal(r.mean, runs[0].mean)
    dev = float(np.abs(runs[0].std().astype(np.float64) - R.std64(fin)).max())
    print(f"f32 Welford vs float64 std: max|d| {dev:.3e} (stated {R.REF_STD_DEV:.1e})")
    assert dev <= R.REF_STD_DEV
    # the clamp matters on these inputs, and the mean of the clamped crops is what mc holds
    assert (raw < 0).any() and (raw > 1).any()
    assert np.abs(runs[0].mc() - np.clip(raw[..., :17, :21], 0, 1).astype(np.float64).mean(axis=1)).max() < 3e-7
    assert np.array_equal(R.run(fin[:, :1], (1,)).std(), np.zeros((2, 3, 17, 21), np.float32))


def test_restatement_survives_cancellation_where_sum_of_squares_does_not():
    c = R.cancellation_inputs()
    ref = R.std64(c)
    rel = float((np.abs(R.run(c, (8,)).std() - ref) / ref).max())
    f = np.float32
    s1, s2 = np.zeros(c.shape[2:], f)[None], np.zeros(c.shape[2:], f)[None]
    for n in range(c.shape[1]):
        s1, s2 = s1 + c[:, n], s2 + c[:, n] * c[:, n]
    naive = np.sqrt(np.maximum((s2 - s1 * s1 / f(8)) / f(7), 0))
    rel_naive = float((np.abs(naive - ref) / ref).max())
    print(f"relative error of the std map at mean 0.9, std 1e-4: Welford f32 {rel:.2e}, sum of squares f32 {rel_naive:.2e}")
    assert rel <= 1e-2 < 1 <= rel_naive
