"""QD model3 in train() mode on the device: the attention dropout of QD/model3.py:98,124-131 inside the fold kernel
(csrc/chan_attn.hip, bem_attn_fold_drop_f32) -- against the reference's own run with its masks injected (tests/golden/g19_model3_train*.npz),
against the float64 restatement of tests/model3_train_ref.py, draw for draw against the CPU model of the in-kernel Philox keep flags, and
bit for bit against the eval form where the dropout is off."""
import ctypes
import glob
import os

import pytest
import torch

import model3_train_ref as R
from conftest import GOLDEN, PKG, load_golden
from model3_train_ref import SEED, STREAM

pytestmark = pytest.mark.gpu

P_DROP = 0.1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bem import native
    native.lib()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def g19():
    g = load_golden("g19_model3_train")
    for path in sorted(glob.glob(os.path.join(GOLDEN, "g19_model3_train_p*.npz"))):
        for k, v in load_golden(os.path.basename(path)[:-4]).items():
            g.setdefault(k, {}).update(v)
    assert set(g["sd"]) == set(g["grads"]) == set(g["params"])
    return g


def close(a, b, rtol, atol, what=""):
    """torch.allclose with the error in the message; returns max |a - b|."""
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite"
    err = float((a - b).abs().max())
    assert torch.allclose(a, b, rtol=rtol, atol=atol), f"{what}: max abs err {err:.3e} (ref max {float(b.abs().max()):.3e})"
    return err


@pytest.fixture(scope="module")
def case(dev):
    """B = 3, 6 x 10 pixels: float32-representable inputs, their device copies, the f64 statistics of the device (computed once: every
    fold below reads the same ones) and the float64 restatement with the mask applied at the softmax."""
    from bem import native
    f1, f2, w, fw, fb, mask = R.random_case(3, 6, 10, seed=1, p=P_DROP)
    f1, f2, fw, fb = (t.float().double() for t in (f1, f2, fw, fb))
    w = {n: (a.float().double(), b.float().double()) for n, (a, b) in w.items()}
    d = dict(f1=f1.float().to(dev), f2=f2.float().to(dev), aw=R.pack_attn_w(w).to(dev), fw=fw.float().contiguous().to(dev), fb=fb.float().to(dev),
             mask=mask.float().to(dev))
    stats = torch.empty(3, 32 * 32 + 64, device=dev, dtype=torch.float64)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    native.check(native.lib().bem_attn_stats_f64(vp(d["f1"]), vp(d["f2"]), vp(stats), 3, 60, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return dict(f1=f1, f2=f2, w=w, fw=fw, fb=fb, mask=mask, dev=d, stats=stats)


def fold_raw(case, B=3, plain=False, mask=None, p=0.0, seed=0, stream_id=0):
    """(Wn (B,32,64), bias (B,32)) on the host from the C ABI itself, images 0 .. B - 1 of the case."""
    from bem import native
    d, dev = case["dev"], case["stats"].device
    Wn = torch.full((B, 32, 64), float("nan"), device=dev)
    bias = torch.full((B, 32), float("nan"), device=dev)
    vp = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if plain:
        rc = native.lib().bem_attn_fold_f32(vp(case["stats"]), vp(d["aw"]), vp(d["fw"]), vp(d["fb"]), vp(Wn), vp(bias), B, 60, s)
    else:
        rc = native.lib().bem_attn_fold_drop_f32(vp(case["stats"]), vp(d["aw"]), vp(d["fw"]), vp(d["fb"]), vp(mask), p, seed, stream_id, vp(Wn), vp(bias), B, 60, s)
    native.check(rc, "attn_fold")
    return Wn.cpu(), bias.cpu()


# ---------------------------------------------------------------------------------------------- 1. what failed before
def test_model3_runs_in_train_mode(dev, g19):
    """Decomp model3 in train() mode raised BemNativeError in its full-resolution form; so did the first training forward of
    Options/DecompDualBranch_3.yml's network."""
    from basicsr.archs import build_network
    from basicsr.utils.options import parse
    from bem.archs import Decomp
    img = g19["img"].to(dev)
    q = Decomp.from_shipped("model3", wavelet_out=False).to(dev).train()(img)
    assert q.shape == (2, 8, 32, 40) and torch.isfinite(q).all()
    opt = parse(os.path.join(PKG, "Options", "DecompDualBranch_3.yml"), is_train=True)
    assert opt["network_g"]["decomp_model"] == "model3"
    torch.manual_seed(3)
    net = build_network(dict(opt["network_g"], n_feat=8, num_blocks=[1, 1, 1])).to(dev).train()
    assert net.decomp.training and net.decomp.cross_attn.p == P_DROP
    x = torch.rand(1, 6, 32, 32, generator=torch.Generator().manual_seed(4)).to(dev)
    out = net(x)[-1]
    assert out.shape == (1, 3, 32, 32) and torch.isfinite(out).all() and out.requires_grad


# ---------------------------------------------------------------------------------------------- 2. the reference's own run
def test_injected_masks_match_the_reference(dev, g19):
    """create_my_decomp('model3') and model3.Decomp of the reference in train() mode, with the masks its dropout drew injected here.
    Tolerance: rtol 2e-4, atol 2e-5, what test_modules_gpu.py::test_decomp_model2_model3_golden allows the eval-mode outputs (the masked
    fold is the same arithmetic plus one scaling).  The fixture's own eval-mode maps lie outside that tolerance, so a run without the
    dropout does not pass."""
    from bem.archs import AttnDrop, Decomp
    img = g19["img"].to(dev)
    errs = {}
    for wav, keys, mkey, ekey in ((True, ("q1w", "q2w"), "mask_w", "q1w_eval"), (False, ("q1", "q2"), "mask_full", "q1_eval")):
        d = Decomp.from_shipped("model3", wavelet_out=wav).to(dev).train()
        d.attn_drop = AttnDrop(masks=[g19[mkey].to(dev)])
        out = d(img).cpu()
        assert d.attn_drop.calls == 1
        h = out.shape[1] // 2
        errs[keys[0]] = close(out[:, :h], g19[keys[0]], 2e-4, 2e-5, keys[0])
        errs[keys[1]] = close(out[:, h:], g19[keys[1]], 2e-4, 2e-5, keys[1])
        assert not torch.allclose(g19[ekey].double(), g19[keys[0]].double(), rtol=2e-4, atol=2e-5)
        d.eval()
        ev = d(img).cpu()
        close(ev[:, :h], g19[ekey], 2e-4, 2e-5, ekey)
        assert d.attn_drop.calls == 1                                    # eval() takes nothing from the record
    print("model3 train() vs reference, max |err|: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))


# ---------------------------------------------------------------------------------------------- 3. float64 restatement
def test_masked_fold_kernel_vs_float64(dev, case):
    """ops.attn_fold(..., drop=(0.1, mask)) + the x6 GEMM on B = 3, 6 x 10 against the float64 restatement (model3_train_ref.folded, which
    test_model3_train_cpu.py ties to the module written out).  Bound on the fused map: rtol 2e-4, atol 2e-5, the bound
    test_modules_gpu.py::test_decomp_model2_model3_golden puts on the decomposition built around the eval fold.  The folded matrix and bias
    themselves: the kernel evaluates them in f64 from f64 statistics of the same f32 inputs and rounds once to f32 (2^-24 relative); 1e-6
    relative + 1e-7 of the largest entry leaves a factor 16 for the conditioning of the softmax."""
    from bem import ops
    d = case["dev"]
    Wb, bias = R.folded(case["f1"], case["f2"], case["w"], case["fw"], case["fb"], case["mask"], P_DROP)
    want = R.apply_folded(Wb, bias, case["f1"], case["f2"])
    Wp, bd = ops.attn_fold(d["f1"], d["f2"], d["aw"], d["fw"], d["fb"], drop=(P_DROP, d["mask"]))
    got = ops.pw_gemm(d["f1"], Wp, 32, x2=d["f2"], in_mode=2, bias=bd)
    err = close(got, want, 2e-4, 2e-5, "fused map")
    Wn, bn = fold_raw(case, mask=d["mask"], p=P_DROP)
    eW = close(Wn, Wb, 1e-6, 1e-7 * float(Wb.abs().max()), "W_b")
    eb = close(bn, bias, 1e-6, 1e-7 * float(bias.abs().max()), "bias_b")
    assert torch.equal(bd.cpu(), bn)
    print(f"masked fold vs float64: fused map {err:.3e}, W_b {eW:.3e}, bias_b {eb:.3e}")
    # the mask is applied: the unmasked restatement is far outside the bound
    plain = R.apply_folded(*R.folded(case["f1"], case["f2"], case["w"], case["fw"], case["fb"]), case["f1"], case["f2"])
    assert not torch.allclose(got.cpu().double(), plain, rtol=2e-4, atol=2e-5)


# ---------------------------------------------------------------------------------------------- 4. the in-kernel draw
def test_philox_keep_flags_draw_for_draw(dev, case):
    """The keep flags the kernel draws under (seed, stream id) are those of the CPU model (model3_train_ref.keep_mask on philox_ref): the
    fold with the drawn flags and the fold with the model's flags injected give the same bits.  A wrong flag moves 1 of 1024 entries of a
    softmaxed map by all of its value."""
    from bem import ops
    d = case["dev"]
    model = torch.from_numpy(R.keep_mask(3, P_DROP, SEED, STREAM))
    assert 0.85 < float(model.mean()) < 0.95
    drawn = fold_raw(case, p=P_DROP, seed=SEED, stream_id=STREAM)
    inject = fold_raw(case, mask=model.to(dev), p=P_DROP)
    assert torch.equal(drawn[0], inject[0]) and torch.equal(drawn[1], inject[1])
    again = fold_raw(case, p=P_DROP, seed=SEED, stream_id=STREAM)
    assert torch.equal(drawn[0], again[0]) and torch.equal(drawn[1], again[1])
    one = fold_raw(case, B=1, p=P_DROP, seed=SEED, stream_id=STREAM)                   # image 0 alone: the draw does not depend on B
    assert torch.equal(one[0], drawn[0][:1]) and torch.equal(one[1], drawn[1][:1])
    for seed, sid in ((SEED, STREAM + 1), (SEED, STREAM ^ (1 << 40)), (SEED + 1, STREAM), (SEED + (1 << 32), STREAM)):
        other = fold_raw(case, p=P_DROP, seed=seed, stream_id=sid)
        assert not torch.equal(other[0], drawn[0]), (seed, sid)
        m = torch.from_numpy(R.keep_mask(3, P_DROP, seed, sid))
        via = fold_raw(case, mask=m.to(dev), p=P_DROP)
        assert torch.equal(other[0], via[0]) and torch.equal(other[1], via[1]), (seed, sid)
    # the same through bem.ops
    a = ops.attn_fold(d["f1"], d["f2"], d["aw"], d["fw"], d["fb"], drop=(P_DROP, SEED, STREAM))
    b = ops.attn_fold(d["f1"], d["f2"], d["aw"], d["fw"], d["fb"], drop=(P_DROP, model.to(dev)))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------- 5. eval unchanged
def test_eval_form_is_unchanged(dev, case, g19, monkeypatch):
    from bem import native, ops
    from bem.archs import Decomp
    d = case["dev"]
    base = fold_raw(case, plain=True)
    for kw in (dict(p=0.0, seed=SEED, stream_id=STREAM), dict(p=0.0, mask=torch.ones(3, 2, 32, 32, device=dev))):
        got = fold_raw(case, **kw)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), kw
    ref = ops.attn_fold(d["f1"], d["f2"], d["aw"], d["fw"], d["fb"])
    for drop in (None, (0.0, SEED, STREAM), (0.0, torch.ones(3, 2, 32, 32, device=dev))):
        got = ops.attn_fold(d["f1"], d["f2"], d["aw"], d["fw"], d["fb"], drop=drop)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    # operand checks of the new argument
    for bad, exc in (((1.0, SEED, STREAM), ValueError), ((-0.1, SEED, STREAM), ValueError), ((0.1,), ValueError),
                     ((0.1, torch.ones(3, 2, 32, 32)), native.BemNativeError), ((0.1, torch.ones(3, 2, 32, 32, device=dev, dtype=torch.float64)), TypeError),
                     ((0.1, torch.ones(2, 2, 32, 32, device=dev)), ValueError), ((0.1, torch.ones(3, 2, 32, 64, device=dev)[..., ::2]), ValueError)):
        with pytest.raises(exc):
            ops.attn_fold(d["f1"], d["f2"], d["aw"], d["fw"], d["fb"], drop=bad)
    with pytest.raises(native.BemNativeError):
        fold_raw(case, p=1.0, seed=SEED, stream_id=STREAM)
    # eval() forwards of model3: no drop reaches the fold, and the output is that of ops.attn_fold called the way the parent called it
    img = g19["img"].to(dev)
    orig, seen = ops.attn_fold, []

    def spy(*a, drop=None, **k):
        seen.append(drop)
        return orig(*a, drop=drop, **k)

    def parent(*a, drop=None, **k):
        return orig(*a, **k)
    for wav in (True, False):
        m = Decomp.from_shipped("model3", wavelet_out=wav).to(dev)
        assert not m.training
        monkeypatch.setattr(ops, "attn_fold", spy)
        out = m(img)
        m.train()
        tr = m(img)
        monkeypatch.setattr(ops, "attn_fold", parent)
        assert torch.equal(m.eval()(img), out) and torch.equal(m.train()(img), out)      # train() without the drop = eval
        assert not torch.equal(tr, out)
    assert [s is None for s in seen] == [True, False, True, False]


# ---------------------------------------------------------------------------------------------- 6. two training steps
def test_two_training_steps_match_the_reference(dev, g19):
    """ImageEnhancer.optimize_parameters with DecompDualBranch + model3 (n_feat 16, one block per level) and the reference's masks injected,
    against the reference's own two steps (its modules, torch.optim.AdamW, clip 1; tests/golden/make_golden_model3_train.py).  Tolerances:
    loss 3e-6 and gradient norm 5e-4 relative as test_train_gpu.py::test_dualbranch_train_step_matches_oracle; every gradient of step 1 to
    5e-3 of its own largest entry + 1e-5 of the net's largest as test_stage2_training_gradients_golden holds the g6 / g10 fixtures;
    the updated parameters by test_dualbranch_train_step_matches_oracle's rule (every update within one full Adam step pair, all but 1 %
    within 5 % + 2e-6)."""
    from basicsr.models import build_model
    from bem import autograd as ag
    from bem.archs import AttnDrop
    opt = dict(model_type="ImageEnhancer", is_train=True, num_gpu=1, dist=False, condition=dict(type="mean", scale_down=16, noise_level=0.0),
               network_g=dict(type="DecompDualBranch", in_channels=6, out_channels=3, n_feat=16, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                              mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[1, 1, 1], decomp_model="model3"),
               path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None),
               train=dict(total_iter=10, warmup_iter=-1, max_grad_norm=1, use_amp=False,
                          scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=[6, 4], restart_weights=[1, 1], eta_mins=[0.0002, 0.000001]),
                          optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]),
                          pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean")))
    sd0 = g19["sd"]
    model = build_model(opt)
    model.net_g.load_state_dict(sd0, strict=False)
    named = {k: p for k, p in model.net_g.named_parameters() if p.requires_grad}
    assert set(named) == set(sd0)
    masks = [g19["step_masks"][i].to(dev).contiguous() for i in range(2)]
    batch = dict(lq=g19["lq"], gt=g19["gt"], gt_down=g19["gt_down"])
    # every gradient of step 1
    model.feed_train_data(batch)
    model.optimizer_g.zero_grad()
    model.net_g.decomp.attn_drop = AttnDrop(masks=masks[:1])
    loss = ag.l1_loss(model.net_g(model._net_input())[-1], model.gt)
    model.net_g.decomp.attn_drop = None
    loss.backward()
    assert abs(float(loss.detach()) - float(g19["loss"][0])) < 3e-6, (float(loss.detach()), float(g19["loss"][0]))
    gmax = max(float(v.abs().max()) for v in g19["grads"].values())
    for k, ref in g19["grads"].items():
        err = float((named[k].grad.cpu().double() - ref.double()).abs().max())
        assert err <= 5e-3 * float(ref.abs().max()) + 1e-5 * gmax, f"gradient {k}: max|err| {err:.3e} vs max|ref| {float(ref.abs().max()):.3e}"
    # the two steps
    for it in range(2):
        model.attn_drop_masks = masks[it:it + 1]
        model.feed_train_data(batch)
        tn = model.optimize_parameters(it + 1)
        assert model.net_g.decomp.attn_drop is None
        lr, nr = float(g19["loss"][it]), float(g19["grad_norm"][it])
        assert abs(float(model.log_dict["l_pix"]) - lr) < 3e-6, (it, float(model.log_dict["l_pix"]), lr)
        assert abs(float(tn) - nr) < 5e-4 * nr, (it, float(tn), nr)
    bad = tot = 0
    for k, v in g19["params"].items():
        u_ref, u_dev = (v - sd0[k]).double(), (named[k].detach().cpu() - sd0[k]).double()
        assert float((u_dev - u_ref).abs().max()) <= 2 * 2 * 2e-4 * 1.05, k
        bad += int(((u_dev - u_ref).abs() > 0.05 * u_ref.abs() + 2e-6).sum())
        tot += v.numel()
    assert bad <= 0.01 * tot, f"{bad} of {tot} parameter updates differ from the reference's"


# ---------------------------------------------------------------------------------------------- 7. resume
def _run_driver(root, yml, total, auto_resume=False):
    from basicsr.train import train_pipeline
    argv = ["--opt", os.path.join(PKG, "Options", yml), "--synthetic", "4",
            "--force_yml", "network_g:n_feat=16", "network_g:num_blocks=[1,1,1]", f"train:total_iter={total}", "logger:save_checkpoint_freq=3",
            "logger:print_freq=1", "datasets:train:batch_size_per_gpu=2", "datasets:train:gt_size=64", "train:scheduler:periods=[4,4,4]"]
    if auto_resume:
        argv.append("--auto_resume")
    torch.manual_seed(100)
    return train_pipeline(str(root), argv=argv)


def test_training_driver_resume_continues_the_dropout_sequence(dev, tmp_path):
    """basicsr/train.py on Options/DecompDualBranch_3.yml at reduced width, the pattern of
    test_train_gpu.py::test_training_driver_save_resume_reproduces_the_run: 6 iterations without a break against 3 + a resumed 3.  The
    dropout draws are a function of (manual_seed, rank, iteration), so the resumed run ends on the parameters of the uninterrupted one; a
    resumed run that replayed the masks of iterations 1-3 would differ by about one learning rate (2e-4) per step."""
    yml, first, total = "DecompDualBranch_3.yml", 3, 6
    a, ia = _run_driver(tmp_path / "A", yml, total)
    assert a.net_g.decomp.model == "model3" and a.net_g.decomp.training
    b0, _ = _run_driver(tmp_path / "B", yml, first)
    assert (tmp_path / "B" / "experiments" / yml[:-4] / "training_states" / f"{first}.state").is_file()
    del b0
    b, ib = _run_driver(tmp_path / "B", yml, total, auto_resume=True)
    assert ia["iter"] == ib["iter"] == total
    assert a.get_current_learning_rate() == b.get_current_learning_rate()
    pa, pb = dict(a.net_g.named_parameters()), dict(b.net_g.named_parameters())
    worst = max(float((pa[k].detach() - pb[k].detach()).abs().max()) for k in pa)
    assert worst <= 4e-5, worst
