"""GPU: the averaged weights (train.ema_decay).  bem_ema_update_f32 against float64 with a derived bound; both model classes' steps
against a CPU replay of the reference's ``mul_(decay).add_(p, alpha=1 - decay)`` from the run's own parameter snapshots (Stage I on the
captured-graph path and, in a child process, kernel by kernel); validation on the averaged net with fresh derived weights; checkpoints."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import ema_ref as R
from conftest import PKG, load_golden

pytestmark = pytest.mark.gpu

NS = [1, 3, 4, 5, 63, 64, 65, 255, 257, 4099, (1 << 20) + 3]
GUARD = -7.25          # what the floats around ema hold


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bem import native
    native.lib()
    return torch.device("cuda")


# ------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ------------------------------------------------------------------------------------------------------------------
_DATA = {}


def _data(n):
    """(ema, p) on the CPU: mixed sign, magnitudes log-uniform in [1e-6, 1e3]; made once per n."""
    if n not in _DATA:
        g = torch.Generator().manual_seed(1000 + n % 997)
        mag = lambda: torch.exp(torch.empty(n).uniform_(-13.8155, 6.9078, generator=g)).clamp(1e-6, 1e3) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        _DATA[n] = (mag(), mag())
    return _DATA[n]


@pytest.mark.parametrize("offs", [(0, 0), (1, 0), (0, 2), (3, 3)], ids=["aligned", "ema+1", "p+2", "both+3"])
@pytest.mark.parametrize("decay", [0.0, 0.5, 0.999, 0.9999])
def test_kernel_vs_float64(dev, decay, offs):
    """Every n of the issue at one (decay, misalignment): |got - ref64| <= 2^-23 (|decay ema| + |(1 - decay) p|) per element
    (ema_ref.bound), decay 0 a bit-exact copy, the floats around ema untouched."""
    from bem import ops
    eo, po = offs
    d32, o32 = R.constants(decay)
    for n in NS:
        ema, p = _data(n)
        G = torch.full((n + 16,), GUARD, device=dev)
        P = torch.zeros(n + 8, device=dev)
        e_dev, p_dev = G[4 + eo:4 + eo + n], P[po:po + n]
        assert e_dev.data_ptr() % 16 == 4 * eo and p_dev.data_ptr() % 16 == 4 * po
        e_dev.copy_(ema); p_dev.copy_(p)
        ops.ema_update_(e_dev, p_dev, decay)
        got = G.cpu()
        out = got[4 + eo:4 + eo + n]
        assert bool((got[:4 + eo] == GUARD).all()) and bool((got[4 + eo + n:] == GUARD).all()), (n, "guard floats written")
        assert torch.equal(P[po:po + n].cpu(), p), (n, "p written")
        if decay == 0:
            assert torch.equal(out.view(torch.int32), p.view(torch.int32)), n
        want, mag = R.update_f64(ema, p, d32, o32)
        err = (out.double() - want).abs()
        assert bool((err <= R.bound(mag)).all()), (n, float((err / mag).max()) / R.EPS)


def test_kernel_edge_arguments(dev):
    """n = 0 is a no-op (no launch: nothing changes, null or not); a negative n and null pointers are refused; the wrapper checks
    dtype, device, contiguity and equal numel."""
    from bem import native, ops
    lib = native.lib()
    G, P = torch.full((16,), GUARD, device=dev), torch.ones(16, device=dev)
    ops.ema_update_(G[4:4], P[:0], 0.5)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gp, pp = ctypes.c_void_p(G.data_ptr()), ctypes.c_void_p(P.data_ptr())
    assert lib.bem_ema_update_f32(gp, pp, 0, 0.5, 0.5, st) == 0
    assert lib.bem_ema_update_f32(gp, pp, -1, 0.5, 0.5, st) != 0 and b"ema_update" in lib.bem_last_error()
    assert lib.bem_ema_update_f32(None, pp, 4, 0.5, 0.5, st) != 0 and lib.bem_ema_update_f32(gp, None, 4, 0.5, 0.5, st) != 0
    torch.cuda.synchronize()
    assert bool((G == GUARD).all())
    with pytest.raises(ValueError):
        ops.ema_update_(G[:8], P[:4], 0.5)
    with pytest.raises(ValueError):
        ops.ema_update_(G[::2], P[:8], 0.5)
    with pytest.raises(TypeError):
        ops.ema_update_(G[:8].double(), P[:8], 0.5)
    with pytest.raises(native.BemNativeError):
        ops.ema_update_(G[:8], P[:8].cpu(), 0.5)
    with pytest.raises(ValueError):
        ops.ema_update_(G[:8], P[:8], 1.5)
    assert bool((G == GUARD).all())


# ------------------------------------------------------------------------------------------------------------------
# 2., 3., 5., 6. Stage II
# ------------------------------------------------------------------------------------------------------------------
def _s2_opt(root, ema_decay=0.9, pretrain=None):
    train = dict(total_iter=10, warmup_iter=-1, max_grad_norm=1, use_amp=False,
                 scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=[6, 4], restart_weights=[1, 1], eta_mins=[0.0002, 0.000001]),
                 optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]),
                 pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean"))
    if ema_decay is not None:
        train["ema_decay"] = ema_decay
    return dict(name="s2", model_type="ImageEnhancer", is_train=True, num_gpu=1, dist=False, rank=0, condition=dict(type="mean", scale_down=16, noise_level=0.0),
                network_g=dict(type="DecompDualBranchDDWavelet", in_channels=6, out_channels=3, n_feat=16, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                               mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[2, 1, 1], decomp_model="model4"),
                path=dict(pretrain_network_g=pretrain, strict_load_g=True, resume_state=None, experiments_root=str(root),
                          models=os.path.join(str(root), "models"), training_states=os.path.join(str(root), "training_states")),
                train=train)


def _snapshot(net):
    return {k: v.detach().cpu().clone() for k, v in net.named_parameters()}


def _pair64():
    g = load_golden("g6_ddw")
    lq, gt = g["x"][:, :3].contiguous(), g["gt"]
    return dict(lq=lq, gt=gt, gt_down=F.interpolate(gt, scale_factor=1 / 16, mode="bilinear"))


def _pair32():
    from bem.pipeline import synthetic_pair
    lq, gt = synthetic_pair((1, 3, 32, 32), seed=5)
    return dict(lq=lq, gt=gt, gt_down=F.interpolate(gt, scale_factor=1 / 16, mode="bilinear"))


class _Loader(list):
    dataset = None


def _check_average(model, snaps, start, decay, roundings):
    """Every net_g_ema parameter against the CPU replay: trained ones within roundings * 2^-23 (|ema_ref| + max_t |p_t|), frozen ones
    bit-equal to net_g's; returns the worst error in units of the bound."""
    ref, peak = R.replay(snaps, decay, start)
    trained = {id(p) for f in model.optimizer_g._flat if f is not None for p in f["params"]}
    live = dict(model.net_g.named_parameters())
    worst = 0.0
    for k, q in model.net_g_ema.named_parameters():
        got = q.detach().cpu()
        if id(live[k]) in trained:
            lim = roundings * R.EPS * (ref[k].abs() + peak[k]).double()
            err = (got.double() - ref[k].double()).abs()
            assert bool((err <= lim).all()), (k, float(err.max()), float(lim.min()))
            worst = max(worst, float((err / lim.clamp_min(1e-300)).max()))
        else:
            assert torch.equal(got, live[k].detach().cpu()), k
    return worst


def _check_layout(model):
    """The flat averages have the optimizer's layout (order, 4-float aligned offsets), the averaged net's parameters are views of them,
    and the padding words (where a parameter's size is no multiple of 4) are 0.  Returns the number of padding words."""
    flats = [f for f in model.optimizer_g._flat if f is not None]
    bufs = model.weight_ema.buffers
    assert len(bufs) == len(flats) >= 1
    names = {id(p): k for k, p in model.net_g.named_parameters()}
    ema_p = dict(model.net_g_ema.named_parameters())
    npad = 0
    for buf, f in zip(bufs, flats):
        assert buf.shape == f["p"].shape and buf.data_ptr() != f["p"].data_ptr()
        pad = torch.ones(buf.numel(), dtype=torch.bool)
        off = 0
        for p in f["params"]:
            n = p.numel()
            assert ema_p[names[id(p)]].data_ptr() == buf.data_ptr() + 4 * off and p.data_ptr() == f["p"].data_ptr() + 4 * off
            pad[off:off + n] = False
            off += (n + 3) // 4 * 4
        assert off == buf.numel()
        assert bool((buf.cpu()[pad] == 0).all())
        npad += int(pad.sum())
    return npad


@pytest.fixture(scope="module")
def s2(dev, tmp_path_factory):
    """One Stage-II model with ema_decay = 0.9 after three steps on one 64x64 pair, with the parameter snapshots of those steps."""
    from basicsr.models import build_model
    torch.manual_seed(100)
    model = build_model(_s2_opt(tmp_path_factory.mktemp("s2")))
    start, start_ema = _snapshot(model.net_g), _snapshot(model.net_g_ema)
    snaps = []
    for it in range(3):
        model.feed_train_data(_pair64())
        model.optimize_parameters(it + 1)
        snaps.append(_snapshot(model.net_g))
    return dict(model=model, start=start, start_ema=start_ema, snaps=snaps)


def test_stage2_average_equals_the_cpu_replay(s2):
    model = s2["model"]
    assert all(torch.equal(v, s2["start"][k]) for k, v in s2["start_ema"].items())             # model_ema(0): a copy
    assert not model.net_g_ema.training and model.net_g.training
    moved = max(float((s2["snaps"][-1][k] - v).abs().max()) for k, v in s2["start"].items())
    assert moved > 1e-4                                                                       # the net trained: the average is not trivially p
    _check_average(model, s2["snaps"], s2["start"], 0.9, 3)
    frozen = [k for k, p in model.net_g.named_parameters() if not p.requires_grad]
    assert frozen, "the decomposition is frozen: the test covers parameters outside the optimizer"
    _check_layout(model)


def test_without_ema_decay_nothing_is_built_or_launched(dev, tmp_path, monkeypatch):
    from basicsr.models import build_model
    from bem import ops
    calls = []
    real = ops.ema_update_
    monkeypatch.setattr(ops, "ema_update_", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    torch.manual_seed(100)
    model = build_model(_s2_opt(tmp_path, ema_decay=None))
    model.feed_train_data(_pair32())
    model.optimize_parameters(1)
    model.validation(_Loader([_pair32()]), 1)
    assert not hasattr(model, "net_g_ema") and model.weight_ema is None and calls == []
    model.save(0, 1, best_metric={"psnr": 0, "iter": 1})
    assert set(torch.load(os.path.join(str(tmp_path), "models", "net_g_1.pth"), weights_only=True)) == {"params"}
    # and the counter counts: the same option with the key set launches
    model = build_model(_s2_opt(tmp_path, ema_decay=0.9))
    n0 = len(calls)
    assert n0 >= 1                                                     # copy_from_net
    model.feed_train_data(_pair32())
    model.optimize_parameters(1)
    assert len(calls) == n0 + len(model.weight_ema.buffers)


def test_validation_runs_the_averaged_net_with_fresh_derived_weights(s2):
    """validation -> two more steps -> validation: the second prediction is what a freshly built net gives with net_g_ema's state dict
    (no packed / folded weight of the first validation survives the kernel's writes), and it differs from the first."""
    from basicsr.archs import build_network
    model = s2["model"]
    seen, seen_live = [], []
    h1 = model.net_g_ema.register_forward_hook(lambda m, a, out: seen.append((a[0].clone(), out[-1].clone())))
    h2 = model.net_g.register_forward_hook(lambda m, a, out: seen_live.append(model.net_g.training))
    try:
        val = _Loader([_pair32()])
        ps1 = model.validation(val, 3)
        for it in (4, 5):
            model.feed_train_data(_pair32())
            model.optimize_parameters(it)
        ps2 = model.validation(val, 5)
    finally:
        h1.remove(); h2.remove()
    assert len(seen) == 2 and seen_live == [True, True]            # validation never ran net_g; the steps ran it in train mode
    assert model.net_g.training and not model.net_g_ema.training
    (x1, p1), (x2, p2) = seen
    assert torch.equal(x1, x2) and not torch.equal(p1, p2) and ps1 != ps2
    fresh = build_network(model.opt["network_g"]).to(x2.device).eval()
    fresh.load_state_dict(model.net_g_ema.state_dict())
    with torch.no_grad():
        p3 = fresh(x2)[-1]
    assert torch.equal(p2, p3), float((p2 - p3).abs().max())
    assert model.metric_results["psnr"] == ps2


def test_checkpoints_hold_both_copies_and_restore_them(s2, tmp_path):
    from basicsr.archs import build_network
    from basicsr.models import build_model
    model = s2["model"]
    model.save(0, 7, best_metric={"psnr": 1.0, "iter": 7})
    path = os.path.join(model.opt["path"]["models"], "net_g_7.pth")
    ck = torch.load(path, weights_only=True)
    assert set(ck) == {"params", "params_ema"}
    live, avg = model.net_g.state_dict(), model.net_g_ema.state_dict()
    assert all(torch.equal(ck["params"][k], v.cpu()) for k, v in live.items()) and all(torch.equal(ck["params_ema"][k], v.cpu()) for k, v in avg.items())
    assert any(not torch.equal(ck["params"][k], ck["params_ema"][k]) for k in ck["params"])
    again = build_model(_s2_opt(tmp_path, pretrain=path))            # what --auto_resume builds: pretrain_network_g -> net_g_<iter>.pth
    assert all(torch.equal(v.cpu(), ck["params"][k]) for k, v in again.net_g.state_dict().items())
    assert all(torch.equal(v.cpu(), ck["params_ema"][k]) for k, v in again.net_g_ema.state_dict().items())
    assert not again.net_g_ema.training
    best = model.save_best({"psnr": 12.345, "iter": 7})
    bk = torch.load(best, weights_only=True)
    assert set(bk) == {"params", "params_ema"} and all(torch.equal(bk["params_ema"][k], v) for k, v in ck["params_ema"].items())
    assert all(torch.equal(bk["params"][k], v) for k, v in ck["params"].items())
    spec = importlib.util.spec_from_file_location("bem_eval_driver", os.path.join(PKG, "Enhancement", "eval.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    net = build_network(model.opt["network_g"])
    drv.load_params(net, path, "params_ema")
    assert all(torch.equal(v, ck["params_ema"][k]) for k, v in net.state_dict().items())
    drv.load_params(net, path)
    assert all(torch.equal(v, ck["params"][k]) for k, v in net.state_dict().items())


# ------------------------------------------------------------------------------------------------------------------
# 4. Stage I: captured graph, and kernel by kernel in a child process
# ------------------------------------------------------------------------------------------------------------------
def _cg_opt(mini_batch):
    """The option of the Stage-I training tests (tests/test_train_gpu.py, _cg_opt) with periods = [2, 8] and ema_decay = 0.9."""
    return dict(name="cg", model_type="ConditionGenerator", is_train=True, num_gpu=1, dist=False, rank=0, sigma_init=0.05, selective=True,
                condition=dict(type="mean", scale_down=16, noise_level=0.1),
                datasets=dict(train=dict(mini_batch_sizes=[mini_batch])),
                network_g=dict(type="Network", in_channels=3, out_channels=3, n_feat=16, d_state=[1, 1, 1], ssm_ratio=1, mlp_ratio=4,
                               mlp_type="gdmlp", use_pixelshuffle=True, drop_path=0.0, sam=False, stage=1, num_blocks=[2, 1, 1]),
                path=dict(pretrain_network_g=None, strict_load_g=True, resume_state=None),
                train=dict(total_iter=10, warmup_iter=-1, max_grad_norm=1, use_amp=False, mixing_augs=dict(mixup=False), ema_decay=0.9,
                           scheduler=dict(type="CosineAnnealingRestartCyclicLR", periods=[2, 8], restart_weights=[1, 1], eta_mins=[0.0002, 0.000001]),
                           optim_g=dict(type="AdamW", lr=2e-4, weight_decay=1e-4, betas=[0.9, 0.999]),
                           pixel_opt=dict(type="L1Loss", loss_weight=1, reduction="mean")))


def _stage1_run():
    """Four steps (two with the MIM mask, two past the first scheduler period) on whichever path the environment selects; the average
    is checked against the replay of this run's own snapshots.  Returns what the caller asserts about the path."""
    from basicsr.models import build_model
    g = load_golden("g11_stage1_train")
    torch.manual_seed(100)
    model = build_model(_cg_opt(int(g["mini_batch"])))
    start = _snapshot(model.net_g)
    assert all(torch.equal(v, start[k]) for k, v in _snapshot(model.net_g_ema).items())
    snaps = []
    for it in range(4):
        model.feed_train_data(dict(lq_down=g["lq"], gt=g["gt"], gt_down=g["gt"], mask=g["mask"]))
        model.optimize_parameters(it + 1)
        snaps.append(_snapshot(model.net_g))
    torch.cuda.synchronize()
    worst = _check_average(model, snaps, start, 0.9, 4)
    tok = "mask_token"
    assert torch.equal(snaps[2][tok], snaps[1][tok]) and torch.equal(snaps[3][tok], snaps[1][tok])       # skipped by AdamW after the period ...
    assert not torch.equal(snaps[1][tok], start[tok])
    avg_tok = dict(model.net_g_ema.named_parameters())[tok].detach().cpu()
    two, _ = R.replay(snaps[:2], 0.9, start)
    assert not torch.equal(avg_tok, two[tok])                                                                 # ... and still averaged
    moved = max(float((snaps[-1][k] - v).abs().max()) for k, v in start.items())
    captured = [x for x in getattr(model, "_graphs", {}).values() if isinstance(x, dict)]
    npad = _check_layout(model)
    assert npad > 0, "the Stage-I net's PReLU slopes are single floats: their slots end in padding words"
    return dict(worst=worst, graphs=len(captured), moved=moved)


def test_stage1_average_on_the_graph_path(dev, monkeypatch):
    monkeypatch.setenv("BEM_STAGE1_GRAPH", "1")
    r = _stage1_run()
    assert r["graphs"] == 2 and r["moved"] > 1e-4            # with and without the mask: each replay carries the averaging node


def test_stage1_average_kernel_by_kernel_in_a_child_process(dev):
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import test_ema_gpu as t; r = t._stage1_run(); "
            "assert r['graphs'] == 0 and r['moved'] > 1e-4, r; print('EMA_CHILD_OK', r['worst'])")
    env = dict(os.environ, BEM_STAGE1_GRAPH="0")
    r = subprocess.run([sys.executable, "-c", code, os.path.dirname(os.path.abspath(__file__))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "EMA_CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
