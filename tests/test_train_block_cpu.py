"""CPU: the host side of the train block -- ``optim_g.type: Adam``, ``pixel_opt.type: MSELoss / CharbonnierLoss`` and the reference's
schedulers.  The schedulers against the learning rates the reference's own classes produced (tests/golden/g20_schedules.npz, written by
tests/golden/make_golden_schedules.py) through BaseModel.setup_schedulers / update_learning_rate; the registry entries and constructor
signatures of the two losses; every refusal by name; the new ABI entries in the derived binding."""
import copy
import ctypes
import inspect
import json

import numpy as np
import pytest
import torch

from conftest import load_golden


@pytest.fixture(scope="module")
def schedules():
    g = load_golden("g20_schedules")
    return json.loads(str(g["configs"])), {k: v.double().numpy() for k, v in g["lr"].items()}, float(g["base_lr"][0])


NAMES = ["multistep_repeated", "multistep_restart", "cosine_uneven", "cosine_even", "cosine_uneven_warmup", "linear_300", "linear_257",
         "vibrate_400", "vibrate_960"]


def _model(train, base_lr):
    """A BaseModel with one SGD optimizer over a CPU parameter (the dummy the fixture was recorded with) and its scheduler set up."""
    from basicsr.models.base_model import BaseModel
    m = BaseModel({"num_gpu": 0, "is_train": True, "train": copy.deepcopy(train)})
    m.optimizers = [torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base_lr)]
    m.setup_schedulers()
    return m


def _one_ulp(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want) <= np.spacing(np.abs(want))


def test_fixture_covers_what_it_should(schedules):
    cfg, lr, base = schedules
    assert sorted(cfg) == sorted(NAMES) == sorted(lr) and base == 2e-4
    kinds = [cfg[k]["train"]["scheduler"]["type"] for k in NAMES]
    assert {k: kinds.count(k) for k in set(kinds)} == {"MultiStepLR": 1, "MultiStepRestartLR": 1, "CosineAnnealingRestartLR": 3, "LinearLR": 2,
                                                       "VibrateLR": 2}
    ms = cfg["multistep_repeated"]["train"]["scheduler"]["milestones"]
    assert len(set(ms)) < len(ms)                                                             # a repeated milestone
    assert len(cfg["multistep_restart"]["train"]["scheduler"]["restarts"]) == 2               # a restart past iteration 0
    cu = cfg["cosine_uneven"]["train"]["scheduler"]
    assert cu["eta_min"] > 0 and len(set(cu["periods"])) == len(cu["periods"]) == 3
    assert cfg["cosine_uneven_warmup"]["warmup_iter"] == 30 and all(cfg[k]["warmup_iter"] == -1 for k in NAMES if k != "cosine_uneven_warmup")
    assert all(200 <= cfg[k]["n"] == len(lr[k]) for k in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_scheduler_reproduces_the_reference_sequence(schedules, name):
    """update_learning_rate(i, warmup_iter) for i = 1 .. n, as basicsr/train.py calls it: every learning rate within 1 ulp of float64."""
    cfg, lr, base = schedules
    c = cfg[name]
    m = _model(c["train"], base)
    got = []
    for i in range(1, c["n"] + 1):
        m.update_learning_rate(i, warmup_iter=c["warmup_iter"])
        got.append(m.get_current_learning_rate()[0])
    ok = _one_ulp(got, lr[name])
    assert ok.all(), (name, int(np.argmin(ok)), got[int(np.argmin(ok))], lr[name][int(np.argmin(ok))])
    assert len(set(got)) > 3                                                                   # the schedule moved


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_round_trip_continues_the_sequence(schedules, name):
    """What --auto_resume does in mid-schedule: the optimizer's and the scheduler's state_dict go through torch.save / torch.load into a
    freshly built pair (BaseModel.resume_training), which then continues the recorded sequence."""
    import io
    cfg, lr, base = schedules
    c = cfg[name]
    stop = 131                                          # past the first milestones, restart-free cycle ends and VibrateLR's first rise
    a = _model(c["train"], base)
    for i in range(1, stop + 1):
        a.update_learning_rate(i, warmup_iter=c["warmup_iter"])
    buf = io.BytesIO()
    torch.save({"optimizers": [o.state_dict() for o in a.optimizers], "schedulers": [s.state_dict() for s in a.schedulers]}, buf)
    buf.seek(0)
    b = _model(c["train"], base)
    b.resume_training(torch.load(buf, weights_only=True))
    got = []
    for i in range(stop + 1, c["n"] + 1):
        b.update_learning_rate(i, warmup_iter=c["warmup_iter"])
        got.append(b.get_current_learning_rate()[0])
    assert _one_ulp(got, lr[name][stop:]).all(), name


def test_scheduler_constructor_keywords():
    """The reference's constructor keywords, in its order (basicsr/models/lr_scheduler.py)."""
    from basicsr.models import lr_scheduler as S
    sig = lambda c: [(p.name, p.default) for p in list(inspect.signature(c.__init__).parameters.values())[2:]]
    assert sig(S.MultiStepRestartLR) == [("milestones", inspect.Parameter.empty), ("gamma", 0.1), ("restarts", (0,)), ("restart_weights", (1,)),
                                         ("last_epoch", -1)]
    assert sig(S.CosineAnnealingRestartLR) == [("periods", inspect.Parameter.empty), ("restart_weights", (1,)), ("eta_min", 0), ("last_epoch", -1)]
    assert sig(S.LinearLR) == sig(S.VibrateLR) == [("total_iter", inspect.Parameter.empty), ("last_epoch", -1)]
    for c in (S.MultiStepRestartLR, S.CosineAnnealingRestartLR, S.LinearLR, S.VibrateLR):
        assert issubclass(c, torch.optim.lr_scheduler._LRScheduler)
    with pytest.raises(AssertionError, match="restarts and their weights do not match"):
        S.MultiStepRestartLR(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0), [1], restarts=[0, 5], restart_weights=[1])


@pytest.mark.parametrize("kind", ["CosineAnnealingWarmupRestarts", "CosineAnnealingLRWithRestart", "StepLR"])
def test_unknown_scheduler_is_refused_by_name(kind):
    """An unknown name, and the two names the reference's setup_schedulers lists but its lr_scheduler.py does not define."""
    with pytest.raises(NotImplementedError, match=f"Scheduler {kind} is not implemented yet"):
        _model({"scheduler": {"type": kind, "periods": [4]}, "total_iter": 8}, 1e-3)


# ---------------------------------------------------------------------------------------------------------------- losses
# (name, default) of the reference's constructors, basicsr/losses/basic_loss.py:65 and :98
REF_LOSS_KEYWORDS = {"MSELoss": [("loss_weight", 1.0), ("reduction", "mean")],
                     "CharbonnierLoss": [("loss_weight", 1.0), ("reduction", "mean"), ("eps", 1e-12)]}


@pytest.mark.parametrize("name", ["MSELoss", "CharbonnierLoss"])
def test_loss_registry_and_signature(name):
    import basicsr.losses as L
    from basicsr.utils.registry import LOSS_REGISTRY
    cls = LOSS_REGISTRY.get(name)
    assert cls is getattr(L, name) and name in L.__all__ and issubclass(cls, torch.nn.Module)
    ps = list(inspect.signature(cls.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in ps] == REF_LOSS_KEYWORDS[name]
    fw = list(inspect.signature(cls.forward).parameters.values())
    assert [p.name for p in fw] == ["self", "pred", "target", "weight", "kwargs"] and fw[3].default is None
    for red in ("mean", "sum"):
        m = L.build_loss({"type": name, "loss_weight": 0.5, "reduction": red})
        assert isinstance(m, cls) and m.loss_weight == 0.5 and m.reduction == red
    assert name != "CharbonnierLoss" or (L.build_loss({"type": name}).eps == 1e-12 and L.build_loss({"type": name, "eps": 1e-6}).eps == 1e-6)
    with pytest.raises(ValueError, match="Unsupported reduction mode: none"):
        cls(reduction="none")
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(NotImplementedError, match=f"{name}: element-wise weights"):
        cls()(x, x, weight=torch.ones_like(x))


def test_l1_loss_is_unchanged():
    import basicsr.losses as L
    assert [(p.name, p.default) for p in list(inspect.signature(L.L1Loss.__init__).parameters.values())[1:]] == [("loss_weight", 1.0), ("reduction", "mean")]
    with pytest.raises(ValueError, match="Unsupported reduction mode: sum"):
        L.L1Loss(reduction="sum")


def test_sum_is_mean_under_n_times_the_weight():
    import basicsr.losses as L
    x = torch.zeros(2, 3, 5, 7)
    m = L.CharbonnierLoss(loss_weight=0.25, reduction="sum")
    assert L._weight(m, x) == 0.25 * 210 and L._weight(L.MSELoss(loss_weight=0.25), x) == 0.25


# ---------------------------------------------------------------------------------------------------------------- optimizer
def _optimizer_model(kind, **cfg):
    from basicsr.models.base_model import BaseModel
    m = BaseModel({"num_gpu": 0, "is_train": True, "train": {"optim_g": dict(type=kind, lr=1e-3, **cfg)}})
    m.net_g = torch.nn.Linear(3, 2)
    return m


@pytest.mark.parametrize("kind", ["SGD", "Adamax", "Lion"])
def test_unknown_optimizer_keeps_its_message(kind):
    with pytest.raises(NotImplementedError, match=f"optimizer {kind} is not supperted yet"):
        _optimizer_model(kind).setup_optimizers()


def test_amsgrad_is_refused_by_name():
    with pytest.raises(NotImplementedError, match="amsgrad"):
        _optimizer_model("Adam", amsgrad=True).setup_optimizers()


def test_adam_and_adamw_reach_their_classes():
    """Adam gets past the name check and the amsgrad check to the flat buffers, which need the device: the refusal names the class."""
    from bem import ops
    from bem.train import BemAdam, BemAdamW
    assert issubclass(BemAdam, BemAdamW) and BemAdam._step_op is ops.adam_step_ and BemAdamW._step_op is ops.adamw_step_
    own = {k for k in vars(BemAdam) if not k.startswith("__")}
    assert own == {"_step_op"}, own                                        # it differs in one place: which op it launches
    d = lambda c: {p.name: p.default for p in inspect.signature(c.__init__).parameters.values()}
    assert d(BemAdam)["weight_decay"] == 0 and d(BemAdamW)["weight_decay"] == 1e-2 and d(BemAdam)["amsgrad"] is False
    for kind in ("Adam", "AdamW"):
        with pytest.raises(ValueError, match="float32 parameters on one HIP device"):
            _optimizer_model(kind, amsgrad=False).setup_optimizers()


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_new_entries_are_in_the_derived_binding():
    from bem import native
    P, L, F, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int
    assert native.SIGNATURES["bem_adam_step_f32"] == native.SIGNATURES["bem_adamw_step_f32"] == [P, P, P, P, L, F, F, F, F, F, I, F, P, P, P, P]
    assert native._PROTOS["bem_adam_step_f32"][0] is ctypes.c_int
    l1 = native.SIGNATURES["bem_l1_loss_f32"]
    assert l1 == native.SIGNATURES["bem_mse_loss_f32"] == [P, P, P, P, P, L, F, P, P]
    assert native.SIGNATURES["bem_charbonnier_loss_f32"] == l1[:7] + [F] + l1[7:]           # bem_l1_loss_f32's list with eps behind the weight
    assert native._PROTOS["bem_charbonnier_loss_ws_elems"] == (ctypes.c_int64, [L])
    text = open(native.HEADER).read()
    assert "int bem_adam_step_f32(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps," in text


def test_ops_wrappers_refuse_host_tensors():
    from bem import native, ops
    a = torch.zeros(8)
    with pytest.raises(native.BemNativeError):
        ops.charbonnier_loss(a, a.clone())
    with pytest.raises(native.BemNativeError):
        ops.charbonnier_loss_bwd(a, a.clone())
    with pytest.raises(native.BemNativeError):
        ops.adam_step_(a, a.clone(), a.clone(), a.clone(), 1e-3, (0.9, 0.999), 1e-8, 0.0, 1)
