"""CPU: the host side of the averaged weights (train.ema_decay): the float64 reference of tests/ema_ref.py against the reference's own
torch line, BaseModel.load_network's ``params_ema`` -> ``params`` fallback (base_model.py:331-335), the ABI declaration of
bem_ema_update_f32 and the binding derived from it, the eval driver's key selection."""
import ctypes
import importlib.util
import os

import pytest
import torch

import ema_ref as R
from conftest import PKG


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9, 0.999, 0.9999])
def test_reference_equals_torchs_in_place_pair(decay):
    """update_f64 with constants() against ``mul_(decay).add_(p, alpha=1 - decay)``.  Rows with ema = 0 and with p = 0 leave one term
    alone, so each constant is pinned to f32 rounding on its own: 1 - (float)decay taken in f32 is off by 1e-5 relative at 0.999."""
    g = torch.Generator().manual_seed(11)
    n = 4096
    mag = lambda: torch.exp(torch.empty(n).uniform_(-13.8, 6.9, generator=g)) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    for ema, p in ((mag(), mag()), (torch.zeros(n), mag()), (mag(), torch.zeros(n))):
        d, o = R.constants(decay)
        want, m = R.update_f64(ema, p, d, o)
        got = R.torch_update_(ema.clone(), p, decay)
        assert bool(((got.double() - want).abs() <= R.bound_unfused(m)).all()), float(((got.double() - want).abs() - R.bound_unfused(m)).max())
    assert R.constants(0.999) == (0.9990000128746033, 0.0010000000474974513) and R.constants(0) == (0.0, 1.0)


def _base_model(tmp_path):
    from basicsr.models.base_model import BaseModel
    return BaseModel({"name": "run", "num_gpu": 0, "is_train": False, "path": {"models": str(tmp_path)}})


def _net(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.PReLU(), torch.nn.Linear(4, 2))


def _same(net, sd):
    return all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())


def test_load_network_falls_back_from_params_ema_to_params(tmp_path):
    m = _base_model(tmp_path)
    a, b = _net(1), _net(2)
    only, both = m.save_network(a, "only", 1), m.save_network([a, b], "both", 1, param_key=["params", "params_ema"])
    assert set(torch.load(only, weights_only=True)) == {"params"} and set(torch.load(both, weights_only=True)) == {"params", "params_ema"}
    net = _net(3)
    m.load_network(net, only, True, param_key="params_ema")            # the key is absent: 'params' is loaded, strictly
    assert _same(net, a.state_dict())
    net = _net(3)
    m.load_network(net, both, True, param_key="params_ema")
    assert _same(net, b.state_dict()) and not _same(net, a.state_dict())
    m.load_network(net, both, True, param_key="params")
    assert _same(net, a.state_dict())
    # unchanged: a bare state dict loads whatever key is asked for
    bare = os.path.join(tmp_path, "bare.pth")
    torch.save(b.state_dict(), bare)
    m.load_network(net, bare, True, param_key="params")
    assert _same(net, b.state_dict())


def test_header_declares_the_entry_point_and_the_binding_follows():
    from bem import native
    text = open(native.HEADER).read()
    assert "int bem_ema_update_f32(float* ema, const float* p, int64_t n, float decay, float one_minus_decay, void* stream);" in text
    assert "fmaf(one_minus_decay, p, decay * ema)" in text
    P, L, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert native.SIGNATURES["bem_ema_update_f32"] == [P, P, L, F, F, P]
    assert native._PROTOS["bem_ema_update_f32"][0] is ctypes.c_int
    # the optimizer entry next to it keeps its declaration
    assert native.SIGNATURES["bem_adamw_step_f32"] == [P, P, P, P, L, F, F, F, F, F, ctypes.c_int, F, P, P, P, P]


def test_ops_wrapper_checks_operands_before_the_library():
    from bem import native, ops
    assert getattr(ops.ema_update_, "__wrapped__", None) is not None          # the launch bracket
    a = torch.zeros(4)
    with pytest.raises(native.BemNativeError):
        ops.ema_update_(a, a.clone(), 0.5)                                      # no CPU implementation


def test_eval_loader_selects_the_key(tmp_path):
    spec = importlib.util.spec_from_file_location("bem_eval_driver", os.path.join(PKG, "Enhancement", "eval.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    args = drv.get_parser().parse_args([])
    assert args.weights_key == "params" and args.cond_weights_key == "params"
    m = _base_model(tmp_path)
    a, b = _net(1), _net(2)
    only, both = m.save_network(a, "only", 1), m.save_network([a, b], "both", 1, param_key=["params", "params_ema"])
    net = _net(3)
    drv.load_params(net, both, "params_ema")
    assert _same(net, b.state_dict())
    drv.load_params(net, both)
    assert _same(net, a.state_dict())
    with pytest.raises(KeyError, match=r"params_ema.*keys present: \['params'\]"):
        drv.load_params(net, only, "params_ema")
