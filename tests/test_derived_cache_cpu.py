"""bem.ops.Derived -- the one derived-weight cache of the host layer -- on CPU tensors: no library, no GPU.

What makes an entry stale (an in-place write, a weight epoch, a replaced or moved source), that ``put`` writes what ``get`` reads, that a
miss replaces the entry instead of adding one, and that ops holds no process-wide container of conv weights any more."""
import gc
import weakref

import torch

from bem import ops


class Counted:
    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return torch.full((3,), float(self.n))


def test_hit_and_the_three_misses():
    c, fn = ops.Derived(), Counted()
    a, b = torch.zeros(4), torch.ones(2)
    v = c.get("k", [a, b], fn)
    assert c.get("k", [a, b], fn) is v and fn.n == 1                      # same sources: a hit, fn not called again
    assert c.get("k", [a.detach(), b], fn) is v and fn.n == 1             # a detached alias is the same source
    b.add_(1)                                                             # in-place write to a source
    v2 = c.get("k", [a, b], fn)
    assert fn.n == 2 and v2 is not v and c.get("k", [a, b], fn) is v2
    ops.bump_weight_epoch()                                               # parameters rewritten behind torch's version counters
    assert c.get("k", [a, b], fn) is not v2 and fn.n == 3
    a2 = torch.zeros(4)                                                   # a source replaced by a new tensor
    assert a2.data_ptr() != a.data_ptr() and a2._version == a._version
    c.get("k", [a2, b], fn)
    assert fn.n == 4
    c.get("k", [a2, b], fn)
    assert fn.n == 4
    other = c.get("k2", [a2], fn)                                         # keys are independent
    assert fn.n == 5 and c.get("k2", [a2], fn) is other and fn.n == 5


def test_fn_runs_without_grad():
    w = torch.ones(3, requires_grad=True)
    assert not ops.Derived().get("k", [w], lambda: w * 2).requires_grad


def test_put_is_what_get_reads():
    c, fn = ops.Derived(), Counted()
    a = torch.zeros(4)
    v = torch.arange(3.0)
    c.put("T", [a], v)
    assert c.get("T", [a], fn) is v and fn.n == 0
    a.mul_(2)                                                             # a put entry goes stale like any other
    assert c.get("T", [a], fn) is not v and fn.n == 1
    c.put("T", [a], v)                                                    # and put replaces a live entry
    assert c.get("T", [a], fn) is v and fn.n == 1


def test_miss_replaces_and_releases():
    c = ops.Derived()
    a = torch.zeros(4)
    old = c.get("k", [a], lambda: torch.ones(5))
    ref = weakref.ref(old)
    n = len(c.d)
    a.add_(1)
    new = c.get("k", [a], lambda: torch.ones(5))
    assert len(c.d) == n == 1
    held = [v for _, v in c.d.values()]
    assert len(held) == 1 and held[0] is new
    del old, held
    gc.collect()
    assert ref() is None                                                  # the cache was the old value's last referrer


def test_device_is_in_the_signature():
    """Two devices can hand out equal addresses; (data_ptr, version) alone would call that a hit."""
    class Src:
        def __init__(self, device):
            self.device = device
            self._version = 0

        def data_ptr(self):
            return 0x1000

        def is_inference(self):
            return False

    s0, s1 = ops.Derived._sig([Src(torch.device("cuda", 0))]), ops.Derived._sig([Src(torch.device("cuda", 1))])
    assert s0 != s1 and s0[0] == s1[0] == ops.WEIGHT_EPOCH[0] and s0[1][:2] == s1[1][:2] == (0x1000, 0)
    assert ops.Derived._sig([torch.zeros(1)])[1][2] == torch.device("cpu")
    c, fn = ops.Derived(), Counted()
    c.get("k", [Src(torch.device("cuda", 0))], fn)
    c.get("k", [Src(torch.device("cuda", 1))], fn)
    assert fn.n == 2


def test_one_cache_per_holder_outside_module_registries():
    m = torch.nn.Linear(2, 2)
    c = ops.derived(m)
    assert ops.derived(m) is c and isinstance(c, ops.Derived) and m.__dict__["_derived"] is c
    assert [k for k, v in m.__dict__.items() if isinstance(v, ops.Derived)] == ["_derived"]
    assert "_derived" not in m.state_dict() and not list(m.children()) and len(list(m.parameters())) == 2
    assert ops.derived(torch.nn.Linear(2, 2)) is not c


def test_ops_keeps_no_conv_weights():
    """conv2d packs a raw tensor for the call only: the process-wide dicts are gone, and no module-level container of ops holds a tensor."""
    assert not hasattr(ops, "_CONV_PACK") and not hasattr(ops, "_CONV_PACK_X6")
    assert not hasattr(ops, "_packed_conv_weight") and not hasattr(ops, "_packed_conv_weight_x6")

    def tensors_in(o, depth=0):
        if torch.is_tensor(o) or isinstance(o, ops.ConvWeight):
            return True
        if depth < 3 and isinstance(o, dict):
            return any(tensors_in(v, depth + 1) for v in o.values())
        if depth < 3 and isinstance(o, (list, tuple, set)):
            return any(tensors_in(v, depth + 1) for v in o)
        return False
    keep = {"_SCRATCH", "_TABLES"}                     # scratch buffers and tables keyed by image size, not by weights
    assert [n for n, o in vars(ops).items() if n not in keep and isinstance(o, (dict, list, tuple, set)) and tensors_in(o)] == []
    w = torch.zeros(4, 8, 3, 3)
    cw = ops.ConvWeight(w)
    assert cw.w is w and cw._x6 is None and cw._f32 is None                 # nothing is packed until conv2d asks for a form
