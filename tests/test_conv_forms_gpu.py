"""GPU: the dense convolution's tap, f32-MFMA and direct forms against F.conv2d in float64, at the instantiations no other test runs by
value: the 3x3 taps with dilation 2 and with stride 2 (QD model2), every f32-MFMA instantiation at paddings 0, 1 and 2 (4 M-tiles on the
MTW = 5 instantiation among them), and the three direct kernels.  The tables, the reference and what tests/test_conv_forms_cpu.py proves
about them are in tests/conv_forms_cases.py.

Bounds, all the suite's own:
* per element rtol 1e-4 / atol 2e-5 and finite (tests/test_stage2_entry.py::conv_close);
* x6 tap families: mean |err| against float64 <= 1.5x that of torch's f32 convolution (test_ops_gpu.py::test_conv3x3_row_form), the errors
  pooled over the family's cases;
* f32-MFMA and direct: pooled mean and max |err| <= 2x those of the f32 convolution (test_stage2_entry.py::_yardstick).
Measured ratios: profiles/conv_forms_parity.txt."""
import pytest
import torch

import conv_forms_cases as T

pytestmark = pytest.mark.gpu
IDS = [T.case_id(f, i) for f, i in T.CASES]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from bem import ops as _ops
    return _ops


def dev(t):
    return None if t is None else t.cuda().contiguous()


class Runs:
    """Each case run once: its inputs on the device, the kernel's output and the float64 / f32 references, kept for the pooled figures."""

    def __init__(self, ops):
        self.ops, self.done = ops, {}

    def call(self, case, d, **over):
        """ops.conv2d under the case's switches -> (route name, output)."""
        B, Ci, Co, H, W, K, s, p, dil, (x6, mf), form, ex = case
        kw = dict(stride=s, pad=p, res1=d["res1"], res2=d["res2"], dilation=dil, res1_rep=ex.get("res1_rep", 1),
                  cin_slice=(ex["cin_slice"][0], Ci) if "cin_slice" in ex else None)
        kw.update(over)
        x = kw.pop("x", d["x"])
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(self.ops, "USE_CONV_X6", x6)
            mp.setattr(self.ops, "USE_CONV_MFMA", mf)
            route = self.ops.conv2d_route(x, d["w"], **kw)
            assert route == form, (route, form)
            return self.ops.conv2d(x, d["w"], d["bias"], relu=bool(ex.get("relu")), **kw)

    def get(self, fam, i):
        if (fam, i) not in self.done:
            case = T.FAMILIES[fam][i]
            inp = T.inputs(case)
            d = {k: dev(v) for k, v in inp.items()}
            y = self.call(case, d).cpu()
            self.done[fam, i] = (case, d, y, T.reference(case, inp), T.reference(case, inp, torch.float32))
        return self.done[fam, i]


@pytest.fixture(scope="module")
def runs(ops):
    return Runs(ops)


@pytest.mark.parametrize("fam,i", T.CASES, ids=IDS)
def test_form_against_float64(runs, fam, i):
    case, d, y, r64, r32 = runs.get(fam, i)
    assert y.shape == r64.shape and y.dtype == torch.float32
    assert torch.isfinite(y).all(), "non-finite values"
    err, e32 = (y.double() - r64).abs(), (r32.double() - r64).abs()
    print(f"{T.case_id(fam, i)} [{T.instantiation(case)}]: max |err| {err.max():.3e} mean {err.mean():.3e} | f32 oracle max {e32.max():.3e} mean {e32.mean():.3e}"
          f" | excess over the bound {T.excess(y, r64):.3f}")
    assert torch.allclose(y.double(), r64, rtol=T.RTOL, atol=T.ATOL), f"max abs err {err.max():.3e} (ref max {r64.abs().max():.3e})"


@pytest.mark.parametrize("fam", list(T.FAMILIES))
def test_family_accuracy(runs, fam):
    """The errors of all the family's cases pooled (a tiny case's f32 oracle is nearly exact): the x6 taps' accuracy claim, and for the
    f32-MFMA and direct forms the suite's float64 yardstick."""
    es, e32s = [], []
    for i in range(len(T.FAMILIES[fam])):
        case, d, y, r64, r32 = runs.get(fam, i)
        es.append((y.double() - r64).abs().flatten())
        e32s.append((r32.double() - r64).abs().flatten())
    e, e32 = torch.cat(es), torch.cat(e32s)
    print(f"PARITY {fam}: {len(es)} cases, {e.numel()} outputs | HIP mean {e.mean():.3e} max {e.max():.3e} | f32 oracle mean {e32.mean():.3e} max {e32.max():.3e}"
          f" | ratio mean {e.mean() / e32.mean():.3f} max {e.max() / e32.max():.3f}")
    if fam.startswith("taps"):
        assert e.mean() <= 1.5 * e32.mean(), (fam, float(e.mean()), float(e32.mean()))
    else:
        assert e.mean() <= 2 * e32.mean() and e.max() <= 2 * e32.max(), (fam, float(e.mean()), float(e32.mean()), float(e.max()), float(e32.max()))


@pytest.mark.parametrize("fam", list(T.FAMILIES))
def test_res1_rep_one_and_channel_slice_bit_for_bit(runs, fam):
    """res1_rep = 1 with the residual rows written out is the call with res1_rep = n, to the bit, and so is the call without the argument; a
    cin_slice call is the call on the materialised slice, to the bit.  One case of each kind per family."""
    cs = T.FAMILIES[fam]
    i = next(i for i, c in enumerate(cs) if c[11].get("res1_rep", 1) > 1)
    case, d, y, _, _ = runs.get(fam, i)
    full = d["res1"].repeat_interleave(case[11]["res1_rep"], 0).contiguous()
    y1 = runs.call(case, d, res1=full, res1_rep=1)
    kw = dict(stride=case[6], pad=case[7], dilation=case[8], res1=full, res2=d["res2"], relu=bool(case[11].get("relu")),
              cin_slice=(case[11]["cin_slice"][0], case[1]) if "cin_slice" in case[11] else None)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(runs.ops, "USE_CONV_X6", case[9][0])
        mp.setattr(runs.ops, "USE_CONV_MFMA", case[9][1])
        y0 = runs.ops.conv2d(d["x"], d["w"], d["bias"], **kw)                      # no res1_rep argument at all
    assert torch.equal(y1.cpu(), y) and torch.equal(y0.cpu(), y), T.case_id(fam, i)
    i = next(i for i, c in enumerate(cs) if "cin_slice" in c[11])
    case, d, y, _, _ = runs.get(fam, i)
    c0 = case[11]["cin_slice"][0]
    ys = runs.call(case, d, x=d["x"][:, c0:c0 + case[1]].contiguous(), cin_slice=None)
    assert torch.equal(ys.cpu(), y), T.case_id(fam, i)
