"""What tests/test_conv_forms_gpu.py relies on, checked without a GPU on the same tables (tests/conv_forms_cases.py): bem_conv2d_route sends
every case to the form the case names, the tables together reach every instantiation behind the tap, f32-MFMA and direct forms that no
other test runs by value, and the per-element bound of the GPU tests notices each mutant of the reference."""
import os

import pytest
import torch

import conv_forms_cases as T

FORM = {2: "taps", 3: "mfma", 4: "direct"}                # BEM_CONV_* of include/bem_hip.h (1 = rows, 0 = refused)
A16 = 0x10000                                             # a 16-byte aligned address
IDS = [T.case_id(f, i) for f, i in T.CASES]


@pytest.fixture(scope="module")
def lib():
    from bem import native
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


@pytest.fixture(scope="module")
def refs():
    """(inputs, float64 reference) per case, made once."""
    out = {}
    for fam, i in T.CASES:
        case = T.FAMILIES[fam][i]
        inp = T.inputs(case)
        out[fam, i] = (inp, T.reference(case, inp))
    return out


@pytest.mark.parametrize("fam,i", T.CASES, ids=IDS)
def test_case_routes_to_its_form(lib, fam, i):
    """The question ops.conv2d asks (out = NULL: its own allocation; 16-byte aligned tensors, x moved to the slice's first channel)."""
    B, Ci, Co, H, W, K, s, p, d, (x6, mf), form, ex = T.FAMILIES[fam][i]
    c0, Ct = ex.get("cin_slice", (0, Ci))
    got = lib.bem_conv2d_route(A16 + 4 * c0 * H * W, Ct * H * W, A16 if ex.get("res1") else None, A16 if ex.get("res2") else None, None,
                               Ci, H, W, Co, K, K, s, p, d, int(x6) | 2 * int(mf))
    assert FORM.get(got, got) == form, lib.bem_last_error()


def test_tables_are_small_and_well_formed():
    for fam, i in T.CASES:
        case = T.FAMILIES[fam][i]
        B, Ci, Co = case[:3]
        Ho, Wo = T.out_hw(case)
        assert Ho > 0 and Wo > 0 and B * Co * Ho * Wo <= T.MAX_OUT_ELEMS, T.case_id(fam, i)
        assert B % case[11].get("res1_rep", 1) == 0 and (case[11].get("res1") or "res1_rep" not in case[11])
    assert len(set(IDS)) == len(IDS)
    for fam, cs in T.FAMILIES.items():                    # the bit-for-bit checks of the GPU file have a case in every family
        assert any("cin_slice" in c[11] for c in cs) and any(c[11].get("res1") for c in cs), fam


def test_tables_reach_every_instantiation():
    """conv_patch_launch's and conv_taps_launch's dispatch ladders, restated in conv_forms_cases.instantiation: every kernel they name is
    run by some case (the dilation-1 3x3 and the 5x5 taps, and the row kernels, have their own tests), with relu and both residuals
    once per instantiation of the f32-MFMA and direct forms."""
    reached = {T.instantiation(T.FAMILIES[f][i]) for f, i in T.CASES}
    assert reached == T.INSTANTIATIONS, (sorted(T.INSTANTIATIONS - reached), sorted(reached - T.INSTANTIATIONS))
    full = {T.instantiation(c) for f in ("mfma", "direct") for c in T.FAMILIES[f] if all(c[11].get(k) for k in ("relu", "res1", "res2"))}
    assert full == {n for n in T.INSTANTIATIONS if not n.startswith("conv_taps")}
    # 4 M-tiles (Cout 97 .. 128) run on the MTW = 5 instantiation, in both kernel sizes
    assert {c[5] for c in T.FAMILIES["mfma"] if 96 < c[2] <= 128} == {3, 4}


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_bound_notices_the_mutant(refs, mutant):
    """Each mutant, in float64, leaves the per-element bound of the GPU tests (by 10x: a kernel with that mistake sits within its own
    rounding of the mutant) in at least one case of every family it applies to; a zeroed last column or row in every case that reads it."""
    every = mutant in ("last_col_zero", "last_row_zero")
    for fam, cs in T.FAMILIES.items():
        seen = []
        for i, case in enumerate(cs):
            if not T.mutant_applies(mutant, case):
                continue
            inp, ref = refs[fam, i]
            seen.append(T.excess(T.reference(case, inp, mutant=mutant), ref))
            if every:
                assert seen[-1] > 10, (mutant, T.case_id(fam, i), seen[-1])
        print(f"{mutant} {fam}: excess over the bound {['%.3g' % e for e in seen]}")
        if mutant == "dilation_one_axis":
            assert bool(seen) == (fam == "taps_dil2")
        else:
            assert seen, (mutant, fam)
        if seen:
            assert max(seen) > 10, (mutant, fam, seen)


def test_f32_yardstick_is_inside_the_bound(refs):
    """torch's own f32 convolution of every case sits well inside the per-element bound: the bound is met by f32 arithmetic at these sizes."""
    for fam, i in T.CASES:
        inp, ref = refs[fam, i]
        r32 = T.reference(T.FAMILIES[fam][i], inp, torch.float32)
        assert r32.dtype == torch.float32 and T.excess(r32, ref) < 0.5, T.case_id(fam, i)
