"""The dense convolution's route table without a GPU: bem_conv2d_route is host arithmetic on its arguments (it reads no pointer), so which
kernel form takes which shape, alignment and pair of allow bits is pinned here row by row; and bem_conv2d_f32 with a forced form refuses
arguments outside that form before any HIP call."""
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from bem import native
    if not os.path.exists(native.LIB_PATH):
        native.build()
    return native.lib()


ROWS, TAPS, MFMA, DIRECT = 1, 2, 3, 4                     # BEM_CONV_* of include/bem_hip.h
X6, MF = 1, 2                                             # BEM_CONV_ALLOW_*
A16, A8 = 0x10000, 0x10008                                # a 16-byte aligned address, and one that is 8-byte aligned only
C4, C3 = (40, 80, 128, 128, 4, 2, 1, 1), (16, 40, 32, 32, 3, 1, 1, 1)

# (Cin, Cout, H, W, K, stride, pad, dilation), {x, res1, allow}, expected form (0 = refused)
TABLE = [
    ((32, 32, 128, 128, 3, 1, 1, 1), {}, ROWS),
    (C3, {}, ROWS),
    (C3, {"res1": A8}, TAPS),
    ((16, 40, 32, 256, 3, 1, 1, 1), {}, TAPS),
    ((16, 40, 24, 40, 3, 1, 1, 1), {}, TAPS),
    ((16, 40, 24, 40, 3, 1, 1, 1), {"allow": MF}, MFMA),
    ((16, 40, 24, 40, 3, 1, 1, 1), {"allow": 0}, DIRECT),
    ((3, 16, 16, 16, 3, 1, 1, 1), {}, MFMA),
    ((8, 40, 36, 47, 3, 1, 1, 1), {}, MFMA),
    ((3, 168, 20, 21, 3, 1, 1, 1), {}, DIRECT),
    ((192, 384, 6, 6, 3, 1, 1, 1), {}, TAPS),
    ((64, 384, 5, 7, 3, 1, 1, 1), {}, DIRECT),
    ((32, 32, 64, 64, 3, 1, 2, 2), {}, TAPS),
    ((12, 32, 64, 64, 3, 1, 2, 2), {}, 0),
    ((32, 64, 64, 64, 3, 2, 1, 1), {}, TAPS),
    ((32, 64, 64, 66, 3, 2, 1, 1), {}, 0),
    ((64, 192, 7, 8, 5, 1, 2, 1), {}, TAPS),
    ((64, 192, 7, 7, 5, 1, 2, 1), {}, DIRECT),
    ((60, 192, 7, 8, 5, 1, 2, 1), {}, 0),
    (C4, {}, ROWS),
    (C4, {"allow": MF}, ROWS),
    (C4, {"res1": A16}, MFMA),
    (C4, {"x": A8}, MFMA),
    ((80, 160, 64, 64, 4, 2, 1, 1), {}, ROWS),
    ((8, 24, 6, 4, 4, 2, 1, 1), {}, ROWS),
    ((24, 48, 64, 48, 4, 2, 1, 1), {}, MFMA),
    ((24, 168, 64, 48, 4, 2, 1, 1), {}, DIRECT),
    ((16, 16, 32, 32, 3, 1, 0, 1), {}, MFMA),
    ((16, 16, 32, 32, 7, 1, 3, 1), {}, 0),
    ((16, 16, 33, 33, 3, 3, 1, 1), {}, 0),
]


def route(lib, shape, x=A16, res1=None, res2=None, out=A16, allow=X6 | MF, x_bstride=None):
    Cin, Cout, H, W, K, s, p, d = shape
    return lib.bem_conv2d_route(x, Cin * H * W if x_bstride is None else x_bstride, res1, res2, out, Cin, H, W, Cout, K, K, s, p, d, allow)


@pytest.mark.parametrize("shape,how,want", TABLE, ids=[f"{'x'.join(map(str, s))}{''.join(f'-{k}={v:#x}' for k, v in h.items())}" for s, h, _ in TABLE])
def test_route_table(lib, shape, how, want):
    got = route(lib, shape, **how)
    assert got == want
    if want == 0:
        assert lib.bem_last_error().startswith(b"conv2d: ") and len(lib.bem_last_error()) > len(b"conv2d: ")


def test_route_alignment_and_the_absent_out(lib):
    """The halves of the row rule the table's rows leave out: out = NULL stands for the caller's own (aligned) allocation; an out, a res2 or
    a batch stride off the 16-byte grid moves the 3x3 to the taps; a batch stride off it moves the 4x4 to the f32-MFMA form; an x that is
    4-byte aligned only leaves the x6 forms altogether."""
    assert route(lib, C3, out=None) == ROWS and route(lib, C3, out=None, res1=A16, res2=A16) == ROWS
    assert route(lib, C3, out=A8) == TAPS and route(lib, C3, res2=A8) == TAPS and route(lib, C3, x=A8) == TAPS
    assert route(lib, C3, x_bstride=16 * 32 * 32 + 2) == TAPS and route(lib, C4, x_bstride=40 * 128 * 128 + 2) == MFMA
    assert route(lib, C3, x=A16 + 4) == MFMA and route(lib, (64, 192, 7, 8, 5, 1, 2, 1), x=A16 + 4) == DIRECT
    assert route(lib, (32, 32, 64, 64, 3, 1, 2, 2), x=A16 + 4) == 0 and route(lib, (32, 32, 64, 64, 3, 1, 2, 2), allow=0) == TAPS
    assert route(lib, (16, 16, 32, 32, 3, 1, 1, 3)) == 0 and route(lib, (32, 64, 64, 64, 3, 2, 2, 2)) == 0
    assert lib.bem_conv2d_route(A16, 16 * 32 * 32, None, None, None, 16, 32, 32, 16, 3, 5, 1, 1, 1, X6 | MF) == 0        # 3x5


def test_forced_form_refuses_without_a_device(lib):
    """bem_conv2d_f32 runs the form it is given; each launcher keeps its own conditions and returns before any HIP call."""
    p = 16   # any non-null value: the checks reject before a pointer is touched

    def call(form, Cin, H, W, Cout, K, s, pad, d=1):
        rc = lib.bem_conv2d_f32(form, p, Cin * H * W, p, None, None, None, p, 1, Cin, H, W, Cout, K, K, s, pad, d, 1, 1, None)
        return rc, lib.bem_last_error()
    rc, msg = call(TAPS, 64, 7, 7, 192, 5, 1, 2)
    assert rc == 1 and b"even output width" in msg
    rc, msg = call(TAPS, 64, 7, 8, 192, 5, 2, 2)
    assert rc == 1 and b"5x5 s1 p2" in msg
    rc, msg = call(ROWS, 16, 24, 40, 40, 3, 1, 1)
    assert rc == 1 and b"outside the row form" in msg
    rc, msg = call(MFMA, 16, 24, 40, 168, 3, 1, 1)
    assert rc == 1 and b"Cout <= 160" in msg
    # what a launcher's own arguments cannot say: a padding other than the form's (the output would not be the caller's size), a dilation
    # outside the tap form, an unknown form
    assert call(TAPS, 64, 8, 8, 192, 3, 1, 0)[0] == 1 and call(ROWS, 16, 32, 32, 40, 3, 1, 0)[0] == 1 and call(ROWS, 16, 32, 32, 40, 4, 2, 2)[0] == 1
    assert call(MFMA, 16, 24, 40, 40, 3, 1, 2, d=2)[0] == 1 and call(DIRECT, 16, 24, 40, 40, 3, 1, 2, d=2)[0] == 1
    assert call(0, 16, 24, 40, 40, 3, 1, 1)[0] == 1 and call(5, 16, 24, 40, 40, 3, 1, 1)[0] == 1
