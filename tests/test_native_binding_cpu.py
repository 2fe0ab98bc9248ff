"""CPU: the ctypes binding that bem.native derives from include/bem_hip.h.  A host C++ compiler reads the same header and must agree
with every derived argument list, return type and struct layout; the parser refuses what it does not understand; the operator seam
(selective_scan_cuda_oflex) holds no binding of its own; the scratch helper of bem.ops keys by tag, device and stream; bem.tables is
numpy only."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

from conftest import PKG, ROOT

LETTER = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_int64: "l", ctypes.c_uint64: "u", ctypes.c_float: "f", ctypes.c_double: "d",
          ctypes.c_char_p: "s"}

PROBE = r"""
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include "bem_hip.h"
template <class T> constexpr char arg() {
    if constexpr (std::is_pointer_v<T>) return 'p';
    else if constexpr (std::is_same_v<T, int>) return 'i';
    else if constexpr (std::is_same_v<T, int64_t>) return 'l';
    else if constexpr (std::is_same_v<T, uint64_t>) return 'u';
    else if constexpr (std::is_same_v<T, float>) return 'f';
    else if constexpr (std::is_same_v<T, double>) return 'd';
    else return '?';
}
template <class T> constexpr char ret() { if constexpr (std::is_same_v<T, const char*>) return 's'; else return arg<T>(); }
template <class F> struct Sig;
template <class R, class... A> struct Sig<R (*)(A...)> {
    static void print(const char* name) { const char s[] = {ret<R>(), ':', arg<A>()..., 0}; std::printf("F %s %s\n", name, s); }
};
#define FN(name) Sig<decltype(&name)>::print(#name);
#define STRUCT(T) std::printf("S %s %zu\n", #T, sizeof(T));
#define FIELD(T, f) std::printf("M %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(T::f));
int main() {
@BODY@
    return 0;
}
"""


@pytest.fixture(scope="module")
def native():
    from bem import native as n
    if not os.path.exists(n.LIB_PATH):
        n.build()
    return n


def _letter(t):
    return "p" if hasattr(t, "contents") else LETTER[t]          # POINTER(PwArgs) / POINTER(WgradArgs) are pointers to the compiler


@pytest.mark.skipif(shutil.which("c++") is None, reason="no host C++ compiler on PATH")
def test_compiler_agrees_with_the_derived_binding(native, tmp_path):
    """decltype(&name) of every entry point and sizeof / offsetof of both argument blocks, printed by a program the host compiler builds
    from the header alone (it needs <stdint.h> only: no HIP, no GPU, nothing is linked or called)."""
    structs = {"bem_pw_args": native.PwArgs, "bem_wgrad_args": native.WgradArgs}
    body = [f"    FN({name})" for name in native.SIGNATURES]
    for cname, cls in structs.items():
        body += [f"    STRUCT({cname})"] + [f"    FIELD({cname}, {f})" for f, _ in cls._fields_]
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(PROBE.replace("@BODY@", "\n".join(body)))
    subprocess.run(["c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    funcs = {w[1]: w[2] for w in (line.split() for line in out) if w and w[0] == "F"}
    sizes = {w[1]: int(w[2]) for w in (line.split() for line in out) if w and w[0] == "S"}
    fields = {(w[1], w[2]): (int(w[3]), int(w[4])) for w in (line.split() for line in out) if w and w[0] == "M"}
    assert len(native.SIGNATURES) >= 120 and set(funcs) == set(native.SIGNATURES)
    lib = native.lib()
    for name, argtypes in native.SIGNATURES.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes or []) == list(argtypes), name
        mine = _letter(fn.restype) + ":" + "".join(_letter(t) for t in argtypes)
        assert "?" not in funcs[name] and funcs[name] == mine, (name, funcs[name], mine)
    for cname, cls in structs.items():
        assert ctypes.sizeof(cls) == sizes[cname], cname
        for f, _ in cls._fields_:
            d = getattr(cls, f)
            assert (d.offset, d.size) == fields[(cname, f)], (cname, f)
    assert native.PwArgs.ln_eps.size == 4 and ctypes.sizeof(native.WgradArgs().perm) == 16


def test_parser_refuses_what_it_does_not_understand():
    from bem.native import BemNativeError, parse_header
    with pytest.raises(BemNativeError, match="line 3.*long double x"):
        parse_header("/* a\n comment */\nint bem_f(const float* a, long double x, void* stream);\n")
    for text in ("int bem_f(int);", "unsigned bem_f(int a);", "int bem_f(int a) { return a; }", "struct bem_t;",
                 "typedef struct { long n; } bem_t_args;", "int bem_f(int a)\nint bem_g(int b);"):
        with pytest.raises(BemNativeError):
            parse_header(text)
    protos, structs = parse_header("#define BEM_ERR 2\nint64_t bem_f(const float* a,   // first\n        int64_t n,\n"
                                   "    void* stream);\nconst char* bem_msg(void);\n")
    assert protos == {"bem_f": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]), "bem_msg": (ctypes.c_char_p, [])}
    assert structs == {}
    protos, structs = parse_header("typedef struct {\n    int perm[4]; const float* p;\n    double d;\n} bem_t_args;\nint bem_g(const bem_t_args* a);")
    assert structs == {"bem_t_args": [("perm", ctypes.c_int * 4), ("p", ctypes.c_void_p), ("d", ctypes.c_double)]}
    assert protos == {"bem_g": (ctypes.c_int, [ctypes.c_void_p])}


def test_the_operator_seam_uses_the_same_binding(native):
    import selective_scan_cuda_oflex as ext
    src = inspect.getsource(ext)
    assert "argtypes" not in src and "restype" not in src and "CDLL" not in src
    assert ext.lib is native.lib and ext.check is native.check
    called = set(re.findall(r"lib\(\)\.(bem_\w+)", src))
    assert called == {"bem_selective_scan_fwd_f32", "bem_selective_scan_fwd_in16", "bem_cast16_to_f32", "bem_cast_f32_to16",
                      "bem_selective_scan_bwd_f32", "bem_selective_scan_bwd_ws_elems"}
    assert called <= set(native.SIGNATURES)


def test_scratch_is_kept_per_tag_device_and_stream(monkeypatch):
    from types import SimpleNamespace
    from bem import ops
    made, stream = [], SimpleNamespace(cuda_stream=11)
    real_empty = torch.empty

    def empty(n, device=None, dtype=None):
        made.append((n, str(device), dtype))
        return real_empty(n, dtype=dtype)
    monkeypatch.setattr(ops, "_SCRATCH", {})
    monkeypatch.setattr(torch, "empty", empty)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: stream)
    a = ops._scratch("t", "cuda:0", 100, torch.float32)
    assert a.numel() == 100 and a.dtype == torch.float32 and made == [(100, "cuda:0", torch.float32)]
    assert ops._scratch("t", "cuda:0", 40, torch.float32) is a and ops._scratch("t", torch.device("cuda:0"), 100, torch.float32) is a
    assert len(made) == 1                                                      # a smaller or equal request allocates nothing
    b = ops._scratch("t", "cuda:0", 101, torch.float32)
    assert b is not a and b.numel() == 101 and ops._scratch("t", "cuda:0", 100, torch.float32) is b      # grown, and it stays grown
    stream.cuda_stream = 12
    c = ops._scratch("t", "cuda:0", 8, torch.float32)
    assert c is not b and c.numel() == 8                                       # another stream never shares
    d = ops._scratch("u", "cuda:0", 8, torch.float32)
    e = ops._scratch("t", "cuda:1", 8, torch.float32)
    assert len({id(x) for x in (b, c, d, e)}) == 4 and len(made) == 5          # nor another tag or device
    stream.cuda_stream = 11
    assert ops._scratch("t", "cuda:0", 1, torch.float32) is b


def test_tables_are_uploaded_once_per_device(monkeypatch):
    import numpy as np
    from bem import ops
    monkeypatch.setattr(ops, "_TABLES", {})
    calls = []

    def build():
        calls.append(1)
        return np.arange(3), np.ones(2, np.float32)
    t = ops._tables(("k", 3), "cpu", build)
    assert isinstance(t, tuple) and t[0].tolist() == [0, 1, 2] and t[1].dtype == torch.float32
    assert ops._tables(("k", 3), "cpu", build) is t and len(calls) == 1
    one = ops._tables("single", "cpu", lambda: np.zeros(4))
    assert torch.is_tensor(one) and one.dtype == torch.float64


def test_tables_module_is_numpy_only():
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import bem.tables as t; assert 'torch' not in sys.modules and 'bem.ops' not in sys.modules; "
            "assert t.uiqm_resized_rows(400, 600) == 170 and t.lab_tables().shape == (3337,)")
    subprocess.run([sys.executable, "-c", code, PKG], check=True)
    from bem import ops, tables
    assert ops.UIQM_WIDTH == tables.UIQM_WIDTH == 256 and ops.NIQE_BLOCK == 96 and ops.UIQM_WINDOW == 10
    for name in ("niqe_gamma_table", "niqe_resize_table", "pil_resize_table", "lab_tables", "uiqm_resized_rows"):
        assert callable(getattr(tables, name)) and getattr(ops, name) is getattr(tables, name)       # one definition, importable from both
