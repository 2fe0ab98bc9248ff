"""ctypes binding of libbem_hip.so, derived from the C ABI's own declaration (include/bem_hip.h).

The header is the one place where an entry point's arguments are written down: this module parses its prototypes and the two
argument-block structs when it is imported (a few milliseconds; the structs must be complete before anyone can fill one) and
``lib()`` applies them to the loaded library.  A wrong argument type at this seam would not raise -- it would shift every later
argument of the call -- so a declaration the parser does not understand is an error, never skipped
(tests/test_native_binding_cpu.py compares the result with what a C++ compiler makes of the same header).

There is deliberately no fallback: if the library is missing or a call is rejected the caller
gets an exception (``BemNativeError``) -- the product path never computes on the CPU."""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_double, c_float, c_int, c_int64, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BEM_HIP_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libbem_hip.so"))
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "bem_hip.h")


class BemNativeError(RuntimeError):
    pass


class PwArgs(ctypes.Structure):
    """``bem_pw_args``; the fields are taken from the header below."""


class WgradArgs(ctypes.Structure):
    """``bem_wgrad_args``; the fields are taken from the header below."""


P, I, I64, U64, F = c_void_p, c_int, c_int64, c_uint64, c_float

# The header's whole vocabulary.  Every pointer is a c_void_p except the two argument blocks; anything else is an error, never a guess.
_SCALARS = {"int": c_int, "int64_t": c_int64, "uint64_t": c_uint64, "float": c_float, "double": c_double}
_RETURNS = {"int": c_int, "int64_t": c_int64, "const char*": ctypes.c_char_p}
_STRUCTS = {"bem_pw_args": PwArgs, "bem_wgrad_args": WgradArgs}


def _ctype(decl: str, line: int):
    """ctypes type and name of one ``type name`` / ``type name[n]`` declaration (a parameter or a struct field)."""
    m = re.fullmatch(r"(.*?[\s*])(\w+)(?:\[(\d+)\])?", decl.strip(), re.S)
    typ = re.sub(r"\s*\*\s*", "*", " ".join(m.group(1).split())) if m else ""
    if typ.endswith("*"):
        block = re.fullmatch(r"const (\w+)\*", typ)
        t = ctypes.POINTER(_STRUCTS[block.group(1)]) if block and block.group(1) in _STRUCTS else P
    elif typ in _SCALARS:
        t = _SCALARS[typ]
    else:
        raise BemNativeError(f"bem_hip.h line {line}: no ctypes mapping for `{' '.join(decl.split())}`")
    return (t * int(m.group(3)) if m.group(3) else t), m.group(2)


def parse_header(text: str):
    """C declarations of the header -> ({function: (restype, [argtypes])}, {struct: [(field, ctype)]}).  Comments and preprocessor lines
    are blanked in place, so errors name the header's own line; a statement that is neither a prototype nor one of the argument-block
    typedefs raises."""
    blank = lambda m: "\n" * m.group(0).count("\n")
    text = re.sub(r"/\*.*?\*/|//[^\n]*", blank, text, flags=re.S)
    text = re.sub(r"^[ \t]*#[^\n]*", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{|\}\s*\Z', "", text)
    line = lambda pos: text.count("\n", 0, pos) + 1
    structs, protos = {}, {}

    def struct(m):
        structs[m.group(2)] = [_ctype(d, line(m.start()))[::-1] for d in m.group(1).split(";") if d.strip()]
        return blank(m)
    text = re.sub(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    for m in re.finditer(r"[^;\s][^;]*", text):
        stmt, at = " ".join(m.group(0).split()), line(m.start())
        p = re.fullmatch(r"(.*?[\s*])(bem_\w+)\s*\((.*)\)", stmt)
        ret = re.sub(r"\s*\*\s*", "*", p.group(1)).strip() if p else None
        if ret not in _RETURNS:
            raise BemNativeError(f"bem_hip.h line {at}: not a prototype this binding understands: `{stmt}`")
        args = [] if p.group(3).strip() in ("", "void") else p.group(3).split(",")
        protos[p.group(2)] = (_RETURNS[ret], [_ctype(a, at)[0] for a in args])
    return protos, structs


try:
    with open(HEADER) as _f:
        _PROTOS, _FIELDS = parse_header(_f.read())
except OSError as e:
    raise BemNativeError(f"{HEADER}: the C ABI header is the source of the binding and must ship with the package ({e})")
PwArgs._fields_, WgradArgs._fields_ = (_FIELDS[n] for n in _STRUCTS)
SIGNATURES = {name: argtypes for name, (_, argtypes) in _PROTOS.items()}     # name -> argtypes, as declared in the header

_lib = None


def build(verbose: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into lib/libbem_hip.so (hipcc cross-compiles without a GPU)."""
    import subprocess
    r = subprocess.run(["make", "-j8", "-C", CSRC], capture_output=True, text=True)
    if r.returncode != 0:
        raise BemNativeError(f"building libbem_hip.so failed:\n{r.stdout}\n{r.stderr}")
    if verbose:
        print(r.stdout)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BemNativeError(
                f"{LIB_PATH} not found: the HIP library is required (no CPU fallback). "
                f"Build it with `make -C {CSRC}` or __graft_entry__.build().")
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _PROTOS.items():
            fn = getattr(L, name)          # AttributeError here = symbol missing from the build
            fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().bem_last_error()
        raise BemNativeError(f"{what or 'bem call'} failed (rc={rc}): {msg.decode() if msg else ''}")
