"""ctypes binding of libdiffma_hip.so (the C ABI declared in include/diffma_hip.h).

The ctypes Structures, the constants (dtype and status codes, DM_FLAG_*, integer #defines) and every
function's argtypes are generated from the header text itself, so the Python view cannot drift from
the C one.  There is deliberately NO fallback: if the shared library is missing or a call fails, the
caller gets an exception (the product path never routes through the CPU oracle).
"""
from __future__ import annotations

import ctypes
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
HEADER = os.path.join(_ROOT, "include", "diffma_hip.h")
# DIFFMA_HIP_LIB: developer override used to A/B two builds of the kernels in one GPU session (tools/ab.sh)
LIB_PATH = os.environ.get("DIFFMA_HIP_LIB") or os.path.join(_HERE, "csrc", "libdiffma_hip.so")

_SCALARS = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double}


def _strip_comments(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _parse_constants(text: str):
    """Return {name: int} for every enumerator (dm_status, dm_dtype, DM_FLAG_*) and every integer `#define` of the header
    (the include guard has no value and is not one)."""
    text = _strip_comments(text)
    out = {}
    for body in re.findall(r"\benum\s*\{(.*?)\}", text, flags=re.S):
        for item in body.split(","):
            if item.strip():
                name, value = item.split("=")
                out[name.strip()] = int(value, 0)
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\w+)[ \t]*$", text, flags=re.M):
        out[name] = int(value, 0)
    return out


def _ctype_of(decl: str):
    """The ctypes type of one parameter declaration: any pointer is c_void_p, a scalar is its own type."""
    if "*" in decl:
        return ctypes.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if not words or words[0] not in _SCALARS:
        raise RuntimeError(f"cannot derive a ctypes type from {decl!r}")
    return _SCALARS[words[0]]


def _parse_structs(text: str):
    """Return {struct_name: [(field, ctype), ...]} for every `typedef struct { ... } name;`."""
    text = _strip_comments(text)
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = []
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            m = re.match(r"(const\s+)?(\w+)\s+(.*)$", decl)
            if not m:
                raise RuntimeError(f"cannot parse field declaration {decl!r} in {name}")
            base, rest = m.group(2), m.group(3)
            for item in rest.split(","):
                item = item.strip()
                fields.append((item.lstrip("* ").strip(), _ctype_of(f"{base} {item}")))
        out[name] = fields
    return out


def _parse_functions(text: str):
    text = _strip_comments(text)
    protos = re.findall(r"^\s*((?:const\s+)?\w+\s*\*?)\s*(dm_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M)
    return [(ret.strip(), name, args.strip()) for ret, name, args in protos]


def _argtypes_of(args: str):
    """The argtypes of a prototype's parameter list, from its text: `(void)` takes none."""
    return [] if args in ("void", "") else [_ctype_of(a) for a in args.split(",")]


with open(HEADER) as _f:
    _HEADER_TEXT = _f.read()

CONSTANTS = _parse_constants(_HEADER_TEXT)        # DM_F32.., DM_OK / DM_ERR_*, DM_FLAG_*, DM_ABI_VERSION, DM_LN_ROWS_PER_BLOCK, ...
STRUCT_FIELDS = _parse_structs(_HEADER_TEXT)
FUNCTIONS = _parse_functions(_HEADER_TEXT)
EXPORTED_SYMBOLS = [name for _, name, _ in FUNCTIONS]
ARGTYPES = {name: _argtypes_of(args) for _, name, args in FUNCTIONS}

# every constant and one ctypes.Structure per args struct, importable by its C name (from ._lib import DM_BF16, dm_gemm_args, ...)
globals().update(CONSTANTS)
globals().update({_name: type(_name, (ctypes.Structure,), {"_fields_": _fields}) for _name, _fields in STRUCT_FIELDS.items()})

_lib = None
_lock = threading.Lock()


class DiffmaHipError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.isfile(LIB_PATH):
            raise DiffmaHipError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C diffma-diffusion-mamba_amd/csrc`.  There is no CPU fallback."
            )
        # torch must own the HIP runtime of the process: importing it first makes libamdhip64.so.7
        # resolve to the copy torch already mapped, so streams/pointers are interchangeable.
        import torch  # noqa: F401

        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for ret, name, args in FUNCTIONS:
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = ctypes.c_char_p if "char" in ret else ctypes.c_int
            fn.argtypes = ARGTYPES[name]
        got = lib.dm_abi_version()
        want = CONSTANTS["DM_ABI_VERSION"]
        if got != want:
            raise DiffmaHipError(f"libdiffma_hip.so ABI {got} != header ABI {want}; rebuild the library")
        _lib = lib
    return _lib


def check(status: int, what: str):
    if status != 0:
        msg = load().dm_last_error().decode(errors="replace")
        raise DiffmaHipError(f"{what} failed with status {status}: {msg}")


def call(name: str, args_struct, stream_handle: int):
    lib = load()
    status = getattr(lib, name)(ctypes.byref(args_struct), ctypes.c_void_p(stream_handle))
    check(status, name)


def call_n(name: str, args_structs, stream_handle: int):
    """`name`_n(args[0..n), n, stream): the structs must be of one ctypes type; congruent neighbours share a launch."""
    lib = load()
    arr = (type(args_structs[0]) * len(args_structs))(*args_structs)
    status = getattr(lib, name + "_n")(ctypes.cast(arr, ctypes.c_void_p), len(args_structs), ctypes.c_void_p(stream_handle))
    check(status, name + "_n")


HAS_N = None


def has_n(name: str) -> bool:
    global HAS_N
    if HAS_N is None:
        HAS_N = {n[:-2] for n in EXPORTED_SYMBOLS if n.endswith("_n")}
    return name in HAS_N


def build_info() -> str:
    return load().dm_build_info().decode()
