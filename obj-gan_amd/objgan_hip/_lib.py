"""ctypes binding of libobjgan_hip.so (the C-ABI declared in include/objgan_hip.h).

The reference binds its native op with cffi through torch.utils.ffi (reference
image_generation/models/roi_align/_ext/roi_align/__init__.py:1-15); torch.utils.ffi no longer
exists and cffi is not installed here, so the zero-dependency equivalent -- ctypes -- is used.
There is NO fallback: if the shared library is missing or a call fails, an exception is raised.

No signature is written here: argtypes and restype of every entry point are read from the header's declarations
(parse_header, once per process, when this module is first imported), the same text every kernel source compiles
against.  A declaration the parser cannot classify is an ObjganHipError that names it, never a silent void*.
"""
import ctypes
import os
import re

from . import build as _build

_c_int = ctypes.c_int
_c_long = ctypes.c_long
_ptr = ctypes.c_void_p
_SCALARS = {"int": _c_int, "long": _c_long, "float": ctypes.c_float, "double": ctypes.c_double}


class ObjganHipError(RuntimeError):
    pass


def parse_header(text):
    """{name: (restype, argtypes)} of the `int | long objgan_x(...);` declarations in a C header's text.  A pointer of any
    kind is c_void_p, a scalar must be int / long / float / double; `()` and `(void)` take no arguments."""
    text = ";" + re.sub(r"/\*.*?\*/|//[^\n]*|^[ \t]*#[^\n]*", " ", text, flags=re.S | re.M)
    table = {}
    for ret, name, params in re.findall(r"(?<=[;{}])([^;{}()]*?)\b(objgan_\w+)\s*\(([^()]*)\)\s*;", text):
        if ret.strip() not in ("int", "long"):
            raise ObjganHipError("%s: return type %r is neither int nor long" % (name, ret.strip()))
        argtypes = []
        for p in [] if params.strip() in ("", "void") else params.split(","):
            scalar = re.fullmatch(r"\s*(?:const\s+)?(int|long|float|double)(?:\s+\w+)?\s*", p)
            if not scalar and not re.fullmatch(r"[\w\s]+\*[\w\s*]*", p):
                raise ObjganHipError("%s: cannot classify parameter %r" % (name, p.strip()))
            argtypes.append(_SCALARS[scalar.group(1)] if scalar else _ptr)
        table[name] = (_SCALARS[ret.strip()], argtypes)
    unparsed = sorted(set(re.findall(r"\b(objgan_\w+)\s*\(", text)) - set(table))
    if unparsed:
        raise ObjganHipError("cannot classify the declaration of " + ", ".join(unparsed))
    return table


_TABLE = parse_header(open(_build.HEADER).read())
# name -> argtypes of the functions that return int (1 ok, 0 bad args, <0 -hipError) / of the size queries that return long
SIGNATURES = {name: args for name, (ret, args) in _TABLE.items() if ret is _c_int}
LONG_RETURN = {name: args for name, (ret, args) in _TABLE.items() if ret is _c_long}

_LIB = None


def lib_path():
    return _build.LIB_PATH


def load(build_if_missing=True):
    """Load (building first if the .so is absent and hipcc is available). Never falls back."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        if not build_if_missing:
            raise ObjganHipError("libobjgan_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _build.build(verbose=False)
    # torch first: it ships its own libamdhip64, and the library's launches go to torch's streams.
    # Loaded the other way round, libobjgan_hip.so binds the system HIP runtime, the process ends up
    # with two runtimes, and every launch on a torch stream fails with hipErrorNoDevice (100).
    import torch  # noqa: F401
    lib = ctypes.CDLL(path)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the symbol is missing: loud by design
        fn.argtypes = argtypes
        fn.restype = _c_int
    for name, argtypes in LONG_RETURN.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = _c_long
    _LIB = lib
    return lib


def call(name, *args):
    """Call an entry point and turn the reference-style return code into an exception."""
    rc = getattr(load(), name)(*args)
    if rc == 1:
        return
    if rc == 0:
        raise ObjganHipError("%s: invalid arguments (returned 0)" % name)
    raise ObjganHipError("%s: HIP launch failed (hipError %d)" % (name, -rc))
