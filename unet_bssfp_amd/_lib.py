"""ctypes binding of the C-ABI library ``libmi355_unet.so``, derived from include/mi355_unet.h at import.

The header is the one statement of the ABI: its constants (``H``), structures and prototypes are parsed here, nothing is
restated.  The header stays within the small C subset named at its top; anything else fails the import and names the text.
The product path has NO fallback: if the library is missing or a call fails this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmi355_unet.so")   # the one shipped build; no environment override (tools/diaglib.py swaps it for A/B runs)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mi355_unet.h")

# Python class name -> C typedef name; a header struct without an entry fails the import
_STRUCT_NAMES = {
    "WpackDesc": "mi355_wpack_desc",
    "ConvDesc": "mi355_conv_desc",
    "WgradDesc": "mi355_wgrad_desc",
    "WreduceJob": "mi355_wreduce_job",
    "NormActDesc": "mi355_normact_desc",
    "NormSmallDesc": "mi355_normact_small_desc",
    "ResTailDesc": "mi355_restail_desc",
    "QueueLoad": "mi355_queue_load",
    "QueueSource": "mi355_queue_source",
    "QueueSpatial": "mi355_queue_spatial",
    "QueueResampling": "mi355_queue_resampling",
    "ScalarTable": "mi355_scalar_table",
}


class Mi355Error(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------------------------------------
# The header parser.  Type mapping: the scalars below; `const char*` as a return type is c_char_p; a pointer to a header
# struct is POINTER(its class); every other pointer, in arguments and in fields, is c_void_p.
# ---------------------------------------------------------------------------------------------------------------------
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_POINTEES = set(_SCALARS) | {"void", "char", "uint8_t"}         # what a pointer that becomes c_void_p may point to
_DEFINE = re.compile(r"#define\s+MI355_(\w+)\s+(-?\d+|\(-?\d+\))")
_DECLARATOR = r"\w+(?:\s*\[\s*\w+\s*\])?"
_FIELD = re.compile(rf"(.*?[\s*])\s*({_DECLARATOR}(?:\s*,\s*{_DECLARATOR})*)", re.S)
_PARAM = re.compile(r"\s*(.*?[\s*])\s*\w+\s*", re.S)
_STRUCT = re.compile(r"\s*typedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"\s*([\w\s*]*?[\s*])(\w+)\s*\(([^()]*)\)\s*;")


def _bad(what: str, text: str) -> Mi355Error:
    return Mi355Error(f"mi355_unet.h: {what}: {' '.join(text.split())!r} -- the binding is derived from the header, "
                      "which must stay within the C subset stated at its top")


def _ctype(text: str, structs: dict, ret: bool = False):
    words = text.replace("*", " * ").split()
    stars = words.count("*")
    base = [w for w in words if w not in ("const", "*")]
    if len(base) == 1:
        base = base[0]
        if stars == 0 and base in _SCALARS:
            return _SCALARS[base]
        if stars == 0 and base in structs:
            return structs[base]
        if stars == 1 and base in structs:
            return C.POINTER(structs[base])
        if ret and words == ["const", "char", "*"]:
            return C.c_char_p
        if stars and (base in _POINTEES or base in structs):
            return C.c_void_p
    raise _bad("unknown type", text)


def _length(text: str, consts: dict) -> int:
    text = text.strip()
    if text.isdigit():
        return int(text)
    if text.startswith("MI355_") and text[6:] in consts:
        return consts[text[6:]]
    raise _bad("array length is neither a literal nor a known MI355_ constant", text)


def parse_header(text: str, names: dict):
    """``(constants, structures, signatures)`` of a header in the subset: {NAME: int} of every ``#define MI355_NAME``,
    {C typedef name: ctypes.Structure subclass named names[typedef]} and {function: (restype, argtypes)}, all in header
    order.  No declaration is skipped: what is not recognised raises Mi355Error."""
    consts, structs, sigs = {}, {}, {}
    guard, cpp, code = None, False, []
    for line in re.sub(r"/\*.*?\*/", " ", text, flags=re.S).splitlines():
        line = line.strip()
        m = _DEFINE.fullmatch(line)
        if m:
            consts[m[1]] = int(m[2].strip("()"))
        elif guard is None and re.fullmatch(r"#ifndef\s+\w+", line):
            guard = line.split()[1]
        elif line == "#ifdef __cplusplus":
            cpp = True
        elif line == "#endif":
            cpp = False
        elif line == f"#define {guard}" or re.fullmatch(r"#include\s*<[\w./]+>", line) or (cpp and line in ('extern "C" {', "}")):
            pass
        elif line.startswith("#") or cpp:
            raise _bad("unsupported preprocessor line", line)
        else:
            code.append(line)
    code, pos = "\n".join(code).strip(), 0
    while pos < len(code):
        m = _STRUCT.match(code, pos) or _PROTO.match(code, pos)
        if not m:
            raise _bad("unrecognised declaration", code[pos:].split(";")[0][:200])
        if m.re is _STRUCT:
            if m[2] not in names:
                raise _bad("struct without a Python name in _STRUCT_NAMES", m[2])
            fields = []
            for decl in filter(None, (d.strip() for d in m[1].split(";"))):
                f = _FIELD.fullmatch(decl)
                if not f:
                    raise _bad("unrecognised field declaration", decl)
                declarators = f[2].split(",")
                if "*" in f[1] and len(declarators) > 1:
                    raise _bad("several declarators after a pointer type", decl)
                typ = _ctype(f[1], structs)
                for d in declarators:
                    name, _, length = d.strip().rstrip("]").partition("[")
                    fields.append((name.strip(), typ * _length(length, consts) if length else typ))
            structs[m[2]] = type(names[m[2]], (C.Structure,), {"_fields_": fields})
        else:
            argtypes = []
            for arg in ([] if m[3].strip() == "void" else m[3].split(",")):
                p = _PARAM.fullmatch(arg)
                if not p:
                    raise _bad("unrecognised parameter", arg)
                argtypes.append(_ctype(p[1], structs))
            sigs[m[2]] = (_ctype(m[1], structs, ret=True), argtypes)
        pos = m.end()
    return consts, structs, sigs


def _bind():
    try:
        with open(HEADER_PATH, encoding="utf-8") as f:
            text = f.read()
    except OSError as e:
        raise Mi355Error(f"{HEADER_PATH} not found: the ctypes binding is derived from the C header ({e})") from e
    consts, structs, sigs = parse_header(text, {c: py for py, c in _STRUCT_NAMES.items()})
    absent = sorted(set(_STRUCT_NAMES.values()) - set(structs))
    if absent:
        raise _bad("structs named in _STRUCT_NAMES are not in the header", " ".join(absent))
    return consts, {cls.__name__: cls for cls in structs.values()}, sigs


H, _structs, _SIGNATURES = _bind()      # H["DT_BF16"] = MI355_DT_BF16, ...
globals().update(_structs)              # WpackDesc, ConvDesc, ... (the keys of _STRUCT_NAMES)
DT_F32, DT_BF16, DT_FP8 = H["DT_F32"], H["DT_BF16"], H["DT_FP8"]
EPOCH_MAX_SCALARS = H["EPOCH_MAX_SCALARS"]
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lock = threading.Lock()
_lib = None


def load():
    """Load (once) and return the ctypes library object.  Raises if the .so is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise Mi355Error(
                    f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
            lib = C.CDLL(LIB_PATH)
            for name, (res, args) in _SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().mi355_last_error().decode("utf-8", "replace")
        raise Mi355Error(f"{what or 'mi355 call'} failed ({rc}): {msg}")
