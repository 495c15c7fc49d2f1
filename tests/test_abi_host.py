"""The ctypes binding is derived from include/mi355_unet.h (unet_bssfp_amd/_lib.py).  CPU-only checks of that derivation:
the layout of every structure against what the C++ compiler makes of the real header, the parser on short strings (every
construct it takes, every construct it must refuse), hand-written signatures that between them cover every scalar kind and
both pointer rules, and the constants the Python side reads from the header."""
import ctypes as C
import os
import re
import subprocess

import pytest

from unet_bssfp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355_unet.h")
vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64


def test_layout_matches_the_compiler(tmp_path):
    """sizeof of every structure, offsetof and sizeof of every field: g++ on the real header is the authority, the field
    list comes from the parser -- a field the parser dropped changes a later offset or the size"""
    lines = ['#include "mi355_unet.h"', "#include <cstddef>", "#include <cstdio>", "int main() {"]
    for py, c in _lib._STRUCT_NAMES.items():
        lines.append(f'  std::printf("{py} - %zu 0\\n", sizeof({c}));')
        for name, _ in getattr(_lib, py)._fields_:
            lines.append(f'  std::printf("{py} {name} %zu %zu\\n", sizeof({c}::{name}), offsetof({c}, {name}));')
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    subprocess.check_call(["g++", "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)])
    rows = [line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert len(rows) == sum(1 + len(getattr(_lib, py)._fields_) for py in _lib._STRUCT_NAMES) and len(rows) > 200
    for py, name, size, offset in rows:
        cls = getattr(_lib, py)
        if name == "-":
            assert C.sizeof(cls) == int(size), py
        else:
            f = getattr(cls, name)
            assert (f.size, f.offset) == (int(size), int(offset)), (py, name)


def test_every_header_struct_has_its_python_name():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    typedefs = re.findall(r"\}\s*(mi355_\w+)\s*;", text)
    assert len(typedefs) == 12 and sorted(typedefs) == sorted(_lib._STRUCT_NAMES.values())
    for py in ("WpackDesc", "ConvDesc", "WgradDesc", "WreduceJob", "NormActDesc", "NormSmallDesc", "ResTailDesc", "QueueLoad",
               "QueueSource", "QueueSpatial", "QueueResampling", "ScalarTable"):
        cls = getattr(_lib, py)
        assert issubclass(cls, C.Structure) and cls.__name__ == py and py in _lib._STRUCT_NAMES
    assert dict(_lib.NormSmallDesc._fields_)["base"] is _lib.NormActDesc          # the by-value member is the class built earlier


def test_constants_read_from_the_header_keep_their_values():
    from unet_bssfp_amd import augment, data
    H = _lib.H
    assert (H["DT_F32"], H["DT_BF16"], H["DT_F64"], H["DT_FP8"]) == (0, 1, 2, 3)
    assert (_lib.DT_F32, _lib.DT_BF16, _lib.DT_FP8, _lib.EPOCH_MAX_SCALARS) == (0, 1, 3, 32)
    assert (H["OK"], H["ERR_ARG"], H["ERR_UNSUPPORTED"], H["ERR_HIP"]) == (0, -1, -2, -3)
    assert "UNET_H" not in H                                                     # the include guard is no constant
    assert H["AXIS_MAX_N"] == augment.AXIS_MAX_N == 128 and H["MOTION_MAX_IMAGES"] == augment.MOTION_MAX_IMAGES == 8
    assert data._STAGE_KIND == {augment.RandomBiasField: 1, augment.RandomNoise: 2, augment.RandomGamma: 3}
    assert (H["STAGE_BIAS_FIELD"], H["STAGE_NOISE"], H["STAGE_GAMMA"]) == (1, 2, 3)
    assert H["QUEUE_MAX_IMAGES"] == data._MAX_IMAGES == 4
    assert (H["MAX_PATCHES"], H["QUEUE_MAX_LOADS"], H["QUEUE_MAX_STAGES"]) == (48, 4, 3)
    assert _lib.QueueLoad.stage.size == 4 * H["QUEUE_MAX_STAGES"] and _lib.ScalarTable.src.size == 8 * H["EPOCH_MAX_SCALARS"]


# the type mapping, pinned by hand: int64_t among int32_t, double, uint64_t and float, struct pointers, c_char_p, int64_t return
PINNED = {
    "mi355_pack_ncdhw": (C.c_int, [vp, vp, i32, i32, i64, i32, i32, i32, i32, vp]),
    "mi355_dti_scalar_maps": (C.c_int, [vp, i32, i64, i64, i64, C.c_double, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp]),
    "mi355_aug_noise": (C.c_int, [vp, vp, i64, C.c_float, C.c_float, C.c_uint64, vp]),
    "mi355_patch_queue_gather_spatial": (C.c_int, [
        C.POINTER(_lib.QueueLoad), C.POINTER(_lib.QueueSpatial), i32, C.POINTER(_lib.QueueSource), C.POINTER(_lib.QueueResampling),
        vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, C.c_float, vp]),
    "mi355_last_error": (C.c_char_p, []),
    "mi355_conv_workspace_bytes": (i64, [C.POINTER(_lib.ConvDesc)]),
}


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signatures(name):
    res, args = _lib._SIGNATURES[name]
    assert res is PINNED[name][0]
    assert len(args) == len(PINNED[name][1]) and all(a is b for a, b in zip(args, PINNED[name][1])), args
    assert _lib.EXPORTED_SYMBOLS.index("mi355_version") == 0 and name in _lib.EXPORTED_SYMBOLS


def test_out_parameters_take_byref():
    """the int32_t* out-parameters of mi355_conv_num_tiles are c_void_p like every non-struct pointer; byref still converts"""
    assert _lib._SIGNATURES["mi355_conv_num_tiles"] == (C.c_int, [C.POINTER(_lib.ConvDesc), vp, vp])
    tiles, per = i32(-7), i32(-7)
    assert _lib.load().mi355_conv_num_tiles(None, C.byref(tiles), C.byref(per)) < 0      # null descriptor: refused on the host


# ---- the parser on short strings -------------------------------------------------------------------------------------

NAMES = {"mi355_in": "In", "mi355_t": "T"}


def parse(text, names=NAMES):
    return _lib.parse_header(text, names)


def test_parser_preprocessor_lines():
    consts, structs, sigs = parse("""
        /* a comment with #define MI355_NOT 1 and int f(void); in it
           over two lines */
        #ifndef MI355_X_H
        #define MI355_X_H
        #include <stddef.h>
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define MI355_A 7   /* trailing comment */
        #define MI355_NEG (-3)
        #define MI355_MINUS -2
        #ifdef __cplusplus
        }
        #endif
        #endif /* MI355_X_H */
        """)
    assert consts == {"A": 7, "NEG": -3, "MINUS": -2} and list(consts) == ["A", "NEG", "MINUS"]
    assert structs == {} and sigs == {}


def test_parser_structs():
    _, structs, _ = parse("""
        #define MI355_N 5
        typedef struct mi355_in { int64_t opaque[20]; } mi355_in;
        typedef struct mi355_t {
          const void* x0; int32_t c0; int32_t ld0;      /* several declarations on a line */
          int32_t tbase[3], tstep[3];                   /* several declarators in a declaration */
          float eps, momentum;
          int32_t stage[MI355_N];
          const float* src[MI355_N];
          mi355_in base;
          const uint64_t* seed_ptr; uint8_t* widx; int64_t* tracked; void* y; const double* m;
          uint64_t seed; double w; int flag;
        } mi355_t;
        """)
    assert list(structs) == ["mi355_in", "mi355_t"]
    In, T = structs["mi355_in"], structs["mi355_t"]
    assert (In.__name__, T.__name__) == ("In", "T") and issubclass(T, C.Structure)
    assert In._fields_ == [("opaque", i64 * 20)]
    assert T._fields_ == [
        ("x0", vp), ("c0", i32), ("ld0", i32), ("tbase", i32 * 3), ("tstep", i32 * 3), ("eps", C.c_float), ("momentum", C.c_float),
        ("stage", i32 * 5), ("src", vp * 5), ("base", In), ("seed_ptr", vp), ("widx", vp), ("tracked", vp), ("y", vp), ("m", vp),
        ("seed", C.c_uint64), ("w", C.c_double), ("flag", C.c_int)]
    assert all(typ is vp for name, typ in T._fields_ if name in ("x0", "seed_ptr", "widx", "tracked", "y", "m"))


def test_parser_prototypes():
    _, structs, sigs = parse("""
        typedef struct mi355_t { int32_t n; } mi355_t;
        int mi355_version(void);
        const char* mi355_last_error(void);
        int64_t mi355_bytes(const mi355_t* d);
        int32_t mi355_blocks(int64_t rows);
        int mi355_run(const mi355_t* d, mi355_t* job, const float* a, float* const* outs, const void* const* ptrs,
                      const int64_t* sizes, int32_t n, int64_t v, uint64_t seed, float lr, double w,
                      const uint8_t* mask, const char* tag, void* stream);
        """)
    T = structs["mi355_t"]
    assert list(sigs) == ["mi355_version", "mi355_last_error", "mi355_bytes", "mi355_blocks", "mi355_run"]
    assert sigs["mi355_version"] == (C.c_int, []) and sigs["mi355_last_error"] == (C.c_char_p, [])
    assert sigs["mi355_bytes"] == (i64, [C.POINTER(T)]) and sigs["mi355_blocks"] == (i32, [i64])
    assert sigs["mi355_run"] == (C.c_int, [C.POINTER(T), C.POINTER(T), vp, vp, vp, vp, i32, i64, C.c_uint64, C.c_float, C.c_double,
                                           vp, vp, vp])           # `const char*` is c_char_p as a return type only


REFUSED = {
    "unknown type name": "int mi355_f(size_t n);",
    "unknown field type": "typedef struct mi355_t { uint8_t flag; } mi355_t;",
    "unknown return type": "void mi355_f(int32_t n);",
    "function pointer parameter": "int mi355_f(int (*cb)(int), void* stream);",
    "function pointer field": "typedef struct mi355_t { void (*cb)(void); } mi355_t;",
    "bit-field": "typedef struct mi355_t { int32_t x : 3; } mi355_t;",
    "bit-field, no spaces": "typedef struct mi355_t { int32_t x:3; } mi355_t;",
    "union": "typedef union mi355_t { int32_t i; float f; } mi355_t;",
    "union member": "typedef struct mi355_t { union { int32_t i; float f; } u; } mi355_t;",
    "enum": "enum mi355_mode { MI355_A, MI355_B };",
    "unsigned parameter": "int mi355_f(unsigned n);",
    "unsigned field": "typedef struct mi355_t { unsigned int n; } mi355_t;",
    "#if": "#if 0\nint mi355_f(void);\n#endif",
    "#ifdef other than __cplusplus": "#ifdef MI355_EXTRA\nint mi355_f(void);\n#endif",
    "second #ifndef": "#ifndef MI355_X_H\n#define MI355_X_H\n#ifndef MI355_Y\nint mi355_f(void);\n#endif\n#endif",
    "non-integer define": "#define MI355_SCALE 1.5",
    "expression define": "#define MI355_B (MI355_A + 1)",
    "define outside the namespace": "#define OTHER 3",
    "struct without a Python name": "typedef struct mi355_new { int32_t n; } mi355_new;",
    "unknown array length": "typedef struct mi355_t { int32_t a[MI355_MISSING]; } mi355_t;",
    "declarators after a pointer type": "typedef struct mi355_t { float* a, b; } mi355_t;",
    "unnamed parameter": "int mi355_f(int32_t);",
    "empty parameter list": "int mi355_f();",
    "struct tag as a type": "int mi355_f(const struct mi355_t* d);",
    "line comment": "// int mi355_f(void);",
    "declaration without a semicolon": "int mi355_f(void)",
    "C++ block with other content": "#ifdef __cplusplus\nint mi355_f(void);\n#endif",
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_parser_refuses(case):
    """nothing is skipped: each of these raises, and a declaration after it does not make it pass"""
    for text in (REFUSED[case], REFUSED[case] + "\nint mi355_version(void);"):
        with pytest.raises(_lib.Mi355Error, match="mi355_unet.h: "):
            parse(text)


def test_parser_error_names_the_text():
    with pytest.raises(_lib.Mi355Error, match="unknown type.*size_t"):
        parse("int mi355_ok(void);\nint mi355_f(int32_t a,\n   size_t n);")
    with pytest.raises(_lib.Mi355Error, match="mi355_new"):
        parse(REFUSED["struct without a Python name"])
    with pytest.raises(_lib.Mi355Error, match="#if 0"):
        parse(REFUSED["#if"])


def test_missing_header_fails_loudly(monkeypatch):
    monkeypatch.setattr(_lib, "HEADER_PATH", "/nonexistent/mi355_unet.h")
    with pytest.raises(_lib.Mi355Error, match="/nonexistent/mi355_unet.h"):
        _lib._bind()
