"""CPU-only: the ctypes binding is derived from include/ocrl_hip.h (ocrl_amd/_abi.py).  The reader on literal snippets, one per construct
of the header's dialect; every struct's layout against the compiler's own sizeof / offsetof; and every declared function's prototype on
the loaded library."""
import ctypes
import os
import re
import subprocess
from ctypes import POINTER, c_char_p, c_float, c_int, c_longlong, c_size_t, c_ubyte, c_uint, c_ulonglong, c_void_p

import pytest

from ocrl_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"ocrl_slate_config": "SlateConfig", "ocrl_iodine_config": "IodineConfig", "ocrl_gemm_desc": "GemmDesc", "ocrl_conv_desc": "ConvDesc",
           "ocrl_conv_wgrad_desc": "ConvWgradDesc", "ocrl_xattn_desc": "XattnDesc", "ocrl_acnet_desc": "AcnetDesc",
           "ocrl_sprite_env_desc": "SpriteEnvDesc", "ocrl_scenes_desc": "ScenesDesc", "ocrl_flat_segment": "FlatSegment"}


def header():
    return open(os.path.join(ROOT, "include", "ocrl_hip.h")).read()


def layout(cls):
    return [(n, getattr(cls, n).offset, getattr(cls, n).size) for n, _ in cls._fields_]


# ---- the reader, construct by construct
def test_comments_preprocessor_lines_and_extern_c():
    abi = _abi.read('/* a comment; with int f(void); inside */\n#ifndef G_H\n#define G_H\n#include <stddef.h>\n#ifdef __cplusplus\nextern "C" {\n'
                    '#endif\n#define OCRL_N 7\n  #  define OCRL_NEG -3\nint ocrl_f(void);\n#ifdef __cplusplus\n}\n#endif\n#endif\n')
    assert abi.consts == {"OCRL_N": 7, "OCRL_NEG": -3} and abi.functions == {"ocrl_f": (c_int, [])} and abi.structs == {}


def test_opaque_typedef_is_a_void_pointer():
    abi = _abi.read("typedef struct ocrl_h ocrl_h;\nint ocrl_make(ocrl_h** out);\nvoid ocrl_drop(ocrl_h* h);\nint ocrl_n(const ocrl_h* h);")
    assert abi.structs == {}
    assert abi.functions == {"ocrl_make": (c_int, [c_void_p]), "ocrl_drop": (None, [c_void_p]), "ocrl_n": (c_int, [c_void_p])}


def test_struct_declarators_pointers_and_arrays():
    abi = _abi.read("#define OCRL_L 8\n"
                    "typedef struct ocrl_t {\n    const float* A; float* C; int* idx;     /* pointers */\n    int M, N, K; float alpha;\n"
                    "    unsigned long long seed; unsigned site_p, site_o; long long s; size_t n; unsigned char b; double x;\n"
                    "    int n3[3], c[OCRL_L];\n    int dims[3][OCRL_L];\n} ocrl_t;\n"
                    "typedef struct { int H; } ocrl_untagged;")
    T = abi.structs["ocrl_t"]
    assert T.__name__ == "T" and issubclass(T, ctypes.Structure)
    assert T._fields_ == [("A", c_void_p), ("C", c_void_p), ("idx", c_void_p), ("M", c_int), ("N", c_int), ("K", c_int), ("alpha", c_float),
                          ("seed", c_ulonglong), ("site_p", c_uint), ("site_o", c_uint), ("s", c_longlong), ("n", c_size_t), ("b", c_ubyte),
                          ("x", ctypes.c_double), ("n3", c_int * 3), ("c", c_int * 8), ("dims", (c_int * 8) * 3)]
    d = T()
    d.dims[2][7] = 5                                            # dims[3][8]: the first index is the outer one, as in C
    assert T.dims.offset + 4 * (2 * 8 + 7) + 4 == T.dims.offset + T.dims.size and d.dims[2][7] == 5
    assert abi.structs["ocrl_untagged"]._fields_ == [("H", c_int)]


def test_struct_on_one_line():
    abi = _abi.read("typedef struct { float* p; const float* g; float* s0; float* s1; long long n; } ocrl_flat_segment;   /* s0, s1 */")
    S = abi.structs["ocrl_flat_segment"]
    assert S.__name__ == "FlatSegment" and layout(S) == [("p", 0, 8), ("g", 8, 8), ("s0", 16, 8), ("s1", 24, 8), ("n", 32, 8)]


def test_prototypes():
    abi = _abi.read("typedef struct ocrl_d { int B; } ocrl_d;\ntypedef struct ocrl_h ocrl_h;\n"
                    "int ocrl_a(const ocrl_d* d, const float* x, const float* const* w, float* const* dw, float** ptr,\n"
                    "           const float* uniforms /* NULL = draw */, int n, unsigned site, float p, double q, long long R,\n"
                    "           unsigned long long seed, size_t ws_floats, const unsigned char* mask, char* name, const char* key,\n"
                    "           int shape[4], const float lr[3], int* ndim, void* stream);\n"
                    "size_t ocrl_b(void);\nlong long ocrl_c(const ocrl_h* h);\nconst char* ocrl_e(void);\nfloat* ocrl_f(const ocrl_h* h);\n"
                    "void ocrl_g(ocrl_h* h);\nunsigned long long ocrl_i(int const n);")
    D = abi.structs["ocrl_d"]
    assert abi.functions["ocrl_a"] == (c_int, [POINTER(D), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_uint, c_float,
                                               ctypes.c_double, c_longlong, c_ulonglong, c_size_t, c_void_p, c_char_p, c_char_p,
                                               POINTER(c_int * 4), POINTER(c_float * 3), c_void_p, c_void_p])
    assert abi.functions["ocrl_b"] == (c_size_t, []) and abi.functions["ocrl_c"] == (c_longlong, [c_void_p])
    assert abi.functions["ocrl_e"] == (c_char_p, []) and abi.functions["ocrl_f"] == (c_void_p, [c_void_p])
    assert abi.functions["ocrl_g"] == (None, [c_void_p]) and abi.functions["ocrl_i"] == (c_ulonglong, [c_int])


@pytest.mark.parametrize("text, named", [
    ("int ocrl_f(int (*cb)(int));", "ocrl_f"),                                  # a function pointer
    ("int ocrl_f(int);", "ocrl_f"),                                             # a parameter without a name
    ("int ocrl_f(short n);", "short"),                                          # a base type outside the dialect
    ("int ocrl_f(ocrl_nobody* h);", "ocrl_nobody"),                             # a struct that was never declared
    ("typedef struct ocrl_s { int a; } ocrl_s;\nint ocrl_f(ocrl_s s);", "ocrl_s"),   # a struct by value
    ("int ocrl_f(int a[2][2]);", "a[2][2]"),                                    # a 2-D array parameter
    ("typedef struct { float *a, b; } ocrl_s;", "float *a, b"),                 # one declaration, pointer and scalar declarators
    ("typedef struct { int a[OCRL_LATER]; } ocrl_s;\n#define OCRL_LATER 4", "OCRL_LATER"),     # a length defined after its use
    ("typedef struct { int a : 3; } ocrl_s;", "int a : 3"),                     # a bit field
    ("typedef struct { } ocrl_s;", "ocrl_s"),
    ("typedef struct ocrl_a ocrl_b;", "ocrl_a ocrl_b"),
    ("typedef int ocrl_int;", "typedef int ocrl_int"),
    ("enum ocrl_e { A, B };", "enum ocrl_e"),
    ("static inline int ocrl_f(void) { return 0; }", "ocrl_f"),
    ("int ocrl_f(void)", "ocrl_f"),                                             # no closing semicolon
    ("int ocrl_f(void);\n}", "}"),
    ('extern "C" {\nint ocrl_f(void);', "ocrl_f"),
    ("#define OCRL_X (1 << 3)", "OCRL_X"),
    ("#define OCRL_F(x) x", "OCRL_F"),
    ("#pragma once", "pragma"),
])
def test_what_the_reader_cannot_parse_raises_and_names_it(text, named):
    with pytest.raises(ValueError, match="ocrl_hip.h: ") as e:
        _abi.read(text)
    assert named in str(e.value)


# ---- the real header
def test_header_constants_and_struct_names():
    abi = _abi.read(header())
    assert abi.consts == {n: int(v) for n, v in re.findall(r"^#define (OCRL_\w+) (\d+)$", header(), re.M)} and len(abi.consts) == 15
    assert abi.consts is not _lib.CONSTANTS and abi.consts == _lib.CONSTANTS
    assert _lib.CONSTANTS["OCRL_ABI_VERSION"] == 5 and _lib.FLAT_MAX_SEGMENTS == 8
    assert {n: c.__name__ for n, c in _lib.ABI.structs.items()} == STRUCTS
    assert all(getattr(_lib, py) is _lib.ABI.structs[c] for c, py in STRUCTS.items())


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof and every field's offsetof and size, printed by a C program that includes the header and is compiled with the compiler the
    library was built with (csrc/Makefile's HIPCC), against the ctypes classes field by field"""
    hdr = re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)
    lines = []
    for c in STRUCTS:
        body = re.search(r"typedef struct\s*\w*\s*\{([^{}]*)\}\s*" + c + r"\s*;", hdr).group(1)
        names = [re.sub(r"\[.*", "", d).split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for d in decl.split(",")]
        assert len(names) >= 2
        lines.append(f'    printf("{c} %zu\\n", sizeof({c}));')
        lines += [f'    printf("{c}.{n} %zu %zu\\n", offsetof({c}, {n}), sizeof((({c}*)0)->{n}));' for n in names]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ocrl_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n    return 0;\n}\n")
    makefile = open(os.path.join(ROOT, "ocrl_amd", "csrc", "Makefile")).read()
    cc = os.environ.get("HIPCC") or re.search(r"^HIPCC \?= (\S+)$", makefile, re.M).group(1)
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True, capture_output=True, text=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    want = []
    for c, py in STRUCTS.items():
        cls = getattr(_lib, py)
        want.append(f"{c} {ctypes.sizeof(cls)}")
        want += [f"{c}.{n} {off} {size}" for n, off, size in layout(cls)]
    assert out[:-1] == want and out[-1] == ""
    assert len(want) == 10 + sum(len(getattr(_lib, py)._fields_) for py in STRUCTS.values()) == 10 + 189


def test_every_declared_function_is_bound():
    """argument count, struct-pointer parameters and non-int return types of every prototype, counted from the header's text without the
    reader, against what the loaded library carries"""
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)
    protos = re.findall(r"([\w \*]+?)\b(ocrl_\w+)\s*\(([^()]*)\)\s*;", hdr)
    assert len(protos) == 146 == len(set(n for _, n, _ in protos)) == len(_lib.ABI.functions)
    returns = {"int": c_int, "void": None, "size_t": c_size_t, "long long": c_longlong, "const char*": c_char_p, "float*": c_void_p}
    seen = set()
    for ret, name, params in protos:
        f = getattr(L, name)
        params = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
        assert len(f.argtypes) == len(params), name
        for t, p in zip(f.argtypes, params):
            m = re.fullmatch(r"(?:const )?(ocrl_\w+)\* \w+", p)
            if m and m.group(1) in STRUCTS:
                assert t is POINTER(getattr(_lib, STRUCTS[m.group(1)])), (name, p)
                seen.add(m.group(1))
            else:
                assert not issubclass(t, ctypes._Pointer) or re.search(r"\w+\[\d+\]$", p), (name, p)
                assert (t is c_void_p or t is c_char_p or issubclass(t, ctypes._Pointer)) == ("*" in p or "[" in p), (name, p)
        assert f.restype is returns[ret.strip()], name
    assert seen == set(STRUCTS)                                 # every struct is some function's parameter


def test_load_checks_every_reported_struct_size(monkeypatch):
    """lib() compares each struct that has a <struct>_size() function with the library, the GEMM descriptor among them, and the library's
    ABI version with the header's; a mismatch names the struct and both sizes"""
    sized = sorted(c for c in STRUCTS if c + "_size" in _lib.ABI.functions)
    assert sized == ["ocrl_acnet_desc", "ocrl_conv_desc", "ocrl_conv_wgrad_desc", "ocrl_gemm_desc", "ocrl_slate_config", "ocrl_sprite_env_desc",
                     "ocrl_xattn_desc"]
    L = _lib.lib()
    assert all(getattr(L, c + "_size")() == ctypes.sizeof(getattr(_lib, STRUCTS[c])) for c in sized)
    longer = type("GemmDesc", (ctypes.Structure,), {"_fields_": _lib.GemmDesc._fields_ + [("one_more", c_longlong)]})
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.ABI.structs, "ocrl_gemm_desc", longer)
    with pytest.raises(RuntimeError, match="ocrl_gemm_desc is 352 bytes, this binding's GemmDesc 360"):
        _lib.lib()
    monkeypatch.undo()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.CONSTANTS, "OCRL_ABI_VERSION", 6)
    with pytest.raises(RuntimeError, match="ABI version mismatch: the library is 5, include/ocrl_hip.h 6"):
        _lib.lib()
