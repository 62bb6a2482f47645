"""Reader of include/ocrl_hip.h: the header is the one description of the C ABI, and the ctypes binding (_lib.py) is derived from it.

read() takes the header's text and returns its `#define NAME <integer>` constants, a ctypes.Structure class per struct typedef and
(restype, argtypes) per prototype.  The dialect is the header's own, plain C: comments, preprocessor lines, the extern "C" braces, opaque
and full struct typedefs, prototypes.  Anything else raises a ValueError that names the declaration; nothing is skipped.

Types: a pointer to a struct the header defines is POINTER(ThatStruct), `char*` is c_char_p, a sized array parameter of a scalar
(`int out[6]`) is POINTER(T * n), and every other pointer is c_void_p: opaque handles, device pointers, `T**`, and also host arrays such as
`const int* dims`, because the header cannot tell a host `int*` from a device one.  That is the one place where the binding is less typed
than a hand-written one could be; ctypes takes the arrays and byref() objects the callers pass for a c_void_p."""
import ctypes
import re
from types import SimpleNamespace

SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
           "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong, "size_t": ctypes.c_size_t,
           "char": ctypes.c_char, "unsigned char": ctypes.c_ubyte}
_DECLARATOR = r"(\w+)((?:\s*\[\s*\w+\s*\])*)"          # name, then any [n] suffixes
_DEFINE = r"\s*#\s*define\s+(\w+)\s+(-?\d+)\s*"


def read(text):
    """SimpleNamespace(consts {name: int}, structs {C name: Structure class}, functions {name: (restype, argtypes)}) of a header's text"""
    abi = SimpleNamespace(consts={}, structs={}, functions={})
    opaque = set()

    def fail(what, decl):
        raise ValueError(f"ocrl_hip.h: {what}: {' '.join(decl.split())!r}")

    def ctype(spec, decl, void_ok=False):
        """the ctypes type of `[const] base [*[const]]...`, or None for plain void"""
        stars = spec.count("*")
        base = " ".join(w for w in spec.replace("*", " ").split() if w != "const")
        if base not in SCALARS and base not in abi.structs and base not in opaque and base != "void":
            fail(f"unknown type {base!r} in", decl)
        if stars == 0:
            if base in SCALARS:
                return SCALARS[base]
            if base == "void" and void_ok:
                return None
            fail(f"{base!r} by value in", decl)           # a struct by value or an opaque one: the ABI has neither
        if stars == 1 and base in abi.structs:
            return ctypes.POINTER(abi.structs[base])
        return ctypes.c_char_p if (stars == 1 and base == "char") else ctypes.c_void_p

    def lengths(dims, decl):
        out = []
        for tok in re.findall(r"\w+", dims):
            if not tok.isdigit() and tok not in abi.consts:
                fail(f"array length {tok!r} is neither an integer nor an earlier #define in", decl)
            out.append(int(tok) if tok.isdigit() else abi.consts[tok])
        return out

    def struct(name, body, decl):
        fields = []
        for d in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = d.split(",")
            m = re.fullmatch(r"(.*?)" + _DECLARATOR, first.strip(), re.S)
            rest = [re.fullmatch(_DECLARATOR, r.strip()) for r in more]
            if not m or not all(rest) or (more and "*" in d):           # `float *a, b` would need C's declarator rules: not in the dialect
                fail(f"cannot parse field {d!r} of", decl)
            t = ctype(m.group(1), decl)
            for f in [m.groups()[1:]] + [r.groups() for r in rest]:
                ft = t
                for n in reversed(lengths(f[1], decl)):
                    ft = ft * n
                fields.append((f[0], ft))
        if not fields:
            fail("struct without fields", decl)
        camel = "".join(w.capitalize() for w in name.removeprefix("ocrl_").split("_"))
        abi.structs[name] = type(camel, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"{name} of include/ocrl_hip.h"})

    def prototype(ret, name, params, decl):
        args = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(r"(.*?)" + _DECLARATOR, p.strip(), re.S)
            if not m or not m.group(1).strip():
                fail(f"cannot parse parameter {p.strip()!r} of", decl)
            t, dims = ctype(m.group(1), decl), lengths(m.group(3), decl)
            if len(dims) > 1 or (dims and m.group(1).count("*")):
                fail(f"cannot parse parameter {p.strip()!r} of", decl)
            args.append(ctypes.POINTER(t * dims[0]) if dims else t)
        abi.functions[name] = (ctype(ret, decl, void_ok=True), args)

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    lines = text.splitlines()
    for i, line in enumerate(lines):                # preprocessor lines: an integer #define becomes a declaration in its place (an array
        if line.lstrip().startswith("#"):           # length must be an EARLIER one); guards, #include and #ifdef / #endif carry no ABI
            if re.fullmatch(_DEFINE, line):
                lines[i] = line + ";"
            elif re.fullmatch(r"\s*#\s*(define\s+\w+|include\s*<\w+\.h>|ifn?def\s+\w+|endif)\s*", line):
                lines[i] = ""
            else:
                fail("cannot parse preprocessor line", line)
    text, n = re.subn(r'extern\s+"C"\s*\{', " ", "\n".join(lines))
    if n:                                           # ... and the brace that closes it, the last thing in the header
        text = text.rstrip()
        if n > 1 or not text.endswith("}"):
            fail('extern "C" is not closed at the end of the header', text[-40:])
        text = text[:-1]
    pos = 0
    for d in re.finditer(r"((?:[^;{}]|\{[^{}]*\})*);", text):           # a declaration: up to a `;` outside braces
        decl = d.group(1)
        if text[pos:d.start()].strip():
            fail("cannot parse declaration", text[pos:d.end()])
        pos = d.end()
        if m := re.fullmatch(_DEFINE, decl):
            abi.consts[m.group(1)] = int(m.group(2))
        elif m := re.fullmatch(r"\s*typedef\s+struct\s+(\w+)\s+(\w+)\s*", decl):
            if m.group(1) != m.group(2):
                fail("opaque typedef under another name", decl)
            opaque.add(m.group(2))
        elif m := re.fullmatch(r"\s*typedef\s+struct\s*\w*\s*\{(.*)\}\s*(\w+)\s*", decl, re.S):
            struct(m.group(2), m.group(1), decl)
        elif m := re.fullmatch(r"\s*([\w\s\*]+?)\b(ocrl_\w+)\s*\(([^()]*)\)\s*", decl, re.S):
            prototype(*m.groups(), decl)
        else:
            fail("cannot parse declaration", decl)
    if text[pos:].strip():
        fail("cannot parse declaration", text[pos:])
    return abi
