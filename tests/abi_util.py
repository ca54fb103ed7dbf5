"""include/isdf_hip.h read once for tests/test_abi.py: its prototypes, struct fields and constant names (by regular expressions over
the comment-stripped text), the ctypes type each C parameter type must be bound as, and one C program, compiled with the host gcc,
that prints what the compiler makes of every struct, constant and size macro."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
TEXT = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(os.path.join(INCLUDE, "isdf_hip.h")).read(), flags=re.S)

SCALARS = {"int": C.c_int, "int8_t": C.c_int8, "uint8_t": C.c_uint8, "int32_t": C.c_int32, "uint32_t": C.c_uint32,
           "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}


def _type(decl):
    """'const float *  pts' -> 'const float*' (the declared name dropped; a lone type such as 'void' is kept)"""
    words = " ".join(decl.replace("*", "* ").split()).replace(" *", "*")
    return words.rsplit(" ", 1)[0] if " " in words and not words.endswith("*") else words


def prototypes():
    """name -> (return type, [parameter types]) of every isdf_* function, in header order"""
    out = {}
    for ret, name, params in re.findall(r"^[ \t]*([\w \t\*]+?)[ \t]*\b(isdf_\w+)[ \t]*\(([^()]*)\)[ \t]*;", TEXT, re.M):
        types = [_type(p) for p in params.split(",")]
        out[name] = (_type(ret + " _"), [] if types == ["void"] else types)
    return out


def struct_names():
    return re.findall(r"typedef\s+struct\s+(isdf_\w+)\s*\{", TEXT)


def struct_fields(name):
    """field names in declaration order: 'int32_t nx, ny, nz;' gives three, 'float spacing[3];' gives 'spacing'"""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), TEXT, re.S).group(1)
    return [re.search(r"(\w+)\s*(?:\[[^\]]*\]\s*)*$", d).group(1)
            for decl in body.split(";") if decl.strip() for d in decl.split(",")]


def constant_names():
    """the object-like #define ISDF_* names (the include guard has no value and is not one) and the enumerators"""
    defines = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(ISDF_\w+)[ \t]+\S", TEXT, re.M)
    enums = [n for body in re.findall(r"\benum\s*\{([^}]*)\}", TEXT) for n in re.findall(r"\b(ISDF_\w+)\b\s*(?:=|,|$)", body)]
    return defines + enums


def bindings(ctype, structs):
    """the ctypes types a parameter (or return value) of C type `ctype` may be bound as; structs: _ffi.STRUCTS"""
    t = ctype.replace("const ", "")
    if t == "char*":
        return (C.c_char_p,)
    if t == "isdf_nccl_allreduce_fn":
        return (C.c_void_p,)
    if not t.endswith("*"):
        return (SCALARS[t],)
    if t.startswith("isdf_"):
        return (C.POINTER(structs[t[:-1]]),)
    return (C.c_void_p,) + ((C.POINTER(SCALARS[t[:-1]]),) if t[:-1] in SCALARS else ())


def probe(tmp_path, structs=(), constants=(), macros=()):
    """Compile and run one C program against the header.  structs: C struct names; constants: names; macros: C expressions such as
    'ISDF_NN_WS_BYTES(257)'.  Returns (sizes, offsets, values): sizes[struct], offsets[struct][field] for every field the header
    declares, values[name or expression] as long long."""
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "isdf_hip.h"', 'int main(void) {']
    for s in structs:
        src.append('  printf("S %s - %%zu\\n", sizeof(%s));' % (s, s))
        src += ['  printf("F %s %s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f) for f in struct_fields(s)]
    src += ['  printf("V %s - %%lld\\n", (long long)(%s));' % (e.replace(" ", ""), e) for e in list(constants) + list(macros)]
    src += ['  return 0;', '}']
    (tmp_path / "probe.c").write_text("\n".join(src) + "\n")
    exe = str(tmp_path / "probe")
    subprocess.check_call(["gcc", "-I", INCLUDE, str(tmp_path / "probe.c"), "-o", exe])
    sizes, offsets, values = {}, {}, {}
    for kind, a, b, v in (line.split() for line in subprocess.check_output([exe], text=True).splitlines()):
        if kind == "S":
            sizes[a] = int(v)
        elif kind == "F":
            offsets.setdefault(a, {})[b] = int(v)
        else:
            values[a] = int(v)
    return sizes, offsets, values
