"""The C ABI as Python sees it, read from include/imcui_hip.h: the header is its only statement on this side.

A regular-expression reader of that one header (plain C: prototypes, `typedef struct { ... } name;`, integer `#define`s), not a C
parser.  It is strict: every statement left once comments, preprocessor lines and struct bodies are gone must be a prototype it
understands, and anything else raises HeaderError with the offending text.  Nothing is ever skipped -- a function left without a
restype would default to `int`, which truncates size_t and pointer returns.  Imports neither torch nor the library."""
from __future__ import annotations

import ctypes as C
import functools
import os
import re
from typing import NamedTuple

from .build import INCLUDE

HEADER_PATH = os.path.join(INCLUDE, "imcui_hip.h")

# types passed and returned by value
VALUES = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "long": C.c_long, "unsigned long": C.c_ulong,
          "long long": C.c_longlong, "unsigned long long": C.c_ulonglong, "float": C.c_float, "double": C.c_double,
          "size_t": C.c_size_t}  # fmt: skip
POINTEES = {"void", "char", "unsigned char", "short", "unsigned short"}  # known behind a `*` only (besides VALUES and the typedefs)
TYPE_WORDS = {w for t in VALUES.keys() | POINTEES for w in t.split()} | {"const", "struct", "signed"}


class HeaderError(ValueError):
    pass


class Header(NamedTuple):
    functions: dict  # name -> (restype, [argtype, ...])
    structs: dict  # typedef name -> [(field, ctype), ...] in declaration order
    defines: dict  # name -> int


def _ctype(text: str, typedefs: set, where: str, ret: bool = False):
    """`const float* const*` -> c_void_p, `size_t` -> c_size_t, ...: a type without its declarator."""
    words = text.replace("*", " * ").split()
    depth = words.count("*")
    base = " ".join(w for w in words if w not in ("const", "*"))
    if base not in VALUES and base not in POINTEES and base not in typedefs:
        raise HeaderError(f"unknown type '{text.strip()}' in: {where}")
    if depth:
        return C.c_char_p if base == "char" and depth == 1 else C.c_void_p
    if base == "void" and ret:
        return None
    if base not in VALUES:
        raise HeaderError(f"'{text.strip()}' is passed by value in: {where}")
    return VALUES[base]


def _named(text: str, where: str) -> tuple:
    """`const int* cnt` -> ("const int*", "cnt", None); `int n_row[MAXB]` -> ("int", "n_row", "MAXB")."""
    m = re.fullmatch(r"(.*?)\b(\w+)\s*(?:\[\s*(\w+)\s*\])?", text.strip(), re.S)
    if not m:
        raise HeaderError(f"cannot split '{text.strip()}' into a type and a name in: {where}")
    type_text, name, dim = m.groups()
    if not type_text.strip() or name in TYPE_WORDS:
        raise HeaderError(f"unnamed '{text.strip()}' in: {where}")
    return type_text, name, dim


def _struct_fields(body: str, typedefs: set, defines: dict, where: str) -> list:
    fields = []
    for stmt in filter(None, (" ".join(s.split()) for s in body.split(";"))):
        where_stmt = f"{where}: {stmt}"
        first, *more = stmt.split(",")  # `int M, N, K`: the first declarator carries the type
        decls = [_named(first, where_stmt)]
        base = decls[0][0].replace("*", " ")  # (a `*` belongs to its declarator)
        for d in more:
            m = re.fullmatch(r"\s*([\s*]*)(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", d)
            if not m:
                raise HeaderError(f"cannot read the declarator '{d.strip()}' in: {where_stmt}")
            decls.append((base + m.group(1), m.group(2), m.group(3)))
        for type_text, name, dim in decls:
            t = _ctype(type_text, typedefs, where_stmt)
            if dim is not None:
                if not dim.isdigit() and dim not in defines:
                    raise HeaderError(f"array size '{dim}' is neither a literal nor a #define in: {where_stmt}")
                t = t * (int(dim) if dim.isdigit() else defines[dim])
            fields.append((name, t))
    return fields


def parse(text: str) -> Header:
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    struct_re = r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;"
    bodies = re.findall(struct_re, text)
    text = re.sub(struct_re, " ", text)
    forward_re = r"\btypedef\s+struct\s+\w+\s+(\w+)\s*;"
    typedefs = {name for _, name in bodies} | set(re.findall(forward_re, text))
    text = re.sub(forward_re, " ", text)
    structs = {name: _struct_fields(body, typedefs, defines, name) for body, name in bodies}
    text = re.sub(r'\bextern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)  # the __cplusplus wrapper around everything
    functions = {}
    *stmts, tail = text.split(";")
    if tail.strip():
        raise HeaderError(f"declaration without ';': {' '.join(tail.split())}")
    for stmt in filter(None, (" ".join(s.split()) for s in stmts)):
        m = re.fullmatch(r"([\w\s*]+?)\b(imcui_hip_\w+)\s*\(([^()]*)\)", stmt)
        if not m:
            raise HeaderError(f"not a prototype this reader understands: {stmt}")
        ret, name, params = m.groups()
        if name in functions:
            raise HeaderError(f"{name} is declared twice")
        if not params.strip():
            raise HeaderError(f"empty parameter list (write `(void)`): {stmt}")
        args = [] if params.strip() == "void" else [_named(p, stmt) for p in params.split(",")]
        if any(dim is not None for _, _, dim in args):
            raise HeaderError(f"array parameter: {stmt}")
        functions[name] = (_ctype(ret, typedefs, stmt, ret=True), [_ctype(t, typedefs, stmt) for t, _, _ in args])
    mentioned = re.findall(r"\bimcui_hip_\w+\s*\(", text)
    if len(mentioned) != len(functions):
        raise HeaderError(f"{len(mentioned)} occurrences of `imcui_hip_<name>(` but {len(functions)} prototypes understood")
    return Header(functions, structs, defines)


@functools.lru_cache(maxsize=None)
def read(path: str = HEADER_PATH) -> Header:
    """The parsed header, read once per process."""
    with open(path) as f:
        return parse(f.read())
