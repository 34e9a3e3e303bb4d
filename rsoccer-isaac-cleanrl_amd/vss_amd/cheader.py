"""A C header's constants, structs and prototypes as ctypes -- the subset of C that include/vss.h is written in.

    h = parse(open("include/vss.h").read())
    h.constants["VSS_ABI_VERSION"]        # every `#define NAME <integer literal>`
    h.structs["vss_params"]               # a ctypes.Structure subclass per `typedef struct NAME { ... } NAME;`
    h.functions["vss_step"]               # (restype, [argtypes]) per prototype, in the header's order
    bind(lib, h)                          # set them on a ctypes.CDLL

Pointers (members, parameters, array parameters) are c_void_p: callers pass data_ptr() ints, None, byref(struct)
and ctypes arrays.  Scalars map through SCALARS.  A struct member may also be a struct that the header defined
earlier, by value or as an array (vss_setplay_play's entities).  Anything else -- a type outside the table, a struct
by value as a parameter or a result, a bit-field, a union, a struct defined inside a struct, a statement that is
neither a struct nor a prototype -- raises HeaderError with the name and the token: a guessed type would truncate a
pointer silently, so there is no guess.
stdlib only (no torch): tools and tests can parse a header without loading the GPU runtime.
"""
from __future__ import annotations

import ctypes
import re
from typing import NamedTuple

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}


class HeaderError(ValueError):
    pass


class Header(NamedTuple):
    constants: dict  # name -> int
    structs: dict    # C name -> ctypes.Structure subclass
    functions: dict  # name -> (restype, [argtypes])


def _ctype(decl: str, where: str):
    """The ctypes type of `decl`, a type with or without the declared name ("const float* x", "int32_t")."""
    if "*" in decl or "[" in decl:
        return ctypes.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if not 1 <= len(words) <= 2 or words[0] not in SCALARS:
        raise HeaderError(f"{where}: '{decl.strip()}' is not a pointer or one of {', '.join(SCALARS)}")
    return SCALARS[words[0]]


def _struct(name: str, body: str, constants: dict, structs: dict | None = None) -> type:
    bad = re.search(r"[{:]|\b(struct|union|enum)\b", body)
    if bad:
        raise HeaderError(f"struct {name}: '{bad.group()}' (nested struct, union, enum or bit-field) is not supported")
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = (d.strip() for d in decl.split(","))
        m = re.fullmatch(r"(.*?)(\w+)\s*(?:\[\s*(\w+)\s*\])?", first, re.S)
        if not m or not m.group(1).strip():
            raise HeaderError(f"struct {name}: cannot parse member '{decl}'")
        base, member, length = m.groups()
        words = [w for w in base.split() if w != "const"]
        if structs and len(words) == 1 and words[0] in structs:  # a struct the header defined earlier, by value
            ctype = structs[words[0]]
        else:
            ctype = _ctype(base, f"struct {name}.{member}")
        if length is not None:
            if not (length.isdigit() or length in constants):
                raise HeaderError(f"struct {name}.{member}: array length '{length}' is not an integer or a #define")
            ctype = ctype * (int(length) if length.isdigit() else constants[length])
        if more and (ctype is ctypes.c_void_p or length is not None or not all(re.fullmatch(r"\w+", d) for d in more)):
            raise HeaderError(f"struct {name}: only plain scalars may share a declaration, got '{decl}'")
        fields += [(member, ctype)] + [(d, ctype) for d in more]
    return type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"struct {name} of the parsed header"})


def _prototype(stmt: str):
    m = re.fullmatch(r"(?P<ret>[\w\s*]+?)(?P<name>\w+)\s*\((?P<params>[^()]*)\)", stmt, re.S)
    if not m:
        raise HeaderError(f"neither a struct nor a prototype: '{' '.join(stmt.split())[:120]}'")
    name, ret, params = m.group("name"), " ".join(m.group("ret").replace("*", " * ").split()), m.group("params").strip()
    if ret in ("const char *", "char *"):
        restype = ctypes.c_char_p
    elif ret == "void":
        restype = None
    elif "*" in ret:
        raise HeaderError(f"{name}: return type '{ret}' is a pointer other than const char*")
    else:
        restype = _ctype(ret, f"{name}: return type")
    if params in ("", "void"):
        return name, restype, []
    return name, restype, [_ctype(p, f"{name}: parameter {i}") for i, p in enumerate(params.split(","))]


def parse(text: str) -> Header:
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text).replace("\\\n", " ")
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S+)[ \t]*$", text, flags=re.M):
        try:
            constants[name] = int(value, 0)
        except ValueError:
            pass
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
    text, n_extern = re.subn(r'extern\s+"C"\s*\{', " ", text)

    structs = {}

    def take_struct(m):
        name, body, alias = m.groups()
        if name != alias:
            raise HeaderError(f"struct {name}: typedef'd under another name, '{alias}'")
        if name in structs:
            raise HeaderError(f"struct {name}: defined twice")
        structs[name] = _struct(name, body, constants, structs)
        return " "
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{((?:[^{}]|\{[^{}]*\})*)\}\s*(\w+)\s*;", take_struct, text)

    *stmts, tail = text.split(";")
    functions = {}
    for stmt in stmts:
        name, restype, argtypes = _prototype(stmt.strip())
        if name in functions:
            raise HeaderError(f"{name}: declared twice")
        functions[name] = (restype, argtypes)
    if tail.split() != ["}"] * n_extern:  # what follows the last ';': nothing but the closing brace of extern "C"
        raise HeaderError(f"neither a struct nor a prototype: '{' '.join(tail.split())[:120]}'")
    return Header(constants, structs, functions)


def bind(lib: ctypes.CDLL, header: Header) -> ctypes.CDLL:
    """Set restype and argtypes of every prototype of `header` on `lib`; a symbol it lacks is an AttributeError."""
    for name, (restype, argtypes) in header.functions.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib
