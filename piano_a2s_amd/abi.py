"""The C ABI as include/a2s.h declares it, read once: every `a2s_*` prototype as (name, restype, argtypes) and every `typedef struct a2s_*` as a
ctypes.Structure whose `_fields_` are the members in order.  hip.py binds the library and builds its argument blocks from this and from nothing
else, so the header is the one place where a type is written.  A type the reader does not know is an error that names the declaration."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "a2s.h")


class A2SError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "long": C.c_long, "long long": C.c_longlong, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_POINTEES = set(_SCALARS) | {"void", "uint8_t", "signed char", "unsigned"}          # what a data pointer may point to
_PROTO = re.compile(r"([\w\s*]+?)\b(a2s_\w+)\s*\(([^()]*)\)")
_STRUCT = re.compile(r"typedef\s+struct\s+(a2s_\w+)\s*\{(.*?)\}\s*\1\s*;", re.S)
_DECL = re.compile(r"(.*?)(\w+(?:\s*,\s*\w+)*)")                         # "<type> <name>[, <name>...]"


def _ctype(text, structs, where, result=False):
    """The ctypes twin of the C type `text`: data pointers -> c_void_p, `const char*` -> c_char_p, struct pointers -> POINTER(<struct>)."""
    stars = text.count("*")
    base = " ".join(re.sub(r"\bconst\b|\*", " ", text).split())
    if stars == 0 and (base in _SCALARS or (result and base == "void")):
        return _SCALARS.get(base)                                       # (None: a function that returns nothing)
    if stars == 1 and base == "char" and re.search(r"\bconst\b", text):
        return C.c_char_p
    if stars == 1 and base in structs:
        return C.POINTER(structs[base])
    if (stars == 1 and base in _POINTEES) or (stars == 2 and base == "float"):
        return C.c_void_p
    raise A2SError(f"include/a2s.h, {where}: unknown type {' '.join(text.split())!r}")


def _decls(decls, structs, where):
    """[(name, ctype)] of the declarations "<type> <name>[, <name>...]" (parameters, struct members)."""
    out = []
    for decl in decls:
        m = _DECL.fullmatch(decl)
        if m is None or not m.group(1).strip() or ("," in m.group(2) and "*" in m.group(1)):
            raise A2SError(f"include/a2s.h, {where}: cannot read the declaration {decl!r}")
        names = re.split(r"\s*,\s*", m.group(2))
        out += [(n, _ctype(m.group(1), structs, f"{where}, {names[0]}")) for n in names]
    return out


def parse(text):
    """Header text -> ([(name, restype, [argtypes])] in declaration order, {C struct name: Structure class})."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = "\n".join(l for l in text.splitlines() if not l.lstrip().startswith("#"))
    text = re.sub(r'extern\s+"C"\s*\{|\}\s*$', " ", text)
    structs, protos = {}, []
    for m in _STRUCT.finditer(text):
        fields = _decls(filter(None, map(str.strip, m.group(2).split(";"))), structs, f"struct {m.group(1)}")
        pyname = "".join(w.capitalize() for w in m.group(1).split("_")[1:])          # a2s_note_dec_args -> NoteDecArgs
        structs[m.group(1)] = type(pyname, (C.Structure,), {"_fields_": fields, "__doc__": f"`{m.group(1)}` of include/a2s.h: same members, same order."})
    for stmt in filter(None, map(str.strip, _STRUCT.sub(" ", text).split(";"))):
        m = _PROTO.fullmatch(stmt)
        if m is None:
            raise A2SError(f"include/a2s.h: neither a prototype nor a struct: {' '.join(stmt.split())[:80]!r}")
        params = [p.strip() for p in m.group(3).split(",")]
        args = _decls([] if params in ([""], ["void"]) else params, structs, m.group(2))
        protos.append((m.group(2), _ctype(m.group(1), structs, f"{m.group(2)}, return type", result=True), [t for _, t in args]))
    return protos, structs


def load(path=HEADER):
    try:
        with open(path) as f:
            return parse(f.read())
    except OSError as e:
        raise A2SError(f"the C ABI header is missing: {path} ({e}); the binding is derived from it") from e


PROTOTYPES, STRUCTS = load()          # this tree's header, read once per process: one set of classes
