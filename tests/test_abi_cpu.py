"""The Python side of the C ABI is DERIVED from include/a2s.h (piano_a2s_amd/abi.py), without a GPU: the reader finds every prototype the header
declares and hip.lib() types each of them; it refuses a type it does not know instead of guessing; a plain Python int in a `long` slot is not cut
to 32 bits; and every `.a2s_*()` call site of the tree has the arity of its prototype and, where it wraps an argument in a ctypes constructor,
the declared type.  (The C layout of the four argument blocks: tests/test_cabi.py.)"""
import ast
import ctypes as C
import glob
import os
import re

import pytest

from piano_a2s_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# trace-build-only symbols (tools/, -DRW_TRACE and the like): exported by measurement builds, not declared by the header, called untyped
UNDECLARED_OK = {"a2s_rows_trace_read", "a2s_conv_trace_read", "a2s_conv_wgrad_trace_read", "a2s_gemm_trace_read", "a2s_staff_emb_save_floats"}


@pytest.fixture(scope="module")
def libpath():
    from piano_a2s_amd import build
    return build.build()


@pytest.fixture(scope="module")
def protos():
    return {name: (restype, argtypes) for name, restype, argtypes in abi.PROTOTYPES}


def test_reader_finds_every_declared_prototype_and_lib_types_it(libpath, protos):
    header = open(os.path.join(ROOT, "include", "a2s.h")).read()
    declared = sorted(set(re.findall(r"\b(a2s_[a-z0-9_]+)\s*\(", header)))          # as tests/test_cabi.py derives it
    assert sorted(protos) == declared and len(abi.PROTOTYPES) == len(declared)
    from piano_a2s_amd import hip
    L = hip.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes and len(fn.argtypes) == len(argtypes), name
        assert fn.restype is restype, name
    assert L.a2s_last_error.restype is C.c_char_p and L.a2s_launch_count.restype is C.c_longlong and L.a2s_gemm_workspace_bytes.restype is C.c_size_t
    assert L.a2s_gemm_debug_tile.restype is None
    assert set(abi.STRUCTS) == {"a2s_note_dec_args", "a2s_note_dec_bwd_args", "a2s_beam_args", "a2s_align_args"}
    assert list(L.a2s_note_decoder_fwd_beam.argtypes[1:3]) == [C.POINTER(hip.NoteDecArgs), C.POINTER(hip.BeamArgs)]


def test_reader_maps_the_types_as_documented():
    protos, structs = abi.parse("typedef struct a2s_t { const float* p; long n; int a, b; size_t s; float f; const uint8_t* m; long long* l; } a2s_t;\n"
                                "const char* a2s_f(void);\n"
                                "size_t a2s_g(void* s, const a2s_t* t, const float* const* w, float* const* g, const signed char* c, double d, long long q,\n"
                                "             const char* key /* a comment */, int* out);\n"
                                "void a2s_h(int x);   // another\n")
    T = structs["a2s_t"]
    assert T.__name__ == "T" and T._fields_ == [("p", C.c_void_p), ("n", C.c_long), ("a", C.c_int), ("b", C.c_int), ("s", C.c_size_t), ("f", C.c_float),
                                                 ("m", C.c_void_p), ("l", C.c_void_p)]
    assert protos == [("a2s_f", C.c_char_p, []),
                      ("a2s_g", C.c_size_t, [C.c_void_p, C.POINTER(T), C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_longlong, C.c_char_p, C.c_void_p]),
                      ("a2s_h", None, [C.c_int])]


@pytest.mark.parametrize("text,names", [
    ("int a2s_good(int a);\nint a2s_bad(void* stream, unsigned n, float* out);\n", ("a2s_bad", "unsigned")),
    ("int a2s_bad2(void* stream, int** out);\n", ("a2s_bad2", "int**")),
    ("int a2s_bad5(char* text);\n", ("a2s_bad5", "char*")),
    ("short a2s_bad3(void);\n", ("a2s_bad3", "short")),
    ("int a2s_bad4(const a2s_later_args* args);\n", ("a2s_bad4", "a2s_later_args")),
    ("typedef struct a2s_blk { float* p; int16_t q; } a2s_blk;\nint a2s_f(const a2s_blk* b);\n", ("a2s_blk", "q", "int16_t")),
    ("typedef struct a2s_blk { float *p, *q; } a2s_blk;\n", ("a2s_blk",)),
    ("int a2s_f(int a);\nstatic int helper;\n", ("helper",)),
])
def test_reader_refuses_what_it_does_not_know(text, names):
    with pytest.raises(abi.A2SError) as e:
        abi.parse(text)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_missing_header_is_an_error(tmp_path):
    with pytest.raises(abi.A2SError, match="missing"):
        abi.load(str(tmp_path / "nowhere.h"))


def test_plain_int_in_a_long_slot_is_not_truncated(libpath):
    """a2s_bn_bwd_partial_floats(rows, C, F) = rows * C * 2 for F > 1 (host only, launches nothing): 2^32 + 5 rows differ from 5 rows."""
    from piano_a2s_amd import hip
    L = hip.lib()
    rows, Cc, F = (1 << 32) + 5, 3, 2
    plain = L.a2s_bn_bwd_partial_floats(rows, Cc, F)
    assert plain == L.a2s_bn_bwd_partial_floats(C.c_long(rows), C.c_int(Cc), C.c_int(F)) == rows * Cc * 2
    assert L.a2s_bn_bwd_partial_floats(rows % (1 << 32), Cc, F) == 5 * Cc * 2 != plain
    narrow = C.c_int(5)
    with pytest.raises(C.ArgumentError):
        L.a2s_bn_bwd_partial_floats(narrow, Cc, F)              # an explicit wrapper of another type is refused, not reinterpreted


def _ctypes_ctor(node):
    """`C.c_xxx(...)` / `ctypes.c_xxx(...)` -> the ctypes class, else None."""
    if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and isinstance(node.func.value, ast.Name)
            and node.func.value.id in ("C", "ctypes") and node.func.attr.startswith("c_")):
        return getattr(C, node.func.attr)
    return None


def test_every_call_site_conforms_to_its_prototype(protos):
    files = [os.path.join(ROOT, "bench.py")] + sorted(f for d in ("piano_a2s_amd", "tests", "tools")
                                                      for f in glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True))
    calls, bad = 0, []
    for path in files:
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr.startswith("a2s_")):
                continue
            name, where = node.func.attr, f"{os.path.relpath(path, ROOT)}:{node.lineno} {node.func.attr}"
            if name not in protos:
                if name not in UNDECLARED_OK:
                    bad.append(f"{where}: not declared in include/a2s.h")
                continue
            calls += 1
            if node.keywords:
                bad.append(f"{where}: keyword arguments")
            if any(isinstance(a, ast.Starred) for a in node.args):
                continue
            argtypes = protos[name][1]
            if len(node.args) != len(argtypes):
                bad.append(f"{where}: {len(node.args)} arguments, the prototype has {len(argtypes)}")
                continue
            for i, (a, want) in enumerate(zip(node.args, argtypes)):
                got = _ctypes_ctor(a)
                pointer = want in (C.c_void_p, C.c_char_p) or issubclass(want, C._Pointer)
                if got is not None and not (got is want or (pointer and got in (C.c_void_p, C.c_char_p))):
                    bad.append(f"{where}: argument {i} is wrapped as {got.__name__}, declared {want.__name__}")
    print(f"{calls} call sites of declared entry points in {len(files)} files")
    assert not bad, "\n".join(bad)
    assert calls >= 500, calls          # the walk sees the tree (571 call sites when this test was written)
