"""The library's run-time switches (csrc/a2s_switches.h) without a GPU: the library loads and answers a2s_debug_set / a2s_debug_get on the CPU.
The expected values are the contract recorded from the library before the switches became one table -- they are written out here, not read from
the table.  Every check that depends on a fresh process (defaults, the environment, hip.lib()) runs in a child process."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = (0, 1, 2, 5, 300)

ONOFF_DEFAULT_1 = ("dec_fused", "dec_persist", "gru_persist", "gru_fused", "dec_mid", "attn_pair", "attn_defer_combine", "staff_emb_fast")
ONOFF_DEFAULT_0 = ("gru_persist_alone", "attn_bulk_cap", "persist_force_agent", "persist_inject_abort")
STORED = {"attn_fused_combine": 0, "attn_nt": 64, "attn_deep": 24, "conv_rows": 7, "conv_bf16x3": 3, "conv_f16x2": 3, "wgrad_rows": 1, "conv_c1_fast": 1,
          "wgrad_f16x2": 1, "wgrad_bf16x3": 1, "gemm_bf16x3": 1, "gemm_f16x2": 1, "dec_fused_max_rows": 192}
COUNTERS = ("dec_persist_launches", "dec_mid_launches", "attn_pair_launches", "attn_pair_bwd_launches")
ENV = {"A2S_CONV_ROWS": "conv_rows", "A2S_WGRAD_ROWS": "wgrad_rows", "A2S_GRU_PERSIST": "gru_persist", "A2S_DEC_PERSIST": "dec_persist", "A2S_DEC_FUSED": "dec_fused"}
SETTABLE = ONOFF_DEFAULT_1 + ONOFF_DEFAULT_0 + tuple(STORED) + ("attn_pair_fused_rows",)

# printed by the child: {"default": {key: value}, "set": {key: [[return code, value read back] for v in VALUES]}}
PROBE = """
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
keys = sys.argv[2].split(",")
out = {"default": {k: L.a2s_debug_get(k.encode()) for k in keys}, "set": {}}
for k in keys:
    out["set"][k] = [[L.a2s_debug_set(k.encode(), v), L.a2s_debug_get(k.encode())] for v in %r]
print(json.dumps(out))
""" % (VALUES,)


@pytest.fixture(scope="module")
def libpath():
    from piano_a2s_amd import build
    return build.build()


def _child(code, args=(), env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("A2S_")}
    e.update(env or {})
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", code, *args], capture_output=True, text=True, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def _probe(libpath, keys, env=None):
    return _child(PROBE, (libpath, ",".join(keys)), env)


def test_defaults_and_stored_values(libpath):
    got = _probe(libpath, SETTABLE + COUNTERS + ("gemm_tile",))
    for k in ONOFF_DEFAULT_1 + ONOFF_DEFAULT_0:
        assert got["default"][k] == (1 if k in ONOFF_DEFAULT_1 else 0), k
        assert got["set"][k] == [[0, 0 if v == 0 else 1] for v in VALUES], k
    for k, default in STORED.items():
        assert got["default"][k] == default, k
        assert got["set"][k] == [[0, v] for v in VALUES], k
    # read back under the cap "dec_fused_max_rows", which the loop above left at 300
    assert got["default"]["attn_pair_fused_rows"] == 32
    assert got["set"]["attn_pair_fused_rows"] == [[0, v] for v in VALUES]
    # write-only
    assert got["default"]["gemm_tile"] == -1 and got["set"]["gemm_tile"] == [[0, -1]] * len(VALUES)
    # read-only
    for k in COUNTERS:
        assert got["default"][k] == 0 and got["set"][k] == [[-1, 0]] * len(VALUES), k


def test_pair_fused_rows_reads_back_under_the_fused_cap(libpath):
    got = _probe(libpath, ("attn_pair_fused_rows", "dec_fused_max_rows"))
    # "attn_pair_fused_rows" is probed first, at the default cap of 192: 300 reads back 192
    assert got["set"]["attn_pair_fused_rows"] == [[0, 0], [0, 1], [0, 2], [0, 5], [0, 192]]
    assert got["default"]["dec_fused_max_rows"] == 192


def test_unknown_and_null_keys(libpath):
    import ctypes
    L = ctypes.CDLL(libpath)
    L.a2s_last_error.restype = ctypes.c_char_p
    assert L.a2s_debug_set(b"no_such_key", 1) == -1
    assert L.a2s_last_error() == b"a2s_debug_set: unknown key no_such_key"
    assert L.a2s_debug_get(b"no_such_key") == -1
    assert L.a2s_debug_set(None, 1) == -1
    assert L.a2s_debug_get(None) == -1


def test_environment_overrides_the_defaults_once(libpath):
    keys = tuple(ENV.values())
    got = _probe(libpath, keys, env={name: "0" for name in ENV})
    for k in keys:
        assert got["default"][k] == 0, k
        expect = [[0, v] for v in VALUES] if k in STORED else [[0, 0 if v == 0 else 1] for v in VALUES]
        assert got["set"][k] == expect, k          # still settable: a later a2s_debug_set wins
    got = _probe(libpath, keys, env={"A2S_CONV_ROWS": "3", "A2S_WGRAD_ROWS": "2", "A2S_GRU_PERSIST": "1", "A2S_DEC_PERSIST": "yes", "A2S_DEC_FUSED": "0x"})
    assert got["default"] == {"conv_rows": 3, "wgrad_rows": 2, "gru_persist": 1, "dec_persist": 1, "dec_fused": 0}


@pytest.mark.parametrize("name", ["A2S_CONV_ROWS", "A2S_WGRAD_ROWS"])
def test_unparsable_mask_is_an_error_of_lib(libpath, name):
    code = """
import json
from piano_a2s_amd import hip
seen = []
for _ in range(2):
    try:
        hip.lib()
        seen.append("loaded")
    except hip.A2SError as e:
        seen.append(str(e))
print(json.dumps(seen))
"""
    seen = _child(code, env={name: "seven"})
    assert len(seen) == 2 and all(s.startswith(name + "=seven") for s in seen), seen


def test_arith_is_validated_before_the_library_is_published(libpath):
    code = """
import json
from piano_a2s_amd import hip
seen = []
for _ in range(2):
    try:
        hip.lib()
        seen.append("loaded")
    except hip.A2SError as e:
        seen.append("A2SError")
print(json.dumps(seen))
"""
    assert _child(code, env={"A2S_ARITH": "nonsense"}) == ["A2SError", "A2SError"]


@pytest.mark.parametrize("arith,zero", [("bf16x3", ("conv_f16x2", "wgrad_f16x2", "gemm_f16x2")),
                                        ("f32", ("conv_f16x2", "wgrad_f16x2", "gemm_f16x2", "conv_bf16x3", "wgrad_bf16x3", "gemm_bf16x3")),
                                        ("f16x2", ())])
def test_arith_composite(libpath, arith, zero):
    code = """
import json
from piano_a2s_amd import hip
L = hip.lib()
print(json.dumps({k: L.a2s_debug_get(k.encode()) for k in ("conv_f16x2", "wgrad_f16x2", "gemm_f16x2", "conv_bf16x3", "wgrad_bf16x3", "gemm_bf16x3")}))
"""
    got = _child(code, env={"A2S_ARITH": arith})
    default = {"conv_f16x2": 3, "wgrad_f16x2": 1, "gemm_f16x2": 1, "conv_bf16x3": 3, "wgrad_bf16x3": 1, "gemm_bf16x3": 1}
    assert got == {k: (0 if k in zero else v) for k, v in default.items()}


def _table():
    """(key, default, environment variable or None) of every entry of the library's switch list, in its order."""
    text = open(os.path.join(ROOT, "piano_a2s_amd", "csrc", "a2s_switches.h")).read()
    rows = re.findall(r'^\s*X\((\w+),\s*(-?\d+),\s*\w+,\s*(?:"(A2S_\w+)"|0)\)', text, re.M)
    return [(k, int(d), e or None) for k, d, e in rows]


def test_table_is_the_contract(libpath):
    """The list itself: the keys of the contract, their defaults, the five variables -- and the library answers for exactly these."""
    table = _table()
    expect = {k: 1 for k in ONOFF_DEFAULT_1}
    expect.update({k: 0 for k in ONOFF_DEFAULT_0})
    expect.update(STORED)
    expect["attn_pair_fused_rows"] = 32
    assert {k: d for k, d, _ in table} == expect
    assert {e: k for k, _, e in table if e} == ENV
    got = _probe(libpath, tuple(k for k, _, _ in table))
    assert got["default"] == {k: d for k, d, _ in table}


def test_integration_md_lists_the_table(libpath):
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rows = re.findall(r"^\| `(\w+)` \| (-?\d+) \| [^|]+ \| (?:`(A2S_\w+)`|—) \|$", doc, re.M)
    assert [(k, int(d), e or None) for k, d, e in rows] == _table()
