"""The key "conv_rows_stage" beside the switch list (csrc/a2s_switches.h): default, stored bits, its read-only launch counter, and that it is
documented where the other beside-the-list keys are.  Runs in a child process (fresh defaults); needs no GPU."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = """
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
out = {"default": L.a2s_debug_get(b"conv_rows_stage"), "rows_default": L.a2s_debug_get(b"conv_rows")}
out["set"] = [[L.a2s_debug_set(b"conv_rows_stage", v), L.a2s_debug_get(b"conv_rows_stage")] for v in (0, 1, 2, 3, 7)]
out["counter"] = [L.a2s_debug_get(b"conv_rows_stage_launches"), L.a2s_debug_set(b"conv_rows_stage_launches", 5), L.a2s_debug_get(b"conv_rows_stage_launches")]
out["rows_after"] = L.a2s_debug_get(b"conv_rows")
print(json.dumps(out))
"""


def test_key_default_bits_and_counter():
    from piano_a2s_amd import build
    env = {k: v for k, v in os.environ.items() if not k.startswith("A2S_")}
    r = subprocess.run([sys.executable, "-c", PROBE, build.build()], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["default"] == 3                                           # narrow-wave staging, and the two-set data gradient at 40 -> 40
    assert got["set"] == [[0, 0], [0, 1], [0, 2], [0, 3], [0, 3]]         # two bits are stored
    assert got["counter"] == [0, -1, 0]                                  # read-only; nothing was launched
    assert got["rows_default"] == got["rows_after"] == 7                 # "conv_rows" keeps its default and is not touched


def test_key_is_documented():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    with open(os.path.join(ROOT, "piano_a2s_amd", "csrc", "a2s_switches.h")) as f:
        hdr = f.read()
    for text in (doc, hdr):
        assert '"conv_rows_stage"' in text and '"conv_rows_stage_launches"' in text
    assert "X(conv_rows_stage" not in hdr                                # beside the list, not in it
