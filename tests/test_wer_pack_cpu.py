"""Device-side scoring without a GPU: metrics.pack_words turns id rows into exactly the words the text path splits out, corpus_wer stays on
the host loop in a process that has not opened the GPU, and a2s_edit_distance checks its arguments before it launches anything."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from data_processing.humdrum import LabelsMultiple
from piano_a2s_amd import metrics
from piano_a2s_amd.spec import EOS, PAD, SOS, VOCAB_SIZE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = LabelsMultiple(extended=True).labels_map_inv
# an arbitrary map: an empty symbol, a whitespace-only one, one of two words, and one that collides with the bar separator
CUSTOM = {0: "a", 1: "", 2: " \t ", 3: "two words", 4: "=", 5: "b", 7: "a"}


def _dp(r, h):
    """Plain Levenshtein distance of two integer sequences (independent of metrics.word_error_rate)."""
    prev = list(range(len(h) + 1))
    for i in range(1, len(r) + 1):
        cur = [i] * (len(h) + 1)
        for j in range(1, len(h) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (r[i - 1] != h[j - 1]))
        prev = cur
    return prev[-1]


def _random_clip(rng, ids, special):
    """A clip of 0 ... 5 bars: short (0 ... 12) and long (20 ... 60) rows, the special ids sprinkled in, some rows cut at <eos> by unpad."""
    kind = rng.integers(0, 8)
    if kind == 0:
        return [[] for _ in range(int(rng.integers(0, 6)))]                          # every bar empty (or no bar at all)
    clip = []
    for _ in range(int(rng.integers(1, 6))):
        n = int(rng.integers(0, 13)) if rng.random() < 0.5 else int(rng.integers(20, 61))
        row = rng.choice(ids, size=n)
        hit = rng.random(n) < 0.15
        row[hit] = rng.choice(special, size=int(hit.sum()))
        if rng.random() < 0.5:
            row = metrics.unpad(row)                                                  # rows with <eos>: cut there; without: kept whole
        clip.append(row.tolist() if rng.random() < 0.5 else row)
    return clip


@pytest.mark.parametrize("inv,ids,special", [
    (INV, np.arange(VOCAB_SIZE), np.array([142, 143, 144, SOS, EOS, PAD])),
    (CUSTOM, np.array(sorted(CUSTOM)), np.array([1, 2, 3, 4])),
], ids=["vocabulary", "custom_map"])
def test_pack_words_is_the_text_path(inv, ids, special):
    rng = np.random.default_rng(20240 + len(inv))
    refs = [_random_clip(rng, ids, special) for _ in range(220)]
    hyps = []
    for clip in refs:                                                                 # near copies and unrelated clips
        if rng.random() < 0.5:
            hyps.append([[t for t in np.asarray(row).tolist() if rng.random() > 0.1] for row in clip])
        else:
            hyps.append(_random_clip(rng, ids, special))
    rw, ro, table = metrics.pack_words(refs, inv)
    hw, ho, table2 = metrics.pack_words(hyps, inv, table)
    assert table2 is table and rw.dtype == np.int32 and ro.dtype == np.int64 and len(ro) == len(refs) + 1 and ro[0] == 0
    word_of = {code: w for w, code in table.items()}
    assert len(word_of) == len(table)
    empty_clips = 0
    for c, (ref, hyp) in enumerate(zip(refs, hyps)):
        rt, ht = metrics.ids_to_text(ref, inv), metrics.ids_to_text(hyp, inv)
        r, h = rw[ro[c]:ro[c + 1]].tolist(), hw[ho[c]:ho[c + 1]].tolist()
        assert [word_of[x] for x in r] == rt.split(), c
        assert [word_of[x] for x in h] == ht.split(), c
        expect = metrics.word_error_rate(rt, ht)
        got = _dp(r, h) / len(r) if r else float(len(h) > 0)
        assert got == expect, c
        empty_clips += all(len(row) == 0 for row in ref)
    assert empty_clips >= 5
    if inv is INV:                                                                    # rows that were not cut keep <eos> / <pad> as ordinary words
        assert {table["<eos>"], table["<pad>"], table["<sos>"], table["<b>"]} <= set(rw.tolist())
    assert int(ro[-1]) == len(rw) and int(ho[-1]) == len(hw)


def test_pack_words_edges():
    w, o, table = metrics.pack_words([], INV)
    assert len(w) == 0 and o.tolist() == [0] and set(table) == {x for t in INV.values() for x in t.split()} | {"="}
    w, o, table = metrics.pack_words([[], [[]], [[], []], [[142], [143, 142], []]], INV)
    eq = table["="]
    assert o.tolist() == [0, 0, 0, 1, 3] and w.tolist() == [eq, eq, eq]                # "=" also between empty bars; whitespace symbols vanish
    with pytest.raises(KeyError):
        metrics.pack_words([[[6]]], CUSTOM)
    with pytest.raises(KeyError):
        metrics.pack_words([[[99]]], CUSTOM)


CHILD = """
import json, sys
from piano_a2s_amd import metrics
if sys.argv[1] == "off":
    metrics.WER_DEVICE = False
inv = {1: "4", 2: "c", 3: "e"}
wer, per = metrics.corpus_wer({"x": [[1, 2], [1, 3]]}, {"x": [[1, 2], [1, 2]]}, inv)
stats = metrics.last_wer_stats
wer2, per2 = metrics.corpus_wer({"x": [[1, 2]], "y": [[1], [3, 3]]}, {"x": [[1, 2]], "y": []}, inv)
empty = metrics.corpus_wer({}, {}, inv)
print(json.dumps({"wer": wer, "per": per, "wer2": wer2, "per2": per2, "empty": list(empty), "stats": stats,
                  "gpu_opened": sys.modules["torch"].cuda.is_initialized(), "env_default": metrics.WER_DEVICE}))
"""


@pytest.mark.parametrize("mode", ["fresh", "off"])
def test_corpus_wer_stays_on_the_host_without_an_open_gpu(mode):
    """A fresh process that has not touched CUDA (other tests of this session may have): the host loop, today's values, and scoring has not
    opened the GPU."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("A2S_")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", CHILD, mode], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["per"] == {"x": 1 / 5} and got["wer"] == 1 / 5                         # tests/test_recipe_cpu.py::test_wer_and_unpad
    assert got["per2"] == {"x": 0.0, "y": 1.0} and got["wer2"] == 0.5                 # empty reference: float(len(hyp) > 0)
    assert got["empty"] == [0.0, {}]
    assert got["stats"]["backend"] == "host" and got["stats"]["device_pairs"] == 0 and got["stats"]["pairs"] == got["stats"]["host_pairs"] == 1
    assert got["gpu_opened"] is False
    assert got["env_default"] is (mode == "fresh")


def test_wer_device_switch_reads_the_environment():
    env = {k: v for k, v in os.environ.items() if not k.startswith("A2S_")}
    env.update(PYTHONPATH=ROOT + os.pathsep + env.get("PYTHONPATH", ""), A2S_WER_DEVICE="0")
    r = subprocess.run([sys.executable, "-c", "from piano_a2s_amd import metrics; print(metrics.WER_DEVICE)"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip() == "False", r.stderr


def test_word_error_rate_is_still_the_host_loop():
    assert metrics.word_error_rate("a b c d", "a x c") == 0.5 and metrics.word_error_rate("", "a") == 1.0 and metrics.word_error_rate("", "") == 0.0


@pytest.fixture(scope="module")
def lib():
    from piano_a2s_amd import build
    L = C.CDLL(build.build())
    L.a2s_last_error.restype = C.c_char_p
    L.a2s_edit_distance.argtypes = [C.c_void_p] * 6 + [C.c_int] * 3 + [C.c_void_p]
    return L


def test_edit_distance_argument_checks(lib):
    """Everything is refused before a launch, so this runs without a GPU; the pointers are never dereferenced."""
    cap = lib.a2s_edit_distance_max_len()
    assert cap >= 2047
    launches, counted = lib.a2s_debug_get(b"edit_distance_launches"), lib.a2s_launch_count()
    assert launches >= 0
    p = 4096                                                                          # a non-null "device pointer"
    assert lib.a2s_edit_distance(None, None, None, None, None, None, 0, 0, 0, None) == 0        # nothing to do
    assert lib.a2s_edit_distance(None, p, p, p, p, None, 0, cap, cap, p) == 0
    bad = [
        (p, p, p, p, None, -1, 1, 1, p),                 # negative count
        (p, p, p, p, None, 3, -1, 1, p),                 # negative lengths
        (p, p, p, p, None, 3, 1, -1, p),
        (p, p, p, p, None, 3, cap + 1, 1, p),            # over capacity, either side
        (p, p, p, p, p, 3, 1, cap + 1, p),
        (None, p, p, p, None, 3, 1, 1, p),               # null pointers with pairs to score
        (p, None, p, p, None, 3, 1, 1, p),
        (p, p, None, p, None, 3, 1, 1, p),
        (p, p, p, None, None, 3, 1, 1, p),
        (p, p, p, p, None, 3, 1, 1, None),
    ]
    for args in bad:
        rc = lib.a2s_edit_distance(None, *args)
        assert rc < 0, args
        msg = lib.a2s_last_error()
        assert msg and b"edit_distance" in msg, args
    rc = lib.a2s_edit_distance(None, p, p, p, p, None, 3, cap + 1, 1, p)
    assert rc < 0 and str(cap).encode() in lib.a2s_last_error()
    assert lib.a2s_debug_get(b"edit_distance_launches") == launches and lib.a2s_launch_count() == counted
    assert lib.a2s_debug_set(b"edit_distance_launches", 1) == -1                      # read-only, like the other counters
