"""The note-level metric on the device (csrc/a2s_notes.hip through hip.note_match / metrics.device_note_counts / metrics.corpus_note_f1; DESIGN.md
section 17).  The counts are integers: every comparison with the host definition (metrics.note_counts) is equality, nothing has a tolerance.
Except in the capacity test no pair may fall back to the host: host_rows == 0 is asserted wherever corpus_note_f1 runs."""
import json
import os

import numpy as np
import pytest
import torch

from piano_a2s_amd import metrics, synthetic
from tests import note_cases
from tests.note_cases import EOS, IDS, PAD, SOS, V, enc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024)            # a thread's four tokens, a wave, the workgroup, the capacity


@pytest.fixture(autouse=True)
def gpu_open():
    torch.zeros(1, device="cuda")                                # the model has run on the GPU: the precondition of the device path
    assert torch.cuda.is_initialized()


def _device(pairs):
    ref, hyp = metrics._csr_rows([p[0] for p in pairs]), metrics._csr_rows([p[1] for p in pairs])
    return metrics.device_note_counts(*ref, *hyp)


def _assert_equal_to_host(pairs, what):
    got = _device(pairs)
    assert got.shape == (len(pairs), 8) and got.dtype == np.int32 and not got[:, 7].any()
    want = [metrics.note_counts(r, h) for r, h in pairs]
    wrong = [(i, len(pairs[i][0]), len(pairs[i][1]), got[i, :7].tolist(), list(want[i])) for i in range(len(pairs)) if got[i, :7].tolist() != list(want[i])]
    assert not wrong, f"{what}: {len(wrong)} of {len(pairs)} pairs (index, ref ids, hyp ids, device, host): {wrong[:6]}"
    return got


def test_hand_bars():
    got = _assert_equal_to_host(note_cases.hand_rows(), "hand bars")
    assert got[0, :6].tolist() == [3, 3, 3, 3, 2, 3] and got[6, :6].tolist() == [1, 1, 1, 1, 1, 0]
    nine = enc("\t".join(f"4{p}" for p in "cdefgabcd"))
    malformed = [([IDS["4"], IDS["\n"], IDS["8"]], enc("4c")), (enc("4c\n.\n4d"), enc("4c\t.\n.\t.\n.\t4d")), (nine, enc("4c")), (enc("4c"), nine + [IDS["\n"]] + nine),
                 ([SOS] + enc("4c\n4d")[:2] + [PAD] + enc("4c\n4d")[2:], enc("4c\n4d") + [EOS] + enc("4e")), ([IDS["\t"]] * 8 + enc("4c") + [IDS["\n"]] + enc("4d"), enc("4d")),
                 ([EOS], [EOS]), ([EOS] + enc("4c"), [PAD] * 5)]
    got = _assert_equal_to_host(malformed, "malformed rows")
    assert got[2, 6] == 1 and got[3, 6] == 2 and got[5, :7].tolist() == [1, 1, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("rate", [0.0, 0.05, 0.3])
def test_mutated_well_formed_clips(rate, monkeypatch):
    corpus = synthetic.make_note_corpus(32, rate, 11)
    monkeypatch.setattr(metrics, "NOTE_DEVICE", True)
    for staff in ("upper", "lower"):
        target, pred = corpus[staff]
        pairs = [(r, h) for k in target for r, h in zip(target[k], pred[k])]
        got = _assert_equal_to_host(pairs, f"{staff} at rate {rate}")
        assert got[:, 0].sum() > 500
        if rate == 0.0:
            assert (got[:, :6] == got[:, :1]).all()
        dev = metrics.corpus_note_f1(pred, target)
        stats = dict(metrics.last_note_stats)
        assert stats["backend"] == "device" and stats["host_rows"] == 0 and stats["device_rows"] == stats["rows"] == len(pairs)
        monkeypatch.setattr(metrics, "NOTE_DEVICE", False)
        host = metrics.corpus_note_f1(pred, target)
        assert metrics.last_note_stats["backend"] == "host"
        monkeypatch.setattr(metrics, "NOTE_DEVICE", True)
        assert dev == host and list(dev[1]) == list(host[1])                                # floats included, and the dict order
        print(f"rate {rate} {staff}: device {stats['seconds'] * 1e3:.1f} ms, host {metrics.last_note_stats['seconds'] * 1e3:.1f} ms, "
              f"f1 pitch / onset / value {dev[0]['f1_pitch']:.3f} / {dev[0]['f1_onset']:.3f} / {dev[0]['f1_value']:.3f}")


def test_random_id_rows():
    rng = np.random.default_rng(23)
    row = lambda n: rng.integers(0, V, size=n).tolist()                                       # <eos>, <pad>, <sos> included
    pairs = [(row(a), row(b)) for a in LENGTHS for b in LENGTHS]                            # 196 pairs: every boundary on either side
    pairs += [(row(int(rng.choice(LENGTHS))), row(int(rng.choice(LENGTHS)))) for _ in range(60)]
    assert len(pairs) == 256                                                                  # uniformly random ids over the whole vocabulary
    # uniform ids rarely make an event: 60 MORE pairs over the structural symbols only (not among the 256), so that lines, fields and events cross the boundaries too
    pool = [IDS[s] for s in ("4", "8", "8.", "16", "c", "c", "e", "G", "r", "\t", "\n", "\n", "<b>", ";", "_", "]", "[", ".", "<pad>", "<sos>")]
    dense = lambda n: [pool[i] for i in rng.integers(0, len(pool), size=n)]
    pairs += [(dense(int(rng.choice(LENGTHS))), dense(int(rng.choice(LENGTHS)))) for _ in range(50)]
    pool += [IDS["\t"]] * 8                                                                   # ... and 10 with many spines: fields beyond the eighth
    pairs += [(dense(int(rng.choice(LENGTHS[6:]))), dense(int(rng.choice(LENGTHS[6:])))) for _ in range(10)]
    got = _assert_equal_to_host(pairs, "random rows")
    assert got[256:, 0].max() >= 20 and got[256:, 6].any() and (got[:, 0] >= 0).all()


def test_rows_of_nothing_but_notes_at_capacity():
    """1024 ids that alternate DUR and PITCH are 512 events: the packed prefix sum's event field reaches 512 << 22 = 2^31 (it is unsigned for
    this row), every event slot is taken, and 512 notes against 512 is the longest loop of the quadratic count."""
    rng = np.random.default_rng(41)
    full = [IDS["4"], IDS["c"]] * 512
    durs, pitches = [IDS[s] for s in ("4", "8", "8.", "16")], [IDS[s] for s in ("c", "e", "G", "cc", "d#", "r")]
    mixed = lambda: [t for _ in range(512) for t in (durs[rng.integers(4)], pitches[rng.integers(6)])]
    lines = [t for k in range(341) for t in (durs[k % 4], pitches[k % 5], IDS["\n"])] + [IDS["4"]]      # 341 lines of one note: the longest recurrence
    a, b = mixed(), mixed()
    assert len(full) == len(a) == len(lines) == 1024 and metrics.note_counts(full, [])[0] == 512
    got = _assert_equal_to_host([(full, enc("4c")), (enc("4c"), full), (full, full), (a, b), (b, a), (a, a), (full, a), (lines, lines), (lines, full),
                                 (full[:1022], full), (full, full[2:])], "rows at capacity")
    assert got[0, :6].tolist() == [512, 1, 1, 1, 1, 1] and got[2, :6].tolist() == [512] * 6 and got[7, :6].tolist() == [341] * 6
    assert got[5, 0] == got[5, 4] > 400 and 0 < got[3, 4] < got[3, 2]


def test_duplicates():
    """300 identical notes against 200 of them: the rank rule counts exactly 200 at every level; and the same with a second pitch mixed in."""
    chord = lambda n, note="4c": enc(" ".join([note] * n))
    got = _assert_equal_to_host([(chord(300), chord(200)), (chord(200), chord(300)), (chord(341), chord(341)),
                                 (enc(" ".join(["4c", "4c#", "4d-", "8c"] * 64)), enc(" ".join(["4c", "4d-"] * 100)))], "duplicates")
    assert got[0, :6].tolist() == [300, 200, 200, 200, 200, 200] and got[1, :6].tolist() == [200, 300, 200, 200, 200, 200]
    assert len(chord(341)) == 1022 and got[2, :6].tolist() == [341] * 6
    assert got[3, :6].tolist() == [256, 200, 200, 200, 164, 164]        # pitch: 100 of 128 on either key; value: 64 quarter c + 100; spelled: 100 c + 64 d-


def test_capacity(monkeypatch):
    cap = metrics.note_match_capacity()
    assert cap == 1024
    long_row = enc("\n".join(["4c 4e"] * 171))                                                # 5 tokens a line + 170 NL
    assert len(long_row) == cap + 1
    edge = long_row[:cap]
    got = _device([(long_row, enc("4c")), (enc("4c"), long_row), (edge, edge), (enc("4c"), enc("4c"))])
    assert got[0].tolist() == got[1].tolist() == [-1] * 6 + [0, 0]
    assert got[2, :7].tolist() == list(metrics.note_counts(edge, edge)) and got[2, 0] == 341 and got[3, :6].tolist() == [1] * 6
    target = {"a": [enc("4c\n4d"), long_row, enc("2e")], "b": [long_row], "c": [edge]}
    pred = {"a": [enc("4c\n4d"), enc("4c 4e"), long_row], "b": [enc("4c")], "c": [edge]}
    monkeypatch.setattr(metrics, "NOTE_DEVICE", True)
    dev = metrics.corpus_note_f1(pred, target)
    stats = dict(metrics.last_note_stats)
    assert stats["backend"] == "device" and stats["rows"] == 5 and stats["host_rows"] == 3 and stats["device_rows"] == 2
    monkeypatch.setattr(metrics, "NOTE_DEVICE", False)
    assert dev == metrics.corpus_note_f1(pred, target)
    assert dev[1]["a"]["n_ref"] == 2 + 342 + 1 and dev[1]["a"]["tp_value"] == 2 + 2 + 0


def test_memory_bounds_and_ignored_ids():
    """Exactly sized id buffers, the output between sentinel words; ids of -1 and V (and far outside) are ignored and index no table."""
    from piano_a2s_amd import hip
    tb = metrics.note_tables()
    tabs = [torch.from_numpy(tb[k].copy()).cuda() for k in ("dur_ticks", "midi", "cls")]
    base = enc("4c 4e\n4d\t8g")
    dirty = [-1] + base[:2] + [V, -(2 ** 31), 2 ** 31 - 1] + base[2:] + [V + 1000]
    pairs = [(dirty, base), (base, dirty), ([-1, V], []), (dirty * 40, base * 40)]
    (ref, ref_off), (hyp, hyp_off) = metrics._csr_rows([p[0] for p in pairs]), metrics._csr_rows([p[1] for p in pairs])
    n, fence = len(pairs), 0x5A5A5A5A
    out = torch.full((8 * (n + 2),), fence, dtype=torch.int32, device="cuda")
    d = [torch.from_numpy(a).cuda() for a in (ref, ref_off, hyp, hyp_off)]
    assert d[0].numel() == sum(len(p[0]) for p in pairs) and d[2].numel() == sum(len(p[1]) for p in pairs)
    hip.note_match(d[0], d[1], d[2], d[3], n, *tabs, out[8:-8])
    got = out.cpu().numpy()
    assert (got[:8] == fence).all() and (got[-8:] == fence).all()
    got = got[8:-8].reshape(n, 8)
    assert [row[:7].tolist() for row in got] == [list(metrics.note_counts(r, h)) for r, h in pairs]
    assert got[0, :6].tolist() == [4] * 6 and got[2].tolist() == [0] * 8 and got[3, 0] == 160
    # refused before anything is launched
    before = hip.note_match_launches()
    L = hip.lib()
    args = [hip.stream(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), V,
            out[8:-8].data_ptr()]
    for i, bad in ((1, 0), (2, 0), (3, 0), (4, 0), (5, -1), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0)):
        refused = list(args)
        refused[i] = bad
        assert L.a2s_note_match(*refused) != 0 and b"note_match" in L.a2s_last_error()
    assert L.a2s_note_match(*(args[:5] + [0] + args[6:])) == 0 and hip.note_match_launches() == before     # no pair: nothing to launch
    torch.cuda.synchronize()


def test_one_launch_and_bar_pairing(monkeypatch):
    from piano_a2s_amd import hip
    a, b = enc("4c\n4d"), enc("2e")
    target = {"x": [a, b], "y": [a], "z": [], "w": [b, a, b]}
    pred = {"x": [a], "y": [a, b, b], "z": [], "w": [a, b]}
    monkeypatch.setattr(metrics, "NOTE_DEVICE", True)
    before, counted = hip.note_match_launches(), hip.lib().a2s_launch_count()
    sums = metrics.note_match([target[k] for k in target], [pred[k] for k in target])
    assert hip.note_match_launches() == before + 1 and hip.lib().a2s_launch_count() == counted + 1
    assert metrics.last_note_stats["rows"] == 2 + 3 + 0 + 3 and metrics.last_note_stats["host_rows"] == 0
    assert sums.tolist() == [[3, 2, 2, 2, 2, 2, 0], [2, 4, 2, 2, 2, 2, 0], [0] * 7, [4, 3, 0, 0, 0, 0, 0]]
    dev = metrics.corpus_note_f1(pred, target)
    assert hip.note_match_launches() == before + 2 and metrics.last_note_stats["backend"] == "device"
    monkeypatch.setattr(metrics, "NOTE_DEVICE", False)
    assert dev == metrics.corpus_note_f1(pred, target) and hip.note_match_launches() == before + 2
    assert dev[1]["z"]["f1_onset"] == 1.0 and dev[1]["x"]["recall_value"] == 2 / 3
    side = torch.cuda.Stream()
    monkeypatch.setattr(metrics, "NOTE_DEVICE", True)
    with torch.cuda.stream(side):                                                          # the caller's current stream, whichever it is
        again = metrics.corpus_note_f1(pred, target)
    torch.cuda.synchronize()
    assert again == dev
    assert metrics.corpus_note_f1({}, {}) == ({**{k: 1.0 for k in metrics.NOTE_MEAN_KEYS}, "overflow_rows": 0}, {})


def test_recipe_on_the_device(tmp_path):
    """One epoch of the small synthetic model with --note_metrics=true: VALID and TEST score their notes on the device (two launches a stage), and
    what the TEST stage wrote per clip is the host definition on the rows it recorded."""
    import pretrain
    from piano_a2s_amd import hip
    before = hip.note_match_launches()
    args = [os.path.join(ROOT, "hparams", "pretrain.yaml"), "--device=cuda:0", f"--workspace={tmp_path}", "--soundfont_folder=/none",
            "--synthetic_clips=8", "--hidden_size=32", "--conv_feature_size=32", "--bins_per_octave=24", "--n_octaves=1", "--max_length=(12, 8)",
            "--synthetic_frames=41", "--synthetic_lengths=[[3, 10], [2, 7]]", "--batch_size=4", "--number_of_epochs=1", "--seed=1234",
            "--note_metrics=true", "--constrained_decoding=true"]
    brain = pretrain.main(args)
    assert hip.note_match_launches() == before + 4 and metrics.last_note_stats["backend"] == "device" and metrics.last_note_stats["host_rows"] == 0
    res = os.path.join(str(tmp_path), "1234", "pretrain.epr", "results", "test")
    records = {f[:-5]: json.load(open(os.path.join(res, f))) for f in os.listdir(res)}
    assert set(records) == set(brain.upper_pred) and records
    stats = brain.last_stats
    for staff, pred, target, col in (("upper", brain.upper_pred, brain.upper_target, 3), ("lower", brain.lower_pred, brain.lower_target, 2)):
        for cid, rec in records.items():
            assert [bar[col] for bar in rec["pred"]] == pred[cid]
            ref, hyp, per_clip = metrics._pair_rows([target[cid]], [pred[cid]])
            want = metrics.note_scores(metrics._sum_clips([metrics.note_counts(r, h) for r, h in zip(ref, hyp)], per_clip)[0])
            assert rec["notes"][staff] == want, (cid, staff)
        for level in ("pitch", "onset", "value"):
            assert stats[f"note_f1_{level}_{staff}"] == sum(r["notes"][staff][f"f1_{level}"] for r in records.values()) / len(records)
    assert stats["note_f1"] == (stats["note_f1_onset_upper"] + stats["note_f1_onset_lower"]) / 2
