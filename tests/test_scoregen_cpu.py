"""The score generator of the rendered synthetic corpus (piano_a2s_amd/scoregen.py) and the float64 definition of its synthesiser
(tests/render_oracle.py), on the CPU:

1. 200 seeds over all 7 time signatures and 14 keys, at max_length (398, 189) and (12, 8): every bar is well-formed kern, round-trips through the
   tokenizer, sums exactly to its time signature, fits max_length - 1 tokens and stays in the vocabulary and in the key's scale; seeds reproduce;
2. the note events against a kern parser written here (letter case and repetition -> octave, '#' / '-', reciprocal durations, tempo);
3. the packing of the render program;
4. the oracle itself: one partial against sin at the exact phase, and rendered tones through the VQT oracle."""
import re
from fractions import Fraction

import numpy as np
import pytest

from data_processing.humdrum import LabelsMultiple, _base_labels
from piano_a2s_amd import scoregen, spec
from piano_a2s_amd.kern_grammar import KernGrammar
from piano_a2s_amd.spec import EOS
from tests import render_oracle

SEEDS = range(200)
LENGTHS = [(398, 189), (12, 8)]
BAR_QUARTERS = {"4/4": Fraction(4), "3/4": Fraction(3), "2/4": Fraction(2), "6/8": Fraction(3), "2/2": Fraction(4), "12/8": Fraction(6), "3/8": Fraction(3, 2)}
LETTER_PC = {"c": 0, "d": 2, "e": 4, "f": 5, "g": 7, "a": 9, "b": 11}
# the major scales by their key signature, written out: pitch classes of the seven degrees
MAJOR_TONIC_PC = {-6: 6, -5: 1, -4: 8, -3: 3, -2: 10, -1: 5, 0: 0, 1: 7, 2: 2, 3: 9, 4: 4, 5: 11, 6: 6, 7: 1}
NOTE_RE = re.compile(r"(\d+)(\.*)([a-gA-G]+|r)([#-]?)")

labels = LabelsMultiple(extended=True)
_CLIPS = {}


def _clip(max_length, seed, frames=1201):
    """Seeds below 98 walk every (time signature, key) pair; the others draw both."""
    k = (max_length, seed, frames)
    if k not in _CLIPS:
        cfg = spec.default_cfg(max_length=max_length)
        forced = dict(time_sig=seed % 7, key=seed // 7) if seed < 98 else {}
        _CLIPS[k] = scoregen.make_clip(cfg, seed, frames=frames, **forced)
    return _CLIPS[k]


def _parse_note(note):
    """One kern note -> (length in quarters, MIDI or None for a rest, spelled pitch class or None)."""
    m = NOTE_RE.fullmatch(note)
    assert m, note
    q = Fraction(4, int(m.group(1)))
    q = q * (2 - Fraction(1, 2 ** len(m.group(2))))
    name = m.group(3)
    if name == "r":
        return q, None
    assert len(set(name)) == 1
    octave = 3 + len(name) if name[0].islower() else 4 - len(name)
    midi = 12 * (octave + 1) + LETTER_PC[name[0].lower()] + {"": 0, "#": 1, "-": -1}[m.group(4)]
    return q, midi


def _parse_bar(text):
    """-> [(length in quarters, [MIDI ...])] per time slice."""
    out = []
    for line in text.split("\n"):
        notes = [_parse_note(n) for n in line.split(" ")]
        assert len({q for q, _ in notes}) == 1, "the notes of a chord share their duration"
        out.append((notes[0][0], [m for _, m in notes if m is not None]))
    return out


@pytest.mark.parametrize("max_length", LENGTHS)
def test_generated_bars_are_wellformed_exact_and_in_key(max_length):
    gram = KernGrammar()
    base = set(_base_labels())
    seen_ts, seen_key, tokens = set(), set(), 0
    for seed in SEEDS:
        clip = _clip(max_length, seed)
        seen_ts.add(clip["ts"])
        seen_key.add(clip["key"])
        assert 0 <= clip["ts"] < 7 and 0 <= clip["key"] < 14
        assert clip["time_sig"] == scoregen.time_signatures()[clip["ts"]]
        scale = {(MAJOR_TONIC_PC[clip["key"] - 6] + d) % 12 for d in (0, 2, 4, 5, 7, 9, 11)}
        for staff, limit, octaves in (("upper", max_length[0], (4, 5, 6)), ("lower", max_length[1], (2, 3, 4))):
            assert len(clip["text"][staff]) == len(clip["ids"][staff]) == 5
            for text, ids in zip(clip["text"][staff], clip["ids"][staff]):
                assert ids == labels.encode(text)
                assert gram.accepts(ids + [EOS]), (seed, staff, text)
                assert labels.encode("".join(labels.decode(ids))) == ids
                assert len(ids) <= limit - 1, (seed, staff, len(ids))
                tokens += len(ids)
                slices = _parse_bar(text)
                assert sum(q for q, _ in slices) == BAR_QUARTERS[clip["time_sig"]], (seed, staff, text)
                for line in text.split("\n"):
                    assert 1 <= len(line.split(" ")) <= 3
                    for note in line.split(" "):
                        m = NOTE_RE.fullmatch(note)
                        assert m.group(1) + m.group(2) in base and m.group(1) in ("1", "2", "4", "8", "16", "12") and len(m.group(2)) <= 1
                        if m.group(3) != "r":
                            assert m.group(3) + m.group(4) in base, note
                            midi = _parse_note(note)[1]
                            assert midi % 12 in scale, (seed, clip["key"] - 6, note)
                            assert 12 * (octaves[0] + 1) - 1 <= midi <= 12 * (octaves[2] + 2), note
    assert seen_ts == set(range(7)) and seen_key == set(range(14))
    assert tokens > 0


@pytest.mark.parametrize("max_length", LENGTHS)
def test_seeds_reproduce_and_differ(max_length):
    cfg = spec.default_cfg(max_length=max_length)
    a, b, c = scoregen.make_clip(cfg, 7), scoregen.make_clip(cfg, 7), scoregen.make_clip(cfg, 8)
    assert a["text"] == b["text"] and a["ids"] == b["ids"] and a["tempo"] == b["tempo"] and a["instrument"] == b["instrument"]
    assert np.array_equal(a["events"], b["events"]) and np.array_equal(a["amps"], b["amps"])
    assert np.array_equal(scoregen.pack_program(a), scoregen.pack_program(b))
    assert a["text"] != c["text"] and not np.array_equal(scoregen.pack_program(a), scoregen.pack_program(c))


def test_tiny_max_length_falls_back_to_one_slice_per_bar():
    """max_length (3, 3): two tokens per bar at the most -- one value that fills the bar; the coarsest bar is the bar's single rest."""
    cfg = spec.default_cfg(max_length=(3, 3))
    for seed in range(14):
        clip = scoregen.make_clip(cfg, seed, time_sig=seed % 7)
        for staff in ("upper", "lower"):
            for text, ids in zip(clip["text"][staff], clip["ids"][staff]):
                assert len(ids) == 2 and _parse_bar(text) [0][0] == BAR_QUARTERS[clip["time_sig"]]
    rests = {}
    for name in scoregen.time_signatures():
        clip = scoregen.make_clip(cfg, 0, time_sig=scoregen.time_signatures().index(name), max_events=-1)       # no event fits: every level is refused
        texts = {t for staff in ("upper", "lower") for t in clip["text"][staff]}
        assert len(texts) == 1 and len(clip["events"]) == 0
        rests[name] = texts.pop()
        assert _parse_bar(rests[name]) == [(BAR_QUARTERS[name], [])]
        assert len(labels.encode(rests[name])) == 2
    assert rests == {"4/4": "1r", "3/4": "2.r", "2/4": "2r", "6/8": "2.r", "2/2": "1r", "12/8": "1.r", "3/8": "4.r"}


@pytest.mark.parametrize("max_length,frames", [((398, 189), 1201), ((12, 8), 1201), ((398, 189), 201)])
def test_events_equal_an_independent_parse_of_the_text(max_length, frames):
    heads = 0
    for seed in SEEDS:
        clip = _clip(max_length, seed, frames)
        spq = Fraction(60 * 16000) / Fraction(clip["tempo"]).limit_denominator(10 ** 6)
        assert spq == clip["spq"] and clip["spq"] % 24 == 0
        want = []
        for s, staff in enumerate(("upper", "lower")):
            t = Fraction(0)
            for text in clip["text"][staff]:
                for q, midis in _parse_bar(text):
                    onset, length = clip["lead"] + t * spq, q * spq
                    assert onset.denominator == 1 and length.denominator == 1
                    want += [(int(onset), int(length), m, s) for m in midis]
                    t += q
        want.sort(key=lambda e: (e[0], e[2], e[3]))
        assert np.array_equal(clip["events"], np.array([e[:3] for e in want], dtype=np.int64).reshape(-1, 3)), seed
        assert len(clip["events"]) == len(clip["amps"]) == len(clip["where"]) == len(want)
        assert clip["n_samples"] == (frames - 1) * 160
        if len(want):
            ev = clip["events"]
            assert ev[:, 0].min() >= 0 and (ev[:, 0] + ev[:, 1]).max() <= clip["n_samples"], "every event lies inside the clip"
            assert (ev[:, 1] > 0).all() and (clip["amps"] > 0).all() and (clip["amps"] <= 1).all()
        heads += len(want)
        # every token has the onset of its slice
        on = scoregen.token_onsets(clip)
        for staff in ("upper", "lower"):
            for ids, times in zip(clip["ids"][staff], on[staff]):
                assert len(times) == len(ids) and all(b >= a for a, b in zip(times, times[1:]))
    assert heads > 200


def test_program_packing():
    clip = _clip((398, 189), 5)
    E = 200
    p = scoregen.pack_program(clip, rows=E)
    assert p.shape == (1 + E, 8) and p.dtype == np.int32
    n = len(clip["events"])
    assert 0 < n <= E
    hd = render_oracle.header(p)
    inst = clip["instrument"]
    assert hd["n_samples"] == clip["n_samples"] == 192000 and hd["n_rows"] == n and hd["attack"] == inst["attack"] and hd["rel_len"] == 1600
    assert hd["rel_rate"] == np.float32(1.0 / 800) and hd["noise_seed"] == inst["noise_seed"]
    assert np.float32(10.0 ** (-60 / 20.0)) <= hd["noise_level"] <= np.float32(10.0 ** (-40 / 20.0)) and hd["gain"] > 0
    assert 0.45 <= inst["g"] <= 0.8 and 4 <= inst["n_harm"] <= 10
    assert (p[1 + n:] == 0).all(), "padding rows: zeros (length 0)"
    assert np.array_equal(p[1:1 + n, 0], clip["events"][:, 0]) and np.array_equal(p[1:1 + n, 1], clip["events"][:, 1])
    assert (np.diff(p[1:1 + n, 0]) >= 0).all()
    for i, (onset, length, midi) in enumerate(clip["events"], 1):
        f0 = 440.0 * 2.0 ** ((int(midi) - 69) / 12.0)
        assert int(p[i, 2:3].view(np.uint32)[0]) == int(np.rint(f0 / 16000.0 * 2.0 ** 32))
        assert p[i, 3:4].view(np.float32)[0] == clip["amps"][i - 1] and p[i, 6] == inst["n_harm"] and p[i, 7] == 0
        assert p[i, 5:6].view(np.float32)[0] == np.float32(inst["g"])
    decays = p[1:1 + n, 4].view(np.float32)
    lo, hi = clip["events"][:, 2].argmin(), clip["events"][:, 2].argmax()
    assert decays[lo] < decays[hi], "low notes decay more slowly"
    assert render_oracle.live_rows(p) == list(range(1, n + 1))
    with pytest.raises(ValueError):
        scoregen.pack_program(clip, rows=n - 1)
    # |wave| < 1 by the choice of the gain
    w = render_oracle.render(scoregen.pack_program(_clip((398, 189), 5, 201), rows=E))
    assert 0.01 < np.abs(w).max() < 1.0


def test_oracle_partial_against_sin_at_the_exact_phase():
    """One harmonic, flat envelope: the 24-bit phase costs at most 2 pi 2^-24 = 3.75e-7."""
    N = 192000
    worst = 0.0
    for midi in (21, 60, 108):
        inc = scoregen.inc1(midi)
        p = scoregen.pack_rows(N, [(0, N, midi, 1.0, 0.0, 0.7, 1)], attack=1, rel_len=0, rel_rate=0.0)
        w = render_oracle.render(p)
        m = np.arange(N, dtype=np.uint64)
        exact = np.sin(2.0 * np.pi * (((m * np.uint64(inc)) & np.uint64(0xFFFFFFFF)).astype(np.float64) / 2.0 ** 32))
        worst = max(worst, float(np.abs(w - exact).max()))
        cents = 1200 * np.log2(inc / 2.0 ** 32 * 16000 / (440.0 * 2.0 ** ((midi - 69) / 12.0)))
        assert abs(cents) < 1e-5
    print(f"phase truncation: max error {worst:.3e}")
    assert worst <= 3.75e-7


def test_oracle_padding_and_noise():
    nan = np.array([0x7FC00000], dtype=np.uint32).view(np.int32)[0]
    p = np.full((9, 8), nan, dtype=np.int32)
    p[0] = scoregen.pack_rows(500, [], noise_level=0.0)[0]
    p[0, 1] = 8
    assert render_oracle.live_rows(p) == [] and (render_oracle.render(p) == 0).all()
    q = scoregen.pack_rows(500, [], noise_level=0.01, noise_seed=0xDEADBEEF)
    w = render_oracle.render(q)
    assert np.abs(w).max() <= 0.01 and np.abs(w).max() > 0.009 and abs(w.mean()) < 0.002
    # the hash, once by hand
    x = (0xDEADBEEF + 3 * 0x9E3779B9) & 0xFFFFFFFF
    x ^= x >> 16; x = x * 0x7FEB352D & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846CA68B & 0xFFFFFFFF; x ^= x >> 16
    assert w[3] == float(np.float32(0.01)) * ((x >> 8) * 2.0 ** -23 - 1.0)


def _tone(midi):
    return scoregen.pack_rows(32000, [(1600, 24000, midi, 0.8, 1.0 / 16000, 0.7, 8)], attack=80, rel_len=1600, rel_rate=1.0 / 800)


@pytest.mark.parametrize("midi", [60, 84, 100, 33])
def test_rendered_tone_lands_on_its_vqt_bin(midi):
    """A tone through the VQT oracle: the per-frame argmax (frames 20 .. 150) sits exactly on bin 5 (midi - 21); for MIDI 33 the argmax of the time-mean."""
    from oracle import vqt_ref
    mag = np.abs(vqt_ref.vqt_librosa(render_oracle.render(_tone(midi))))
    mag = mag if mag.shape[0] == 480 else mag.T                            # (bins, frames)
    want = 5 * (midi - 21)
    if midi == 33:
        assert int(mag[:, 20:151].mean(axis=1).argmax()) == want
    else:
        peaks = mag[:, 20:151].argmax(axis=0)
        assert (peaks == want).all(), (midi, np.unique(peaks))


def test_rendered_clips_dataset_contract():
    """The item tuple the recipe's loader stacks, and the onsets for alignment evaluation."""
    import torch
    from datasets.syn import RenderedClips
    cfg = spec.default_cfg(max_length=(48, 32))
    ds = RenderedClips(cfg, 3, seed=77, frames=201)
    item = ds[1]
    assert len(ds) == 3 and len(item) == 9
    program, ts, key, upper, up_len, lower, lo_len, name, version = item
    assert program.dtype == torch.int32 and tuple(program.shape) == (1 + scoregen.MAX_EVENTS, 8) and int(program[0, 0]) == 32000
    assert tuple(upper.shape) == (5, 48) and tuple(lower.shape) == (5, 32) and upper.dtype == torch.long
    assert tuple(ts.shape) == (5,) and tuple(key.shape) == (5,) and name == "ren77_1~rendered" and version == 0
    clip = ds.clip(1)
    for b in range(5):
        n = int(up_len[b])
        assert upper[b, :n].tolist() == clip["ids"]["upper"][b] and int(upper[b, n]) == EOS
    on = ds.onsets(1)
    assert len(on["bar"]) == 5 and all(len(t) == int(n) for t, n in zip(on["upper"], up_len)) and all(len(t) == int(n) for t, n in zip(on["lower"], lo_len))
    assert 0 < on["bar"][0] < on["bar"][4] < 2.0
    assert torch.equal(ds[1][0], program) and not torch.equal(RenderedClips(cfg, 3, seed=10_077, frames=201)[1][0], program)
