"""Seeded **kern scores with their note events, and the render program the device synthesiser reads (host side, numpy only).

`make_clip` draws one clip: a time signature, a key and a tempo that hold for the clip's `max_bars` bars, and per bar and staff one spine of time
slices -- a rest, a note or a chord of 2-3 notes -- whose durations sum EXACTLY (as Fractions) to the bar.  The same draw yields the kern text, its
token ids (`LabelsMultiple(extended=True).encode`, never a table of ids) and one event per sounding note head (onset sample, length in samples,
MIDI number, amplitude).  `pack_program` writes the events and the clip's "instrument" into the (1 + E, 8) int32 program of csrc/a2s_render.hip.

Not produced: ties, fermatas, a second spine per staff, expressive timing.

Time is exact: a quarter note lasts `spq` samples, a multiple of 24, so every duration the generator knows (multiples of a 16th, the dotted 16th
3/8 and the triplet eighth 1/3 of a quarter) is a whole number of samples; tempo = 60 * 16000 / spq quarter notes per minute."""
import json
import os
from fractions import Fraction

import numpy as np

from data_processing.humdrum import LabelsMultiple, _base_labels

SR = 16000
HOP = 160
_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LABELS = LabelsMultiple(extended=True)
_BASE = set(_base_labels())

# bar length in 16th notes and the bar's single rest
_BAR_UNITS = {"4/4": 16, "3/4": 12, "2/4": 8, "6/8": 12, "2/2": 16, "12/8": 24, "3/8": 6}
_BAR_REST = {"4/4": "1r", "3/4": "2.r", "2/4": "2r", "6/8": "2.r", "2/2": "1r", "12/8": "1.r", "3/8": "4.r"}
# binary values 1 .. 16, plain and dotted, by their length in 16ths (the dotted 16th, 3/2 of a unit, only comes in pairs)
_UNIT_DUR = {24: "1.", 16: "1", 12: "2.", 8: "2", 6: "4.", 4: "4", 3: "8.", 2: "8", 1: "16"}
_MIN_UNITS = (1, 2, 4, 8)                  # coarseness levels: the shortest value a level draws
_LETTER_PC = {"c": 0, "d": 2, "e": 4, "f": 5, "g": 7, "a": 9, "b": 11}
_SHARPS, _FLATS = "fcgdaeb", "beadgcf"
STAFF_OCTAVES = {"upper": (4, 5, 6), "lower": (2, 3, 4)}
MAX_EVENTS = 511                           # rows of a program behind the header: 512 rows of 32 bytes = 16 KiB per clip


def time_signatures():
    with open(os.path.join(_HERE, "data_processing", "metadata", "time_signature_list.json")) as f:
        return json.load(f)


def key_scale(key):
    """The major scale of the key with `key` sharps (> 0) or flats (< 0): {letter: -1 | 0 | +1}, single accidentals only (-6 .. +7)."""
    acc = {l: 0 for l in _LETTER_PC}
    for l in (_SHARPS[:key] if key > 0 else _FLATS[:-key]):
        acc[l] = 1 if key > 0 else -1
    return acc


def kern_pitch(letter, acc, octave):
    """Kern spelling: c = C4, cc = C5, C = C3, CC = C2; '#' / '-'."""
    stem = letter * (octave - 3) if octave >= 4 else letter.upper() * (4 - octave)
    return stem + {0: "", 1: "#", -1: "-"}[acc]


def staff_pitches(key, staff):
    """[(kern name, MIDI)] of the key's scale over the staff's three letter-octaves, ascending; only symbols of the base vocabulary."""
    acc = key_scale(key)
    out = []
    for octave in STAFF_OCTAVES[staff]:
        for letter in "cdefgab":
            name = kern_pitch(letter, acc[letter], octave)
            if name in _BASE:
                out.append((name, 12 * (octave + 1) + _LETTER_PC[letter] + acc[letter]))
    return out


def _draw_slices(rng, units, level):
    """Durations of one bar: [(kern duration, length in 16ths as a Fraction)], drawn greedily among the values that still fit."""
    out, left = [], units
    floor = _MIN_UNITS[level]
    while left > 0:
        fit = [n for n in _UNIT_DUR if floor <= n <= left]
        if not fit:                                              # a remainder below the level's shortest value: the longest value that fits
            fit = [max(n for n in _UNIT_DUR if n <= left)]
        groups = []
        if level == 0 and left >= 4:
            groups.append("triplet")
        if level == 0 and left >= 3:
            groups.append("dotted16")
        pick = int(rng.integers(0, len(fit) + len(groups)))
        if pick >= len(fit):
            if groups[pick - len(fit)] == "triplet":             # three triplet eighths fill a quarter
                out += [("12", Fraction(4, 3))] * 3
                left -= 4
            else:                                                # two dotted 16ths: three 16ths
                out += [("16.", Fraction(3, 2))] * 2
                left -= 3
        else:
            out.append((_UNIT_DUR[fit[pick]], Fraction(fit[pick])))
            left -= fit[pick]
    return out


def _draw_bar(rng, ts, level, pitches, where):
    """One bar of one staff: [(duration, length in 16ths, [pitch indices], amplitudes)] -- no pitches: a rest."""
    if level >= len(_MIN_UNITS):
        return [(_BAR_REST[ts][:-1], Fraction(_BAR_UNITS[ts]), [], [])], where
    chord_p, rest_p = (0.3, 0.15, 0.05, 0.0)[level], 0.12
    out = []
    for dur, n in _draw_slices(rng, _BAR_UNITS[ts], level):
        u = rng.random()
        if u < rest_p:
            out.append((dur, n, [], []))
            continue
        where = int(np.clip(where + rng.integers(-3, 4), 0, len(pitches) - 1))
        idx = [where]
        if u > 1.0 - chord_p:
            span = np.arange(max(0, where - 7), min(len(pitches), where + 8))
            idx = sorted(int(i) for i in rng.choice(span, size=min(len(span), int(rng.integers(2, 4))), replace=False))
        out.append((dur, n, idx, [float(np.float32(rng.uniform(0.3, 1.0))) for _ in idx]))
    return out, where


def _bar_text(slices, pitches):
    return "\n".join(" ".join(dur + pitches[i][0] for i in idx) if idx else dur + "r" for dur, _, idx, _ in slices)


def make_clip(cfg, seed, frames=1201, max_events=MAX_EVENTS, time_sig=None, key=None):
    """One seeded clip as a dict:
      text {"upper" | "lower": [kern text per bar]}, ids {staff: [token ids per bar]}, ts (index into the time-signature list), time_sig,
      key (index = key + 6), tempo (quarter notes per minute), spq (samples per quarter), lead (samples before bar 1), n_samples,
      events (n, 3) int64 [onset, length, midi] in (onset, midi) order, amps (n,) float32, where (n, 3) int64 [bar, staff 0 upper / 1 lower, slice],
      slice_onsets {staff: [[onset sample per slice] per bar]}, instrument (dict).
    `time_sig` / `key` (indices) fix what is otherwise drawn."""
    rng = np.random.default_rng(seed)
    sigs = time_signatures()
    ts = int(rng.integers(0, len(sigs))) if time_sig is None else int(time_sig)
    k = int(rng.integers(0, 14)) if key is None else int(key)
    fill = float(rng.uniform(0.75, 0.98))
    inst = dict(g=float(np.float32(rng.uniform(0.45, 0.8))), n_harm=int(rng.integers(4, 11)), tau=float(rng.uniform(0.4, 1.2)),
                noise_db=float(rng.uniform(-60.0, -40.0)), attack=int(rng.integers(32, 129)), noise_seed=int(rng.integers(0, 2 ** 32)))
    name, bars = sigs[ts], cfg["max_bars"]
    n_samples = (frames - 1) * HOP
    lead = min(SR // 10, n_samples // 20)
    bar_q = Fraction(_BAR_UNITS[name], 4)
    spq = max(24, int(fill * (n_samples - lead) / float(bars * bar_q)) // 24 * 24)
    limits = dict(zip(("upper", "lower"), cfg["max_length"]))
    for start in range(len(_MIN_UNITS) + 1):
        text, ids, drawn = {}, {}, {}
        for staff in ("upper", "lower"):
            pitches = staff_pitches(k - 6, staff)
            where = int(rng.integers(0, len(pitches)))
            text[staff], ids[staff], drawn[staff] = [], [], []
            for _ in range(bars):
                for level in range(start, len(_MIN_UNITS) + 1):          # redrawn coarser until the bar fits max_length - 1 tokens
                    slices, w = _draw_bar(rng, name, level, pitches, where)
                    t = _bar_text(slices, pitches)
                    tok = _LABELS.encode(t)
                    if len(tok) <= limits[staff] - 1:
                        break
                where = w
                text[staff].append(t)
                ids[staff].append(tok)
                drawn[staff].append((slices, pitches))
        if sum(len(idx) for staff in drawn for slices, _ in drawn[staff] for _, _, idx, _ in slices) <= max_events:
            break
    ev, slice_onsets = [], {}
    for s, staff in enumerate(("upper", "lower")):
        slice_onsets[staff] = []
        for b, (slices, pitches) in enumerate(drawn[staff]):
            t, row = b * bar_q, []
            for j, (dur, n, idx, amps) in enumerate(slices):
                onset, length = lead + t * spq, n / 4 * spq
                assert onset.denominator == 1 and length.denominator == 1
                row.append(int(onset))
                ev += [(int(onset), int(length), pitches[i][1], a, b, s, j) for i, a in zip(idx, amps)]
                t += n / 4
            assert t == (b + 1) * bar_q, "the bar's durations sum exactly to the time signature"
            slice_onsets[staff].append(row)
    ev.sort(key=lambda e: (e[0], e[2], e[5]))
    return dict(text=text, ids=ids, ts=ts, time_sig=name, key=k, tempo=60.0 * SR / spq, spq=spq, lead=lead, n_samples=n_samples, seed=seed,
                events=np.array([e[:3] for e in ev], dtype=np.int64).reshape(-1, 3), amps=np.array([e[3] for e in ev], dtype=np.float32),
                where=np.array([e[4:] for e in ev], dtype=np.int64).reshape(-1, 3), slice_onsets=slice_onsets, instrument=inst)


def token_onsets(clip):
    """{"upper" | "lower": [[seconds per token] per bar]}: a token's time is the onset of its time slice (a line break belongs to the slice it ends)."""
    nl = _LABELS.labels_map["\n"]
    out = {}
    for staff in ("upper", "lower"):
        out[staff] = []
        for ids, onsets in zip(clip["ids"][staff], clip["slice_onsets"][staff]):
            row, j = [], 0
            for t in ids:
                row.append(onsets[j] / SR)
                j += t == nl
            out[staff].append(row)
    return out


def inc1(midi):
    """Phase increment per sample of the fundamental, in 2^-32 revolutions: rint(f0 / sr * 2^32) in float64."""
    return int(np.rint(440.0 * 2.0 ** ((midi - 69) / 12.0) / SR * 2.0 ** 32))


def _f32_bits(x):
    return np.array(x, dtype=np.float32).view(np.int32)


def pack_rows(n_samples, notes, attack=80, rel_len=1600, rel_rate=1.0 / 800, gain=1.0, noise_level=0.0, noise_seed=0, rows=None):
    """A program from explicit notes [(onset, length, midi, amp, decay per sample, g, n_harm)]: (1 + rows, 8) int32."""
    rows = len(notes) if rows is None else rows
    if len(notes) > rows:
        raise ValueError(f"{len(notes)} notes do not fit a program of {rows} rows")
    p = np.zeros((1 + rows, 8), dtype=np.int32)
    p[0, :4] = (n_samples, len(notes), attack, rel_len)
    p[0, 4:7] = _f32_bits([rel_rate, gain, noise_level])
    p[0, 7] = np.array(noise_seed, dtype=np.uint32).view(np.int32)
    for i, (onset, length, midi, amp, decay, g, n_harm) in enumerate(notes, 1):
        p[i, :2] = (onset, length)
        p[i, 2] = np.array(inc1(midi), dtype=np.uint32).view(np.int32)
        p[i, 3:6] = _f32_bits([amp, decay, g])
        p[i, 6] = n_harm
    return p


def pack_program(clip, rows=MAX_EVENTS):
    """The clip's render program, (1 + rows, 8) int32: its events in order, then padding rows of zeros (length 0)."""
    inst = clip["instrument"]
    g, nh = inst["g"], inst["n_harm"]
    partials = (1.0 - g ** nh) / (1.0 - g)
    ev, amps = clip["events"], clip["amps"]
    # gain: 0.9 over the largest sum of the amplitudes that sound together (releases included), times the partials' sum: |wave| < 1
    rel_len = 1600
    peak, marks = 0.0, sorted([(int(o), float(a)) for (o, l, m), a in zip(ev, amps)] + [(int(o + l + rel_len), -float(a)) for (o, l, m), a in zip(ev, amps)],
                              key=lambda x: (x[0], x[1]))
    run = 0.0
    for _, a in marks:
        run += a
        peak = max(peak, run)
    gain = 0.9 / max(1e-3, peak * partials)
    notes = [(int(o), int(l), int(m), float(a), 1.0 / (inst["tau"] * 2.0 ** ((60 - int(m)) / 24.0) * SR), g, nh) for (o, l, m), a in zip(ev, amps)]
    return pack_rows(clip["n_samples"], notes, attack=inst["attack"], rel_len=rel_len, rel_rate=1.0 / 800, gain=gain,
                     noise_level=10.0 ** (inst["noise_db"] / 20.0), noise_seed=inst["noise_seed"], rows=rows)


def detune_program(program, cents):
    """A copy of a render program ((1 + E, 8) int32, or a batch of them) whose notes sound `cents` cents beside their pitch: word 2 of every event
    row, the phase increment of the fundamental, becomes rint(inc * 2^(cents / 1200)) on its uint32 view (at most 2^32 - 1).  The header rows and
    everything else stay; 0 cents returns an equal program."""
    p = np.array(program, dtype=np.int32, copy=True)
    inc = p[..., 1:, 2].view(np.uint32).astype(np.float64)
    p[..., 1:, 2] = np.minimum(np.rint(inc * 2.0 ** (float(cents) / 1200.0)), 2.0 ** 32 - 1).astype(np.uint32).view(np.int32)
    return p
