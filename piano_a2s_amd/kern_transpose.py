"""Transposition of **kern scores by a spelled interval (host side, pure Python + numpy).

Everything is derived from the vocabulary itself, `LabelsMultiple(extended=True)`: no table is listed.

A pitch token is a repeated letter a-g / A-G plus at most one `#` or `-` (136 of the 173 symbols).  It has
    octave      c = C4, cc = C5, C = C3, CC = C2, CCC = C1 (scoregen.kern_pitch),
    MIDI        12 (octave + 1) + pitch class of the letter + alteration,
    position    p = {F: -1, C: 0, G: 1, D: 2, A: 3, E: 4, B: 5}[letter] + 7 alteration on the line of fifths; one accidental: p in [-8, 12].
A transposition is a pair (s, f): s semitones, f steps on the line of fifths.  The key moves first: from k in [-6, 7] (class k + 6) by s semitones
to the k' in [-6, 7] with k' = k + 7 s (mod 12) that has the smallest |k' - k|, then the smallest |k'|, then the positive one; f = k' - k.  A pitch
token (p, m) then goes to the spelling at p + f in the octave that makes its MIDI m + s; it is NOT REPRESENTABLE (-1) when p + f leaves [-8, 12] or
the symbol is not in the vocabulary (CCC .. ffff, without CCC- and ffff#).  Every other token is a fixed point.

Tables (numpy int32, what csrc/a2s_augment.hip reads):
    NEW_KEY[s + 6][key class]   -> key class
    INTERVAL[s + 6][key class]  -> row of TOKEN_MAP
    TOKEN_MAP[row][token id]    -> token id or -1;  PAIRS[row] = (s, f), the 25 pairs that occur, sorted."""
import re

import numpy as np

from data_processing.humdrum import LabelsMultiple, _NOTE_RE

MAX_SEMITONES = 6
KEYS = range(-6, 8)                                  # key k (sharps > 0, flats < 0) has class k + 6
N_KEYS = 14
_LABELS = LabelsMultiple(extended=True)
V = len(_LABELS.labels)
_FIFTHS = "fcgdaeb"                                  # position -1 .. 5 of the naturals
_PC = {"c": 0, "d": 2, "e": 4, "f": 5, "g": 7, "a": 9, "b": 11}
_PITCH = re.compile(r"(?:([a-g])\1{0,3}|([A-G])\2{0,2})([#-]?)")
_ALT = {"": 0, "#": 1, "-": -1}
_ACC = {0: "", 1: "#", -1: "-"}


def parse_pitch(sym):
    """(position on the line of fifths, MIDI) of a pitch symbol; None for every other symbol."""
    m = _PITCH.fullmatch(sym)
    if m is None:
        return None
    stem = sym.rstrip("#-")
    letter, alt = stem[0].lower(), _ALT[m.group(3)]
    octave = 3 + len(stem) if stem[0].islower() else 4 - len(stem)
    return _FIFTHS.index(letter) - 1 + 7 * alt, 12 * (octave + 1) + _PC[letter] + alt


def spell(p, midi):
    """The kern symbol at line-of-fifths position p with MIDI number `midi` (None: more than one accidental, or no such octave name)."""
    if not -8 <= p <= 12:
        return None
    alt, letter = (p + 1) // 7, _FIFTHS[(p + 1) % 7]
    octave, rem = divmod(midi - _PC[letter] - alt, 12)
    octave -= 1
    if rem:
        raise ValueError(f"position {p} has no MIDI number {midi}")
    stem = letter * (octave - 3) if octave >= 4 else letter.upper() * (4 - octave)
    return stem + _ACC[alt] if stem else None


def move_key(k, s):
    """Key k in [-6, 7] moved by s semitones -> k' by the key rule."""
    cands = [c for c in KEYS if (c - k - 7 * s) % 12 == 0]
    return min(cands, key=lambda c: (abs(c - k), abs(c), -c))


def _build():
    new_key = np.zeros((2 * MAX_SEMITONES + 1, N_KEYS), dtype=np.int32)
    fifths = np.zeros_like(new_key)
    for s in range(-MAX_SEMITONES, MAX_SEMITONES + 1):
        for k in KEYS:
            k2 = move_key(k, s)
            new_key[s + MAX_SEMITONES, k + 6] = k2 + 6
            fifths[s + MAX_SEMITONES, k + 6] = k2 - k
    pairs = sorted({(s - MAX_SEMITONES, int(f)) for s in range(new_key.shape[0]) for f in fifths[s]})
    row_of = {sf: i for i, sf in enumerate(pairs)}
    interval = np.array([[row_of[(s - MAX_SEMITONES, int(f))] for f in fifths[s]] for s in range(new_key.shape[0])], dtype=np.int32)
    token_map = np.tile(np.arange(V, dtype=np.int32), (len(pairs), 1))
    ids = _LABELS.labels_map
    for row, (s, f) in enumerate(pairs):
        for sym, i in ids.items():
            pm = parse_pitch(sym)
            if pm is not None:
                token_map[row, i] = ids.get(spell(pm[0] + f, pm[1] + s), -1)
    for t in (new_key, interval, token_map):
        t.setflags(write=False)
    return new_key, interval, token_map, pairs


NEW_KEY, INTERVAL, TOKEN_MAP, PAIRS = _build()
PITCH_IDS = frozenset(i for sym, i in _LABELS.labels_map.items() if parse_pitch(sym) is not None)


def tables():
    """(new_key (13, 14), interval (13, 14), token_map (rows, 173)): the three int32 arrays the device kernel reads."""
    return NEW_KEY, INTERVAL, TOKEN_MAP


def _check(key, s):
    if not -MAX_SEMITONES <= s <= MAX_SEMITONES:
        raise ValueError(f"a transposition by {s} semitones: expected -{MAX_SEMITONES} .. {MAX_SEMITONES}")
    if not 0 <= key < N_KEYS:
        raise ValueError(f"key class {key}: expected 0 .. {N_KEYS - 1}")


def transpose_ids(ids, key, s):
    """Token ids of music in key class `key`, moved by s semitones -> (new ids, new key class); None when a token is not representable."""
    _check(key, s)
    row = TOKEN_MAP[INTERVAL[s + MAX_SEMITONES, key]]
    out = [int(row[i]) for i in ids]
    if -1 in out:
        return None
    return out, int(NEW_KEY[s + MAX_SEMITONES, key])


def transpose_text(kern_text, key, s):
    """**kern text (lines of tab-separated spines of space-separated notes, as LabelsMultiple.encode reads it) in key class `key`, moved by s
    semitones -> (new text, new key class); None when a pitch is not representable.  Only the pitch names change."""
    _check(key, s)
    row = TOKEN_MAP[INTERVAL[s + MAX_SEMITONES, key]]
    ids, inv = _LABELS.labels_map, _LABELS.labels_map_inv
    bad = []

    def note(m):
        pitch = m.group(3)
        if pitch not in ids or ids[pitch] not in PITCH_IDS:
            return m.group(0)
        new = int(row[ids[pitch]])
        if new < 0:
            bad.append(pitch)
            return m.group(0)
        return m.group(1) + m.group(2) + inv[new] + m.group(4) + m.group(5)

    out = "\n".join("\t".join(" ".join(_NOTE_RE.sub(note, n) if _NOTE_RE.fullmatch(n) else n for n in chord.split(" ")) for chord in line.split("\t"))
                    for line in kern_text.split("\n"))
    if bad:
        return None
    return out, int(NEW_KEY[s + MAX_SEMITONES, key])
