"""An independent transposer for the tests of the transposition augmentation: it works on kern pitch NAMES as strings and shares no table and no
code with piano_a2s_amd/kern_transpose.py.

    parse(name)  -> (letter 'A'..'G', alteration -1 | 0 | +1, octave), or None for anything that is not a pitch name
    fmt(letter, alteration, octave) -> the kern name (c = C4, cc = C5, C = C3, CC = C2, CCC = C1)
    move(name, s, f) -> the name s semitones up and f fifths along, or None when it needs more than one accidental
    move_key(k, s)  -> the key rule, restated from its definition
    shift_bins(x, n) -> float64: y[..., j] = (1 - a) x[..., j - m] + a x[..., j - m - 1], m = floor(n), a = n - m, zero outside the row."""
import math

import numpy as np

SEMITONE_OF = {"C": 0, "D": 2, "E": 4, "F": 5, "G": 7, "A": 9, "B": 11}
LINE = ["F", "C", "G", "D", "A", "E", "B"]               # the naturals along the line of fifths; C is position 0


def parse(name):
    body = name.rstrip("#-")
    tail = name[len(body):]
    if not body or len(tail) > 1 or len(set(body)) != 1 or body[0].upper() not in SEMITONE_OF or not body[0].isalpha():
        return None
    if body[0].islower():
        if len(body) > 4:
            return None
        octave = 3 + len(body)
    else:
        if len(body) > 3:
            return None
        octave = 4 - len(body)
    return body[0].upper(), {"": 0, "#": 1, "-": -1}[tail], octave


def fmt(letter, alteration, octave):
    body = letter.lower() * (octave - 3) if octave >= 4 else letter * (4 - octave)
    return body + {0: "", 1: "#", -1: "-"}[alteration]


def midi(letter, alteration, octave):
    return 12 * (octave + 1) + SEMITONE_OF[letter] + alteration


def position(letter, alteration):
    return LINE.index(letter) - 1 + 7 * alteration


def move(name, s, f):
    letter, alteration, octave = parse(name)
    target_midi = midi(letter, alteration, octave) + s
    q = position(letter, alteration) + f
    # walk along the line of fifths: seven steps up are the same letter one sharp higher
    new_alt = 0
    while q > 5:
        q -= 7
        new_alt += 1
    while q < -1:
        q += 7
        new_alt -= 1
    if abs(new_alt) > 1:
        return None
    new_letter = LINE[q + 1]
    for new_octave in range(-2, 11):
        if midi(new_letter, new_alt, new_octave) == target_midi:
            return fmt(new_letter, new_alt, new_octave)          # (whether the vocabulary has the name is the caller's question)
    raise AssertionError(f"{name} by ({s}, {f}): no octave gives MIDI {target_midi}")


def move_key(k, s):
    best = None
    for c in range(-6, 8):
        if (c - (k + 7 * s)) % 12:
            continue
        rank = (abs(c - k), abs(c), 0 if c > 0 else 1)
        if best is None or rank < best[0]:
            best = (rank, c)
    return best[1]


def shift_bins(x, n):
    x = np.asarray(x, dtype=np.float64)
    F = x.shape[-1]
    m = math.floor(n)
    a = float(n) - m

    def tap(offset):
        out = np.zeros_like(x)
        for j in range(F):
            src = j - offset
            if 0 <= src < F:
                out[..., j] = x[..., src]
        return out

    return (1.0 - a) * tap(m) + a * tap(m + 1)
