"""Bar-wise dynamic time warping without a GPU: the oracle of tests/dtw_oracle.py against brute force, the tie rule, the band,
a hand-made example with its warp, the host side's warp_from_path / warp_time / performed_notes / dtw_geometry against the oracle's plain statements,
the hand-written MIDI file, and the refusal of align_notes without resynthesis."""
import struct

import numpy as np
import pytest

from piano_a2s_amd import audio, resynth
from tests import dtw_oracle as oracle


# ------------------------------------------------------------------------------------------- the oracle itself
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_oracle_against_all_monotone_paths(n):
    rng = np.random.default_rng(n)
    for trial in range(6):
        # small integers: many ties, so the enumeration also sees that the reported path is one of the best and the FIRST by the tie rule
        d = rng.integers(0, 4, size=(n, n)).astype(np.float64) if trial % 2 else rng.uniform(0.0, 1.0, size=(n, n))
        for r in (-1, 0, 1, 2, n):
            path, total = oracle.align(d, r)
            best, paths = oracle.brute_force(d, r)
            assert path in paths and abs(total - best) <= 1e-12 * max(1.0, best), (n, trial, r, total, best)
            assert abs(sum(d[i, j] for i, j in path) - total) <= 1e-12 * max(1.0, total)
            assert path[0] == (0, 0) and path[-1] == (n - 1, n - 1) and len(path) <= 2 * n - 1
            assert all(oracle.in_band(i, j, -1 if r >= n else r) for i, j in path)
            assert all((a - i, b - j) in ((1, 1), (1, 0), (0, 1)) for (i, j), (a, b) in zip(path, path[1:]))


def test_ties_go_to_the_diagonal_then_up_then_left():
    for n in (1, 2, 7):
        path, total = oracle.align(np.zeros((n, n)), -1, np.float32)
        assert path == [(k, k) for k in range(n)] and total == 0.0
    # the diagonal predecessor is walled off: the two others tie, and "up" (i - 1, j) is listed before "left" (i, j - 1)
    D, codes = oracle.dp(np.array([[0.0, 1.0, 9.0], [1.0, 9.0, 1.0], [9.0, 1.0, 0.0]]))
    assert codes[2, 2] == 1 and D[2, 2] == 2.0, "D[1][1] = 9, D[1][2] = D[2][1] = 2: the first of the equal two"
    assert oracle.backtrack(codes) == [(0, 0), (0, 1), (1, 2), (2, 2)]


def test_a_band_of_zero_is_the_diagonal_whatever_the_costs():
    rng = np.random.default_rng(0)
    d = rng.uniform(0.0, 1.0, size=(6, 6))
    d[np.arange(6), np.arange(6)] = 100.0
    path, total = oracle.align(d, 0)
    assert path == [(k, k) for k in range(6)] and abs(total - 600.0) < 1e-9
    assert oracle.align(d, -1)[1] < total and oracle.align(d, 6)[1] == oracle.align(d, -1)[1], "r >= n is no band"


# ------------------------------------------------------------------------------------------- a hand-made example
HAND = np.array([[0.0, 9.0, 9.0, 9.0],
                 [0.0, 9.0, 9.0, 9.0],
                 [0.0, 9.0, 9.0, 9.0],
                 [9.0, 0.0, 0.0, 0.0]])
HAND_PATH = [(0, 0), (1, 0), (2, 0), (3, 1), (3, 2), (3, 3)]


def test_hand_made_example_with_a_vertical_run():
    """The score's first frame lasts for three frames of the recording, then the recording's last frame holds the score's other three."""
    for dtype in (np.float64, np.float32):
        path, total = oracle.align(HAND, -1, dtype)
        assert path == HAND_PATH and total == 0.0
    assert oracle.brute_force(HAND)[1] == [HAND_PATH]
    for packed in (False, True):
        warp, inverse = resynth.warp_from_path(oracle.pack(HAND_PATH) if packed else HAND_PATH, 4)
        assert warp.dtype == np.float64 and inverse.dtype == np.float64
        assert warp.tolist() == [1.0, 3.0, 3.0, 3.0], "score frame 0 is heard at the recording frames 0 .. 2: centre 1"
        assert inverse.tolist() == [0.0, 0.0, 0.0, 2.0], "recording frame 3 holds the score frames 1 .. 3: centre 2"
    w0, i0 = oracle.warp_from_path(HAND_PATH, 4)
    assert np.array_equal(w0, warp) and np.array_equal(i0, inverse)
    assert resynth.warp_time(warp, 0.0) == 1.0 and resynth.warp_time(warp, 0.5) == 2.0 and resynth.warp_time(warp, 1.0) == 3.0
    assert resynth.warp_time(warp, 2.25) == 3.0 and resynth.warp_time(warp, 3.5) == 3.5 and resynth.warp_time(warp, 4.0) == 4.0, "slope 1 behind the last frame"
    assert resynth.warp_time(warp, -3.0) == 1.0 and resynth.warp_time(warp, 99.0) == 4.0, "clipped to the bar"


def test_warp_from_path_against_the_plain_statement_and_its_refusals():
    rng = np.random.default_rng(5)
    for n in (1, 2, 9, 40):
        path, _ = oracle.align(rng.uniform(0.0, 1.0, size=(n, n)), n // 3 if n > 4 else -1)
        warp, inverse = resynth.warp_from_path(oracle.pack(path), n)
        w0, i0 = oracle.warp_from_path(path, n)
        assert np.array_equal(warp, w0) and np.array_equal(inverse, i0)
        assert np.all(np.diff(warp) >= 0) and np.all(np.diff(inverse) >= 0), "monotone"
    for bad in ([(0, 0), (2, 2)], [(0, 0), (1, 1)], [(1, 1), (2, 2)], [(0, 0), (1, 1), (1, 1), (2, 2)], [(0, 0), (1, 1), (0, 1), (2, 2)]):
        with pytest.raises(ValueError):
            resynth.warp_from_path(bad, 3)


def test_the_identity_warp_moves_no_note_by_a_single_bit():
    n, hop, first = 225, 160, 50
    warp = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(1)
    for u in np.concatenate([rng.uniform(0.0, n, 200), [0.0, 1.0, n - 1.0, float(n), n - 1e-9]]):
        assert resynth.warp_time(warp, u) == u
    start, stop = first * hop + 37, (first + n) * hop + 91            # bar lines that are no multiples of the hop
    notes = np.array([[start, 5000, 60], [start + 1234, 3, 61], [stop - 1, 1, 62], [start + 17777, stop - start - 17777, 63]], dtype=np.int64)
    moved = resynth.performed_notes(notes, warp, first, hop, start, stop)
    assert [m[0] for m in moved] == [float(o) for o in notes[:, 0]], "onsets come back exactly"
    assert [m[2] for m in moved] == [60, 61, 62, 63]
    assert moved[0][1] == 5000.0 and moved[1][1] == float(hop) and moved[2][1] == 1.0 and moved[3][1] == float(stop - start - 17777)
    assert resynth.performed_notes(notes, None, first, hop, start, stop) == [(float(o), float(l), int(m)) for o, l, m in notes], "no warp: the notes"
    # a warp that plays the bar's first half in a third of the time: a note in the middle of the score is heard early, inside the bar
    late = np.concatenate([np.linspace(0.0, n / 3.0, n // 2, endpoint=False), np.linspace(n / 3.0, n - 1.0, n - n // 2)])
    (on, ln, _), = resynth.performed_notes(np.array([[start + (n // 2) * hop, 800, 60]]), late, first, hop, start, stop)
    assert start <= on < start + (n // 2) * hop - 30 * hop and ln >= hop and on + ln <= stop


def test_band_and_buffer_geometry():
    from piano_a2s_amd import hip
    assert [resynth.dtw_band(n) for n in (1, 31, 32, 36, 240, 1201)] == [8, 8, 8, 9, 60, 300]
    for table in ([(0, 0, 37, -1)], [(0, 0, 37, 3), (1, 5, 22, 0)], [(0, 0, 37, 3), (1, 5, 22, -1)], [(0, 0, 300, 5)], [(0, 3, 3, 0)], [(0, 0, 2, 40), (0, 0, 9, 4)]):
        t = np.array(table, dtype=np.int64)
        n_max, r_max = hip.dtw_geometry(t)
        assert (n_max, r_max) == oracle.geometry(t)[:2]
        w_max = oracle.geometry(t)[2]
        for _, f0, f1, r in table:
            n = f1 - f0
            assert n <= n_max and (2 * r + 1 if 0 <= r and 2 * r + 1 < n else n) <= w_max, "every segment fits its block"


# ------------------------------------------------------------------------------------------- the MIDI file
def test_the_exact_bytes_of_a_one_note_file(tmp_path):
    want = (b"MThd" + bytes([0, 0, 0, 6, 0, 0, 0, 1, 0x01, 0xF4])                 # format 0, one track, 500 ticks per quarter
            + b"MTrk" + bytes([0, 0, 0, 20])
            + bytes([0x00, 0xFF, 0x51, 0x03, 0x07, 0xA1, 0x20])                     # 500000 us per quarter
            + bytes([0x00, 0x90, 60, 64])                                           # note on at 0
            + bytes([0x83, 0x74, 0x80, 60, 64])                                     # 500 ticks = 0.5 s later (variable length: 3 * 128 + 116) note off
            + bytes([0x00, 0xFF, 0x2F, 0x00]))
    assert audio.midi_bytes([[0.0, 0.5, 60]]) == want
    audio.write_midi(tmp_path / "one.mid", [[0.0, 0.5, 60]])
    assert (tmp_path / "one.mid").read_bytes() == want
    for bad in ([[-0.1, 0.5, 60]], [[0.0, 0.5, 128]], [[0.0, 0.5, 60.5]]):
        with pytest.raises(ValueError):
            audio.midi_bytes(bad)
    with pytest.raises(ValueError):
        audio.write_midi(tmp_path / "loud.mid", [[0.0, 0.5, 60]], velocity=128)


def _read_midi(data):
    """A format-0 file -> (ticks per quarter, microseconds per quarter, [(tick, "on" | "off", pitch, velocity)]); no running status (the writer uses none)."""
    assert data[:4] == b"MThd" and struct.unpack(">I", data[4:8])[0] == 6
    fmt, tracks, division = struct.unpack(">HHH", data[8:14])
    assert (fmt, tracks) == (0, 1) and data[14:18] == b"MTrk"
    size = struct.unpack(">I", data[18:22])[0]
    body, at, tick, tempo, events, ended = data[22:], 0, 0, None, [], False
    assert len(body) == size
    while at < size:
        delta = 0
        while True:
            byte = body[at]
            at += 1
            delta = (delta << 7) | (byte & 0x7F)
            if not byte & 0x80:
                break
        tick += delta
        status = body[at]
        if status == 0xFF:
            kind, length = body[at + 1], body[at + 2]
            payload = body[at + 3:at + 3 + length]
            at += 3 + length
            if kind == 0x51:
                tempo = int.from_bytes(payload, "big")
            ended = kind == 0x2F
        else:
            assert status in (0x90, 0x80) and not ended
            events.append((tick, "on" if status == 0x90 else "off", body[at + 1], body[at + 2]))
            at += 3
    assert ended and at == size
    return division, tempo, events


def test_midi_round_trip_chord_order_and_long_deltas():
    notes = [[0.25, 0.5, 64], [0.25, 0.5, 60], [0.25, 0.25, 67],          # a chord, one note shorter
             [0.75, 1.0, 60],                                               # starts where two others end: their note-offs come first
             [20.0, 0.0004, 72]]                                            # a gap of 18.25 s (a three-byte delta), and a length that rounds to no tick
    division, tempo, events = _read_midi(audio.midi_bytes(notes, velocity=64))
    assert (division, tempo) == (500, 500000), "one tick is one millisecond"
    assert events == [(250, "on", 60, 64), (250, "on", 64, 64), (250, "on", 67, 64), (500, "off", 67, 64), (750, "off", 60, 64), (750, "off", 64, 64),
                      (750, "on", 60, 64), (1750, "off", 60, 64), (20000, "on", 72, 64), (20001, "off", 72, 64)]
    assert audio._vlq(0) == b"\x00" and audio._vlq(127) == b"\x7f" and audio._vlq(128) == b"\x81\x00" and audio._vlq(18250) == b"\x81\x8e\x4a"
    assert _read_midi(audio.midi_bytes([]))[2] == []


def test_write_midi_prefers_the_performed_notes(tmp_path):
    result = {"windows": [{"bars": [{"notes": [[1.0, 0.5, 60]], "performed": [[1.125, 0.5, 60]]}, {"notes": [[2.0, 0.5, 62]]}, {"upper": "x"}]}]}
    assert audio.result_notes(result) == [[1.125, 0.5, 60], [2.0, 0.5, 62]]
    audio.write_midi(tmp_path / "take.mid", result)
    assert [e[0] for e in _read_midi((tmp_path / "take.mid").read_bytes())[2]] == [1125, 1625, 2000, 2500]


# ------------------------------------------------------------------------------------------- the option
def test_align_notes_needs_the_resynthesis():
    from piano_a2s_amd import transcribe
    with pytest.raises(ValueError, match="align_notes"):
        transcribe.transcribe_waveform(None, np.zeros(16000, dtype=np.float32), 16000, downbeats=[0.1, 0.5], hparams={}, align_notes=True, resynthesis=False)
    with pytest.raises(ValueError, match="align_notes"):
        transcribe.transcribe_waveform(None, np.zeros(16000, dtype=np.float32), 16000, downbeats=[0.1, 0.5], hparams={}, align_notes=True)
