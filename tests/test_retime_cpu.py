"""Resynthesis at the performed timing without a GPU: the integer definition of tests/retime_oracle.py against the float
definitions it restates (resynth.warp_from_path, resynth.performed_notes), its three stated properties, the host tables (resynth.event_rows,
hip.event_table) and the refusal of the option without align_notes."""
import itertools

import numpy as np
import pytest

from piano_a2s_amd import audio, resynth
from tests import dtw_oracle
from tests import retime_oracle as oracle


def _monotone_paths(n):
    """Every path from (0, 0) to (n - 1, n - 1) by steps (1, 1), (1, 0), (0, 1)."""
    out = []

    def walk(path):
        i, j = path[-1]
        if (i, j) == (n - 1, n - 1):
            out.append(path)
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < n and j + dj < n:
                walk(path + [(i + di, j + dj)])

    walk([(0, 0)])
    return out


# ------------------------------------------------------------------------------------------- the doubled warp
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_warp2_is_twice_warp_from_path_on_every_monotone_path(n):
    paths = _monotone_paths(n)
    assert len(paths) == [1, 3, 13, 63, 321][n - 1], "the Delannoy numbers: every path is there"
    for path in paths:
        packed = dtw_oracle.pack(path)
        warp, inverse = resynth.warp_from_path(packed, n)
        for n_max in (n, n + 3):
            w2, v2 = oracle.warp2(np.concatenate([packed, [-1, -1]]), len(path), n, n_max)
            assert w2.shape == v2.shape == (n_max + 1,)
            assert np.array_equal(w2[:n], 2 * warp) and np.array_equal(v2[:n], 2 * inverse), path
            assert w2[n] == w2[n - 1] + 2 and v2[n] == v2[n - 1] + 2, "slope 1 behind the last frame, as resynth.warp_time goes on"
            assert w2[n] == 2 * resynth.warp_time(warp, float(n)) and np.all(np.diff(w2[:n + 1]) >= 0) and np.all(np.diff(v2[:n + 1]) >= 0)
            assert np.array_equal(w2[n + 1:], 2 * np.arange(n + 1, n_max + 1)) and np.array_equal(v2[n + 1:], 2 * np.arange(n + 1, n_max + 1))


def test_hand_made_example_and_the_paths_that_are_not_taken():
    hand = [(0, 0), (1, 0), (2, 0), (3, 1), (3, 2), (3, 3)]                       # tests/test_dtw_cpu.py: HAND_PATH
    w2, v2 = oracle.warp2(dtw_oracle.pack(hand), 6, 4, 4)
    assert w2.tolist() == [2, 6, 6, 6, 8] and v2.tolist() == [0, 0, 0, 4, 6]
    ident = (2 * np.arange(5)).tolist()
    good = dtw_oracle.pack(hand)
    for cells, steps, n in ((good, 0, 4), (good, 6, 0), (good, 5, 4), (good, 6, 5), (good, 6, 3), (good[:4], 6, 4), (good, 8, 4), (good, -1, 4),
                            (dtw_oracle.pack([(0, 0), (1, 0), (2, 0), (3, 1), (3, 2), (3, 2)]), 6, 4),          # wrong end cell
                            (dtw_oracle.pack([(0, 1), (1, 1), (2, 2), (3, 3)]), 4, 4),                          # wrong first cell
                            (dtw_oracle.pack([(0, 0), (2, 1), (3, 2), (3, 3)]), 4, 4),                          # a step of two
                            (dtw_oracle.pack([(0, 0), (1, 1), (1, 1), (2, 2), (3, 3)]), 5, 4),                  # a step of none
                            (dtw_oracle.pack([(0, 0), (1, 1), (0, 2), (1, 3), (2, 3), (3, 3)]), 6, 4),          # a step back
                            (np.array([0, (1 << 16) | 1, (9 << 16) | 2, -1, (3 << 16) | 3]), 5, 4),             # cells outside [0, n)
                            (np.array([0, (1 << 16) | 1, (2 << 16) | 70000 % 65536, (3 << 16) | 3]), 4, 4)):
        w2, v2 = oracle.warp2(cells, steps, n, 4)
        assert w2.tolist() == ident and v2.tolist() == ident, (cells, steps, n)
    assert oracle.warp2(good, 6, 4, 3)[0].tolist() == [0, 2, 4, 6], "a segment longer than n_max is read as empty"
    assert oracle.warp2([0], 1, 1, 2)[0].tolist() == [0, 2, 4], "one frame: warp2[1] = warp2[0] + 2"


# ------------------------------------------------------------------------------------------- move
def test_move_at_its_corners():
    h, f0, n = 16, 3, 4
    w2 = np.array([2, 6, 6, 6, 8])                                                # d = warp2 - 2 k = [2, 4, 2, 0, 0]
    at = lambda p: f0 * h + p
    assert oracle.move(at(0), w2, f0, n, h) == at(0) + 16, "rem = 0: shift2 = h d[0] = 32"
    assert oracle.move(at(15), w2, f0, n, h) == at(15) + (1 * 2 + 15 * 4) // 2, "rem = h - 1"
    assert oracle.move(at(16), w2, f0, n, h) == at(16) + 32
    assert oracle.move(at(-40), w2, f0, n, h) == at(-40) + 16, "p clamped at 0: the shift of the first frame"
    assert oracle.move(at(n * h + 99), w2, f0, n, h) == at(n * h + 99), "p clamped at n h: k = n - 1, rem = h, the shift of the entry n"
    assert oracle.move(at(3 * h + 5), w2, f0, n, h) == at(3 * h + 5), "k = n - 1 reads warp2[n]"
    assert oracle.move(at(n * h), w2, f0, n, h) == at(n * h), "p = n h: k = n - 1, not n"
    back = np.array([0, 1, 4, 6, 8])                                              # d = [0, -1, 0, 0, 0]
    assert oracle.move(at(7), back, f0, n, h) == at(7) + (-7) // 2 == at(7) - 4, "shift2 = -7: the floor goes towards -inf, not towards 0"
    assert oracle.move(at(h), back, f0, n, h) == at(h) - 8 and oracle.move(at(h + 1), back, f0, n, h) == at(h + 1) - 8, "shift2 = -16, -15"
    assert oracle.move(12345, w2, f0, 0, h) == 12345, "an empty segment moves nothing"


# ------------------------------------------------------------------------------------------- the event rule
def test_event_rule_clamps_and_lengths():
    h, f0, n = 16, 0, 4
    late = np.array([6, 6, 6, 6, 8])                                              # everything is heard at frame 3
    early = np.array([0, 0, 0, 0, 2])                                             # everything is heard at frame 0
    assert oracle.move(40, late, f0, n, h) == 48 and oracle.move(44, late, f0, n, h) == 48 and oracle.move(40, early, f0, n, h) == 0
    assert oracle.retime(40, 4, late, f0, n, h, 0, 45) == (44, 1), "the onset clamped to bar_stop, then to bar_stop - 1; the one-sample length"
    assert oracle.retime(40, 4, early, f0, n, h, 20, 64) == (20, 16), "onset and end clamped to bar_start; a length of one hop where the bar has room"
    assert oracle.retime(0, 60, late, f0, n, h, 0, 56) == (48, 8), "the end (60) clamped to bar_stop"
    assert oracle.retime(0, 60, late, f0, n, h, 0, 64) == (48, 16), "12 samples left of the note: raised to one hop"
    assert oracle.retime(60, 3, 2 * np.arange(5), f0, n, h, 0, 64) == (60, 4), "a short note near the bar line: what room there is"
    assert oracle.retime(30, 20, 2 * np.arange(5), f0, n, h, 0, 64) == (30, 20)
    assert oracle.retime(30, 5, 2 * np.arange(5), f0, n, h, 0, 64) == (30, 16), "the identity still raises a note shorter than one hop, as performed_notes does"


def _random_case(rng):
    n, h = int(rng.integers(1, 40)), int(rng.choice([1, 7, 16, 160]))
    path = [(0, 0)]
    while path[-1] != (n - 1, n - 1):
        i, j = path[-1]
        steps = [(di, dj) for di, dj in ((1, 1), (1, 0), (0, 1)) if i + di < n and j + dj < n]
        di, dj = steps[int(rng.integers(0, len(steps)))]
        path.append((i + di, j + dj))
    f0 = int(rng.integers(0, 30))
    b0 = f0 * h + int(rng.integers(-h, h + 1))
    b1 = max(b0 + 1, (f0 + n) * h + int(rng.integers(-h, h + 1)))
    return n, h, path, f0, b0, b1


def test_within_one_sample_of_the_float_definition_and_order_kept():
    rng = np.random.default_rng(28)
    worst = 0.0
    for _ in range(1000):
        n, h, path, f0, b0, b1 = _random_case(rng)
        warp, _ = resynth.warp_from_path(path, n)
        w2, _ = oracle.warp2(dtw_oracle.pack(path), len(path), n, n)
        onsets = np.sort(rng.integers(b0 - 2 * h, b1 + 2 * h, size=6))
        lengths = rng.integers(1, 3 * h + 2, size=6)
        want = resynth.performed_notes([(o, ln, 60) for o, ln in zip(onsets, lengths)], warp, f0, h, b0, b1)
        got = [oracle.retime(o, ln, w2, f0, n, h, b0, b1) for o, ln in zip(onsets, lengths)]
        for (on, ln), (fon, fln, _) in zip(got, want):
            assert abs(on - fon) <= 1.0 and abs((on + ln) - (fon + fln)) <= 1.0, (n, h, path, on, ln, fon, fln)
            assert b0 <= on <= b1 - 1 and 1 <= ln <= b1 - on
            worst = max(worst, abs(on - fon), abs((on + ln) - (fon + fln)))
        assert all(a[0] <= b[0] for a, b in zip(got, got[1:])), "the onsets keep their order"
        ts = np.arange(b0 - h, b1 + h)
        assert np.all(np.diff([oracle.move(t, w2, f0, n, h) for t in ts[::max(1, len(ts) // 200)]]) >= 0), "move is non-decreasing"
    assert worst > 0.0, "the cases do leave the grid of whole samples"


def test_identity_moves_nothing_by_a_bit():
    rng = np.random.default_rng(7)
    for _ in range(200):
        n, h, _, f0, b0, b1 = _random_case(rng)
        ident = 2 * np.arange(n + 1)
        for t in rng.integers(b0 - 3 * h, b1 + 3 * h, size=8):
            assert oracle.move(t, ident, f0, n, h) == t
        on = int(rng.integers(b0, b1))
        ln = int(rng.integers(h, 4 * h + 1))
        if on + ln <= b1:
            assert oracle.retime(on, ln, ident, f0, n, h, b0, b1) == (on, ln)
        assert oracle.retime(on, ln, ident, f0, n, h, b0, b1)[0] == on


def test_retime_programs_skips_what_the_kernel_skips():
    prog = np.zeros((2, 4, 8), dtype=np.int32)
    prog[:, 1:3, 0], prog[:, 1:3, 1], prog[:, :, 3] = 20, 20, 77                  # two notes per clip, one padding row
    late = np.array([[6, 6, 6, 6, 8]])
    table = np.array([[0, 0, 4, 8]])
    rows = [(0, 1, 0, 0, 64), (0, 3, 0, 0, 64), (1, 1, -1, 0, 64), (1, 2, 1, 0, 64), (2, 1, 0, 0, 64), (-1, 1, 0, 0, 64), (0, 0, 0, 0, 64), (0, 4, 0, 0, 64),
            (0, 2, 0, 64, 64)]
    out = oracle.retime_programs(prog, [r + (0, 0, 0) for r in rows], late, table, 4, 16)
    assert out[0, 1, :2].tolist() == [48, 16]
    changed = np.argwhere(out != prog)
    assert changed.tolist() == [[0, 1, 0], [0, 1, 1]], "only the one good row of a real note moves: words 0 and 1"


# ------------------------------------------------------------------------------------------- the host tables
def test_event_rows_puts_a_note_on_a_bar_line_into_the_bar_that_starts_there():
    lines = [100, 200, 300, 450]
    ev = np.array([(50, 10, 60), (100, 10, 61), (199, 30, 62), (200, 5, 63), (449, 1, 64), (450, 3, 65), (900, 3, 66)])
    rows = resynth.event_rows(ev, lines, [7, -1, 9], clip=2)
    assert rows.dtype == np.int32 and rows.shape == (7, 8) and (rows[:, 0] == 2).all() and rows[:, 1].tolist() == list(range(1, 8))
    assert rows[:, 2].tolist() == [7, 7, 7, -1, 9, 9, 9], "before the first line: bar 0; on a line: the bar that starts there; behind the last: the last"
    assert rows[:, 3].tolist() == [100, 100, 100, 200, 300, 300, 300] and rows[:, 4].tolist() == [200, 200, 200, 300, 450, 450, 450]
    assert not rows[:, 5:].any()
    for e, r in zip(ev, rows):                                                      # the bar performed_onsets picks
        b = min(max(int(np.searchsorted(lines, e[0], side="right")) - 1, 0), len(lines) - 2)
        assert (r[3], r[4]) == (lines[b], lines[b + 1])
    assert resynth.event_rows(np.zeros((0, 3)), lines, [0, 1, 2]).shape == (0, 8)
    with pytest.raises(ValueError, match="event_rows"):
        resynth.event_rows(ev, lines, [0, 1])


def test_event_table_refuses_what_the_kernel_cannot():
    from piano_a2s_amd import hip
    table = np.array([(0, 0, 10, 8), (0, 10, 20, 8), (1, 0, 12, 8)])
    good = np.array([(0, 1, 0, 0, 1600), (0, 2, 1, 1600, 3200), (0, 3, -1, 3200, 4000), (1, 1, 2, 0, 1920)])
    dev = hip.event_table(good, 2, 5, table, "cpu")
    assert dev.dtype.is_floating_point is False and tuple(dev.shape) == (4, 8) and dev.is_contiguous()
    assert np.array_equal(dev.numpy()[:, :5], good) and not dev.numpy()[:, 5:].any()
    assert tuple(hip.event_table(np.zeros((0, 8)), 2, 5, table, "cpu").shape) == (0, 8)
    assert np.array_equal(hip.event_table(np.concatenate([good, np.zeros((4, 3), dtype=np.int64)], axis=1), 2, 5, table[:, :3], "cpu").numpy(), dev.numpy())

    def bad(row, col, value):
        rows = good.copy()
        rows[row, col] = value
        return rows

    for rows in (good[[0, 3, 1, 2]], bad(0, 0, -1), bad(3, 0, 2), bad(0, 1, 0), bad(0, 1, 5), bad(0, 1, -3), bad(1, 1, 1), bad(0, 2, 2), bad(3, 2, 0), bad(0, 2, 3),
                 bad(0, 2, -2), good + 0.5, good[:, :4], bad(0, 3, 2 ** 31)):
        with pytest.raises(hip.A2SError, match="event_table"):
            hip.event_table(rows, 2, 5, table, "cpu")
    with pytest.raises(hip.A2SError, match="event_table"):
        hip.event_table(good, 2, 5, table[:, :2], "cpu")
    with pytest.raises(hip.A2SError, match="event_table"):
        hip.event_table(good, 0, 5, table, "cpu")
    with pytest.raises(hip.A2SError, match="event_table"):
        hip.event_table(good[:1], 2, 1, table, "cpu")


# ------------------------------------------------------------------------------------------- the option
def test_performed_timing_needs_align_notes():
    from piano_a2s_amd import transcribe
    x = np.zeros(16000, dtype=np.float32)
    with pytest.raises(ValueError, match="performed_timing"):
        transcribe.transcribe_waveform(None, x, 16000, downbeats=[0.1, 0.5], hparams={}, resynthesis=True, performed_timing=2)
    with pytest.raises(ValueError, match="performed_timing"):
        transcribe.transcribe_waveform(None, x, 16000, downbeats=[0.1, 0.5], hparams={}, performed_timing=1)
    with pytest.raises(ValueError, match="performed_timing"):
        transcribe.transcribe_waveform(None, x, 16000, downbeats=[0.1, 0.5], hparams={}, resynthesis=True, align_notes=True, performed_timing=-1)
    with pytest.raises(ValueError, match="retime"):
        resynth.resynthesise([], None, None, 160, retime=2)


def test_result_notes_prefers_the_retimed_notes():
    bar = {"notes": [[1.0, 0.5, 60]], "performed": [[1.125, 0.5, 60]], "retimed": [[1.25, 0.5, 60]]}
    assert audio.result_notes({"windows": [{"bars": [bar]}]}) == [[1.25, 0.5, 60]]
    del bar["retimed"]
    assert audio.result_notes({"windows": [{"bars": [bar]}]}) == [[1.125, 0.5, 60]]
