"""Note dynamics, host side and definition (piano_a2s_amd/resynth.py, piano_a2s_amd/audio.py, tests/dynamics_oracle.py), without a
GPU: the note table, the oracle's level sums against a brute-force loop, the update (lower median with ties, both clamps, count = 0, clips of one
row and of none) in float64 and in the float32 restatement, the velocity mapping, the MIDI writer with per-note velocities, and the float64 loop on
one short rendered clip: the levels after round 3 are nearer to the amplitudes the clip was rendered with than after round 1."""
import numpy as np
import pytest

from piano_a2s_amd import audio, resynth, scoregen, spec
from tests import dynamics_oracle as oracle


def test_note_rows():
    hop, T, F = 160, 37, 480
    ev = np.array([[0, 100, 21],            # MIDI 21: b1 = 0; shorter than a frame: n = 1
                   [1600, 4000, 108],       # the top key: only the fundamental is a bin
                   [325, 160 * 30, 60],     # a long note: n stops at 12
                   [159, 2, 93],            # crosses one frame line: (159 + 2) // 160 - 159 // 160 = 1
                   [5600, 1600, 72]])       # fy + i runs past T = 37: the rows stay, the device drops the frames
    rows = resynth.note_rows(ev, None, hop, T, F, clip=3)
    assert rows.dtype == np.int32 and rows.shape == (5, 8)
    assert rows.tolist() == [[3, 1, 1, 1, 0, 60, 95, 1],
                             [3, 11, 11, 12, 435, -1, -1, 2],
                             [3, 3, 3, 12, 195, 255, 290, 3],
                             [3, 1, 1, 1, 360, 420, 455, 4],
                             [3, 36, 36, 10, 255, 315, 350, 5]]
    assert rows[4, 1] + rows[4, 3] > T, "the case the kernel has to clamp"
    # a third partial that leaves F while the second stays: 5 (midi - 21) + 95 >= F > 5 (midi - 21) + 60
    assert resynth.note_rows([[0, 1600, 100]], None, hop, T, F)[0, 4:7].tolist() == [395, 455, -1]
    assert resynth.note_rows([[0, 1600, 20]], None, hop, T, F)[0, 4:7].tolist() == [-1, 55, 90], "below the VQT's first bin"
    # performed onsets move fx alone
    moved = resynth.note_rows(ev, [10.0, 1919.9, 0.0, 480.5, 5600.0], hop, T, F)
    assert moved[:, 1].tolist() == [1, 12, 1, 4, 36] and np.array_equal(moved[:, 2:], resynth.note_rows(ev, None, hop, T, F)[:, 2:])
    assert resynth.note_rows(np.zeros((0, 3)), None, hop, T, F).shape == (0, 8)
    with pytest.raises(ValueError):
        resynth.note_rows(ev, None, 0, T, F)


def _brute(x, y, rows):
    B, T, F = x.shape
    out = np.zeros((len(rows), 3))
    for s, (clip, fx, fy, n, b1, b2, b3, _) in enumerate(rows):
        if not 0 <= clip < B:
            continue
        for i in range(max(0, n)):
            for b in (b1, b2, b3):
                if b < 0:
                    continue
                for col in (b - 1, b, b + 1):
                    if 0 <= col < F and 0 <= fx + i < T and 0 <= fy + i < T:
                        out[s] += (x[clip, fx + i, col], y[clip, fy + i, col], 1.0)
    return out


def test_level_sums_against_brute_force():
    rng = np.random.default_rng(1)
    B, T, F = 3, 37, 24
    x, y = rng.integers(0, 9, size=(2, B, T, F)) / 8.0
    rows = [(0, 3, 3, 5, 0, 10, 23, 1), (1, -2, 0, 5, 5, -1, 22, 2), (2, 30, 33, 12, 1, 2, 3, 3), (3, 0, 0, 5, 5, 6, 7, 1), (-1, 0, 0, 5, 5, 6, 7, 1),
            (0, 0, 0, 0, 5, 6, 7, 1), (1, 36, 36, 1, 23, -1, -1, 4), (2, 5, 9, 12, -1, -1, -1, 2), (0, 3, 3, 5, 0, 10, 23, 1), (1, 40, 2, 3, 4, 5, 6, 1)]
    got, want = oracle.levels(x, y, rows), _brute(x, y, rows)
    assert np.array_equal(got, want), "on a grid of 1/8 both are exact"
    assert got[0, 2] == 5 * (2 + 3 + 2) and got[6, 2] == 2 and not got[[3, 4, 5, 7, 9]].any() and np.array_equal(got[0], got[8])
    assert got[1, 2] == 3 * (3 + 3) and got[2, 2] == 4 * 9, "only the frames inside [0, T) on BOTH sides count"


def test_update_median_clamps_and_empty_clips():
    # clip 0: five rows, a tie at the lower median; clip 1: none; clip 2: one row; clip 3: two rows (lower median = the smaller); clip 4: clamps
    d = [[1.0, 3.0, 3.0, 3.0, 7.0], [], [4.5], [2.0, -2.0], [-50.0, 0.0, 0.0, 40.0]]
    first = np.concatenate([[0], np.cumsum([len(v) for v in d])])
    sums = np.array([(v / 80.0 * 4.0, 0.0, 4.0) for c in d for v in c]).reshape(-1, 3)
    sums[1] = (123.0, 7.0, 0.0)                                  # count = 0: d = 0 whatever the sums hold
    cum0 = np.arange(len(sums), dtype=np.float64) * 0.25
    for dtype in (np.float64, np.float32):
        got = oracle.update(sums, first, cum0.astype(dtype), dtype)
        assert got.dtype == dtype
        c0 = cum0[:5] + [1.0, 0.0, 3.0, 3.0, 7.0]                 # 1.0, 0.25, 3.5, 3.75, 8.0: lower median 3.5
        assert np.array_equal(got[:5], c0 - 3.5)
        assert got[5] == 0.0, "a clip of one row is its own median"
        assert np.array_equal(got[6:8], [(1.5 + 2.0) - (1.75 - 2.0), 0.0]), "of two rows the smaller is the median"
        assert np.array_equal(got[8:], [-30.0, 0.0, 0.25, 12.0]), "both clamps; of the tied pair the first is the median"
    assert oracle.lower_median([3.0, 1.0, 2.0, 2.0]) == 2.0 and oracle.lower_median([5.0, 1.0]) == 1.0 and oracle.lower_median([9.0]) == 9.0
    # no clips with rows: nothing moves
    assert np.array_equal(oracle.update(np.zeros((0, 3)), [0, 0, 0], np.zeros(0)), np.zeros(0))
    # the amplitudes: 10^(cum / 20), and the bound is a few units of 2^-24
    amp = oracle.amplitudes_f64([-20.0, 0.0, 12.0], 0.5)
    assert np.allclose(amp, [0.05, 0.5, 0.5 * 10 ** 0.6], rtol=1e-15)
    assert np.all(oracle.amp_bound([-30.0, 0.0, 12.0], 0.5) / oracle.amplitudes_f64([-30.0, 0.0, 12.0], 0.5) < 10 * 2.0 ** -24)


def test_velocity_mapping():
    assert [resynth.velocity(v) for v in (-30.0, 0.0, 12.0)] == [11, 64, 127]          # 64 * 10^-0.75 = 11.4; 64 * 10^0.3 = 127.7, capped
    assert [oracle.velocity(v) for v in (-30.0, 0.0, 12.0)] == [11, 64, 127]
    assert resynth.velocity(-200.0) == 1 and resynth.velocity(40.0) == 127
    assert all(resynth.velocity(v) == oracle.velocity(v) for v in np.linspace(-30, 12, 85))


def test_midi_bytes_with_and_without_velocities():
    # the exact-bytes case of tests/test_dtw_cpu.py, unchanged: a note without a velocity of its own gets the default 64
    want = (b"MThd" + bytes([0, 0, 0, 6, 0, 0, 0, 1, 0x01, 0xF4])                 # format 0, one track, 500 ticks per quarter
            + b"MTrk" + bytes([0, 0, 0, 20])
            + bytes([0x00, 0xFF, 0x51, 0x03, 0x07, 0xA1, 0x20])                     # 500000 us per quarter
            + bytes([0x00, 0x90, 60, 64])                                           # note on at 0
            + bytes([0x83, 0x74, 0x80, 60, 64])                                     # 500 ticks = 0.5 s later (variable length: 3 * 128 + 116) note off
            + bytes([0x00, 0xFF, 0x2F, 0x00]))
    assert audio.midi_bytes([[0.0, 0.5, 60]]) == want
    assert audio.midi_bytes([[0.0, 0.5, 60, 64]]) == want and audio.midi_bytes([[0.0, 0.5, 60, None]]) == want
    soft = want.replace(bytes([0x90, 60, 64]), bytes([0x90, 60, 11])).replace(bytes([0x80, 60, 64]), bytes([0x80, 60, 11]))
    assert audio.midi_bytes([[0.0, 0.5, 60, 11]]) == soft and audio.midi_bytes([[0.0, 0.5, 60, 11]], velocity=100) == soft
    assert audio.midi_bytes([[0.0, 0.5, 60]], velocity=11) == soft
    # mixed: the note with a velocity keeps it, the other gets the argument; on and off carry the same
    mixed = audio.midi_bytes([[0.0, 0.5, 60, 127], [0.25, 0.5, 64]], velocity=100)
    assert mixed[29:] == bytes([0x00, 0x90, 60, 127, 0x81, 0x7A, 0x90, 64, 100, 0x81, 0x7A, 0x80, 60, 127, 0x81, 0x7A, 0x80, 64, 100, 0x00, 0xFF, 0x2F, 0x00])
    for bad in (0, 128, 64.5):
        with pytest.raises(ValueError, match="velocity"):
            audio.midi_bytes([[0.0, 0.5, 60, bad]])
    with pytest.raises(ValueError):
        audio.midi_bytes([[0.0, 0.5, 60, 64, 1]])
    # a result with "dynamics" carries the velocities; "quiet" notes are left out; bars without either are as before
    result = {"windows": [{"bars": [{"notes": [[0.0, 0.5, 60], [0.25, 0.25, 64]], "dynamics": [[-3.0, 54], [None, None]]},
                                    {"notes": [[1.0, 0.5, 62]], "performed": [[1.1, 0.4, 62]], "dynamics": [[-25.0, 15]], "quiet": [True]},
                                    {"notes": [[2.0, 0.5, 65]]}]}]}
    assert audio.result_notes(result) == [[0.0, 0.5, 60, 54], [0.25, 0.25, 64], [2.0, 0.5, 65]]


def test_program_amplitudes():
    ev = np.array([[0, 1600, 60], [800, 1600, 64]])
    plain = resynth.program(ev, 9600)
    assert np.array_equal(resynth.program(ev, 9600, amps=None), plain) and np.array_equal(resynth.program(ev, 9600, [0.5, 0.5]), plain), "the default is unchanged"
    p = resynth.program(ev, 9600, amps=[0.25, 1.0])
    assert p[1:3, 3].view(np.float32).tolist() == [0.25, 1.0] and p[0, 6] == 0
    assert np.array_equal(np.delete(p[1:], 3, axis=1), np.delete(plain[1:], 3, axis=1)) and p[0, 5] != plain[0, 5], "the gain follows the amplitudes"


def test_float64_loop_on_one_short_clip():
    frames = 301
    clip = scoregen.make_clip(spec.default_cfg(max_length=(200, 200)), 103, frames=frames)
    scn = oracle.scenario(clip, np.random.default_rng(5), phantom_every=3)
    assert scn["real"].sum() == len(clip["events"]) >= 20 and (~scn["real"]).sum() >= 5
    n_samples = (frames - 1) * scoregen.HOP
    x = oracle.features64(resynth.program(scn["events"], n_samples, amps=scn["amps"]), n_samples)
    cums = oracle.loop64(x, scn["score"], n_samples, scoregen.HOP, 3)
    (rms1, auc1, spread), (rms3, auc3, _) = oracle.level_errors(cums[0], scn), oracle.level_errors(cums[2], scn)
    print(f"rms error {rms1:.3f} dB after round 1, {rms3:.3f} dB after round 3 (spread of the true levels {spread:.3f} dB); AUC {auc1:.3f}, {auc3:.3f}")
    assert rms3 < rms1 < spread, "the iteration sorts out what the one-shot reading cannot"
    assert auc3 > 0.9 and all(c.min() >= -30.0 and c.max() <= 12.0 for c in cums)
