"""The per-kernel references of the VQT front end (tests/vqt_ops_oracle.py) pinned, without a GPU, to the project's own oracle (oracle/vqt_ref.py), so
that tests/test_gpu_vqt_ops.py rests on something checked here:

1. logmag_ref at top_db = 80 on one clip is oracle.vqt_ref.amplitude_to_unit;
2. decimate_ref, fed the padding and the reversed taps piano_a2s_amd.vqt builds for the device, is oracle.vqt_ref._decimate2;
3. pack_octaves is a pure permutation of pack_plain, the highest octave first;
4. framed_gemm_ref against an explicit loop, and the frames of oracle.vqt_ref._cqt_response;
5. the inputs of the epilogue tests are what they claim to be."""
import numpy as np
import pytest

from oracle import vqt_ref as V
from piano_a2s_amd import vqt as product
from tests import vqt_ops_oracle as O


# ------------------------------------------------------------------------------------------- 1. the epilogue
@pytest.mark.parametrize("peak", [1e4, 1.0, 3e-6, 0.0])
def test_logmag_ref_is_the_oracles_amplitude_to_unit(peak):
    re, im = O.logmag_case((1, 37, 480, 60), (peak,), "high_block", 5)
    out, db = O.logmag_ref(re, im, 80.0)
    want = V.amplitude_to_unit((re[0].astype(np.float64) + 1j * im[0].astype(np.float64)).T)          # (bins, frames) in, (frames, bins) out
    assert out.shape == (1, 37, 480) and np.abs(out[0] - want).max() <= 1e-12
    assert db.max() == 0.0 and np.array_equal(out == 0.0, db <= -80.0)
    if peak >= 1.0:
        assert (db < -80.0).any() and (db > -80.0).any(), "cells on both sides of the clamp"
    else:
        assert np.all(out == 1.0), "a clip that stays below the floor is 1.0 everywhere, as silence is"


def test_logmag_ref_clamps_at_top_db_and_takes_each_clips_own_maximum():
    re, im = O.logmag_case((3, 7, 24, 4), O.PEAK_SETS["far"], "last_cell", 6)
    out60, db = O.logmag_ref(re, im, 60.0)
    assert out60.min() == 0.25 and np.array_equal(out60 == 0.25, db <= -60.0)
    for b in range(3):                                                                    # a batch is its clips one by one
        one, _ = O.logmag_ref(re[b:b + 1], im[b:b + 1], 60.0)
        assert np.array_equal(one[0], out60[b]) and out60[b, 6, 23] == 1.0


# ------------------------------------------------------------------------------------------- 2. the decimator
@pytest.mark.parametrize("N", [1, 2, 361, 362, 5121])
def test_decimate_ref_is_the_oracles_decimator(N):
    y = np.random.default_rng(N).standard_normal(N)
    h, half = product.decimation_filter()
    taps = product.decimator_taps(h)                                                      # float64: the class rounds them to float32 for the device
    assert len(taps) == 364 and len(h) == 361 == 2 * half + 1 and np.all(taps[361:] == 0.0) and np.array_equal(taps[:361], h[::-1])
    off, plen, n_out = product.decimate_layout(N, half, len(taps))
    assert off == half and n_out == (N + 1) // 2 and plen % 4 == 0 and plen >= 2 * n_out + len(taps)
    ypad = np.zeros((1, plen))
    ypad[0, off:off + N] = y
    out, mag = O.decimate_ref(ypad, taps, n_out)
    want = V._decimate2(y)
    assert out.shape == (1, n_out) == (1,) + want.shape
    assert np.abs(out[0] - want).max() <= 1e-12
    assert np.all(mag >= np.abs(out) - 1e-15)
    # the same from a row cut right behind the signal: what lies at or beyond the row length is zero
    short, _ = O.decimate_ref(ypad[:, :off + N], taps, n_out)
    assert np.array_equal(short, out)


def test_decimate_ref_against_an_explicit_loop():
    g = np.random.default_rng(2)
    ypad, taps, n_out = g.standard_normal((2, 23)), g.standard_normal(6), 11                # 2 * 10 + 6 = 26 > 23: the last outputs reach beyond the row
    out, mag = O.decimate_ref(ypad, taps, n_out)
    for b in range(2):
        for m in range(n_out):
            terms = [ypad[b, 2 * m + j] * taps[j] for j in range(6) if 2 * m + j < 23]
            assert abs(out[b, m] - sum(terms)) < 1e-14 and abs(mag[b, m] - sum(abs(t) for t in terms)) < 1e-14


# ------------------------------------------------------------------------------------------- 3. the two layouts
@pytest.mark.parametrize("B,rows,bins,bpo", [(2, 3, 480, 60), (3, 7, 24, 4), (1, 5, 60, 60)])
def test_pack_octaves_is_a_permutation_of_pack_plain(B, rows, bins, bpo):
    cells = np.arange(B * rows * bins, dtype=np.float64).reshape(B, rows, bins)           # every cell a value of its own; im = -1 - re
    re, im = cells, -1.0 - cells
    plain, octs = O.pack_plain(re, im), O.pack_octaves(re, im, bpo)
    assert plain.shape == octs.shape == (B, rows, 2 * bins)
    assert np.array_equal(np.sort(plain, axis=2), np.sort(octs, axis=2)), "row by row the same values"
    assert np.array_equal(plain[:, :, :bins], re) and np.array_equal(plain[:, :, bins:], im)
    for o in range(bins // bpo):                                                           # include/a2s.h: octave o (highest first) = [re | im] of its bins
        lo = bins - (o + 1) * bpo
        assert np.array_equal(octs[:, :, o * 2 * bpo:o * 2 * bpo + bpo], re[:, :, lo:lo + bpo])
        assert np.array_equal(octs[:, :, o * 2 * bpo + bpo:(o + 1) * 2 * bpo], im[:, :, lo:lo + bpo])
    with pytest.raises(ValueError):
        O.pack_octaves(re, im, bpo + 1)


def test_pack_octaves_is_the_column_order_the_front_end_writes():
    """VQT.__call__ gives octave i (highest first) the columns [i * 2 nb, (i + 1) * 2 nb) and its bank is [Re g | Im g] of bins lo .. hi."""
    col = 0
    re = np.arange(480, dtype=np.float64)[None, None, :]
    octs = O.pack_octaves(re, re + 1000.0, 60)
    for o in product.octave_banks():
        nb = o["hi"] - o["lo"]
        assert np.array_equal(octs[0, 0, col:col + nb], np.arange(o["lo"], o["hi"]))
        assert np.array_equal(octs[0, 0, col + nb:col + 2 * nb], 1000.0 + np.arange(o["lo"], o["hi"]))
        col += 2 * nb
    assert col == 960


# ------------------------------------------------------------------------------------------- 4. the framed product
def test_framed_gemm_ref_against_an_explicit_loop_and_the_oracles_frames():
    g = np.random.default_rng(4)
    hop, n_fft, frames = 5, 32, 9
    padded, bank = g.standard_normal((2, (frames - 1) * hop + n_fft)), g.standard_normal((n_fft, 6))
    out, mag = O.framed_gemm_ref(padded, hop, bank, frames)
    assert out.shape == mag.shape == (2, frames, 6)
    for b in range(2):
        for n in range(frames):
            row = padded[b, n * hop:n * hop + n_fft]
            assert np.abs(out[b, n] - row @ bank).max() < 1e-13 and np.abs(mag[b, n] - np.abs(row) @ np.abs(bank)).max() < 1e-13
    with pytest.raises(ValueError):
        O.framed_gemm_ref(padded[:, :-1], hop, bank, frames)
    # the oracle's response of an octave is this product with the DFT as the bank: fft_basis @ rfft(frames) = frames @ (fft_basis @ DFT)^T
    y = g.standard_normal(3 * hop + 1)
    basis = g.standard_normal((6, n_fft // 2 + 1)) + 1j * g.standard_normal((6, n_fft // 2 + 1))
    want = V._cqt_response(y, n_fft, hop, basis)                                            # (6, frames)
    yp = np.concatenate([np.zeros(n_fft // 2), y, np.zeros(n_fft // 2)])[None, :]
    dft = np.exp(-2j * np.pi * np.outer(np.arange(n_fft // 2 + 1), np.arange(n_fft)) / n_fft)
    gk = (basis @ dft).T                                                                    # (n_fft, 6) complex
    got_re, _ = O.framed_gemm_ref(yp, hop, gk.real, want.shape[1])
    got_im, _ = O.framed_gemm_ref(yp, hop, gk.imag, want.shape[1])
    assert np.abs(got_re[0].T + 1j * got_im[0].T - want).max() < 1e-11


# ------------------------------------------------------------------------------------------- 5. the inputs of the epilogue tests
@pytest.mark.parametrize("shape", O.LOGMAG_SHAPES)
@pytest.mark.parametrize("place", O.PEAK_PLACES)
def test_epilogue_inputs_hold_their_maximum_where_they_say(shape, place):
    B, rows, bins, _ = shape
    r, k = O.peak_cell(place, rows, bins)
    assert 0 <= r < rows and 0 <= k < bins
    if place == "high_block":
        assert ((r * bins + k) // 256) % 64 == min(63, (rows * bins - 1) // 256)
    for name, peaks in O.PEAK_SETS.items():
        re, im = O.logmag_case(shape, peaks, place, 1)
        mag = np.hypot(re.astype(np.float64), im.astype(np.float64))
        for b in range(B):
            want = float(np.float32(peaks[b]))
            assert mag[b].max() == want and (want == 0.0 or (mag[b, r, k] == want and np.sum(mag[b] > 0.495 * want) == 1)), (name, b)
            assert want == 0.0 or want < 1.0 or mag[b].min() < 1e-5 < np.sort(mag[b].ravel())[-2], "cells on both sides of the floor"


def test_the_device_bounds_separate_the_faults_they_are_meant_for():
    """The bounds of tests/test_gpu_vqt_ops.py against restated faults: a dropped tap, a window shifted by a sample, a neighbour's maximum, two bins
    swapped.  (An ulp between two clips' maxima is NOT visible in the output -- 1e-6 dB is a seventh of a unit; a part in a thousand is.)"""
    g = np.random.default_rng(9)
    ntaps, n_out = 364, 255
    taps, ypad = g.standard_normal(ntaps), g.standard_normal((1, 2 * n_out + ntaps))
    ref, mag = O.decimate_ref(ypad, taps, n_out)
    bound = ntaps * 2.0 ** -24
    for j in np.flatnonzero(np.abs(taps) > 0.01):
        dropped = taps.copy()
        dropped[j] = 0.0
        assert (np.abs(O.decimate_ref(ypad, dropped, n_out)[0] - ref) / mag).max() > 10 * bound, j
    shifted = O.decimate_ref(np.concatenate([ypad[:, 1:], np.zeros((1, 1))], axis=1), taps, n_out)[0]
    assert (np.abs(shifted - ref) / mag).max() > 1000 * bound
    tol = (2 * 4 * 1.8 + 3) * 2.0 ** -17 / 80.0
    re, im = O.logmag_case((3, 7, 24, 4), O.PEAK_SETS["close"], "first_row", 1)
    ref, _ = O.logmag_ref(re, im, 80.0)
    extra = np.zeros((1, 1, 24), dtype=np.float32)
    extra[0, 0, 0] = 1.001                                                                 # clip 1 under clip 2's maximum: one more row that holds it
    leaked, _ = O.logmag_ref(np.concatenate([re[1:2], extra], axis=1), np.concatenate([im[1:2], 0 * extra], axis=1), 80.0)
    mag1 = np.hypot(re[1].astype(np.float64), im[1].astype(np.float64))
    assert np.abs(leaked[0, :7] - ref[1])[mag1 > 1e-3].min() > 50 * tol
    re, im = O.layout_case(2, 5, 480, 60, 10.0)
    ref, _ = O.logmag_ref(re, im, 80.0)
    for a in (0, 59, 60, 478):                                                             # inside an octave and across a boundary
        sw = ref.copy()
        sw[:, :, [a, a + 1]] = sw[:, :, [a + 1, a]]
        assert np.abs(sw - ref).max() > 1000 * tol


def test_layout_inputs_are_distinct_cell_by_cell():
    for args, floor in (((2, 5, 480, 60, 10.0), False), ((3, 7, 24, 4, 20.0), True)):
        re, im = O.layout_case(*args)
        out, db = O.logmag_ref(re, im, 80.0)
        assert (db.min() < -80.0) == floor
        row = db[0, 0][db[0, 0] > -80.0]
        assert len(row) >= 16 and np.all(np.diff(row) > 0.1), "above the clamp monotone along the bins, neighbours 0.15 dB or more apart: 1.8e-3 of the output range"
