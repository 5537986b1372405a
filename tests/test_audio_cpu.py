"""Host side of the audio front door (piano_a2s_amd/audio.py): the resampling filter and what the float64 definition of the
resampler (tests/resample_oracle.py) does with it, the WAV reader, the window plan.  No GPU."""
import math
import os
import struct
import sys
import wave

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_oracle as ro  # noqa: E402

from piano_a2s_amd import audio  # noqa: E402
from piano_a2s_amd.vqt import decimation_filter  # noqa: E402

RATES = {44100: (160, 441, 497), 48000: (1, 3, 541), 32000: (1, 2, 361), 22050: (320, 441, 249), 8000: (2, 1, 181), 96000: (1, 6, 1079)}


# ------------------------------------------------------------------------------------------- filter
@pytest.mark.parametrize("sr", sorted(RATES))
def test_filter_geometry(sr):
    L, M, K = RATES[sr]
    table, l, m, k, hh = audio.resample_filter(sr)
    assert (l, m, k, hh) == (L, M, K, (K - 1) // 2)
    assert table.shape == (L, K) and table.dtype == np.float32 and table.flags["C_CONTIGUOUS"]
    sums = table.astype(np.float64).sum(axis=1)
    print(f"sr {sr}: phase sums within {np.abs(sums - 1).max():.2e}")
    assert np.abs(sums - 1.0).max() < 1e-6
    h, half = audio.resample_prototype(sr)
    assert np.array_equal(h, h[::-1]) and len(h) == 2 * half + 1 and hh == -(-half // L)
    assert abs(h.sum() - L) < 1e-12
    # table[p][i] = h[p + (i - Hh) L], 0 outside
    for p in sorted({0, 1 % L, L // 2, L - 1}):
        for i in (0, 1, hh, K - 2, K - 1):
            t = p + (i - hh) * L
            want = h[t + half] if abs(t) <= half else 0.0
            assert table[p, i] == np.float32(want)


def test_table_size_44100():
    table = audio.resample_filter(44100)[0]
    assert 300_000 < table.nbytes < 320_000


def test_identity_filter():
    table, L, M, K, Hh = audio.resample_filter(16000)
    assert (L, M, K, Hh) == (1, 1, 1, 0) and table.tolist() == [[1.0]]


def test_32k_prototype_is_the_vqt_decimator():
    h, half = audio.resample_prototype(32000)
    d, dhalf = decimation_filter()
    assert half == dhalf == 180
    assert np.abs(h - d / math.sqrt(2.0)).max() <= 1e-15


# ------------------------------------------------------------------------------------------- quality of the float64 definition (design target 120 dB)
def _tone(sr, f, seconds=0.5):
    return np.sin(2.0 * np.pi * f * np.arange(int(sr * seconds)) / sr).astype(np.float32)


@pytest.fixture(scope="module")
def tables():
    return {sr: audio.resample_filter(sr) for sr in (44100, 48000, 8000)}


@pytest.mark.parametrize("sr,f", [(44100, 1000), (44100, 7000), (48000, 1000), (48000, 7000), (8000, 1000)])
def test_oracle_passes_tones(tables, sr, f):
    table, L, M, K, Hh = tables[sr]
    y = ro.resample(_tone(sr, f), table, M, Hh)
    assert len(y) == 8000
    want = np.sin(2.0 * np.pi * f * np.arange(len(y)) / 16000.0)
    err = np.abs(y - want)[400:-400].max()
    print(f"{sr} Hz, tone {f} Hz: oracle within {err:.2e} of the analytic sine")
    assert err < 1e-6


@pytest.mark.parametrize("sr,f", [(44100, 9000), (44100, 12000), (48000, 9000), (48000, 12000)])
def test_oracle_stops_tones(tables, sr, f):
    table, L, M, K, Hh = tables[sr]
    y = ro.resample(_tone(sr, f), table, M, Hh)
    left = np.abs(y)[400:-400].max()
    print(f"{sr} Hz, tone {f} Hz: {left:.2e} left")
    assert left < 1e-6


def test_oracle_n_out_and_edges():
    table = (1 + (7 * np.arange(3)[:, None] + 3 * np.arange(9)[None, :]) % 5).astype(np.float32)
    x = np.arange(1, 11, dtype=np.float32)
    y = ro.resample(x, table, 7, 4)
    assert len(y) == ro.n_out(10, 3, 7) == 5
    for n in range(5):
        q = n * 7
        want = sum(table[q % 3, i] * (x[q // 3 + 4 - i] if 0 <= q // 3 + 4 - i < 10 else 0.0) for i in range(9))
        assert y[n] == want
    assert len(ro.resample(np.zeros(0, dtype=np.float32), table, 7, 4)) == 0
    st = np.stack([x, 3 * x], axis=1)
    assert np.array_equal(ro.mono_mix(st), 2 * x)


# ------------------------------------------------------------------------------------------- WAV files
def _stdlib_wav(path, ints, width, sr, channels):
    if width == 1:
        raw = (ints + 128).astype(np.uint8).tobytes()
    elif width == 3:
        raw = b"".join(int(v).to_bytes(3, "little", signed=True) for v in ints.reshape(-1))
    else:
        raw = ints.astype("<i2" if width == 2 else "<i4").tobytes()
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(sr)
        w.writeframes(raw)


@pytest.mark.parametrize("bits", [8, 16, 24, 32])
def test_read_wav_pcm_written_by_the_stdlib(tmp_path, bits):
    rng = np.random.default_rng(bits)
    full = 2 ** (bits - 1)
    ints = rng.integers(-full, full, size=(37, 2), dtype=np.int64)
    ints[0], ints[1] = -full, full - 1
    _stdlib_wav(tmp_path / "a.wav", ints, bits // 8, 44100, 2)
    x, sr = audio.read_wav(tmp_path / "a.wav")
    assert sr == 44100 and x.shape == (37, 2) and x.dtype == np.float32
    assert np.array_equal(x, (ints.astype(np.float64) / full).astype(np.float32))


@pytest.mark.parametrize("bits", [8, 16, 24, 32, -32])
def test_write_wav_round_trip(tmp_path, bits):
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, size=(51, 3))
    x[0] = (-1.0, 1.0, 0.0)
    audio.write_wav(tmp_path / "b.wav", x, 22050, bits=bits)
    y, sr = audio.read_wav(tmp_path / "b.wav")
    assert sr == 22050 and y.shape == (51, 3)
    if bits == -32:
        assert np.array_equal(y, x.astype(np.float32))
    else:
        assert np.array_equal(y, (audio.quantise(x, bits) / 2.0 ** (bits - 1)).astype(np.float32))
        assert np.abs(y[1:] - x[1:]).max() <= 2.0 ** -bits + 2.0 ** -24          # half a step, and the float32 the reader returns
    if bits in (8, 16, 24, 32):                                             # the stdlib reads what write_wav wrote
        with wave.open(str(tmp_path / "b.wav"), "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (3, bits // 8, 22050, 51)
    mono = tmp_path / "m.wav"
    audio.write_wav(mono, x[:, 0], 8000)
    assert audio.read_wav(mono)[0].shape == (51, 1)


def _chunk(cid, body, pad=True):
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if pad and len(body) & 1 else b"")


def _riff(*chunks):
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def _fmt(code, channels, sr, bits, ext_sub=None):
    base = struct.pack("<HHIIHH", code, channels, sr, sr * channels * bits // 8, channels * bits // 8, bits)
    if ext_sub is None:
        return base
    guid_tail = bytes.fromhex("000000001000800000aa00389b71")
    return base + struct.pack("<HHI", 22, bits, 3) + struct.pack("<H", ext_sub) + guid_tail


def test_read_wav_float_and_extensible(tmp_path):
    v = np.array([[0.25, -0.5], [1.5, -1e-3], [0.0, 3.0]])
    p = tmp_path / "f.wav"
    p.write_bytes(_riff(_chunk(b"fmt ", _fmt(3, 2, 48000, 32)), _chunk(b"data", v.astype("<f4").tobytes())))
    x, sr = audio.read_wav(p)
    assert sr == 48000 and np.array_equal(x, v.astype(np.float32))
    p.write_bytes(_riff(_chunk(b"fmt ", _fmt(3, 2, 96000, 64)), _chunk(b"data", v.astype("<f8").tobytes())))
    x, sr = audio.read_wav(p)
    assert sr == 96000 and np.array_equal(x, v.astype(np.float32))
    ints = np.array([[1000, -2000], [32767, -32768]], dtype="<i2")
    p.write_bytes(_riff(_chunk(b"fmt ", _fmt(0xFFFE, 2, 44100, 16, ext_sub=1)), _chunk(b"data", ints.tobytes())))
    x, sr = audio.read_wav(p)
    assert sr == 44100 and np.array_equal(x, ints.astype(np.float32) / 32768)
    p.write_bytes(_riff(_chunk(b"fmt ", _fmt(0xFFFE, 2, 44100, 32, ext_sub=3)), _chunk(b"data", v.astype("<f4").tobytes())))
    assert np.array_equal(audio.read_wav(p)[0], v.astype(np.float32))


def test_read_wav_chunk_walk(tmp_path):
    ints = np.array([[1], [-2], [3]], dtype="<i2")
    fmt = _chunk(b"fmt ", _fmt(1, 1, 16000, 16))
    p = tmp_path / "c.wav"
    # an odd-sized unknown chunk (with its pad byte) and an even one in front of the data
    p.write_bytes(_riff(fmt, _chunk(b"LIST", b"abc"), _chunk(b"bext", b"wxyz"), _chunk(b"data", ints.tobytes())))
    x, sr = audio.read_wav(p)
    assert sr == 16000 and np.array_equal(x, ints.astype(np.float32) / 32768)
    # a data chunk that claims more than the file holds: cut to whole frames (here 2 stereo frames and a stray sample)
    five = np.array([10, 20, 30, 40, 50], dtype="<i2").tobytes()
    p.write_bytes(_riff(_chunk(b"fmt ", _fmt(1, 2, 16000, 16)), b"data" + struct.pack("<I", 4000) + five))
    x, sr = audio.read_wav(p)
    assert x.shape == (2, 2) and np.array_equal(x, np.array([[10, 20], [30, 40]], dtype=np.float32) / 32768)
    # an odd-sized data chunk (8-bit mono, 3 frames) followed by another chunk
    p.write_bytes(_riff(_chunk(b"fmt ", _fmt(1, 1, 8000, 8)), _chunk(b"data", bytes([128, 0, 255])), _chunk(b"LIST", b"zz")))
    x, sr = audio.read_wav(p)
    assert np.array_equal(x[:, 0], np.array([0.0, -1.0, 127 / 128], dtype=np.float32))


@pytest.mark.parametrize("code", [2, 6])
def test_read_wav_refuses_other_formats(tmp_path, code):
    p = tmp_path / "r.wav"
    p.write_bytes(_riff(_chunk(b"fmt ", _fmt(code, 1, 8000, 8)), _chunk(b"data", b"\0\0")))
    with pytest.raises(ValueError, match=rf"format code {code}\b"):
        audio.read_wav(p)


def test_read_wav_refuses_what_is_no_wave_file(tmp_path):
    p = tmp_path / "n.wav"
    p.write_bytes(b"RIFX" + b"\0" * 40)
    with pytest.raises(ValueError, match="RIFF"):
        audio.read_wav(p)
    p.write_bytes(_riff(_chunk(b"data", b"\0\0")))
    with pytest.raises(ValueError, match="fmt"):
        audio.read_wav(p)
    p.write_bytes(_riff(_chunk(b"fmt ", _fmt(1, 1, 8000, 12)), _chunk(b"data", b"\0\0")))
    with pytest.raises(ValueError, match="format code 1"):
        audio.read_wav(p)


# ------------------------------------------------------------------------------------------- window plan
S = 16000


def test_plan_regular_downbeats():
    db = [1.0 + 2.0 * i for i in range(12)]                                  # 11 bars of 2 s
    plan = audio.plan_windows(40 * S, downbeats=db)
    assert plan == [(1 * S, 11 * S, 5), (11 * S, 21 * S, 5), (21 * S, 23 * S, 1)]
    assert audio.plan_flags(40 * S, downbeats=db) == [[], [], []]


def test_plan_group_longer_than_the_window():
    db = [0.0, 3.0, 6.0, 9.0, 12.0, 15.0, 16.0]                              # five bars of 3 s last 15 s: four are kept
    assert audio.plan_windows(20 * S, downbeats=db) == [(0, 12 * S, 4), (12 * S, 16 * S, 2)]


def test_plan_one_long_bar_is_cut_and_flagged():
    db = [2.0, 16.0, 18.0]
    assert audio.plan_windows(20 * S, downbeats=db) == [(2 * S, 14 * S, 1), (16 * S, 18 * S, 1)]
    assert audio.plan_flags(20 * S, downbeats=db) == [["bar_cut"], []]


def test_plan_downbeats_behind_the_end():
    assert audio.plan_windows(5 * S, downbeats=[1.0, 3.0, 7.0, 9.0]) == [(1 * S, 5 * S, 2)]
    with pytest.raises(ValueError, match="ascend"):
        audio.plan_windows(5 * S, downbeats=[2.0, 1.0])


def test_plan_without_downbeats():
    assert audio.plan_windows(30 * S) == [(0, 12 * S, 5), (12 * S, 24 * S, 5), (24 * S, 30 * S, 5)]
    assert audio.plan_flags(30 * S) == [[], [], ["short"]]
    assert audio.plan_windows(30 * S, window_seconds=10.0, hop_seconds=8.0, max_bars=3) == [(0, 10 * S, 3), (8 * S, 18 * S, 3), (16 * S, 26 * S, 3),
                                                                                            (24 * S, 30 * S, 3)]
    assert audio.plan_windows(24 * S) == [(0, 12 * S, 5), (12 * S, 24 * S, 5)]
    assert audio.plan_windows(30 * S, window_seconds=20.0) == audio.plan_windows(30 * S)          # never more than 12 s
    assert audio.plan_windows(30 * S, max_samples=1200 * 160) == audio.plan_windows(30 * S)
    assert audio.plan_windows(2000, max_samples=800) == [(0, 800, 5), (800, 1600, 5), (1600, 2000, 5)]


def test_plan_short_and_empty_recordings():
    assert audio.plan_windows(5000) == [(0, 5000, 5)]
    assert audio.plan_windows(0) == []
    assert audio.plan_windows(0, downbeats=[0.0, 1.0]) == []
    assert audio.plan_windows(5000, downbeats=[0.1]) == []
