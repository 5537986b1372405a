"""a2s_resample_rows (csrc/a2s_resample.hip) against its float64 definition (tests/resample_oracle.py): exact on integers, the
a-priori bound of a K-term fp32 chain on the real tables, 64-bit positions, batch independence, a band-limited signal through resampler and VQT,
refusals and counters."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_oracle as ro  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _int_table(L, K):
    return (1 + (7 * np.arange(L)[:, None] + 3 * np.arange(K)[None, :]) % 5).astype(np.float32)


def _n_in_around(tile, L, M):
    """n_in for an n_out just below, at and just above the tile: tile - 1, tile and tile + 1 where ceil(n_in L / M) takes those values; when upsampling
    it skips some, and then the largest n_out below the tile, the tile itself if it is taken, and the smallest n_out above it."""
    outs = {}
    n = max(0, (tile - 8) * M // L - 2)
    while ro.n_out(n, L, M) <= tile + 8:
        outs.setdefault(ro.n_out(n, L, M), n)
        n += 1
    below, above = max(o for o in outs if o < tile), min(o for o in outs if o > tile)
    assert below >= tile - L and above <= tile + L
    return [outs[below]] + ([outs[tile]] if tile in outs else []) + [outs[above]]


def _run(dev, clips, table, M, Hh, C, aligned, extra_out=5):
    """clips: list of (n_in, C) arrays.  x rows hold NaN behind every clip, y rows have sentinels on both sides.  Returns (y (B, n_out_max) on the host,
    n_out_max)."""
    from piano_a2s_amd import hip
    L, K = table.shape
    B = len(clips)
    n_in = [len(c) for c in clips]
    n_in_max = max(n_in)
    n_out_max = ro.n_out(n_in_max, L, M) + extra_out
    xs = n_in_max * C + ((-n_in_max * C) % 4 + 4 if aligned else 3)          # row strides: a multiple of 16 bytes, or one that breaks the alignment
    if not aligned and xs % 4 == 0:
        xs += 1
    x_off = 0 if aligned else 1
    xbuf = torch.full((B * xs + 8,), float("nan"), dtype=torch.float32)
    for b, c in enumerate(clips):
        xbuf[x_off + b * xs: x_off + b * xs + n_in[b] * C] = torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32).reshape(-1))
    xbuf = xbuf.to(dev)
    x = torch.as_strided(xbuf, (B, n_in_max * C), (xs, 1), x_off)
    pad = 4 if aligned else 3
    ys = pad + n_out_max + pad
    ys += (-ys) % 4 if aligned else (1 if ys % 4 == 0 else 0)
    ybuf = torch.full((B, ys), 777.0, dtype=torch.float32, device=dev)
    y = ybuf[:, pad:pad + n_out_max]
    assert (x.data_ptr() % 16 == 0 and xs % 4 == 0) == aligned and (y.data_ptr() % 16 == 0 and ys % 4 == 0) == aligned
    t = torch.from_numpy(table).to(dev)
    out = hip.resample_rows(x, torch.tensor(n_in, dtype=torch.int32, device=dev), t, M, Hh, channels=C, y=y, n_out_max=n_out_max, n_in_max=n_in_max)
    assert out.data_ptr() == y.data_ptr()
    torch.cuda.synchronize()
    full = ybuf.cpu()
    assert (full[:, :pad] == 777.0).all() and (full[:, pad + n_out_max:] == 777.0).all(), "the sentinels around y"
    return full[:, pad:pad + n_out_max].clone(), n_out_max


# ------------------------------------------------------------------------------------------- 1. exact on integers
@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("L,M", [(3, 7), (5, 2)])
def test_exact_on_integers(dev, L, M, C, aligned):
    from piano_a2s_amd import hip
    K, Hh = 9, 4
    tile = hip.resample_tile_samples()
    table = _int_table(L, K)
    rng = np.random.default_rng(100 * L + 10 * M + C)
    edge = _n_in_around(tile, L, M)
    if M >= L:
        assert [ro.n_out(n, L, M) for n in edge] == [tile - 1, tile, tile + 1]
    for lens in ([0, 1, edge[0], edge[-2]], [edge[-1], 1, 0, edge[-2]]):
        clips = [rng.integers(-8, 9, size=(n, C)).astype(np.float32) for n in lens]
        y, n_out_max = _run(dev, clips, table, M, Hh, C, aligned)
        for b, c in enumerate(clips):
            want = ro.resample(c, table, M, Hh)
            n = ro.n_out(len(c), L, M)
            assert len(want) == n
            assert torch.equal(y[b, :n], torch.from_numpy(want.astype(np.float32))), (lens, b)
            assert (y[b, n:] == 0).all() and n_out_max > n, (lens, b)


# ------------------------------------------------------------------------------------------- 2. the real tables
@pytest.mark.parametrize("sr", [44100, 48000, 22050, 8000])
def test_real_tables_within_the_fp32_chain_bound(dev, sr):
    from piano_a2s_amd import audio
    table, L, M, K, Hh = audio.resample_filter(sr)
    rng = np.random.default_rng(sr)
    clips = [rng.uniform(-1, 1, size=(n, 2)).astype(np.float32) for n in (3001, 4999, 4100)]
    worst, ratio = 0.0, 0.0
    for aligned in (True, False):
        y, _ = _run(dev, clips, table, M, Hh, 2, aligned)
        for b, c in enumerate(clips):
            y64, bound = ro.resample_blocks(c, table, M, Hh)
            err = np.abs(y[b, :len(y64)].numpy().astype(np.float64) - y64)
            worst, ratio = max(worst, err.max()), max(ratio, (err / np.maximum(bound, 1e-300)).max())
            assert (err <= bound).all(), f"clip {b}: {err.max():.3e}"
            assert (y[b, len(y64):] == 0).all()
    print(f"resample {sr} -> 16000: max |y - y64| = {worst:.3e}, at most {ratio:.3f} of the bound")


# ------------------------------------------------------------------------------------------- 3. 64-bit positions
def test_positions_beyond_31_bits(dev):
    from piano_a2s_amd import audio, hip
    table, L, M, K, Hh = audio.resample_filter(44100)
    N = 14_000_000
    x = np.random.default_rng(7).uniform(-1, 1, size=N).astype(np.float32)
    total = ro.n_out(N, L, M)
    first = -(-2 ** 31 // M)                                                # the first output whose position n M needs more than 31 bits
    assert 4_869_000 < first < 4_870_500 < total and first * M >= 2 ** 31 > (first - 1) * M
    y = hip.resample_rows(torch.from_numpy(x).to(dev)[None], torch.tensor([N], dtype=torch.int32, device=dev), torch.from_numpy(table).to(dev), M, Hh)
    assert tuple(y.shape) == (1, total)
    for start, stop in ((4_869_000, 4_870_500), (total - 600, total)):
        y64, bound = ro.resample(x, table, M, Hh, start, stop, with_bound=True)
        err = np.abs(y[0, start:stop].cpu().numpy().astype(np.float64) - y64)
        print(f"outputs [{start}, {stop}): max |y - y64| = {err.max():.3e}")
        assert (err <= bound).all() and np.abs(y64).max() > 0.1


# ------------------------------------------------------------------------------------------- 4. batch independence
def test_a_clips_bits_do_not_depend_on_the_batch(dev):
    from piano_a2s_amd import audio
    table, L, M, K, Hh = audio.resample_filter(44100)
    rng = np.random.default_rng(11)
    clip = rng.uniform(-1, 1, size=(3800, 2)).astype(np.float32)
    others = [rng.uniform(-1, 1, size=(n, 2)).astype(np.float32) for n in (5000, 17)]
    alone, _ = _run(dev, [clip], table, M, Hh, 2, True)
    n = ro.n_out(len(clip), L, M)
    batch, _ = _run(dev, [others[0], clip, others[1]], table, M, Hh, 2, False)
    wide, _ = _run(dev, [clip], table, M, Hh, 2, False, extra_out=3001)
    assert torch.equal(alone[0, :n], batch[1, :n]) and torch.equal(alone[0, :n], wide[0, :n])
    assert (batch[1, n:] == 0).all() and (wide[0, n:] == 0).all() and alone[0, :n].abs().max() > 0.1


# ------------------------------------------------------------------------------------------- 5. a band-limited signal, resampler and VQT
TONES = [55.0, 110.0, 261.6, 440.0, 987.8, 1760.0, 3136.0, 3400.0, 4186.0, 5588.0, 7000.0]


def _signal(sr, fmax):
    """Gaussian-enveloped tones, 1.5 s, peak about 1, sampled analytically at the rate sr (float64)."""
    t = np.arange(int(round(1.5 * sr))) / float(sr)
    tones = [f for f in TONES if f <= fmax]
    s = np.zeros_like(t)
    for k, f in enumerate(tones):
        centre, sigma = 0.45 + 0.6 * k / len(TONES), 0.055 + 0.004 * (k % 3)
        s += 0.45 * np.exp(-0.5 * ((t - centre) / sigma) ** 2) * np.sin(2.0 * np.pi * f * t + 0.7 * k)
    return s


@pytest.mark.parametrize("sr", [44100, 48000, 22050, 8000])
def test_band_limited_signal_and_its_features(dev, sr):
    from piano_a2s_amd import audio
    from piano_a2s_amd.vqt import VQT
    fmax = 3500.0 if sr == 8000 else 8000.0
    native = _signal(16000, fmax)
    assert 0.5 < np.abs(native).max() < 1.5
    x = _signal(sr, fmax).astype(np.float32)
    rs = audio.Resampler(dev, sr)
    y, n_out = rs(torch.from_numpy(x).to(dev)[None])
    assert tuple(y.shape) == (1, len(native)) and n_out.tolist() == [len(native)]
    table = rs.table.cpu().numpy()
    y64, bound = ro.resample_blocks(x, table, rs.M, rs.Hh)
    own = np.abs(y64 - native)                                               # what the filter itself leaves: the float64 definition against the signal
    err = np.abs(y[0].cpu().numpy().astype(np.float64) - native)
    print(f"{sr} -> 16000: float64 definition off by {own.max():.3e}, device result off by {err.max():.3e}")
    assert (err <= own + bound).all()
    vqt = VQT(dev)
    f_rs = vqt(y)
    f_native = vqt(torch.from_numpy(native.astype(np.float32)).to(dev)[None])
    diff = (f_rs - f_native).abs().max().item()
    print(f"{sr} -> 16000: VQT features of the resampled signal within {diff:.3e} of the native ones")
    assert tuple(f_rs.shape) == (1, 1, 151, 480) and diff < 1e-3


def test_resampler_front_door(dev):
    """Resampler: (B, N, C) and (B, N), n_in, the identity rate, CPU tensors."""
    from piano_a2s_amd import audio, hip
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.uniform(-1, 1, size=(2, 900, 2)).astype(np.float32)).to(dev)
    same = audio.Resampler(dev, 16000)
    mono = x[:, :, 0].contiguous()
    y, n = same(mono)
    assert y.data_ptr() == mono.data_ptr() and n.tolist() == [900, 900]
    n0 = hip.resample_launches()
    y, n = same(x, n_in=[900, 10])                                           # two channels: the kernel runs with the identity table
    assert hip.resample_launches() == n0 + 1 and n.tolist() == [900, 10]
    want = (x[:, :, 0] + x[:, :, 1]) * 0.5
    assert torch.equal(y[0], want[0]) and torch.equal(y[1, :10], want[1, :10]) and (y[1, 10:] == 0).all()
    rs = audio.Resampler(dev, 48000)
    y, n = rs(x, n_in=torch.tensor([900, 301]))
    assert tuple(y.shape) == (2, 300) and n.tolist() == [300, 101] and (y[1, 101:] == 0).all()
    y64 = ro.resample(x[1, :301].cpu().numpy(), rs.table.cpu().numpy(), rs.M, rs.Hh)
    assert np.abs(y[1, :101].cpu().numpy() - y64).max() < 1e-5
    with pytest.raises(hip.A2SError):
        rs(x.cpu())
    empty, n = rs(x[:, :0])
    assert tuple(empty.shape) == (2, 0) and n.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------- 6. refusals and counters
def test_refusals_and_counters(dev):
    import ctypes as C
    from piano_a2s_amd import hip
    L = hip.lib()
    st = hip.stream()
    x = torch.zeros((2, 64), dtype=torch.float32, device=dev)
    y = torch.zeros((2, 40), dtype=torch.float32, device=dev)
    n_in = torch.tensor([32, 5], dtype=torch.int32, device=dev)
    table = torch.from_numpy(_int_table(3, 9)).to(dev)
    # a2s_resample_rows(stream, x, x_bstride, n_in, n_in_max, C, table, L, M, K, Hh, y, y_bstride, n_out_max, B)
    ok = (hip._p(x), 64, hip._p(n_in), 32, 2, hip._p(table), 3, 7, 9, 4, hip._p(y), 40, 14, 2)
    torch.cuda.synchronize()
    n0, k0 = hip.resample_launches(), L.a2s_launch_count()
    bad = [(0, None), (2, None), (5, None), (10, None), (13, -1), (13, 65536), (4, 0), (4, 9), (6, 0), (6, 4097), (7, 0), (7, 4097), (8, 0), (8, 8193),
           (9, -1), (9, 9), (1, 63), (11, 13), (3, -1), (12, 0), (10, hip._p(x)), (7, 4000)]
    for i, v in bad:
        args = list(ok)
        args[i] = v
        assert L.a2s_resample_rows(st, *args) == -1, (i, v)                  # A2S_ERR_ARG
        assert b"resample_rows" in L.a2s_last_error()
    args = list(ok)
    args[13] = 0
    assert L.a2s_resample_rows(st, *args) == 0                              # no clips: fine, and nothing to launch
    assert hip.resample_launches() == n0 and L.a2s_launch_count() == k0, "nothing was launched"
    assert L.a2s_resample_rows(st, *ok) == 0
    torch.cuda.synchronize()
    assert hip.resample_launches() == n0 + 1 and L.a2s_launch_count() == k0 + 1, "one launch per call"
    assert hip.resample_tile_samples() >= 64
    for kw in (dict(channels=9), dict(M=0), dict(Hh=9)):
        with pytest.raises(hip.A2SError):
            hip.resample_rows(x, n_in, table, **{**dict(M=7, Hh=4, channels=2), **kw})
    with pytest.raises(hip.A2SError):
        hip.resample_rows(x, n_in.long(), table, 7, 4, channels=2)
    with pytest.raises(hip.A2SError):
        hip.resample_rows(x, n_in, table, 7, 4, channels=2, y=x)
    assert hip.resample_launches() == n0 + 1
