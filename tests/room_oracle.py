"""Float64 numpy restatement of the room acoustics (the device kernels are csrc/a2s_room.hip, the host part piano_a2s_amd/room.py).

Per clip one 32-bit room_seed (in the recipe: noise_seed ^ 0x524F4F4D).  With hash32 and 0x9E3779B9 as in tests/render_oracle.py:

    v(j)   = (hash32(room_seed + j * 0x9E3779B9) >> 8) * 2^-24                 in [0, 1)
    rt60   = lerp(rt60_range, v(0)),  drr_db = lerp(drr_range, v(1)),  pre = rint(lerp(predelay_ms_range, v(2)) * sr / 1000)   (pre >= 1)
    decay  = ln(1000) / (rt60 * sr),  L = min(L_max, pre + ceil(rt60 * sr)),  wet = 10^(-drr_db / 20) * sqrt(3 * (1 - exp(-2 * decay)))
    table  = [pre, L, float32(wet), float32(decay)]
    h[0]   = 1;  h[k] = 0 for 0 < k < pre;  h[k] = wet * u(k) * exp(-(k - pre) * decay) for pre <= k < L     (from the float32 table values)
    u(k)   = (hash32(room_seed + (k + 3) * 0x9E3779B9) >> 8) * 2^-23 - 1
    y[n]   = sum_{k = 0 .. min(L - 1, n)} h[k] * x[n - k]

Everything but the hash is evaluated in float64."""
import math

import numpy as np

from tests.render_oracle import hash32

GOLDEN = 0x9E3779B9
DEFAULTS = dict(rt60=(0.2, 0.6), drr_db=(0.0, 12.0), predelay_ms=(5.0, 25.0))


def unit(seed, j):
    """v(j) in [0, 1)."""
    h = hash32(np.array([(int(seed) + j * GOLDEN) & 0xFFFFFFFF], dtype=np.uint64))[0]
    return float(int(h) >> 8) * 2.0 ** -24


def default_L_max(rt60=DEFAULTS["rt60"], predelay_ms=DEFAULTS["predelay_ms"], sr=16000):
    full = int(round(predelay_ms[1] * sr / 1000.0)) + math.ceil(rt60[1] * sr)
    return (full + 3) // 4 * 4


def params(seed, rt60=DEFAULTS["rt60"], drr_db=DEFAULTS["drr_db"], predelay_ms=DEFAULTS["predelay_ms"], sr=16000, L_max=None):
    """One clip's room: a dict with the float64 draws and the table row [pre, L, wet f32, decay f32] (wet and decay as float32 VALUES)."""
    L_max = default_L_max(rt60, predelay_ms, sr) if L_max is None else L_max
    lerp = lambda r, t: r[0] + (r[1] - r[0]) * t
    t60, drr = lerp(rt60, unit(seed, 0)), lerp(drr_db, unit(seed, 1))
    pre = int(np.rint(lerp(predelay_ms, unit(seed, 2)) * sr / 1000.0))
    decay = math.log(1000.0) / (t60 * sr)
    L = min(L_max, pre + math.ceil(t60 * sr))
    wet = 10.0 ** (-drr / 20.0) * math.sqrt(3.0 * (1.0 - math.exp(-2.0 * decay)))
    return dict(rt60=t60, drr_db=drr, pre=pre, L=L, wet64=wet, decay64=decay, wet=float(np.float32(wet)), decay=float(np.float32(decay)))


def table_row(p):
    """The int32 row [pre, L, wet f32 bits, decay f32 bits] of params()'s result."""
    f = np.array([p["wet"], p["decay"]], dtype=np.float32).view(np.int32)
    return np.array([p["pre"], p["L"], f[0], f[1]], dtype=np.int32)


def impulse_response(seed, pre, L, wet, decay, L_max=None):
    """h[0 .. L_max) in float64 (zeros behind L), from the float32 table values wet and decay."""
    L_max = L if L_max is None else L_max
    L = min(max(L, 1), L_max)
    h = np.zeros(L_max, dtype=np.float64)
    h[0] = 1.0
    if L > pre:
        k = np.arange(pre, L, dtype=np.uint64)
        hs = hash32(np.uint64(int(seed) & 0xFFFFFFFF) + (k + np.uint64(3)) * np.uint64(GOLDEN))
        u = (hs >> np.uint64(8)).astype(np.float64) * 2.0 ** -23 - 1.0
        h[pre:L] = float(wet) * u * np.exp(-(k.astype(np.float64) - pre) * float(decay))
        h[0] = 1.0                                                     # (pre >= 1 in every table; a row that says 0 still keeps the direct path)
    return h


def fir(x, h, L=None):
    """y[n] = sum_{k = 0 .. min(L - 1, n)} h[k] x[n - k] in float64, n in [0, len(x)); written as the definition's double loop over k."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    L = len(h) if L is None else L
    y = np.zeros(len(x), dtype=np.float64)
    for k in range(min(L, len(x))):
        if h[k] != 0.0:
            y[k:] += h[k] * x[:len(x) - k]
    return y


def apply(x, seed, L_max=None, **ranges):
    """A clip's waveform through its room: (y float64, the params dict)."""
    p = params(seed, L_max=L_max, **ranges)
    h = impulse_response(seed, p["pre"], p["L"], p["wet"], p["decay"])
    return fir(x, h), p
