"""The spectrogram augmentation's definition on the host (csrc/a2s_specaug.hip computes the same): powers, peak and logarithms
in float64; the content rule, the floor compare and the mask plan in the float32 and integer forms the definition gives them."""
import numpy as np

MAX_MASKS = 4
FLOOR_EPS = np.float32(2.0 ** -18)


def content_rows(x):
    """1 + the last row of x (rows, F) that holds a value != 0 (a NaN is content, -0.0 is not); 0 for an all-zero clip."""
    hit = np.nonzero((np.asarray(x) != 0).any(axis=1))[0]
    return int(hit[-1]) + 1 if hit.size else 0


def power(x):
    """P(x) = 10^(8 (x - 1)): the power, relative to the clip's peak, of a feature x = dB / 80 + 1."""
    return 10.0 ** (8.0 * (np.asarray(x, dtype=np.float64) - 1.0))


def mask_plan(n, F, draws, Wt, Wf, m):
    """16 ints, 4 x [t0, w] then 4 x [k0, wk], from 16 draws of 32 bits (four per mask) in integer arithmetic (Python ints: no product overflows)."""
    d = [int(v) & 0xFFFFFFFF for v in np.asarray(draws).reshape(-1)]
    assert len(d) == 4 * MAX_MASKS
    wmax_t, wmax_f = min(int(Wt), n // 5), min(int(Wf), F // 5)
    out = [0] * (4 * MAX_MASKS)
    for i in range(min(int(m), MAX_MASKS)):
        w = (d[4 * i] * (wmax_t + 1)) >> 32
        t0 = (d[4 * i + 1] * (n - w + 1)) >> 32
        wk = (d[4 * i + 2] * (wmax_f + 1)) >> 32
        k0 = (d[4 * i + 3] * (F - wk + 1)) >> 32
        out[2 * i], out[2 * i + 1], out[2 * MAX_MASKS + 2 * i], out[2 * MAX_MASKS + 2 * i + 1] = t0, w, k0, wk
    return out


def table(F, e, phi, level_db, tilt, bins_per_octave, eq=True, noise=True):
    """(2, F) float32 from one clip's draws, in float64 and rounded once: e (3,) dB and phi (2,) turns give
    g_k = e0 (2z - 1) + e1 cos 2 pi (z + phi1) + e2 cos 2 pi (2z + phi2), z = k / (F - 1) (0.5 when F = 1), G_k = 10^(g_k / 10);
    v_k = 10^((-level_db + tilt (k - (F - 1) / 2) / bins_per_octave) / 10).  eq False: G = 1; noise False: v = 0."""
    out = np.zeros((2, F), dtype=np.float64)
    for k in range(F):
        z = k / (F - 1) if F > 1 else 0.5
        g = e[0] * (2 * z - 1) + e[1] * np.cos(2 * np.pi * (z + phi[0])) + e[2] * np.cos(2 * np.pi * (2 * z + phi[1]))
        out[0, k] = 10.0 ** (g / 10.0) if eq else 1.0
        out[1, k] = 10.0 ** ((-level_db + tilt * (k - (F - 1) / 2.0) / bins_per_octave) / 10.0) if noise else 0.0
    return out.astype(np.float32)


def apply(x, tab, plan=None):
    """x (rows, F) float32, tab (2, F) float32 [G, v], plan 16 ints or None (no mask) -> dict(out (rows, F) float64, n, x_min (float32), M (float64),
    y (n, F) float64, floor (n, F) bool, masked (rows, F) bool: the cells a mask covers)."""
    x = np.asarray(x, dtype=np.float32)
    rows, F = x.shape
    tab = np.asarray(tab, dtype=np.float32).astype(np.float64)
    n = content_rows(x)
    out = np.zeros((rows, F), dtype=np.float64)
    masked = np.zeros((rows, F), dtype=bool)
    if n == 0:
        return dict(out=out, n=0, x_min=np.float32(0), M=0.0, y=np.zeros((0, F)), floor=np.zeros((0, F), dtype=bool), masked=masked)
    c = x[:n]
    x_min = c.min()
    floor = (c - x_min) <= FLOOR_EPS                       # float32 - float32 -> float32, compared with a float32: as the kernel
    p_min = float(power(x_min))
    q = np.where(floor, 0.0, tab[0][None, :] * power(c))
    y = np.maximum(p_min, q + tab[1][None, :])
    M = float(y.max())
    out[:n] = np.clip(1.0 + np.log10(y / M) / 8.0, 0.0, 1.0)
    if plan is not None:
        for i in range(MAX_MASKS):
            t0, w, k0, wk = plan[2 * i], plan[2 * i + 1], plan[2 * MAX_MASKS + 2 * i], plan[2 * MAX_MASKS + 2 * i + 1]
            masked[t0:t0 + w, :] = True
            masked[:n, k0:k0 + wk] = True
        out[masked] = 0.0
    return dict(out=out, n=n, x_min=x_min, M=M, y=y, floor=floor, masked=masked)


A0_HZ = 27.5


def filter_gain_table(c, F=480, bins_per_octave=60, sr=16000.0):
    """(2, F) float32 for the two-tap filter y[n] = x[n] + c x[n - 1]: its power gains 1 + c^2 + 2 c cos(2 pi f_k / sr) at the bins' centre
    frequencies f_k = 27.5 * 2^(k / bins_per_octave), no noise (the physics checks of the CPU and the GPU tests)."""
    f = A0_HZ * 2.0 ** (np.arange(F) / bins_per_octave)
    return np.stack([1.0 + c * c + 2.0 * c * np.cos(2.0 * np.pi * f / sr), np.zeros(F)]).astype(np.float32)
