"""The tempo augmentation's definition on the host (csrc/a2s_tempo.hip computes the same): integer positions and weights in Q16,
the weighted sum in float64; and the plan rule restated in np.float32."""
import numpy as np

ONE = 65536
MIN_STEP, MAX_STEP = 52429, 87381          # rint(65536 / 1.25), rint(65536 / 0.75)


def taps(step, t):
    """Output row t at the Q16 source advance `step`: -> ([k ...], [w_k ...], W), every integer k with w_k = h - |k * 65536 - t * step| > 0 (in range
    of the clip or not), h = max(65536, step), W their sum.  Found by a search wider than the support, not by the kernel's closed form."""
    pos, h = int(t) * int(step), max(ONE, int(step))
    centre = pos // ONE
    ks, ws = [], []
    for k in range(centre - 4, centre + 6):
        w = h - abs(k * ONE - pos)
        if w > 0:
            ks.append(k)
            ws.append(w)
    return ks, ws, sum(ws)


def stretch(x, step):
    """x (rows, F) -> y (rows, F) float64: y[t] = sum_k (w_k / W) x[k], x = 0 outside [0, rows); zeros for a step outside [MIN_STEP, MAX_STEP]."""
    x = np.asarray(x, dtype=np.float64)
    rows = x.shape[0]
    y = np.zeros_like(x)
    if not MIN_STEP <= step <= MAX_STEP:
        return y
    for t in range(rows):
        ks, ws, W = taps(step, t)
        for k, w in zip(ks, ws):
            if 0 <= k < rows:
                y[t] += (w / W) * x[k]
    return y


def content_rows(x):
    """1 + the last row of x (rows, F) that holds a value != 0 (a NaN is content, -0.0 is not); 0 for an all-zero clip."""
    hit = np.nonzero((np.asarray(x) != 0).any(axis=1))[0]
    return int(hit[-1]) + 1 if hit.size else 0


def interval(n, rows, R, min_frames):
    """(lo, hi) as the kernel forms them in fp32, or None when the clip is kept as it is (n == 0 or lo > hi)."""
    f = np.float32
    if n == 0:
        return None
    lo = max(f(1) - f(R), f(min_frames) / f(n))
    hi = min(f(1) + f(R), f(rows) / f(n))
    return None if lo > hi else (f(lo), f(hi))


def plan(n, rows, u, R, min_frames):
    """(step, kept) of a clip with n content rows under the draw u, the kernel's rule in np.float32.  The one step that numpy has no fp32 form of is
    the fused multiply-add: u * (hi - lo) is exact in float64 and the sum is rounded twice (to 53, then to 24 bits), which can differ from the fused
    result by one fp32 ulp of c -- 0.004 of a step at most, inside the band around half-integers that `quotient` lets a test leave out."""
    f = np.float32
    iv = interval(n, rows, R, min_frames)
    if iv is None:
        return ONE, True
    lo, hi = iv
    c = f(np.float64(f(u)) * np.float64(f(hi - lo)) + np.float64(lo))
    q = np.rint(f(ONE) / c)
    return int(min(max(q, MIN_STEP), MAX_STEP)), False


def quotient(n, rows, u, R, min_frames):
    """65536 / c in float64 from the exact ratios (None for a kept clip): how far the planned step is from a rounding boundary."""
    if n == 0:
        return None
    lo, hi = max(1.0 - float(np.float32(R)), min_frames / n), min(1.0 + float(np.float32(R)), rows / n)
    if lo > hi:
        return None
    return ONE / (lo + float(np.float32(u)) * (hi - lo))
