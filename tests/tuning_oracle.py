"""Definition of the tuning estimate (the device kernels are csrc/a2s_tuning.hip), in float64 and exact integers: what the
kernels must reproduce integer for integer (profile) and bit for bit (estimate).

Constants: S bins per semitone, H = 100 cells per semitone (one cent each), Q = 4096, the smoothing window 7 - |j|, j = -6 .. 6 (sum 49).

profile, per clip b over the frames t < clamp(n_rows[b], 0, rows) and the bins 1 <= f <= F - 2, with a = x[t][f - 1], c = x[t][f], e = x[t][f + 1]:
    a peak iff c > a and c >= e and c >= thr (a comparison with NaN is false: a plateau, silence and NaN give no peak).  For a peak, in double:
        delta  = 0.5 (a - e) / ((a - c) + (e - c));          a NaN (only cells at +-inf give one) is read as 0
        u      = ((f mod S) + delta) + S / 2, and u -= S where u >= S
        cell   = min(H - 1, floor(u * H / S))
        weight = 1 + rint(min(c - thr, 1) * Q)              (ties to even)
    hist[b][cell] += weight, hist[b][H] += 1 (the peak count), int64.  Cell k stands for a deviation of [k - 50, k - 49) cents.
estimate, per group g of the clips first[g] .. first[g + 1] - 1:
    h = the group's histograms added; sm[k] = sum_j (7 - |j|) h[(k + j) mod H]; k* = the first arg max of sm;
    conf = sm[k*] * H / sum(sm) (0 where the sum is 0);  with A, C, E = sm[k* - 1], sm[k*], sm[k* + 1] (circular) and den = (A - C) + (E - C):
    delta = 0.5 (A - E) / den where den < 0, else 0;  cents = ((k* + 0.5) + delta) * 100 / H - 50, and cents -= 100 where it reaches 50;
    determined = peaks >= min_peaks and conf >= min_conf;  est[g] = [cents, conf, peaks];  eff_bins[b] = float32(-cents * S / 100) for the clips
    of a determined group, else 0.  An empty group (and any group of zeros): sm = 0, k* = 0, est = [-49.5, 0, 0], not determined.

`profile_loops` is the same statement as a plain triple loop (tests/test_tuning_cpu.py holds the two against each other)."""
import math

import numpy as np

H = 100
Q = 4096
HALF_WINDOW = 6


def _clamp_rows(n, rows):
    return max(0, min(int(n), rows))


def profile(x, n_rows, thr=0.5, bins_per_semitone=5):
    """x (B, rows, F) float32, n_rows (B,) -> hist (B, H + 1) int64."""
    x = np.asarray(x, dtype=np.float32)
    B, rows, F = x.shape
    S = int(bins_per_semitone)
    thr64 = float(np.float32(thr))
    hist = np.zeros((B, H + 1), dtype=np.int64)
    for b in range(B):
        n = _clamp_rows(n_rows[b], rows)
        if F < 3 or n == 0:
            continue
        xs = x[b, :n].astype(np.float64)
        a, c, e = xs[:, :-2], xs[:, 1:-1], xs[:, 2:]
        with np.errstate(invalid="ignore"):
            peak = (c > a) & (c >= e) & (c >= thr64)
        t, j = np.nonzero(peak)
        a, c, e, f = a[t, j], c[t, j], e[t, j], j + 1
        with np.errstate(invalid="ignore", divide="ignore"):
            delta = 0.5 * (a - e) / ((a - c) + (e - c))
        delta = np.where(np.isnan(delta), 0.0, delta)
        u = ((f % S).astype(np.float64) + delta) + S / 2.0
        u = np.where(u >= S, u - S, u)
        cell = np.minimum(H - 1, np.floor(u * H / S)).astype(np.int64)
        weight = 1 + np.rint(np.minimum(c - thr64, 1.0) * Q).astype(np.int64)
        np.add.at(hist[b], cell, weight)
        hist[b, H] = len(f)
    return hist


def profile_loops(x, n_rows, thr=0.5, bins_per_semitone=5):
    """The same, cell by cell in Python floats (IEEE double) and ints."""
    x = np.asarray(x, dtype=np.float32)
    B, rows, F = x.shape
    S = int(bins_per_semitone)
    thr64 = float(np.float32(thr))
    hist = [[0] * (H + 1) for _ in range(B)]
    for b in range(B):
        for t in range(_clamp_rows(n_rows[b], rows)):
            for f in range(1, F - 1):
                a, c, e = float(x[b, t, f - 1]), float(x[b, t, f]), float(x[b, t, f + 1])
                if not (c > a and c >= e and c >= thr64):
                    continue
                with np.errstate(all="ignore"):                       # (numpy scalars: IEEE results where cells are infinite, no exception)
                    delta = float(np.float64(0.5 * (a - e)) / np.float64((a - c) + (e - c)))
                if math.isnan(delta):
                    delta = 0.0
                u = ((f % S) + delta) + S / 2.0
                if u >= S:
                    u -= S
                cell = min(H - 1, math.floor(u * H / S))
                w = min(c - thr64, 1.0) * Q
                r = math.floor(w)
                if w - r > 0.5 or (w - r == 0.5 and r % 2 == 1):      # rint, ties to even
                    r += 1
                hist[b][cell] += 1 + r
                hist[b][H] += 1
    return np.array(hist, dtype=np.int64).reshape(B, H + 1)


def estimate(hist, first, min_conf, min_peaks, bins_per_semitone=5):
    """hist (B, H + 1) whole numbers, first (G + 1,) ascending from 0 to B -> (est (G, 3) float64, eff_bins (B,) float32, determined (G,) bool).
    Python ints (exact at any size) and Python floats (IEEE double)."""
    rows = [[int(v) for v in r] for r in np.asarray(hist).reshape(-1, H + 1)]
    B, S = len(rows), int(bins_per_semitone)
    first = [int(v) for v in first]
    assert first[0] == 0 and first[-1] == B and all(p <= q for p, q in zip(first, first[1:])), first
    G = len(first) - 1
    est, eff, det = np.zeros((G, 3), dtype=np.float64), np.zeros(B, dtype=np.float32), np.zeros(G, dtype=bool)
    for g in range(G):
        h = [sum(rows[b][k] for b in range(first[g], first[g + 1])) for k in range(H + 1)]
        sm = [sum((HALF_WINDOW + 1 - abs(j)) * h[(k + j) % H] for j in range(-HALF_WINDOW, HALF_WINDOW + 1)) for k in range(H)]
        k = max(range(H), key=lambda i: (sm[i], -i))                  # the first arg max
        total = sum(sm)
        conf = float(sm[k]) * float(H) / float(total) if total != 0 else 0.0
        A, C, E = sm[(k - 1) % H], sm[k], sm[(k + 1) % H]
        den = (A - C) + (E - C)
        delta = 0.5 * float(A - E) / float(den) if den < 0 else 0.0
        cents = ((k + 0.5) + delta) * 100.0 / float(H) - 50.0
        if cents >= 50.0:
            cents -= 100.0
        peaks = h[H]
        det[g] = peaks >= min_peaks and conf >= min_conf
        est[g] = (cents, conf, float(peaks))
        if det[g]:
            eff[first[g]:first[g + 1]] = np.float32(-cents * float(S) / 100.0)
    return est, eff, det


def feature_cases(rng, B=3, T=7, F=24):
    """Feature-like inputs: a grid of 1/8, uniform random, rows of one constant, cells of NaN, +-inf and values above 1."""
    grid = rng.integers(0, 9, (B, T, F)).astype(np.float32) / 8
    uni = rng.random((B, T, F)).astype(np.float32)
    flat = np.repeat(rng.random((B, T, 1)).astype(np.float32), F, axis=2)
    wild = rng.random((B, T, F)).astype(np.float32) * 1.5
    idx = rng.integers(0, B * T * F, 40)
    wild.reshape(-1)[idx] = np.resize(np.array([np.nan, np.inf, -np.inf, 3.0, 1.0], dtype=np.float32), 40)
    return {"grid": grid, "uniform": uni, "constant rows": flat, "wild": wild}


# ---- the float64 chain on rendered clips (tests/test_tuning_cpu.py, tools/tuning_check.py)
def rendered_features(program, n_samples):
    """A render program -> (T, F) float64 features: the float64 synthesiser and the float64 front end."""
    from oracle import vqt_ref
    from tests import render_oracle
    return vqt_ref.vqt_features_librosa(render_oracle.render(program, n_samples))


def clip_program(seed, frames, instrument):
    """The render program of scoregen.make_clip(seed) on resynth's fixed instrument ("resynth") or on the clip's own drawn one ("own")."""
    from piano_a2s_amd import resynth, scoregen, spec
    clip = scoregen.make_clip(spec.default_cfg(max_length=(200, 200)), seed, frames=frames)
    n_samples = (frames - 1) * scoregen.HOP
    if instrument == "resynth":
        return resynth.program(clip["events"], n_samples), n_samples
    return scoregen.pack_program(dict(clip, n_samples=n_samples)), n_samples


def chain(seed, cents, frames=301, instrument="resynth", thr=0.5, min_conf=0.0, min_peaks=H, features=False):
    """Render clip `seed` detuned by `cents`, make its features, profile and estimate as one group -> [estimated cents, confidence, peaks]
    (and the features, on request)."""
    from piano_a2s_amd import scoregen
    program, n_samples = clip_program(seed, frames, instrument)
    x = rendered_features(scoregen.detune_program(program, cents), n_samples)
    hist = profile(x[None].astype(np.float32), [x.shape[0]], thr)
    est = estimate(hist, [0, 1], min_conf, min_peaks)[0][0]
    return (est, x) if features else est


def cents_error(got, true):
    """The difference of two tunings on the circle of 100 cents, in [-50, 50)."""
    return (float(got) - float(true) + 50.0) % 100.0 - 50.0


def noise_tensors(n=4, rows=301, F=480, seed=27):
    """Feature-like tensors without a tuning: uniform in [0, 1), and a Gaussian around 0.5 (sigma 0.2) clipped to [0, 1]; n of each."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        out.append(rng.random((rows, F)).astype(np.float32))
        out.append(np.clip(0.5 + 0.2 * rng.standard_normal((rows, F)), 0.0, 1.0).astype(np.float32))
    return out


def shift_bins64(x, n):
    """a2s_shift_bins in float64: y[t][j] = (1 - a) x[t][j - m] + a x[t][j - m - 1], m = floor(n), a = n - m, x taken as 0 outside [0, F)."""
    x = np.asarray(x, dtype=np.float64)
    T, F = x.shape
    m = math.floor(n)
    a = n - m
    pad = np.zeros((T, F + 2 * (abs(m) + 2)))
    o = abs(m) + 2
    pad[:, o:o + F] = x
    j = np.arange(F) + o
    return (1.0 - a) * pad[:, j - m] + a * pad[:, j - m - 1]


def correlation(x, y):
    x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
    return float(np.corrcoef(x, y)[0, 1])
