"""Definition of the bar-wise dynamic time warping (the device kernels are csrc/a2s_dtw.hip), in float64 and restated in numpy
float32, plus the a-priori bound of the fp32 cost and a brute-force check of the recurrence.

    segment [clip, f0, f1, r]: f0, f1 clamped to [0, T], n = f1 - f0 rows of clip `clip`, the same rows of x and y; a clip outside [0, B) or n <= 0:
        empty.  r: Sakoe-Chiba half-width, cell (i, j) is inside when |i - j| <= r; r < 0 or r >= n: no band.
    cost:  d[i][j] = sum_f ((x[f0 + i][f] - y[f0 + j][f]) - off)^2
    DP:    D[0][0] = d[0][0];  D[i][j] = d[i][j] + min(D[i-1][j-1], D[i-1][j], D[i][j-1]) over the predecessors that exist and lie in the band, the
           first of equals in that order (codes 0, 1, 2).  One addition per cell: in float32 (dp(..., np.float32)) the device's bits.
    path:  back from (n - 1, n - 1) along the codes; reported ascending.

Bound of the cost (Higham, Accuracy and Stability of Numerical Algorithms, sections 3.1 and 4.2; u = 2^-24).  Per term the device forms
e^ = fl(fl(x - y) - off): with a = |x - y| and e the true value, |e^ - e| <= eta = u a + u (|e| + u a).  The product e^ * e^ is exact inside the FMA,
so the term differs from e^2 by at most 2 |e| eta + eta^2, and the F-term chain acc = fl(e^ e^ + acc) is recursive summation with one rounding per
term: off by at most gamma(F) * sum (|e| + eta)^2.  The bound adds 4 gamma_64(F) sum e^2 for this file's own float64 arithmetic.  On inputs that are
multiples of 1/8 in [0, 1] with off = 0 every term is a multiple of 1/64, at most 1, and a sum below 2^24 / 64: all of it is exact."""
import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53


def gamma(k, u=U):
    return k * u / (1.0 - k * u)


def segment(row, B, T):
    """-> (clip, f0, n, r) with r = -1 for no band, or None for an empty segment."""
    clip, f0, f1 = int(row[0]), int(row[1]), int(row[2])
    r = int(row[3]) if len(row) > 3 else -1
    f0, f1 = min(max(f0, 0), T), min(max(f1, 0), T)
    if clip < 0 or clip >= B or f1 <= f0:
        return None
    n = f1 - f0
    return clip, f0, n, (-1 if r < 0 or r >= n else r)


def in_band(i, j, r):
    return r < 0 or abs(i - j) <= r


def band_mask(n, r):
    i = np.arange(n)
    return np.ones((n, n), dtype=bool) if r < 0 else np.abs(i[:, None] - i[None, :]) <= r


def cost(x, y, row, off=0.0, with_bound=False):
    """x, y (B, T, F) -> the (n, n) float64 costs of the segment (every cell, also outside the band) [, the bound of the fp32 evaluation]; None for
    an empty segment."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    B, T, F = x.shape
    sg = segment(row, B, T)
    if sg is None:
        return (None, None) if with_bound else None
    clip, f0, n, _ = sg
    a = x[clip, f0:f0 + n][:, None, :] - y[clip, f0:f0 + n][None, :, :]
    e = a - float(off)
    d = np.sum(e * e, axis=2)
    if not with_bound:
        return d
    eta = U * np.abs(a) + U * (np.abs(e) + U * np.abs(a))
    bound = np.sum(2.0 * np.abs(e) * eta + eta * eta, axis=2) + gamma(F) * np.sum((np.abs(e) + eta) ** 2, axis=2) + 4.0 * gamma(F, U64) * d
    return d, bound


def dp(d, r=-1, dtype=np.float64):
    """d (n, n) -> (D (n, n) of `dtype`, nan outside the band; codes (n, n) int8, -1 outside the band)."""
    n = d.shape[0]
    r = -1 if r < 0 or r >= n else r
    d = np.asarray(d).astype(dtype)
    D = np.full((n, n), np.nan, dtype=dtype)
    codes = np.full((n, n), -1, dtype=np.int8)
    for i in range(n):
        lo, hi = (0, n - 1) if r < 0 else (max(0, i - r), min(n - 1, i + r))
        for j in range(lo, hi + 1):
            best, code = None, 0
            if i > 0 and j > 0:
                best = D[i - 1, j - 1]
            if i > 0 and in_band(i - 1, j, r) and (best is None or D[i - 1, j] < best):
                best, code = D[i - 1, j], 1
            if j > 0 and in_band(i, j - 1, r) and (best is None or D[i, j - 1] < best):
                best, code = D[i, j - 1], 2
            D[i, j] = d[i, j] if best is None else d[i, j] + best          # (numpy scalars of `dtype`: one rounding in that type)
            codes[i, j] = code
    return D, codes


def backtrack(codes):
    """codes of dp -> the path [(i, j)] from (0, 0) to (n - 1, n - 1)."""
    n = codes.shape[0]
    i = j = n - 1
    path = [(i, j)]
    while i > 0 or j > 0:
        c = int(codes[i, j])
        assert c in (0, 1, 2) and (c != 2 or j > 0) and (c != 1 or i > 0) and (c != 0 or (i > 0 and j > 0)), (i, j, c)
        i, j = i - (c != 2), j - (c != 1)
        path.append((i, j))
    return path[::-1]


def align(d, r=-1, dtype=np.float64):
    """-> (path [(i, j)], total of `dtype`)."""
    D, codes = dp(d, r, dtype)
    return backtrack(codes), D[-1, -1]


def pack(path):
    return np.array([(i << 16) | j for i, j in path], dtype=np.int32)


def brute_force(d, r=-1):
    """The smallest total over ALL monotone paths from (0, 0) to (n - 1, n - 1) inside the band, by enumeration (n <= 5), and the paths that reach it."""
    n = d.shape[0]
    r = -1 if r < 0 or r >= n else r
    best, argbest = None, []

    def walk(i, j, total, path):
        nonlocal best, argbest
        if (i, j) == (n - 1, n - 1):
            if best is None or total < best:
                best, argbest = total, [path]
            elif total == best:
                argbest.append(path)
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            a, b = i + di, j + dj
            if a < n and b < n and in_band(a, b, r):
                walk(a, b, total + d[a, b], path + [(a, b)])

    walk(0, 0, d[0, 0], [(0, 0)])
    return best, argbest


def warp_from_path(path, n):
    """-> (warp, inverse): warp[j] = (first i + last i) / 2 over the cells (i, j) of the path, inverse[i] the same over j; plain loops."""
    rows, cols = [[] for _ in range(n)], [[] for _ in range(n)]
    for i, j in path:
        cols[j].append(i)
        rows[i].append(j)
    return (np.array([(min(c) + max(c)) / 2.0 for c in cols]), np.array([(min(c) + max(c)) / 2.0 for c in rows]))


# ---- the block layout of the device buffers (include/a2s.h)
def geometry(table):
    """(n_max, w_max) of the valid host table [clip, f0, f1, r] as piano_a2s_amd.hip.dtw_geometry sizes the buffers."""
    widths, ns = [], []
    for row in table:
        n, r = int(row[2]) - int(row[1]), int(row[3])
        ns.append(n)
        widths.append(2 * r + 1 if 0 <= r and 2 * r + 1 < n else n)
    n_max, need = max(1, max(ns)), max(widths)
    r_max = -1 if need >= n_max else need // 2
    return n_max, r_max, (n_max if r_max < 0 or 2 * r_max + 1 > n_max else 2 * r_max + 1)


def unpack(flat, s, n, r, n_max, w_max, fill=np.nan):
    """Segment s's block of a flat device buffer -> (n, n), `fill` outside the band."""
    r = -1 if r < 0 or r >= n else r
    block = np.asarray(flat)[s * n_max * w_max:(s + 1) * n_max * w_max]
    out = np.full((n, n), fill, dtype=block.dtype)
    W = 2 * r + 1 if r >= 0 and 2 * r + 1 < n else n
    i, j = np.nonzero(band_mask(n, r))
    out[i, j] = block[i * W + (j - i + r)] if W < n else block[i * n + j]
    return out


# ---- rendered clips whose events are warped inside every bar: the true onsets are known (tests/test_gpu_dtw.py, tools/dtw_bench.py)
def bar_warp(u, a):
    """g(u) = u + a sin(pi u) on [0, 1]: fixes both bar lines, monotone for |a| < 1 / pi."""
    return u + a * np.sin(np.pi * u)


def clip_lines(clip, bars):
    """The bar lines of a scoregen.make_clip clip in samples."""
    from fractions import Fraction
    from piano_a2s_amd import scoregen
    bar_q = Fraction(scoregen._BAR_UNITS[clip["time_sig"]], 4)
    return [int(clip["lead"] + b * bar_q * clip["spq"]) for b in range(bars + 1)]


def warped_clip(clip, bars, amp, rng):
    """-> {"lines", "bars": [{"a", "notes" (n, 3) the straight events of the bar, "true" (n, 3) the same notes with onset and end moved by the bar's
    g, a = +-amp with the sign drawn from rng}], "straight", "warped": the clip's events (n, 3) in (onset, midi) order}."""
    from piano_a2s_amd import resynth
    lines = clip_lines(clip, bars)
    out = {"lines": lines, "bars": []}
    for b in range(bars):
        notes = resynth.score_events(clip["ids"]["upper"][b:b + 1], clip["ids"]["lower"][b:b + 1], [clip["time_sig"]], lines[b:b + 2], max_events=1 << 30)[0]
        a = float(amp) * (1.0 if rng.integers(0, 2) else -1.0)
        span = lines[b + 1] - lines[b]
        true = notes.copy()
        if len(notes):
            on = lines[b] + np.rint(span * bar_warp((notes[:, 0] - lines[b]) / span, a)).astype(np.int64)
            end = lines[b] + np.rint(span * bar_warp((notes[:, 0] + notes[:, 1] - lines[b]) / span, a)).astype(np.int64)
            on = np.minimum(on, lines[b + 1] - 1)
            true[:, 0], true[:, 1] = on, np.maximum(1, np.minimum(end, lines[b + 1]) - on)
        out["bars"].append({"a": a, "notes": notes, "true": true})
    for key, which in (("straight", "notes"), ("warped", "true")):
        ev = np.concatenate([bar[which] for bar in out["bars"]]).reshape(-1, 3)
        out[key] = ev[np.lexsort((ev[:, 2], ev[:, 0]))]
    return out


def onset_errors(scenario, warps, hop, performed_notes):
    """The absolute onset errors in samples, per note over all bars: (of linear placement = the straight onsets, of the onsets moved through the bars'
    warps).  warps: per bar (warp, first_frame) or None (the note stays where linear placement puts it)."""
    linear, moved = [], []
    for b, (bar, w) in enumerate(zip(scenario["bars"], warps)):
        if not len(bar["notes"]):
            continue
        got = performed_notes(bar["notes"], None if w is None else w[0], 0 if w is None else w[1], hop, scenario["lines"][b], scenario["lines"][b + 1])
        linear += np.abs(bar["notes"][:, 0] - bar["true"][:, 0]).tolist()
        moved += [abs(g[0] - t) for g, t in zip(got, bar["true"][:, 0])]
    return linear, moved
