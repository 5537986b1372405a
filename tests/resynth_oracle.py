"""Float64 definition of the segment agreement (the device kernel is csrc/a2s_agree.hip) and the a-priori bound of any
evaluation that keeps fp32 partial sums over at most k cells and adds everything above them in double.

    sums[s] = [sum x, sum y, sum x^2, sum y^2, sum x y] over x[clip][f0:f1][:], the same cells of y;
    a clip outside [0, B) gives zeros, f0 and f1 are clamped to [0, T], an empty range gives zeros.

Bound (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2, as tests/beat_oracle.py uses it): a partial over k cells rounds each product
once and its sum at most k - 1 times whatever the order, so it is off by at most gamma(k) * sum |terms|; the partials of a segment cover disjoint cells,
so the whole sum is off by at most gamma(k) * sum |terms| over the segment, plus the double additions above them: gamma_64(n) * sum |terms| at the
most, which the bound carries twice -- once for the evaluation under test, once for this file's own float64 sums (numpy's pairwise np.sum).  On
inputs that are multiples of 1/8 in [0, 1] every term is a multiple of 1/64 and every sum below 2^24 / 64 per partial: all of it is exact."""
import math

import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53


def gamma(k, u=U):
    """The error factor of k roundings in a row: k u / (1 - k u)."""
    return k * u / (1.0 - k * u)


def _range(row, B, T):
    clip, f0, f1 = int(row[0]), int(row[1]), int(row[2])
    f0, f1 = min(max(f0, 0), T), min(max(f1, 0), T)
    if clip < 0 or clip >= B or f1 <= f0:
        return None
    return clip, f0, f1


def five_sums(x, y, seg, with_bound=False, k=None):
    """x, y (B, T, F), seg (S, 3 or 4) -> sums (S, 5) float64 [, bound (S, 5): what an evaluation with fp32 partials over at most k cells may differ
    by]."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    B, T, F = x.shape
    seg = np.asarray(seg).reshape(len(seg), -1) if len(seg) else np.zeros((0, 3), dtype=np.int64)
    sums, bound = np.zeros((len(seg), 5)), np.zeros((len(seg), 5))
    for s, row in enumerate(seg):
        r = _range(row, B, T)
        if r is None:
            continue
        a, b = x[r[0], r[1]:r[2]].reshape(-1), y[r[0], r[1]:r[2]].reshape(-1)
        terms = (a, b, a * a, b * b, a * b)
        sums[s] = [float(np.sum(t, dtype=np.float64)) for t in terms]          # (pairwise in float64: far inside the double term of the bound)
        if with_bound:
            bound[s] = [(gamma(k) + 2.0 * gamma(len(a), U64)) * float(np.sum(np.abs(t), dtype=np.float64)) for t in terms]
    return (sums, bound) if with_bound else sums


def n_cells(seg, B, T, F):
    """Cells per segment of the table (0 where the segment reads nothing)."""
    out = []
    for row in np.asarray(seg):
        r = _range(row, B, T)
        out.append(0 if r is None else (r[2] - r[1]) * F)
    return out


def correlation(sums, n):
    """Pearson correlation from the five sums over n cells in float64, unclipped; None where n is 0 or a variance is not positive."""
    sx, sy, sxx, syy, sxy = (float(v) for v in sums)
    vx, vy = n * sxx - sx * sx, n * syy - sy * sy
    if n <= 0 or not vx > 0.0 or not vy > 0.0:
        return None
    return (n * sxy - sx * sy) / math.sqrt(vx * vy)


def correlation_bound(sums, bound, n):
    """How far the correlation formed from sums that are each within `bound` of `sums` may lie from correlation(sums, n): the bound propagated through
    numerator and denominator, plus 1e-12 for the float64 arithmetic of the formula itself.  inf where a variance may vanish within the bounds."""
    sx, sy, sxx, syy, sxy = (float(v) for v in sums)
    dx, dy, dxx, dyy, dxy = (float(v) for v in bound)
    num = n * sxy - sx * sy
    d_num = n * dxy + abs(sx) * dy + abs(sy) * dx + dx * dy
    vx, vy = n * sxx - sx * sx, n * syy - sy * sy
    d_vx, d_vy = n * dxx + 2.0 * abs(sx) * dx + dx * dx, n * dyy + 2.0 * abs(sy) * dy + dy * dy
    if vx - d_vx <= 0.0 or vy - d_vy <= 0.0:
        return math.inf
    lo, hi = math.sqrt((vx - d_vx) * (vy - d_vy)), math.sqrt((vx + d_vx) * (vy + d_vy))
    return d_num / lo + abs(num) * (1.0 / lo - 1.0 / hi) + 1e-12
