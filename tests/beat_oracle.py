"""The three device stages of the beat tracker (csrc/a2s_beat.hip) on the CPU: onset strength and tempogram in float64, the
definitions the kernels are measured against, with the a-priori fp32 error bounds of the kernels' sums; and the beat dynamic programme restated in numpy
float32, operation for operation (one subtraction, one addition per value), which the kernel must equal bit for bit.  `stages()` packs them as the
beats.Stages that beats.track takes."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32


def gamma(k):
    """The error factor of k fp32 roundings in a row: k u / (1 - k u)."""
    return k * U / (1.0 - k * U)


def onset_strength(x, n_rows, lag, f_split, with_bound=False):
    """x (B, rows, F), n_rows (B,) -> (env_full, env_low) float64 (B, rows): sum_f max(0, x[t][f] - x[t - lag][f]) for lag <= t < n_rows[b], 0 elsewhere;
    env_low over f < f_split.  with_bound: also the bounds (B, rows) on what any fp32 evaluation may differ by, whatever its order of summation: the
    subtraction rounds once and a sum of F terms at most F - 1 times, so the error is at most gamma(F + 1) * sum |terms| (Higham, Accuracy and Stability
    of Numerical Algorithms, section 4.2)."""
    x = np.asarray(x, dtype=np.float64)
    B, rows, F = x.shape
    full, low = np.zeros((B, rows)), np.zeros((B, rows))
    for b in range(B):
        n = min(max(int(n_rows[b]), 0), rows)
        if n > lag:
            d = np.maximum(x[b, lag:n] - x[b, :n - lag], 0.0)
            full[b, lag:n] = d.sum(axis=1)
            low[b, lag:n] = d[:, :f_split].sum(axis=1)
    if with_bound:
        return full, low, gamma(F + 1) * full, gamma(F + 1) * low          # (the terms are >= 0: sum |terms| is the sum)
    return full, low


def tempogram(env, n, win, hop_b, lag_min, lag_max, J, with_bound=False):
    """env (R, stride), n (R,) -> (R, J, lag_max - lag_min + 1) float64: block j holds the frames g = j hop_b - win // 2 + u, u in [0, win);
    d[u] = env[g] - mean over the window's frames inside [0, n) for g inside, 0 outside; A[l] = sum_{u < win - l} d[u] d[u + l] / sum d^2, 0 where the
    denominator is 0.
    with_bound: also the bound on what an fp32 evaluation (fp32 mean, fp32 d, fp32 dot products in any order, one division) may differ by:
      the mean of cnt <= win values: |dm| <= gamma(win + 1) * mean|env|;   d: |dd[u]| <= u |d[u]| + |dm| (inside), 0 (outside);
      a dot product of win terms: gamma(win) sum |d d'| + sum (|d| dd' + |d'| dd + dd dd');
      the quotient: (eN + |N| / D * eD) / (D - eD) + u |N / D| (+ a vanishing denominator: no bound, the caller skips such blocks)."""
    env = np.asarray(env, dtype=np.float64)
    R, stride = env.shape
    nl = lag_max - lag_min + 1
    out, bound = np.zeros((R, J, nl)), np.zeros((R, J, nl))
    for r in range(R):
        nn = min(max(int(n[r]), 0), stride)
        for j in range(J):
            g = j * hop_b - win // 2 + np.arange(win)
            inside = (g >= 0) & (g < nn)
            if not inside.any():
                continue
            v = env[r, g[inside]]
            d, dd = np.zeros(win), np.zeros(win)
            d[inside] = v - v.mean()
            dd[inside] = U * np.abs(d[inside]) + gamma(win + 1) * np.abs(v).mean()
            ad = np.abs(d)
            D = float((d * d).sum())
            eD = gamma(win) * D + float((2.0 * ad * dd + dd * dd).sum())
            if D <= 0.0:
                continue
            for l in range(lag_min, lag_max + 1):
                if l >= win:
                    continue
                a, b = slice(0, win - l), slice(l, win)
                N = float((d[a] * d[b]).sum())
                out[r, j, l - lag_min] = N / D
                eN = gamma(win) * float((ad[a] * ad[b]).sum()) + float((ad[a] * dd[b] + ad[b] * dd[a] + dd[a] * dd[b]).sum())
                bound[r, j, l - lag_min] = (eN + abs(N) / D * eD) / (D - eD) + U * abs(N / D) if D > eD else np.inf
    return (out, bound) if with_bound else out


def beat_dp(ls, period, pen, n, hop_b, lag_min, max_beats, sentinel=None):
    """The dynamic programme of a2s_beat_dp in numpy float32.  ls (R, stride) float32, period (R, J) int32, pen float32 (lag_max - lag_min + 1,
    2 lag_max + 1), n (R,) -> (S (R, stride) float32, back (R, stride) int32, beats (R, max_beats) int32, count (R,) int32).  What the kernel does not
    write keeps `sentinel` = (S, back, beats) fill values (default 0, 0, -1)."""
    ls = np.asarray(ls, dtype=np.float32)
    pen = np.asarray(pen, dtype=np.float32)
    period = np.asarray(period)
    R, stride = ls.shape
    J = period.shape[1]
    lag_max = (pen.shape[1] - 1) // 2
    fS, fB, fT = (0.0, 0, -1) if sentinel is None else sentinel
    S = np.full((R, stride), fS, dtype=np.float32)
    back = np.full((R, stride), fB, dtype=np.int32)
    beats = np.full((R, max_beats), fT, dtype=np.int32)
    count = np.zeros((R,), dtype=np.int32)
    tau_of = lambda r, t: int(min(max(int(period[r, min(t // hop_b, J - 1)]), lag_min), lag_max))
    for r in range(R):
        nn = min(max(int(n[r]), 0), stride)
        for t in range(nn):
            tau = tau_of(r, t)
            lo, hi = max(0, t - 2 * tau), t - (tau + 1) // 2
            best, bp = np.float32(0.0), -1
            if hi >= lo:
                p = np.arange(lo, hi + 1)
                c = S[r, p] - pen[tau - lag_min, t - p]                       # float32 - float32: one rounding
                m = c.max()
                if m > 0:
                    best, bp = m, int(p[np.nonzero(c == m)[0][-1]])            # the nearest to t among equals
            S[r, t] = np.float32(ls[r, t] + np.float32(best))
            back[r, t] = bp
        if nn == 0:
            continue
        a = max(0, nn - tau_of(r, nn - 1))
        t = a + int(np.argmax(S[r, a:nn]))                                     # the first of equals
        chain = []
        while t >= 0:
            chain.append(t)
            t = int(back[r, t])
        chain.reverse()
        count[r] = len(chain)
        k = min(len(chain), max_beats)
        beats[r, :k] = chain[:k]
    return S, back, beats, count


def stages():
    """The definitions as the beats.Stages that beats.track and beats.track_recording take (numpy in, numpy out)."""
    from piano_a2s_amd import beats

    def onset(x, n_rows, lag, f_split):
        x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
        if x.ndim == 4:
            x = x[:, 0]
        full, low = onset_strength(x, n_rows, lag, f_split)
        return full.astype(np.float32), low.astype(np.float32)

    return beats.Stages(onset, tempogram, beat_dp)
