"""Float64 statement of the rational polyphase resampler (a2s_resample_rows), plain numpy.

    y[n] = sum_{i = 0 .. K-1} table[p][i] * mono[m0 + Hh - i]      n in [0, n_out)
      q = n * M,  p = q mod L,  m0 = q div L
      mono[m] = (sum_{c ascending} x[m][c]) * (1.0f / C)  for m in [0, n_in),  0 elsewhere
      n_out = ceil(n_in * L / M)

The mono mix is the product's own fp32 arithmetic (an input of the definition, not part of the chain under test); the sum over the taps is float64.
`bound` is the standard a-priori bound of a K-term fp32 chain for the same outputs."""
import numpy as np


def n_out(n_in, L, M):
    return -(-int(n_in) * int(L) // int(M))


def mono_mix(x):
    """x (frames, C) or (frames,) float32 -> (frames,) float32: ascending fp32 sum of the channels, times float32(1) / float32(C)."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim == 1:
        x = x[:, None]
    s = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        s = (s + x[:, c]).astype(np.float32)
    return (s * (np.float32(1.0) / np.float32(x.shape[1]))).astype(np.float32)


def resample(x, table, M, Hh, start=0, stop=None, with_bound=False):
    """Outputs [start, stop) of the clip x (frames, C) or (frames,): float64 (and the fp32-chain bound K 2^-24 sum_i |table[p][i]| |mono[...]|)."""
    table = np.asarray(table)
    L, K = table.shape
    mono = mono_mix(x).astype(np.float64)
    n_in = len(mono)
    stop = n_out(n_in, L, M) if stop is None else int(stop)
    n = np.arange(int(start), stop, dtype=np.int64)
    q = n * int(M)
    p, m0 = q % L, q // L
    idx = m0[:, None] + int(Hh) - np.arange(K, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < n_in)
    xs = np.where(ok, mono[np.clip(idx, 0, max(n_in - 1, 0))] if n_in else 0.0, 0.0)
    t = table.astype(np.float64)[p]
    y = (t * xs).sum(axis=1)
    if with_bound:
        return y, K * 2.0 ** -24 * (np.abs(t) * np.abs(xs)).sum(axis=1)
    return y


def resample_blocks(x, table, M, Hh, block=4096):
    """All outputs of a clip, `block` at a time (the gather above holds block * K float64)."""
    L = np.asarray(table).shape[0]
    total = n_out(len(np.asarray(x)), L, M)
    parts = [resample(x, table, M, Hh, s, min(s + block, total), with_bound=True) for s in range(0, total, block)]
    if not parts:
        return np.zeros(0), np.zeros(0)
    return np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])
