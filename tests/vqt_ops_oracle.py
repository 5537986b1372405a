"""Float64 numpy restatements of the VQT front end's device stages, one per kernel (csrc/a2s_vqt.hip, and the framed form in which
piano_a2s_amd/vqt.py calls a2s_gemm_f32).  include/a2s.h is the definition:

    decimator   out[b][m] = sum_j ypad[b][2 m + j] taps[j],  ypad[b][s] = 0 for s >= padded_len
    epilogue    db  = 20 log10(max(1e-5, |C|)) - 20 log10(max(1e-5, max over the clip of |C|))
                out = (max(db, -top_db) + 80) / 80
    layouts     plain:    C (B, rows, 2 bins) = [re (bins) | im (bins)]
                octaves:  C (B, rows, n_oct * 2 bpo), octave o (the HIGHEST first) = [re (bpo) | im (bpo)] of bins  bins - (o + 1) bpo ... bins - o bpo - 1
    framed GEMM C[b][n][c] = sum_m padded[b][n hop + m] bank[m][c]

Each reference also returns what its test's tolerance is stated against (sum |a||b| of a contraction, the unclamped dB of a cell).
tests/test_vqt_ops_oracle_cpu.py pins them to oracle/vqt_ref.py."""
import numpy as np

AMIN = 1e-5


def decimate_ref(ypad, taps, n_out):
    """ypad (B, padded_len), taps (ntaps,) -> out (B, n_out), mag (B, n_out) = sum_j |ypad[b][2 m + j]| |taps[j]|."""
    ypad, taps = np.asarray(ypad, dtype=np.float64), np.asarray(taps, dtype=np.float64).reshape(-1)
    B, plen = ypad.shape
    need = 2 * (n_out - 1) + len(taps)
    y = np.zeros((B, max(need, plen)))
    y[:, :plen] = ypad                                                      # zero at or beyond the row length
    win = np.lib.stride_tricks.sliding_window_view(y, len(taps), axis=1)[:, ::2][:, :n_out]       # (B, n_out, ntaps) view
    return win @ taps, np.abs(win) @ np.abs(taps)


def logmag_ref(re, im, top_db):
    """re, im (B, rows, bins) -> out (B, rows, bins) in [(80 - top_db) / 80, 1], db (B, rows, bins) before the clamp."""
    mag = np.hypot(np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64))
    peak = mag.reshape(mag.shape[0], -1).max(axis=1)[:, None, None]
    db = 20.0 * np.log10(np.maximum(AMIN, mag)) - 20.0 * np.log10(np.maximum(AMIN, peak))
    return (np.maximum(db, -float(top_db)) + 80.0) / 80.0, db


def pack_plain(re, im):
    """(B, rows, bins) planes -> C (B, rows, 2 bins) = [re | im]."""
    return np.concatenate([re, im], axis=2)


def pack_octaves(re, im, bpo):
    """(B, rows, bins) planes -> C (B, rows, n_oct * 2 bpo): octave by octave, the highest first, [re | im] inside each."""
    bins = re.shape[2]
    if bins % bpo:
        raise ValueError("bins must be a multiple of the bins per octave")
    parts = []
    for o in range(bins // bpo):
        lo = bins - (o + 1) * bpo
        parts += [re[:, :, lo:lo + bpo], im[:, :, lo:lo + bpo]]
    return np.concatenate(parts, axis=2)


def framed_gemm_ref(padded, hop, bank, frames):
    """padded (B, plen), bank (n_fft, N) -> C (B, frames, N), mag (B, frames, N) = sum_m |padded[b][n hop + m]| |bank[m][c]|."""
    padded, bank = np.asarray(padded, dtype=np.float64), np.asarray(bank, dtype=np.float64)
    n_fft = bank.shape[0]
    if (frames - 1) * hop + n_fft > padded.shape[1]:
        raise ValueError("the last frame reaches beyond the padded clip")
    win = np.lib.stride_tricks.sliding_window_view(padded, n_fft, axis=1)[:, ::hop][:, :frames]   # (B, frames, n_fft) view: the Hankel operand
    return win @ bank, np.abs(win) @ np.abs(bank)


def logmag_f32(re, im, top_db):
    """The epilogue's formula restated in float32 numpy, operation by operation (an emulation of the arithmetic, not the kernel): what fp32
    rounding alone costs against logmag_ref.  The tolerance of the device tests is derived from it (tests/test_gpu_vqt_ops.py)."""
    f = np.float32
    re, im = np.asarray(re, dtype=f), np.asarray(im, dtype=f)
    mag = np.sqrt(re * re + im * im)
    peak = mag.reshape(mag.shape[0], -1).max(axis=1)[:, None, None]
    db = f(20) * np.log10(np.maximum(f(AMIN), mag)) - f(20) * np.log10(np.maximum(f(AMIN), peak))
    return (np.maximum(db, f(-top_db)) + f(80)) / f(80)


# ----------------------------------------------------------------------------- inputs of the epilogue tests (shared by the CPU and the GPU file)
LOGMAG_SHAPES = [(3, 37, 480, 60), (2, 1, 480, 60), (3, 7, 24, 4), (1, 5, 60, 60), (2, 200, 480, 60)]       # (B, rows, bins, bpo)
PEAK_PLACES = ("first_row", "last_cell", "high_block")
# per-clip maxima of one batch (cut to the shape's B): four decades apart; an ulp apart (and, for a third clip, a part in a thousand); silence and a
# clip below the floor beside an ordinary one; the clip below the floor alone (for B = 1)
PEAK_SETS = {"far": (1e4, 1.0, 1e-4), "close": (1.0, 1.0000001, 1.001), "special": (0.0, 3e-6, 1.0), "floor": (3e-6, 0.0, 1.0)}


def peak_cell(place, rows, bins):
    """(row, bin) of the cell that holds the clip maximum.  high_block: the last cell owned by the highest-numbered of the 64 partial-maximum
    blocks that owns any (cell i = row * bins + bin belongs to block (i // 256) % 64)."""
    n = rows * bins
    if place == "first_row":
        i = 7 % bins
    elif place == "last_cell":
        i = n - 1
    else:
        idx = np.arange(n)
        blk = (idx // 256) % 64
        i = int(idx[blk == blk.max()][-1])
    return i // bins, i % bins


def logmag_case(shape, peaks, place, seed):
    """float32 planes re, im (B, rows, bins): magnitudes 10^U(-7, 4) with random phase, in each clip capped at 0.49 of its maximum peaks[b],
    which sits alone (re = peak, im = 0) in the cell `place` names; peaks[b] = 0 makes the clip silent."""
    B, rows, bins, _ = shape
    g = np.random.default_rng(seed)
    re, im = np.zeros((B, rows, bins), dtype=np.float32), np.zeros((B, rows, bins), dtype=np.float32)
    r, k = peak_cell(place, rows, bins)
    for b in range(B):
        peak = np.float32(peaks[b])
        if peak == 0:
            continue
        top = min(4.0, np.log10(0.49 * float(peak)))
        mag = 10.0 ** g.uniform(-7.0, top, size=(rows, bins))
        ph = g.uniform(0.0, 2.0 * np.pi, size=(rows, bins))
        re[b], im[b] = (mag * np.cos(ph)).astype(np.float32), (mag * np.sin(ph)).astype(np.float32)
        re[b, r, k], im[b, r, k] = peak, 0.0
    return re, im


def layout_case(B, rows, bins, bpo, db_per_octave):
    """Every (octave, bin) cell a magnitude of its own: `db_per_octave` apart from octave to octave (the highest bins loudest), falling
    monotonically by 0.9 of that inside an octave; rows scaled by distinct factors in (0.95, 1], clips in (0.8, 1].  Random phase."""
    g = np.random.default_rng(bins + bpo)
    k = np.arange(bins)
    o, kk = (bins - 1 - k) // bpo, (bins - 1 - k) % bpo                      # octave 0 = the highest bins, kk = 0 at its top bin
    db = -db_per_octave * (o + 0.9 * kk / bpo)
    mag = 10.0 ** (db / 20.0)[None, None, :] * (1.0 - 0.05 * np.arange(rows) / rows)[None, :, None] * (1.0 - 0.2 * np.arange(B) / B)[:, None, None]
    ph = g.uniform(0.0, 2.0 * np.pi, size=mag.shape)
    return (mag * np.cos(ph)).astype(np.float32), (mag * np.sin(ph)).astype(np.float32)
