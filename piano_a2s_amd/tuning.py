"""The tuning of a recording, estimated on the device, and the features corrected for it (the kernels are csrc/a2s_tuning.hip,
the float64 definition is tests/tuning_oracle.py).

The features have bins_per_octave bins per octave, bin 0 is A0 at A4 = 440 Hz.  A piano that sits c cents away from 440 Hz puts every partial
c * S / 100 bins beside the column the model learnt (S = bins per semitone).  Three device stages, none with a read-back:

    profile   every spectral peak (a cell above its left neighbour, not below its right one, at least `thr`) is placed between the columns by a
              three-point parabola; its position modulo one semitone goes into a histogram of H = 100 cells (one cent each), weighted by its height
    estimate  the histograms of one recording's clips are added, smoothed circularly by a triangle, and the arg max is refined by a second parabola:
              cents in [-50, 50), a confidence (the peak of the smoothed histogram over its mean) and the number of peaks
    shift     a2s_shift_bins by -cents * S / 100 bins (linear interpolation; the kernel of the transposition augmenter)

`estimate_host` restates the second stage in numpy, bit for bit.  A detuning beyond +-50 cents is a transposition and cannot be told apart."""
import numpy as np

H = 100                      # histogram cells per semitone: one cell is one cent
Q = 4096                     # weight of a peak: 1 + rint(min(height above thr, 1) * Q)
HALF_WINDOW = 6              # the smoothing window is the triangle (HALF_WINDOW + 1) - |j|, j = -HALF_WINDOW .. HALF_WINDOW: its sum is 49
THR = 0.5                    # features are dB / 80 + 1: 40 dB below the window's peak
MIN_PEAKS = H                # with fewer peaks than cells the contrast is large by construction
MIN_CONF = 3.31              # midway between the largest confidence on noise and the smallest on rendered clips (tools/tuning_check.py, section 27)
A4_HZ = 440.0


def bins_per_semitone(bins_per_octave):
    b = int(bins_per_octave)
    if b != bins_per_octave or b < 12 or b % 12:
        raise ValueError(f"tuning: bins_per_octave must be a multiple of 12 (got {bins_per_octave!r})")
    return b // 12


def check_first(first, n_clips):
    """The HOST table of group offsets as int64 (G + 1,), or ValueError: it ascends from 0 to n_clips (a group may be empty)."""
    try:
        f = np.asarray(first)
        whole = f.size > 0 and (np.issubdtype(f.dtype, np.integer) or bool(np.all(f == np.rint(f))))
    except (TypeError, ValueError):
        f, whole = None, False
    if not whole or f.ndim != 1:
        raise ValueError("tuning: `first` must be a 1-D table of whole numbers")
    f = f.astype(np.int64)
    if f[0] != 0 or f[-1] != n_clips or bool(np.any(np.diff(f) < 0)):
        raise ValueError(f"tuning: `first` must ascend from 0 to the number of clips, {n_clips} (got {f.tolist()[:8]}{' ...' if f.size > 8 else ''})")
    return f


def estimate_host(hist, first, min_conf=MIN_CONF, min_peaks=MIN_PEAKS, bins_per_semitone=5):
    """The second stage in numpy, with the kernel's operations: hist (B, H + 1) int64 (cell H is the peak count), first (G + 1,) ascending from 0 to B
    -> (est (G, 3) float64 [cents, confidence, peaks], eff_bins (B,) float32: -cents * S / 100 for every clip of a determined group, else 0)."""
    hist = np.asarray(hist, dtype=np.int64).reshape(-1, H + 1)
    B, S = hist.shape[0], int(bins_per_semitone)
    first = check_first(first, B)
    G = len(first) - 1
    est, eff = np.zeros((G, 3), dtype=np.float64), np.zeros(B, dtype=np.float32)
    tri = [HALF_WINDOW + 1 - abs(j) for j in range(-HALF_WINDOW, HALF_WINDOW + 1)]
    for g in range(G):
        lo, hi = int(first[g]), int(first[g + 1])
        h = hist[lo:hi].sum(axis=0, dtype=np.int64)
        sm = np.zeros(H, dtype=np.int64)
        for j, w in zip(range(-HALF_WINDOW, HALF_WINDOW + 1), tri):
            sm += w * np.roll(h[:H], -j)                              # h[(k + j) mod H]
        k = int(np.argmax(sm))                                        # (the first of equals)
        total = int(sm.sum(dtype=np.int64))
        conf = np.float64(sm[k]) * np.float64(H) / np.float64(total) if total != 0 else np.float64(0.0)
        A, C, E = int(sm[(k - 1) % H]), int(sm[k]), int(sm[(k + 1) % H])
        den = (A - C) + (E - C)
        delta = np.float64(0.5) * np.float64(A - E) / np.float64(den) if den < 0 else np.float64(0.0)
        cents = ((np.float64(k) + np.float64(0.5)) + delta) * np.float64(100.0) / np.float64(H) - np.float64(50.0)
        if cents >= 50.0:
            cents = cents - np.float64(100.0)
        peaks = int(h[H])
        est[g] = (cents, conf, np.float64(peaks))
        if peaks >= min_peaks and conf >= min_conf:
            eff[lo:hi] = np.float32(-cents * np.float64(S) / np.float64(100.0))
    return est, eff


def a4_hz(cents):
    return A4_HZ * 2.0 ** (float(cents) / 1200.0)


def describe(est_row, min_conf=MIN_CONF, min_peaks=MIN_PEAKS):
    """One row [cents, confidence, peaks] of `est`, read back -> the record transcribe reports."""
    cents, conf, peaks = float(est_row[0]), float(est_row[1]), int(est_row[2])
    return {"cents": cents, "confidence": conf, "peaks": peaks, "determined": bool(peaks >= min_peaks and conf >= min_conf), "a4_hz": a4_hz(cents)}


class Tuner:
    """tuner(feats, n_rows=None, first=None, cents=None) -> (corrected feats, est (G, 3) float64 on the device, eff_bins (B,) float32 on the device).
    feats: (B, rows, F) or (B, 1, rows, F) float32 on the device, contiguous; n_rows (B,) int32 on the device: the rows of every clip that count
    (default: all); first: the HOST table of the groups' offsets, ascending from 0 to B (default: every clip a group of its own); a group is what
    shares one tuning.  cents=None: profile -> estimate -> shift, nothing is read back; a group that is not determined (fewer than min_peaks peaks
    or a confidence below min_conf) is left as it is.  cents given (a number): neither new kernel runs, every clip is shifted by -cents * S / 100
    bins and est holds [cents, 0, 0] for every group."""

    def __init__(self, device, bins_per_octave=60, thr=THR, min_conf=MIN_CONF, min_peaks=MIN_PEAKS):
        import torch
        self.device = torch.device(device)
        self.S = bins_per_semitone(bins_per_octave)
        if not 1 <= self.S <= 64:
            raise ValueError(f"tuning: at most 64 bins per semitone (got {self.S})")
        self.thr, self.min_conf, self.min_peaks = float(thr), float(min_conf), int(min_peaks)
        if not 0.0 <= self.thr <= 1.0:
            raise ValueError(f"tuning: thr must be in 0 .. 1 (got {thr!r})")
        if not np.isfinite(self.min_conf) or self.min_peaks < 0:
            raise ValueError(f"tuning: min_conf must be finite and min_peaks >= 0 (got {min_conf!r}, {min_peaks!r})")
        self._tables = {}

    def _table(self, first, B):
        """`first` on the device, checked on the host before the upload; the default (every clip its own group) is kept per batch size."""
        import torch
        if first is None:
            if B not in self._tables:
                self._tables[B] = torch.arange(B + 1, dtype=torch.int32, device=self.device)
            return self._tables[B]
        return torch.from_numpy(check_first(first, B).astype(np.int32)).to(self.device)

    def __call__(self, feats, n_rows=None, first=None, cents=None):
        import torch
        from . import hip
        x = feats[:, 0] if feats.dim() == 4 else feats
        B, rows = x.shape[0], x.shape[1]
        table = self._table(first, B)
        G = table.shape[0] - 1
        if cents is not None:
            c = float(cents)
            if not np.isfinite(c):
                raise ValueError(f"tuning: cents must be finite (got {cents!r})")
            est = torch.zeros((G, 3), dtype=torch.float64, device=self.device)
            est[:, 0] = c
            eff = torch.full((B,), float(np.float32(-c * self.S / 100.0)), dtype=torch.float32, device=self.device)
        else:
            if n_rows is None:
                n_rows = torch.full((B,), rows, dtype=torch.int32, device=self.device)
            hist = hip.tuning_profile(x, n_rows, thr=self.thr, bins_per_semitone=self.S)
            est, eff = hip.tuning_estimate(hist, table, self.min_conf, self.min_peaks, bins_per_semitone=self.S)
        return hip.shift_bins(feats, eff), est, eff
