"""Definition of the note dynamics (the device kernels are csrc/a2s_dynamics.hip), in float64 and, for the update, restated in
numpy float32, plus the float64 analysis-by-synthesis loop on the float64 synthesiser and front end (tests/render_oracle.py, oracle/vqt_ref.py).

    note row [clip, fx, fy, n, b1, b2, b3, prog_row]; n is read as min(n, 64).
    levels:  the cells of a row are the frames i < n crossed with the columns b_h - 1 .. b_h + 1 of every b_h >= 0; a cell counts only if its column
             is in [0, F) and BOTH fx + i and fy + i are in [0, T).  out = [sum x[clip][fx + i][col], sum y[clip][fy + i][col], count]; a clip outside
             [0, B) or n <= 0: zeros.
    update (per clip over its rows first[b] .. first[b + 1]):
             d = 80 (Sx - Sy) / count (0 where count = 0): the features are dB / 80 + 1, so d is the mean level difference in dB;
             c = cum + d;  med = the lower median of c, the (k - 1) // 2-th smallest of k;  cum' = min(max(c - med, -30), 12);
             amplitude of program row prog_row = base_amp * 2^(cum' * log2(10) / 20) = base_amp * 10^(cum' / 20).
    velocity = min(127, max(1, rint(64 * 10^(level_db / 40)))).

update_f32 does every step in numpy float32, one operation per step, as the kernel does: on the same sums and the same cum it gives the kernel's bits of
cum'.  The amplitude is checked against amplitudes_f64(cum') within amp_bound (derived there)."""
import numpy as np

U = 2.0 ** -24
N_MAX = 64
LEVEL_LO, LEVEL_HI = -30.0, 12.0
K32 = np.float32(0.16609640474436813)          # log2(10) / 20, rounded to float32 as the kernel holds it


def cells(row, B, T, F):
    """The cells that count of one row, in the kernel's order k = 9 i + 3 h + c: [(fx + i, fy + i, col)]."""
    clip, fx, fy, n = (int(v) for v in row[:4])
    out = []
    if clip < 0 or clip >= B:
        return out
    for i in range(max(0, min(n, N_MAX))):
        for b in (int(v) for v in row[4:7]):
            for col in (b - 1, b, b + 1):
                if b >= 0 and 0 <= col < F and 0 <= fx + i < T and 0 <= fy + i < T:
                    out.append((fx + i, fy + i, col))
    return out


def levels(x, y, rows):
    """x, y (B, T, F), rows (S, 8) -> (S, 3) float64 [sum x, sum y, count]."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    B, T, F = x.shape
    out = np.zeros((len(rows), 3))
    for s, row in enumerate(rows):
        cs = cells(row, B, T, F)
        if cs:
            tx, ty, col = (np.array(v) for v in zip(*cs))
            out[s] = [x[int(row[0]), tx, col].sum(), y[int(row[0]), ty, col].sum(), len(cs)]
    return out


def lower_median(c):
    return np.sort(np.asarray(c), kind="stable")[(len(c) - 1) // 2]


def update(sums, first, cum, dtype=np.float64):
    """One update of every clip -> cum' (S,) of `dtype` (float32: the kernel's steps, one rounding each; float64: the definition)."""
    sums = np.asarray(sums, dtype=np.float64)
    out = np.array(cum, dtype=dtype)
    for b in range(len(first) - 1):
        lo, hi = int(first[b]), int(first[b + 1])
        if hi <= lo:
            continue
        sx, sy, n = sums[lo:hi, 0], sums[lo:hi, 1], sums[lo:hi, 2]
        d = np.where(n > 0, 80.0 * (sx - sy) / np.where(n > 0, n, 1.0), 0.0).astype(dtype)          # (the division in double, then ONE rounding)
        c = out[lo:hi] + d
        med = lower_median(c)
        out[lo:hi] = np.minimum(np.maximum(c - med, dtype(LEVEL_LO)), dtype(LEVEL_HI))
    return out


def update_f32(sums, first, cum):
    return update(sums, first, np.asarray(cum, dtype=np.float32), np.float32)


def amplitudes_f64(cum, base_amp):
    """base_amp * 10^(cum / 20) in float64 from the levels as they are stored."""
    return float(np.float32(base_amp)) * 10.0 ** (np.asarray(cum, dtype=np.float64) / 20.0)


def amp_bound(cum, base_amp, exp2_ulps=1.0):
    """How far the kernel's fp32 amplitude base_amp * exp2f(cum * K32) may lie from amplitudes_f64: K32 is log2(10) / 20 within a relative u and the
    product rounds once more, so the argument a = cum log2(10) / 20 (|a| <= 30 * 0.1661 < 4.99) is off by at most |a| (2 u + u^2); 2^a moves by the
    factor 2^(that) - 1 <= ln 2 * 2.0001 |a| u; the device's exp2f is within exp2_ulps = 1 ulp (HIP's math tables; v_exp_f32, as
    tests/attn_range_oracle.py counts it), an ulp being at most a relative 2 u; the last product rounds once (u).  All relative to the true
    amplitude: 9.92 u at |cum| = 30, 3 u at cum = 0; the few u^2 cross terms are covered by the factor 1.001."""
    a = np.abs(np.asarray(cum, dtype=np.float64)) * np.log2(10.0) / 20.0
    rel = np.log(2.0) * 2.0001 * a * U + 2.0 * exp2_ulps * U + U
    return 1.001 * rel * amplitudes_f64(cum, base_amp)


def velocity(level_db):
    return int(min(127, max(1, np.rint(64.0 * 10.0 ** (float(level_db) / 40.0)))))


def auc(real, phantom):
    """The probability that a real note's level lies above a phantom's (ties count half): the area under the ROC curve."""
    real, phantom = np.asarray(real, dtype=np.float64), np.asarray(phantom, dtype=np.float64)
    if not len(real) or not len(phantom):
        return None
    gt = (real[:, None] > phantom[None, :]).sum() + 0.5 * (real[:, None] == phantom[None, :]).sum()
    return float(gt) / (len(real) * len(phantom))


# ---- rendered clips with known amplitudes and phantom notes (tests/test_gpu_dynamics.py, tools/dynamics_check.py, tools/dynamics_bench.py)
def scenario(clip, rng, phantom_every=3):
    """A scoregen.make_clip clip -> {"events" (n, 3) and "amps" (n,): what is performed; "score" (m, 3): those notes plus the phantoms -- a copy of
    every phantom_every-th note moved by +-3 .. 8 semitones, dropped where that onset and pitch already sound or leave MIDI 21 .. 108 -- in (onset,
    midi) order; "real" (m,) bool; "true_db" (m,) 20 log10(amp), nan for a phantom}."""
    ev, amps = np.asarray(clip["events"], dtype=np.int64), np.asarray(clip["amps"], dtype=np.float64)
    have = {(int(o), int(m)) for o, _, m in ev}
    rows = [(int(o), int(l), int(m), True, float(a)) for (o, l, m), a in zip(ev, amps)]
    if phantom_every > 0:
        for o, l, m in ev[::phantom_every]:
            p = int(m) + int(rng.integers(3, 9)) * (1 if rng.integers(0, 2) else -1)
            if 21 <= p <= 108 and (int(o), p) not in have:
                have.add((int(o), p))
                rows.append((int(o), int(l), p, False, float("nan")))
    rows.sort(key=lambda r: (r[0], r[2]))
    return {"events": ev, "amps": amps.astype(np.float32), "score": np.array([r[:3] for r in rows], dtype=np.int64).reshape(-1, 3),
            "real": np.array([r[3] for r in rows], dtype=bool), "true_db": np.array([20.0 * np.log10(r[4]) for r in rows])}


def features64(program, n_samples):
    from oracle import vqt_ref
    from tests import render_oracle
    return vqt_ref.vqt_features_librosa(render_oracle.render(program, n_samples))


def loop64(x, score, n_samples, hop, rounds, performed=None):
    """The float64 loop on ONE clip: x (T, F) the performance's features, score (m, 3) the notes on the score side -> [cum after round 1, .., after
    round `rounds`], (m,) float64 each.  Programs as piano_a2s_amd.resynth packs them; the header's gain stays that of the first pack."""
    from piano_a2s_amd import resynth
    T, F = x.shape
    rows = resynth.note_rows(score, performed, hop, T, F)
    prog = resynth.program(score, n_samples)
    cum, out = np.zeros(len(score)), []
    for _ in range(int(rounds)):
        y = features64(prog, n_samples)
        cum = update(levels(x[None], y[None], rows), [0, len(rows)], cum)
        prog[rows[:, 7], 3] = amplitudes_f64(cum, resynth.RESYNTH_AMP).astype(np.float32).view(np.int32)
        out.append(cum.copy())
    return out


def level_errors(cum, scn):
    """(rms error in dB of the real notes' levels against the truth, both centred on their means over the real notes; AUC of real over phantom;
    the standard deviation of the true levels)."""
    real = scn["real"]
    got, true = np.asarray(cum, dtype=np.float64)[real], scn["true_db"][real]
    err = (got - got.mean()) - (true - true.mean())
    return float(np.sqrt(np.mean(err * err))), auc(got, np.asarray(cum)[~real]), float(true.std())
