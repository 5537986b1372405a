"""From decoded bars back to sound, and how well each decoded bar fits the audio it came from.

The reverse path of a transcription, joined from parts the tree already has: `metrics.note_events` reads a decoded bar row as notes, the bar lines of
the window (audio.plan_bar_lines) place them in time, `scoregen.pack_program` and `render.render` synthesise them on the GPU (csrc/a2s_render.hip)
with ONE fixed instrument, the GPU VQT turns the result into the model's own features, and `hip.segment_agreement` (csrc/a2s_agree.hip) compares
those with the recording's features bar by bar.  The agreement of a bar is the Pearson correlation of the two feature tensors over the bar's frames
(all bins): the dB features sit on a non-zero background, which a plain cosine does not take out.  It needs no ground-truth score.

What the number is not: a note accuracy.  The instrument is not a piano, tied chains sound short, and on a real recording timbre and reverberation
lower it for a perfect transcription by an amount nobody has measured.  Host side: numpy, Fractions and torch only."""
import math
from fractions import Fraction

import numpy as np
import torch

from . import hip, metrics, render, scoregen

# the one instrument a decoded score is played on (scoregen.make_clip's keys; the corpus draws g in 0.45 .. 0.8, n_harm in 4 .. 10, tau in 0.4 .. 1.2,
# attack in 32 .. 128): mid-range everywhere, every note at the same amplitude, no noise floor
RESYNTH_INSTRUMENT = dict(g=0.6, n_harm=8, tau=0.8, attack=80)
RESYNTH_AMP = 0.5
SAMPLE_RATE = scoregen.SR


def bar_ticks(time_signature):
    """Ticks (metrics.NOTE_W to the whole note) of a bar of the time signature "num/den", as a Fraction."""
    num, den = str(time_signature).split("/")
    num, den = int(num), int(den)
    if num < 1 or den < 1:
        raise ValueError(f"resynth: not a time signature: {time_signature!r}")
    return Fraction(metrics.NOTE_W * num, den)


def bar_events(ids_row, ticks):
    """One decoded bar row -> ([(onset, length, midi)] with onset and length as Fractions of the bar, overflow): metrics.note_events scaled by
    end = max(ticks, the latest onset + duration).  A bar whose durations add up to more than its time signature is SQUEEZED into its bar, never
    spilled into the next one; a bar that is too short keeps its silence at the end.  Rests and tie continuations are dropped exactly as note_events
    drops them, and note_events does not merge ties: a tied chain therefore sounds only as long as its first note -- tied chains sound short."""
    notes, overflow = metrics.note_events(ids_row)
    if not notes:
        return [], overflow
    end = max(Fraction(ticks), max(Fraction(on + dur) for on, _, dur, _ in notes))
    return [(Fraction(on) / end, Fraction(dur) / end, int(midi)) for on, midi, dur, _ in notes], overflow


def score_events(upper_rows, lower_rows, time_signatures, bar_lines, max_events=scoregen.MAX_EVENTS):
    """The notes of one window in samples: upper_rows / lower_rows = the decoded id rows per bar, time_signatures = "num/den" per bar, bar_lines = the
    n_bars + 1 ascending sample positions of the bar lines in the window -> (events (n, 3) int64 [onset, length, midi] in (onset, midi) order,
    truncated).  A note of bar b starts at line[b] + floor(span * onset) and lasts floor(span * length) samples, at least 1, and ends at the bar's
    closing line at the latest (integer / Fraction arithmetic: a score whose durations are whole samples comes back exactly).  More than max_events
    notes: the earliest are kept, truncated = True."""
    lines = [int(t) for t in bar_lines]
    n_bars = len(lines) - 1
    if n_bars < 0 or any(b <= a for a, b in zip(lines, lines[1:])):
        raise ValueError(f"resynth: bar lines must ascend strictly (got {lines})")
    if not (len(upper_rows) >= n_bars and len(lower_rows) >= n_bars and len(time_signatures) >= n_bars):
        raise ValueError(f"resynth: {n_bars} bars between the lines, but {len(upper_rows)} / {len(lower_rows)} rows and {len(time_signatures)} time signatures")
    ev = []
    for b in range(n_bars):
        ticks, span = bar_ticks(time_signatures[b]), lines[b + 1] - lines[b]
        for staff, rows in enumerate((upper_rows, lower_rows)):
            for on, ln, midi in bar_events(rows[b], ticks)[0]:
                onset = min(lines[b] + math.floor(span * on), lines[b + 1] - 1)
                length = min(max(1, math.floor(span * ln)), lines[b + 1] - onset)
                ev.append((onset, length, midi, staff))
    ev.sort(key=lambda e: (e[0], e[2], e[3]))
    truncated = len(ev) > max_events
    return np.array([e[:3] for e in ev[:max_events]], dtype=np.int64).reshape(-1, 3), truncated


def program(events, n_samples, rows=scoregen.MAX_EVENTS):
    """The render program (1 + rows, 8) int32 of `events` (n, 3) [onset, length, midi] on RESYNTH_INSTRUMENT, through scoregen.pack_program: the gain
    rule (|wave| < 1) and the pitch-dependent decay are the corpus's."""
    events = np.asarray(events, dtype=np.int64).reshape(-1, 3)
    inst = dict(RESYNTH_INSTRUMENT, noise_db=-200.0, noise_seed=0)
    clip = dict(events=events, amps=np.full(len(events), RESYNTH_AMP, dtype=np.float32), instrument=inst, n_samples=int(n_samples))
    p = scoregen.pack_program(clip, rows=rows)
    p[0, 6] = 0                                                  # noise off: the level is exactly 0.0, not 10^-10
    return p


def agreement(sums, n_cells):
    """Pearson correlation from the five sums [sum x, sum y, sum x^2, sum y^2, sum x y] over n_cells cells, in float64 on the host:
    (n Sxy - Sx Sy) / sqrt((n Sxx - Sx^2)(n Syy - Sy^2)), clipped to [-1, 1]; None where n_cells is 0 or either variance is not positive."""
    n = float(n_cells)
    sx, sy, sxx, syy, sxy = (float(v) for v in sums)
    vx, vy = n * sxx - sx * sx, n * syy - sy * sy
    if n <= 0 or not vx > 0.0 or not vy > 0.0:
        return None
    return min(1.0, max(-1.0, (n * sxy - sx * sy) / math.sqrt(vx * vy)))


def bar_segments(windows, hop, n_frames):
    """The segment table of a batch: per window with events its bars as [window index, line[b] // hop, line[b + 1] // hop], frames clamped to
    n_frames -> (int64 array (S, 3), [(window index, bar index)] per row)."""
    seg, where = [], []
    for w, win in enumerate(windows):
        if not len(win["events"]):
            continue
        lines = win["bar_lines"]
        for b in range(len(lines) - 1):
            f0, f1 = min(int(lines[b]) // hop, n_frames), min(int(lines[b + 1]) // hop, n_frames)
            seg.append((w, f0, max(f0, f1)))
            where.append((w, b))
    return np.array(seg, dtype=np.int64).reshape(-1, 3), where


def dtw_band(n):
    """The Sakoe-Chiba half-width the alignment of a bar of n frames runs with: a quarter of the bar, at least 8 frames."""
    return max(8, int(n) // 4)


def warp_from_path(path, n):
    """A DTW path over an n x n grid -- cells (i, j) from (0, 0) to (n - 1, n - 1), as pairs or packed (i << 16) | j, i the recording's frame and j
    the score's -> (warp, inverse), float64 (n,) each: warp[j] = (first i + last i) / 2 over the recording frames matched to score frame j, and
    inverse[i] the same over the score frames matched to recording frame i.  A path visits every row and every column, so every entry is set."""
    cells = np.asarray(path, dtype=np.int64)
    if cells.ndim == 1:
        cells = np.stack([cells >> 16, cells & 0xFFFF], axis=1)
    n = int(n)
    if cells.ndim != 2 or cells.shape[1] != 2 or n < 1 or len(cells) < n or tuple(cells[0]) != (0, 0) or tuple(cells[-1]) != (n - 1, n - 1):
        raise ValueError(f"resynth: not a path from (0, 0) to ({n - 1}, {n - 1})")
    step = np.diff(cells, axis=0)
    if len(step) and not (np.all((step >= 0) & (step <= 1)) and np.all(step.sum(axis=1) >= 1)):
        raise ValueError("resynth: a path moves by (1, 1), (1, 0) or (0, 1)")
    out = []
    for own, other in ((1, 0), (0, 1)):
        first, last = np.full(n, n, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        np.minimum.at(first, cells[:, own], cells[:, other])
        np.maximum.at(last, cells[:, own], cells[:, other])
        out.append((first + last) / 2.0)
    return out[0], out[1]


def warp_time(warp, u):
    """The warp at the fractional frame u, interpolated linearly between the frames floor(u) and floor(u) + 1; u is clipped to [0, n], and behind the
    last frame the map goes on at slope 1 (the identity warp therefore returns u itself, exactly)."""
    n = len(warp)
    u = min(max(float(u), 0.0), float(n))
    k = min(int(math.floor(u)), n - 1)
    nxt = float(warp[k + 1]) if k + 1 < n else float(warp[n - 1]) + 1.0
    return float(warp[k]) + (u - k) * (nxt - float(warp[k]))


def performed_notes(notes, warp, first_frame, hop, bar_start, bar_stop):
    """notes (n, 3) [onset, length, midi] in samples of the window, all of ONE bar whose segment starts at frame first_frame and whose lines are at the
    samples bar_start < bar_stop; warp: the bar's warp_from_path, or None -> [(onset, length, midi)] in samples (floats): onset and end moved by
    what the warp moves their frame position, clamped to the bar, a length of at least one frame where the bar has room, of one sample otherwise.  The
    identity warp moves nothing: onsets come back exactly."""
    out = []
    for onset, length, midi in notes:
        if warp is None:
            out.append((float(onset), float(length), int(midi)))
            continue
        moved = []
        for t in (int(onset), int(onset) + int(length)):
            u = t / hop - first_frame
            moved.append(min(max(t + (warp_time(warp, u) - min(max(u, 0.0), float(len(warp)))) * hop, float(bar_start)), float(bar_stop)))
        on = min(moved[0], float(bar_stop) - 1.0)
        out.append((on, max(1.0, min(max(moved[1] - on, float(hop)), float(bar_stop) - on)), int(midi)))
    return out


def resynthesise(windows, feats, vqt, hop, n_samples=None, align=False):
    """windows: per window of a batch a dict with "events" ((n, 3) int64 of score_events) and "bar_lines"; feats: the recording's features of the same
    windows, (W, 1, T, F) or (W, T, F) float32 on the device; vqt: the front end that made them (waveforms (B, N) -> features); hop: its hop length.
    -> (waves: per window the rendered waveform, float32 numpy (n_samples,), or None; agreements: per window a list with one entry per bar, a float in
    [-1, 1] or None).  n_samples defaults to (T - 1) * hop, the window the features cover.
    The windows that hold at least one note are rendered in ONE synthesiser launch, go through the VQT together, and their bars are compared in ONE
    hip.segment_agreement call.  A window without any note is neither rendered nor compared and its bars get None: the front end normalises to the
    window's peak, so the features of silence are all ones (csrc/a2s_vqt.hip: max(1e-5, 0) on both sides) and no correlation is defined.
    align=True -> (waves, agreements, alignments): additionally ONE hip.dtw_segments call warps the resynthesis onto the
    recording inside every bar (band dtw_band(n); the offset of the differences is mean(recording) - mean(resynthesis) of the bar, from the five sums),
    and one more hip.segment_agreement call scores the recording against the resynthesis read along the inverse warp.  alignments: per window a
    list with one entry per bar, {"first_frame", "frames", "warp", "inverse", "total", "agreement_warped"} or None where the bar has no agreement."""
    f3 = feats[:, 0] if feats.dim() == 4 else feats
    W, T, F = f3.shape
    if len(windows) != W:
        raise ValueError(f"resynth: {len(windows)} windows but features of {W}")
    n_samples = (T - 1) * int(hop) if n_samples is None else int(n_samples)
    waves = [None] * W
    agreements = [[None] * (len(win["bar_lines"]) - 1) for win in windows]
    live = [w for w, win in enumerate(windows) if len(win["events"])]
    alignments = [[None] * len(a) for a in agreements] if align else None
    if not live:
        return (waves, agreements, alignments) if align else (waves, agreements)
    progs = np.stack([program(windows[w]["events"], n_samples) for w in live])
    wave = render.render(torch.from_numpy(progs).to(f3.device), n_samples)
    y = vqt(wave)
    y3 = y[:, 0] if y.dim() == 4 else y
    if tuple(y3.shape[1:]) != (T, F):
        raise hip.A2SError(f"resynth: the resynthesis has features {tuple(y3.shape[1:])} per window, the recording {(T, F)}")
    seg, where = bar_segments([windows[w] for w in live], int(hop), T)
    x3 = f3[live].contiguous() if len(live) != W else f3
    sums = hip.segment_agreement(x3, y3, seg).cpu().numpy()
    for (i, b), row, s in zip(where, seg, sums):
        agreements[live[i]][b] = agreement(s, (int(row[2]) - int(row[1])) * F)
    if align:
        _align_bars(x3, y3, seg, where, sums, [live[i] for i, _ in where], agreements, alignments)
    host = wave.cpu().numpy()
    for i, w in enumerate(live):
        waves[w] = host[i]
    return (waves, agreements, alignments) if align else (waves, agreements)


def _align_bars(x3, y3, seg, where, sums, window_of, agreements, alignments):
    """The align=True half of resynthesise: fills `alignments` for the bars of the table `seg` that have an agreement."""
    _, T, F = x3.shape
    x3, y3 = x3.contiguous(), y3.contiguous()          # (the gathered tensor below is contiguous, and both operands share one clip stride)
    rows = [k for k, ((_, b), w) in enumerate(zip(where, window_of)) if agreements[w][b] is not None]
    if not rows:
        return
    table = np.array([[seg[k][0], seg[k][1], seg[k][2], dtw_band(seg[k][2] - seg[k][1])] for k in rows], dtype=np.int64)
    cells = (table[:, 2] - table[:, 1]) * F
    off = torch.from_numpy(((sums[rows, 0] - sums[rows, 1]) / cells).astype(np.float32)).to(x3.device)
    paths, steps, totals = (t.cpu().numpy() for t in hip.dtw_segments(x3, y3, table, off))
    index = np.tile(np.arange(T, dtype=np.int64), (x3.shape[0], 1))             # (clips, T): the score frame heard at every recording frame
    found = []
    for k, (clip, f0, f1, _) in enumerate(table):
        warp, inverse = warp_from_path(paths[k, :steps[k]], f1 - f0)
        index[clip, f0:f1] = f0 + np.floor(inverse + 0.5).astype(np.int64)
        found.append({"first_frame": int(f0), "frames": int(f1 - f0), "warp": warp, "inverse": inverse, "total": float(totals[k])})
    index = torch.from_numpy(index).to(x3.device)
    heard = y3[torch.arange(x3.shape[0], device=x3.device)[:, None], index]     # row i of a bar: the resynthesis frame matched to recording frame i
    warped = hip.segment_agreement(x3, heard, table[:, :3]).cpu().numpy()
    for k, row, s, n in zip(rows, found, warped, cells):
        row["agreement_warped"] = agreement(s, int(n))
        alignments[window_of[k]][where[k][1]] = row


def mean_agreement(values):
    """The mean of the entries that are not None; None where there is none."""
    got = [v for v in values if v is not None]
    return sum(got) / len(got) if got else None
