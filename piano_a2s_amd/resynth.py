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


def resynthesise(windows, feats, vqt, hop, n_samples=None):
    """windows: per window of a batch a dict with "events" ((n, 3) int64 of score_events) and "bar_lines"; feats: the recording's features of the same
    windows, (W, 1, T, F) or (W, T, F) float32 on the device; vqt: the front end that made them (waveforms (B, N) -> features); hop: its hop length.
    -> (waves: per window the rendered waveform, float32 numpy (n_samples,), or None; agreements: per window a list with one entry per bar, a float in
    [-1, 1] or None).  n_samples defaults to (T - 1) * hop, the window the features cover.
    The windows that hold at least one note are rendered in ONE synthesiser launch, go through the VQT together, and their bars are compared in ONE
    hip.segment_agreement call.  A window without any note is neither rendered nor compared and its bars get None: the front end normalises to the
    window's peak, so the features of silence are all ones (csrc/a2s_vqt.hip: max(1e-5, 0) on both sides) and no correlation is defined."""
    f3 = feats[:, 0] if feats.dim() == 4 else feats
    W, T, F = f3.shape
    if len(windows) != W:
        raise ValueError(f"resynth: {len(windows)} windows but features of {W}")
    n_samples = (T - 1) * int(hop) if n_samples is None else int(n_samples)
    waves = [None] * W
    agreements = [[None] * (len(win["bar_lines"]) - 1) for win in windows]
    live = [w for w, win in enumerate(windows) if len(win["events"])]
    if not live:
        return waves, agreements
    progs = np.stack([program(windows[w]["events"], n_samples) for w in live])
    wave = render.render(torch.from_numpy(progs).to(f3.device), n_samples)
    y = vqt(wave)
    y3 = y[:, 0] if y.dim() == 4 else y
    if tuple(y3.shape[1:]) != (T, F):
        raise hip.A2SError(f"resynth: the resynthesis has features {tuple(y3.shape[1:])} per window, the recording {(T, F)}")
    seg, where = bar_segments([windows[w] for w in live], int(hop), T)
    sums = hip.segment_agreement(f3[live].contiguous() if len(live) != W else f3, y3, seg).cpu().numpy()
    for (i, b), row, s in zip(where, seg, sums):
        agreements[live[i]][b] = agreement(s, (int(row[2]) - int(row[1])) * F)
    host = wave.cpu().numpy()
    for i, w in enumerate(live):
        waves[w] = host[i]
    return waves, agreements


def mean_agreement(values):
    """The mean of the entries that are not None; None where there is none."""
    got = [v for v in values if v is not None]
    return sum(got) / len(got) if got else None
