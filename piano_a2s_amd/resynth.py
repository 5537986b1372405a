"""From decoded bars back to sound, and how well each decoded bar fits the audio it came from.

The reverse path of a transcription, joined from parts the tree already has: `metrics.note_events` reads a decoded bar row as notes, the bar lines of
the window (audio.plan_bar_lines) place them in time, `scoregen.pack_program` and `render.render` synthesise them on the GPU (csrc/a2s_render.hip)
with ONE fixed instrument, the GPU VQT turns the result into the model's own features, and `hip.segment_agreement` (csrc/a2s_agree.hip) compares
those with the recording's features bar by bar.  The agreement of a bar is the Pearson correlation of the two feature tensors over the bar's frames
(all bins): the dB features sit on a non-zero background, which a plain cosine does not take out.  It needs no ground-truth score.

What the number is not: a note accuracy.  The instrument is not a piano, tied chains sound short, and on a real recording timbre and reverberation
lower it for a perfect transcription by an amount nobody has measured.  Host side: numpy, Fractions and torch only.

Note dynamics: `estimate_dynamics` closes the loop -- the level of every note's own partials in the recording against the
resynthesis (`hip.note_levels`) moves the note's amplitude in the render program (`hip.note_amp_update`, csrc/a2s_dynamics.hip), and the score is
rendered again."""
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
# note dynamics: a note is measured at its first three partials, over at most 12 frames from the frame behind its onset
DYNAMICS_ROUNDS = 3
DYNAMICS_FRAMES = 12
DYNAMICS_BIN_OFFSETS = (0, 60, 95)                   # rint(60 log2 h), h = 1, 2, 3, in bins of a 60-per-octave VQT whose bin 0 is MIDI 21
LEVEL_DB_RANGE = (-30.0, 12.0)
# resynthesis at the performed timing: rounds of warp -> retime; round 1 reads the paths of the alignment pass
RETIME_ROUNDS = 2


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


def program(events, n_samples, amps=None, rows=scoregen.MAX_EVENTS):
    """The render program (1 + rows, 8) int32 of `events` (n, 3) [onset, length, midi] on RESYNTH_INSTRUMENT, through scoregen.pack_program: the gain
    rule (|wave| < 1) and the pitch-dependent decay are the corpus's.  amps: one amplitude per event; None: RESYNTH_AMP for every note."""
    events = np.asarray(events, dtype=np.int64).reshape(-1, 3)
    inst = dict(RESYNTH_INSTRUMENT, noise_db=-200.0, noise_seed=0)
    amps = np.full(len(events), RESYNTH_AMP, dtype=np.float32) if amps is None else np.asarray(amps, dtype=np.float32).reshape(len(events))
    clip = dict(events=events, amps=amps, instrument=inst, n_samples=int(n_samples))
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


def note_rows(events, performed, hop, T, F, clip=0):
    """The note table of the dynamics kernels (include/a2s.h: a2s_note_levels): events (n, 3) [onset, length, midi] in the order of their render
    program, performed: the n onsets in samples where the notes are HEARD in the recording, or None (where the score has them) -> (n, 8) int32
    [clip, fx, fy, n_frames, b1, b2, b3, prog_row]: fy = onset // hop + 1 the first frame wholly behind the onset in the score's render, fx the same of
    the performed onset, n_frames = min(DYNAMICS_FRAMES, max(1, (onset + length) // hop - onset // hop)), b_h = 5 (midi - 21) + the offset of partial
    h, -1 where that is no bin of [0, F), prog_row = the event's index + 1.  T is the clip's frame count: frames at or behind it stay in the table and
    do not count on the device, where also negative ones are dropped."""
    events = np.asarray(events, dtype=np.int64).reshape(-1, 3)
    heard = events[:, 0] if performed is None else np.floor(np.asarray(performed, dtype=np.float64).reshape(len(events))).astype(np.int64)
    hop, T, F = int(hop), int(T), int(F)
    if hop < 1 or T < 1 or F < 1:
        raise ValueError(f"resynth: note_rows needs hop, T, F >= 1 (got {hop}, {T}, {F})")
    out = np.zeros((len(events), 8), dtype=np.int32)
    out[:, 0] = clip
    out[:, 1] = heard // hop + 1
    out[:, 2] = events[:, 0] // hop + 1
    out[:, 3] = np.minimum(DYNAMICS_FRAMES, np.maximum(1, (events[:, 0] + events[:, 1]) // hop - events[:, 0] // hop))
    for h, off in enumerate(DYNAMICS_BIN_OFFSETS):
        b = 5 * (events[:, 2] - 21) + off
        out[:, 4 + h] = np.where((b >= 0) & (b < F), b, -1)
    out[:, 7] = np.arange(1, len(events) + 1)
    return out


def velocity(level_db):
    """MIDI velocity of a level in dB relative to the window's median note: 64 at 0 dB, 40 dB per decade of velocity, in 1 .. 127."""
    return int(min(127, max(1, np.rint(64.0 * 10.0 ** (float(level_db) / 40.0)))))


def estimate_dynamics(programs, x3, vqt, n_samples, rows, first, rounds=DYNAMICS_ROUNDS, y3=None):
    """The device loop of DESIGN.md section 26: programs (B, 1 + E, 8) int32 on the device with every amplitude RESYNTH_AMP (they are UPDATED IN
    PLACE), x3 the recording's features (B, T, F), rows / first the device tables of hip.note_table; y3: the features of the programs as they stand,
    where the caller has rendered them already (they save round 1 its render and VQT).  `rounds` times render -> VQT -> hip.note_levels ->
    hip.note_amp_update, with no host work and no read-back in between -> cum (S,) float32 on the device: every note's level in dB relative to its
    clip's median note, in LEVEL_DB_RANGE.
    The header's gain stays that of the first pack while the amplitudes move: the front end normalises the features to the window's peak, so a common
    factor on the waveform does not reach them (and the synthesiser itself does not clip)."""
    cum = torch.zeros(rows.shape[0], dtype=torch.float32, device=programs.device)
    sums = torch.zeros((rows.shape[0], 3), dtype=torch.float64, device=programs.device)
    for k in range(int(rounds)):
        if k or y3 is None:
            y = vqt(render.render(programs, n_samples))
            y3 = y[:, 0] if y.dim() == 4 else y
        hip.note_levels(x3, y3, rows, out=sums)
        hip.note_amp_update(sums, rows, first, cum, programs, RESYNTH_AMP)
    return cum


def event_rows(events, bar_lines, seg_of_bar, clip=0):
    """The event table of the retiming kernel (include/a2s.h: a2s_retime_events): events (n, 3) [onset, length, midi] in the order of their render
    program, bar_lines the window's lines in samples, seg_of_bar: per bar the row of the segment table that holds the bar's warp, or -1 (the bar was
    not aligned: its notes stay) -> (n, 8) int32 [clip, prog_row = index + 1, seg, bar_start, bar_stop, 0, 0, 0].  The bar of an event is the one its
    onset lies in (a note ON a bar line belongs to the bar that starts there), as in performed_onsets."""
    events = np.asarray(events, dtype=np.int64).reshape(-1, 3)
    lines = np.asarray([int(t) for t in bar_lines], dtype=np.int64)
    if len(lines) < 2 or len(seg_of_bar) != len(lines) - 1:
        raise ValueError(f"resynth: event_rows needs one segment (or -1) per bar: {len(lines) - 1} bars, {len(seg_of_bar)} entries")
    bar = np.clip(np.searchsorted(lines, events[:, 0], side="right") - 1, 0, len(lines) - 2)
    out = np.zeros((len(events), 8), dtype=np.int32)
    out[:, 0] = clip
    out[:, 1] = np.arange(1, len(events) + 1)
    out[:, 2] = np.asarray(seg_of_bar, dtype=np.int64)[bar] if len(events) else 0
    out[:, 3], out[:, 4] = lines[bar], lines[bar + 1]
    return out


def refine_timing(programs, x3, vqt, n_samples, hop, table, events, paths, steps, rounds=RETIME_ROUNDS):
    """The device loop of DESIGN.md section 28: programs (B, 1 + E, 8) int32 on the device (their onsets and lengths are UPDATED IN PLACE), x3 the
    recording's features (B, T, F), table the HOST segment table (S, 4) [clip, f0, f1, band] of the aligned bars, events the device table of
    hip.event_table over that table, paths / steps the device tensors of the alignment pass's hip.dtw_segments on these programs.  Round 1 turns those
    paths into warps (hip.path_warp) and moves every event through the warp of its bar (hip.retime_events); every later round renders the programs as
    they stand, -> VQT -> hip.segment_agreement -> the offsets (sum x - sum y) / cells with torch -> hip.dtw_segments -> warp -> retime, and moves the
    events from where they now stand.  No per-note or per-path host work and no read-back in between -> words 0 and 1 of every program row,
    (B, 1 + E, 2) int64 numpy: the one read-back."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 4)
    dev_table = torch.from_numpy(table.astype(np.int32)).to(programs.device)
    n_max = max(1, int((table[:, 2] - table[:, 1]).max())) if len(table) else 1
    cells = torch.from_numpy(((table[:, 2] - table[:, 1]) * x3.shape[2]).astype(np.float64)).to(programs.device)
    for k in range(int(rounds)):
        if k:
            y = vqt(render.render(programs, n_samples))
            y3 = (y[:, 0] if y.dim() == 4 else y).contiguous()
            sums = hip.segment_agreement(x3, y3, table)
            paths, steps, _ = hip.dtw_segments(x3, y3, table, ((sums[:, 0] - sums[:, 1]) / cells).to(torch.float32))
        warp2, _ = hip.path_warp(paths, steps, dev_table, n_max, inverse=False)
        hip.retime_events(warp2, dev_table, events, hop, programs)
    return programs[:, :, :2].cpu().numpy().astype(np.int64)


def resynthesise(windows, feats, vqt, hop, n_samples=None, align=False, dynamics=0, retime=0):
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
    list with one entry per bar, {"first_frame", "frames", "warp", "inverse", "total", "agreement_warped"} or None where the bar has no agreement.
    dynamics=K > 0 -> one more result, dynamics: per window None or {"level_db" (n,) float32 and "velocity" (n,) int64 per event,
    "agreement": per bar, ["agreement_warped": per bar, with align]}.  K rounds of estimate_dynamics set every note's amplitude from the recording
    (round 1 reads the unit-amplitude pass; the warp of align is that pass's too and is not recomputed), the levels are read back ONCE, and the
    programs are packed on the host and rendered once more with the final amplitudes, so that pack_program's gain rule keeps |wave| < 1: `waves`
    are then THAT render and dynamics' agreements are scored on it as "agreements" and "agreement_warped" are on the first.  With 0 nothing of this
    is allocated, launched or returned.
    retime=R > 0 (needs align, ValueError without) -> one more result behind alignments, retimed: per window None or {"events":
    (n, 3) int64, the window's events at the PERFORMED timing (same order, same pitches), "agreement": per bar the PLAIN agreement of the recording
    with the render of those events -- no gather and no warp}.  R rounds of refine_timing move the programs' onsets and lengths on the device, words 0
    and 1 are read back ONCE, the programs are packed on the host at the moved events (pack_program's gain rule follows the notes' new overlaps) and
    rendered: `waves` are then THAT render.  With dynamics=K as well, the dynamics rounds run on the retimed programs against the retimed render:
    a note is read at the same frames of both (fx = fy), the final pack holds the moved events at the estimated amplitudes, `waves` and dynamics'
    "agreement" are of that render, and dynamics' "agreement_warped" entries are None: the render is at the performed timing already, and the
    warp of the alignment pass does not belong to it.  "agreements" and alignments stay those of the first, straight pass.  With 0 nothing of this is
    allocated, launched or returned."""
    if retime and not align:
        raise ValueError("resynth: retime moves the notes through the warps of align=True: it needs align")
    if int(retime) < 0:
        raise ValueError(f"resynth: retime counts rounds: it must not be negative (got {retime!r})")
    f3 = feats[:, 0] if feats.dim() == 4 else feats
    W, T, F = f3.shape
    if len(windows) != W:
        raise ValueError(f"resynth: {len(windows)} windows but features of {W}")
    n_samples = (T - 1) * int(hop) if n_samples is None else int(n_samples)
    waves = [None] * W
    agreements = [[None] * (len(win["bar_lines"]) - 1) for win in windows]
    live = [w for w, win in enumerate(windows) if len(win["events"])]
    alignments = [[None] * len(a) for a in agreements] if align else None
    levels = [None] * W if dynamics else None
    retimed = [None] * W if retime else None
    result = lambda: (waves, agreements) + ((alignments,) if align else ()) + ((retimed,) if retime else ()) + ((levels,) if dynamics else ())
    if not live:
        return result()
    progs = torch.from_numpy(np.stack([program(windows[w]["events"], n_samples) for w in live])).to(f3.device)
    wave = render.render(progs, n_samples)
    y = vqt(wave)
    y3 = y[:, 0] if y.dim() == 4 else y
    if tuple(y3.shape[1:]) != (T, F):
        raise hip.A2SError(f"resynth: the resynthesis has features {tuple(y3.shape[1:])} per window, the recording {(T, F)}")
    seg, where = bar_segments([windows[w] for w in live], int(hop), T)
    x3 = f3[live].contiguous() if len(live) != W else f3
    sums = hip.segment_agreement(x3, y3, seg).cpu().numpy()
    for (i, b), row, s in zip(where, seg, sums):
        agreements[live[i]][b] = agreement(s, (int(row[2]) - int(row[1])) * F)
    heard = _align_bars(x3, y3, seg, where, sums, [live[i] for i, _ in where], agreements, alignments) if align else None
    if retime:
        wave, progs, y3, windows = _retime(windows, live, progs, x3.contiguous(), vqt, int(hop), n_samples, int(retime), seg, where, heard, retimed)
    if dynamics:
        wave = _dynamics(windows, live, progs, x3, y3, vqt, int(hop), n_samples, int(dynamics), seg, where, None if retime else alignments,
                         None if retime else heard, levels)
        for w in live if retime else ():
            levels[w]["agreement_warped"] = [None] * len(levels[w]["agreement"])
    host = wave.cpu().numpy()
    for i, w in enumerate(live):
        waves[w] = host[i]
    return result()


def performed_onsets(events, bar_lines, aligned, hop):
    """The onsets (samples, floats) at which the events (n, 3) of one window are heard: every note moved through the warp of its bar (aligned: the
    window's entry of resynthesise's alignments; a bar without one moves nothing)."""
    lines = [int(t) for t in bar_lines]
    out = []
    for ev in np.asarray(events, dtype=np.int64).reshape(-1, 3):
        b = min(max(int(np.searchsorted(lines, ev[0], side="right")) - 1, 0), len(lines) - 2)
        al = aligned[b]
        out.append(performed_notes([ev], None if al is None else al["warp"], 0 if al is None else al["first_frame"], hop, lines[b], lines[b + 1])[0][0])
    return np.array(out, dtype=np.float64)


def _dynamics(windows, live, progs, x3, y3, vqt, hop, n_samples, rounds, seg, where, alignments, heard, levels):
    """The dynamics=K half of resynthesise: fills `levels` for the live windows and returns the final render (len(live), n_samples) on the device."""
    _, T, F = x3.shape
    table = []
    for i, w in enumerate(live):
        ev = windows[w]["events"]
        table.append(note_rows(ev, None if alignments is None else performed_onsets(ev, windows[w]["bar_lines"], alignments[w], hop), hop, T, F, clip=i))
    first = np.concatenate([[0], np.cumsum([len(t) for t in table])])
    rows, first_d = hip.note_table(np.concatenate(table), first, len(live), progs.shape[1], x3.device)
    cum = estimate_dynamics(progs, x3.contiguous(), vqt, n_samples, rows, first_d, rounds, y3=y3).cpu().numpy()          # (the one read-back)
    final = []
    for i, w in enumerate(live):
        db = cum[first[i]:first[i + 1]]
        levels[w] = {"level_db": db, "velocity": np.array([velocity(v) for v in db], dtype=np.int64), "agreement": [None] * (len(windows[w]["bar_lines"]) - 1)}
        final.append(program(windows[w]["events"], n_samples, amps=RESYNTH_AMP * 10.0 ** (db.astype(np.float64) / 20.0)))
    wave = render.render(torch.from_numpy(np.stack(final)).to(x3.device), n_samples)
    z = vqt(wave)
    z3 = z[:, 0] if z.dim() == 4 else z
    sums = hip.segment_agreement(x3, z3, seg).cpu().numpy()
    for (i, b), row, s in zip(where, seg, sums):
        levels[live[i]]["agreement"][b] = agreement(s, (int(row[2]) - int(row[1])) * F)
    if alignments is not None:
        for w in live:
            levels[w]["agreement_warped"] = [None] * len(levels[w]["agreement"])
        if heard is not None:
            index, table4, at = heard[:3]
            z3 = z3.contiguous()
            warped = hip.segment_agreement(x3.contiguous(), z3[torch.arange(z3.shape[0], device=z3.device)[:, None], index], table4[:, :3]).cpu().numpy()
            for k, s, row in zip(at, warped, table4):
                levels[live[where[k][0]]]["agreement_warped"][where[k][1]] = agreement(s, int(row[2] - row[1]) * F)
    return wave


def _align_bars(x3, y3, seg, where, sums, window_of, agreements, alignments):
    """The align=True half of resynthesise: fills `alignments` for the bars of the table `seg` that have an agreement -> (index: (clips, T) the score
    frame heard at every recording frame, the aligned bars' table (S', 4), their rows of `seg`, (paths, steps) of the DTW as they lie on the device),
    or None where no bar has an agreement."""
    _, T, F = x3.shape
    x3, y3 = x3.contiguous(), y3.contiguous()          # (the gathered tensor below is contiguous, and both operands share one clip stride)
    rows = [k for k, ((_, b), w) in enumerate(zip(where, window_of)) if agreements[w][b] is not None]
    if not rows:
        return None
    table = np.array([[seg[k][0], seg[k][1], seg[k][2], dtw_band(seg[k][2] - seg[k][1])] for k in rows], dtype=np.int64)
    cells = (table[:, 2] - table[:, 1]) * F
    off = torch.from_numpy(((sums[rows, 0] - sums[rows, 1]) / cells).astype(np.float32)).to(x3.device)
    on_device = hip.dtw_segments(x3, y3, table, off)
    paths, steps, totals = (t.cpu().numpy() for t in on_device)
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
    return index, table, rows, on_device[:2]


def _retime(windows, live, progs, x3, vqt, hop, n_samples, rounds, seg, where, heard, retimed):
    """The retime=R half of resynthesise: fills `retimed` for the live windows -> (the render at the performed timing (len(live), n_samples) on the
    device, its programs on the device, its features, the windows with their events moved)."""
    F = x3.shape[2]
    moved = [np.array(windows[w]["events"], dtype=np.int64).reshape(-1, 3) for w in live]
    if heard is not None:
        _, table, at, (paths, steps) = heard
        seg_of = {where[k]: t for t, k in enumerate(at)}                        # (live window, bar) -> row of the aligned bars' table
        rows = [event_rows(moved[i], windows[w]["bar_lines"], [seg_of.get((i, b), -1) for b in range(len(windows[w]["bar_lines"]) - 1)], clip=i)
                for i, w in enumerate(live)]
        events = hip.event_table(np.concatenate(rows), len(live), progs.shape[1], table, x3.device)
        words = refine_timing(progs, x3, vqt, n_samples, hop, table, events, paths, steps, rounds)          # (the one read-back)
        for i, ev in enumerate(moved):
            ev[:, :2] = words[i, 1:1 + len(ev)]
    out = list(windows)
    for i, w in enumerate(live):
        out[w] = dict(windows[w], events=moved[i])
    progs = torch.from_numpy(np.stack([program(ev, n_samples) for ev in moved])).to(x3.device)
    wave = render.render(progs, n_samples)
    z = vqt(wave)
    z3 = z[:, 0] if z.dim() == 4 else z
    sums = hip.segment_agreement(x3, z3, seg).cpu().numpy()
    for i, w in enumerate(live):
        retimed[w] = {"events": moved[i], "agreement": [None] * (len(windows[w]["bar_lines"]) - 1)}
    for (i, b), row, s in zip(where, seg, sums):
        retimed[live[i]]["agreement"][b] = agreement(s, (int(row[2]) - int(row[1])) * F)
    return wave, progs, z3, out


def mean_agreement(values):
    """The mean of the entries that are not None; None where there is none."""
    got = [v for v in values if v is not None]
    return sum(got) / len(got) if got else None
