"""Beats and downbeats of a recording from the model's own VQT features, so that a recording without an annotation can be cut
into the bar-aligned clips the model was trained on.

The heavy stages run on the device (csrc/a2s_beat.hip, through the wrappers of hip.py): the onset strength of every feature row, the tempogram (a
blockwise normalised autocorrelation) and the beat dynamic programme.  The small decisions between and behind them are the pure numpy of this module, in
float64, and are their own definition: the tempo path over the blocks, the penalty table, the bar position of every beat.

`track` takes the device stages as a parameter (`Stages`): the product passes `hip_stages(device)`, the CPU tests pass the definitions of
tests/beat_oracle.py.  There is no CPU implementation of the stages in the product."""
import collections
import math

import numpy as np

WIN, HOP_B, LAG_MIN, LAG_MAX = 800, 100, 20, 200          # tempogram: window and hop of a block in frames; periods of 300 .. 30 beats per minute at 100 frames/s
LAMBDA = 100.0                                            # beat DP: the price of a beat interval d at the period tau is LAMBDA ln(d / tau)^2
PRIOR_CENTRE, PRIOR_OCTAVES, PRIOR_WEIGHT = 50.0, 1.0, 0.1          # tempo path: a weak log-normal prior on the period (120 beats per minute, one octave wide)
TRANSITION_WEIGHT = 20.0                                  # tempo path: -TRANSITION_WEIGHT log2(l / l')^2 between neighbouring blocks
SLIP = 4.0                                                # downbeats: the price of a repeated or skipped bar position, in standard deviations of the accents
ACCENT_REACH = 2                                          # downbeats: an accent is the largest envelope value within +- this many frames of the beat
ONSET_LAG, F_SPLIT = 1, 180                               # onset strength: difference over one frame; env_low sums the three lowest octaves (60 bins each)
MARGIN = 8                                                # track_recording: frames of overlap on either side of a window (the longest VQT filter: 4.9 hops)
METERS = (2, 3, 4)
TIE = 1e-9                                                # two meters whose contrasts differ by less (relative) are equal: the larger one wins

# the device stages: numpy in, numpy out (onset_strength also takes the features as a device tensor)
#   onset_strength(x (B, rows, F), n_rows (B,), lag, f_split)              -> (env_full, env_low), (B, rows) each
#   tempogram(env (R, stride), n (R,), win, hop_b, lag_min, lag_max, J)     -> (R, J, lag_max - lag_min + 1)
#   beat_dp(ls (R, stride), period (R, J), pen, n (R,), hop_b, lag_min, max_beats) -> (S, back, beats (R, max_beats), count (R,))
Stages = collections.namedtuple("Stages", "onset_strength tempogram beat_dp")


def hip_stages(device):
    """The three stages on the device (hip.onset_strength, hip.tempogram, hip.beat_dp): uploads the small host arrays, reads the small results back."""
    import torch

    from . import hip
    dev = torch.device(device)

    def up(a, dtype):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)

    def onset_strength(x, n_rows, lag, f_split):
        x = x.to(dev) if torch.is_tensor(x) else up(x, torch.float32)
        ef, el = hip.onset_strength(x, up(n_rows, torch.int32), lag, f_split)
        return ef.cpu().numpy(), el.cpu().numpy()

    def tempogram(env, n, win, hop_b, lag_min, lag_max, J):
        return hip.tempogram(up(env, torch.float32), up(n, torch.int32), win, hop_b, lag_min, lag_max, J=J).cpu().numpy()

    def beat_dp(ls, period, pen, n, hop_b, lag_min, max_beats):
        out = hip.beat_dp(up(ls, torch.float32), up(period, torch.int32), up(pen, torch.float32), up(n, torch.int32), hop_b, lag_min, max_beats)
        return tuple(t.cpu().numpy() for t in out)

    return Stages(onset_strength, tempogram, beat_dp)


# ------------------------------------------------------------------------------------------- the penalty table
def penalty_table(lag_min=LAG_MIN, lag_max=LAG_MAX, lam=LAMBDA):
    """pen (lag_max - lag_min + 1, 2 lag_max + 1) float32: pen[tau - lag_min][d] = lam ln(d / tau)^2 for d in [ceil(tau / 2), 2 tau], the beat intervals
    the dynamic programme tries at the period tau, computed in float64 and rounded once; 0 elsewhere (never read)."""
    lag_min, lag_max = int(lag_min), int(lag_max)
    if not 1 <= lag_min <= lag_max:
        raise ValueError(f"penalty_table: needs 1 <= lag_min <= lag_max (got {lag_min}, {lag_max})")
    pen = np.zeros((lag_max - lag_min + 1, 2 * lag_max + 1), dtype=np.float64)
    for tau in range(lag_min, lag_max + 1):
        d = np.arange((tau + 1) // 2, 2 * tau + 1)
        pen[tau - lag_min, d] = float(lam) * np.log(d / float(tau)) ** 2
    return pen.astype(np.float32)


# ------------------------------------------------------------------------------------------- the tempo path
def tempo_path(tempogram, lag_min=LAG_MIN, centre=PRIOR_CENTRE, octaves=PRIOR_OCTAVES, prior_weight=PRIOR_WEIGHT, transition_weight=TRANSITION_WEIGHT):
    """tempogram (J, lags) -> one period per block, (J,) int64: the Viterbi path that maximises sum_j (A_j[l_j] + prior(l_j)) + sum_j trans(l_{j-1}, l_j),
    prior(l) = -prior_weight / 2 (log2(l / centre) / octaves)^2, trans(l', l) = -transition_weight log2(l / l')^2.  Among equal paths the one with the
    smaller lags wins (first arg max); a value that is not finite counts as 0.  No blocks: an empty path."""
    A = np.nan_to_num(np.asarray(tempogram, dtype=np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    if A.ndim != 2:
        raise ValueError(f"tempo_path: the tempogram must be (blocks, lags) (got {A.shape})")
    if int(lag_min) < 1:
        raise ValueError(f"tempo_path: needs lag_min >= 1 (got {lag_min})")
    J, nl = A.shape
    if J == 0 or nl == 0:
        return np.zeros((0,), dtype=np.int64)
    lags = int(lag_min) + np.arange(nl, dtype=np.float64)
    prior = -0.5 * float(prior_weight) * (np.log2(lags / float(centre)) / float(octaves)) ** 2
    trans = -float(transition_weight) * np.log2(lags[None, :] / lags[:, None]) ** 2          # [l', l]
    score = A[0] + prior
    ptr = np.zeros((J, nl), dtype=np.int64)
    for j in range(1, J):
        cand = score[:, None] + trans
        ptr[j] = cand.argmax(axis=0)
        score = cand[ptr[j], np.arange(nl)] + A[j] + prior
    path = np.zeros((J,), dtype=np.int64)
    path[-1] = int(score.argmax())
    for j in range(J - 1, 0, -1):
        path[j - 1] = ptr[j, path[j]]
    return path + int(lag_min)


# ------------------------------------------------------------------------------------------- downbeats
def accents(beats, env_low, env_full, reach=ACCENT_REACH):
    """Per beat the largest env_low plus the largest env_full within +- reach frames, z-scored over the beats (all 0 where they do not vary)."""
    beats = np.asarray(beats, dtype=np.int64).reshape(-1)
    lo_env, full_env = np.asarray(env_low, dtype=np.float64).reshape(-1), np.asarray(env_full, dtype=np.float64).reshape(-1)
    a = np.zeros((len(beats),), dtype=np.float64)
    for i, b in enumerate(beats):
        for env in (lo_env, full_env):
            seg = env[max(int(b) - reach, 0):max(int(b) + reach + 1, 0)]
            a[i] += seg.max() if len(seg) else 0.0
    if len(a) == 0:
        return a
    sd = a.std()
    return (a - a.mean()) / sd if sd > 0 and np.isfinite(sd) else np.zeros_like(a)


def bar_positions(accent, m, slip=SLIP):
    """The bar position j_i in [0, m) of every beat that maximises sum_i r(i, j_i) - slip * (steps that are not j -> j + 1 mod m), with the reward
    r(i, 0) = accent[i] and r(i, j) = -accent[i] / (m - 1) elsewhere (the accent on the downbeat minus the mean accent on the other beats).  A step may
    repeat a position or skip one, each at the price `slip`.  Among equal paths: the regular step before the repeat before the skip, the smaller last
    position.  -> (positions (N,) int64, the path's score / N: the contrast per beat)."""
    a = np.asarray(accent, dtype=np.float64)
    N, m = len(a), int(m)
    if N == 0:
        return np.zeros((0,), dtype=np.int64), 0.0
    reward = np.where(np.arange(m)[None, :] == 0, a[:, None], -a[:, None] / (m - 1))
    back_by = np.array([1, 0, 2])
    score = reward[0].copy()
    ptr = np.zeros((N, m), dtype=np.int64)
    cols = np.arange(m)
    for i in range(1, N):
        cand = np.stack([np.roll(score, 1), score - slip, np.roll(score, 2) - slip])
        k = cand.argmax(axis=0)
        ptr[i] = (cols - back_by[k]) % m
        score = cand[k, cols] + reward[i]
    pos = np.zeros((N,), dtype=np.int64)
    pos[-1] = int(score.argmax())
    for i in range(N - 1, 0, -1):
        pos[i - 1] = ptr[i, pos[i]]
    return pos, float(score.max()) / N


def downbeats(beats, env_low, env_full, beats_per_bar=None, slip=SLIP):
    """beats (frames, ascending) and the two envelopes -> {"downbeats": the beats at bar position 0, "beats_per_bar": m, "positions": the bar position of
    every beat, "contrast": the winning path's score per bar}.  m is beats_per_bar where given, else the meter of METERS with the largest contrast per
    BAR, m times the path's score per beat: with N / m downbeats and N (m - 1) / m other beats that is the mean accent on the downbeats minus the mean
    accent elsewhere.  (Per beat a bar of four would score exactly what two bars of two score, since z-scored accents sum to zero: the choice would
    hang on rounding and on the beats at the recording's ends.)  Contrasts within TIE (relative) are equal, and the larger meter wins."""
    beats = np.asarray(beats, dtype=np.int64).reshape(-1)
    if beats_per_bar is not None and int(beats_per_bar) not in METERS:
        raise ValueError(f"downbeats: beats_per_bar must be one of {METERS} (got {beats_per_bar!r})")
    a = accents(beats, env_low, env_full)
    best = None
    for m in (METERS if beats_per_bar is None else (int(beats_per_bar),)):
        pos, per_beat = bar_positions(a, m, slip)
        contrast = per_beat * m
        if best is None or contrast >= best[2] - TIE * max(1.0, abs(best[2])):
            best = (m, pos, max(contrast, best[2]) if best is not None else contrast)
    m, pos, contrast = best
    return {"downbeats": beats[pos == 0], "beats_per_bar": m, "positions": pos, "contrast": contrast}


# ------------------------------------------------------------------------------------------- everything behind the envelopes
def track(env_full, env_low, n, stages, beats_per_bar=None, *, win=WIN, hop_b=HOP_B, lag_min=LAG_MIN, lag_max=LAG_MAX, lam=LAMBDA, slip=SLIP):
    """The envelopes of one recording (1-D, at least n frames) -> {"beats", "downbeats" (frames, int64 arrays), "beats_per_bar", "period_frames" (one
    period per block of hop_b frames)}: tempogram (device) -> tempo_path -> the envelope over its standard deviation and the penalty table -> beat
    dynamic programme (device) -> downbeats."""
    n = int(n)
    env_full = np.asarray(env_full, dtype=np.float32).reshape(-1)
    env_low = np.asarray(env_low, dtype=np.float32).reshape(-1)
    if n < 0 or n > len(env_full) or n > len(env_low):
        raise ValueError(f"track: n = {n} frames, the envelopes hold {len(env_full)} and {len(env_low)}")
    env = np.zeros((1, max(n, 1)), dtype=np.float32)
    env[0, :n] = env_full[:n]
    count_of = np.array([n], dtype=np.int32)
    J = max(1, -(-n // int(hop_b)))
    tg = np.asarray(stages.tempogram(env, count_of, int(win), int(hop_b), int(lag_min), int(lag_max), J))[0]
    period = tempo_path(tg, lag_min)
    sd = float(env[0, :n].astype(np.float64).std()) if n else 0.0
    ls = (env.astype(np.float64) / sd).astype(np.float32) if sd > 0 and math.isfinite(sd) else np.zeros_like(env)
    max_beats = env.shape[1] // ((int(lag_min) + 1) // 2) + 1          # beats lie at least ceil(lag_min / 2) frames apart
    S, back, beats, count = stages.beat_dp(ls, period[None].astype(np.int32), penalty_table(lag_min, lag_max, lam), count_of, int(hop_b), int(lag_min),
                                           max_beats)
    count = int(np.asarray(count).reshape(-1)[0])
    if count > max_beats:
        raise ValueError(f"track: {count} beats, room for {max_beats}")
    beats = np.asarray(beats).reshape(1, -1)[0, :count].astype(np.int64)
    db = downbeats(beats, env_low[:n], env_full[:n], beats_per_bar, slip)
    return {"beats": beats, "downbeats": db["downbeats"], "beats_per_bar": db["beats_per_bar"], "period_frames": period}


# ------------------------------------------------------------------------------------------- a recording
def tile_plan(n_frames, window_frames, margin=MARGIN):
    """The overlapping windows a recording of n_frames feature frames is tiled into and the window every frame's envelope value is taken from:
    (starts (W,) int64: window w holds the frames [starts[w], starts[w] + window_frames); owner (n_frames,) int64).  Neighbouring windows overlap by
    2 * margin frames; a frame in the overlap belongs to the window in which it lies farther from an edge, so it is at least `margin` frames from the
    edge of its window unless that edge is the recording's own start or end."""
    n_frames, T, margin = int(n_frames), int(window_frames), int(margin)
    step = T - 2 * margin
    if n_frames < 0 or margin < 0 or step < 1:
        raise ValueError(f"tile_plan: needs n_frames >= 0, margin >= 0 and window_frames > 2 * margin (got {n_frames}, {margin}, {T})")
    W = 1 if n_frames <= T else 1 + -(-(n_frames - T) // step)
    starts = np.arange(W, dtype=np.int64) * step
    owner = np.clip((np.arange(n_frames, dtype=np.int64) - margin) // step, 0, W - 1)
    return starts, owner


def track_recording(wave16k, hparams, stages=None, beats_per_bar=None, margin=MARGIN, lag=ONSET_LAG, f_split=F_SPLIT):
    """wave16k (N,) float32 on the device at the hparams' sample rate -> {"beats_s", "downbeats_s" (seconds, lists), "beats_per_bar", "period_frames"}.
    The recording is tiled into windows of max_frame_num frames (tile_plan), the VQT runs on all windows at once, the onset strength on all their rows;
    every frame takes its envelope values from its owner window (a window's features are relative to its own peak, which a difference along time
    does not see), and `track` does the rest."""
    import torch

    from . import transcribe
    if not torch.is_tensor(wave16k) or wave16k.dim() != 1 or not wave16k.is_cuda:
        raise ValueError("track_recording: wave16k must be a 1-D tensor on the device")
    if margin < lag:
        raise ValueError(f"track_recording: the margin ({margin}) must cover the onset lag ({lag})")
    hp = transcribe._hp
    hop, T, rate = int(hp(hparams, "hop_length", 160)), int(hp(hparams, "max_frame_num", 1201)), int(hp(hparams, "sample_rate", 16000))
    stages = hip_stages(wave16k.device) if stages is None else stages
    N = int(wave16k.shape[0])
    n_frames = 1 + N // hop if N else 0
    if n_frames == 0:
        return {"beats_s": [], "downbeats_s": [], "beats_per_bar": int(beats_per_bar) if beats_per_bar is not None else METERS[-1], "period_frames": []}
    starts, owner = tile_plan(n_frames, T, margin)
    length = (T - 1) * hop
    windows = torch.zeros((len(starts), length), dtype=torch.float32, device=wave16k.device)
    for w, f0 in enumerate(starts.tolist()):
        piece = wave16k[f0 * hop:f0 * hop + length]
        windows[w, :piece.shape[0]] = piece
    feats = transcribe._vqt(wave16k.device, hparams)(windows)                 # (W, 1, T, F)
    n_rows = np.minimum(T, n_frames - starts).astype(np.int32)
    ef, el = stages.onset_strength(feats, n_rows, int(lag), min(int(f_split), int(feats.shape[-1])))
    local = np.arange(n_frames, dtype=np.int64) - starts[owner]
    env_full, env_low = np.asarray(ef)[owner, local], np.asarray(el)[owner, local]
    out = track(env_full, env_low, n_frames, stages, beats_per_bar)
    to_s = lambda frames: [float(f) * hop / rate for f in frames]
    return {"beats_s": to_s(out["beats"]), "downbeats_s": to_s(out["downbeats"]), "beats_per_bar": int(out["beats_per_bar"]),
            "period_frames": [int(p) for p in out["period_frames"]]}
