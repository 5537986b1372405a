"""The host side of the beat tracker (piano_a2s_amd/beats.py) with the device stages replaced by their definitions
(tests/beat_oracle.py): click trains with a known meter, degenerate inputs, the penalty table, the tiling of a recording, the window plan from tracked
downbeats and the command line's argument checks.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beat_oracle as bo  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = 200          # frames from either end inside which nothing is asked of the beats


def _train(n, clicks, meter, first_accent):
    """Envelopes of a click train: env_full 1 at every click, env_low 1 at every meter-th click from click first_accent on."""
    env_full, env_low = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    clicks = np.asarray(clicks)
    env_full[clicks] = 1.0
    accented = clicks[first_accent::meter]
    env_low[accented] = 1.0
    return env_full, env_low, clicks, accented


def _ramp_clicks(n, p0, p1, first):
    out, t = [], float(first)
    while t < n:
        out.append(int(round(t)))
        t += p0 + (p1 - p0) * t / n
    return out


CASES = {
    "120 bpm in four": dict(n=3000, clicks=list(range(30, 3000, 50)), meter=4, first_accent=1, period=50),
    "period 37 in three": dict(n=3000, clicks=list(range(11, 3000, 37)), meter=3, first_accent=2, period=37),
    "ramp 50 to 60 in four": dict(n=6000, clicks=_ramp_clicks(6000, 50.0, 60.0, 20), meter=4, first_accent=0, period=None),
    "period 150 in two": dict(n=4000, clicks=list(range(70, 4000, 150)), meter=2, first_accent=1, period=150),
}


@pytest.fixture(scope="module")
def tracked():
    """Every case tracked once: name -> (case, clicks, accented, result of beats.track)."""
    from piano_a2s_amd import beats
    out = {}
    for name, c in CASES.items():
        env_full, env_low, clicks, accented = _train(c["n"], c["clicks"], c["meter"], c["first_accent"])
        out[name] = (c, clicks, accented, beats.track(env_full, env_low, c["n"], bo.stages()))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_click_trains(tracked, name):
    c, clicks, accented, res = tracked[name]
    inner = lambda a: [int(t) for t in a if EDGE <= t <= c["n"] - 1 - EDGE]
    got = set(int(b) for b in res["beats"])
    assert len(inner(clicks)) >= 10
    missing = [t for t in inner(clicks) if t not in got]
    extra = [t for t in inner(res["beats"]) if t not in set(clicks.tolist())]
    assert not missing, f"clicks without a beat: {missing}"
    assert not extra, f"beats off the clicks: {extra}"
    assert res["beats_per_bar"] == c["meter"]
    assert inner(res["downbeats"]) == inner(accented)
    period = np.asarray(res["period_frames"])
    assert len(period) == -(-c["n"] // 100)
    if c["period"] is not None:
        assert (period == c["period"]).all(), period
    else:
        assert (np.diff(period) >= 0).all() and 49 <= period[0] <= 52 and 58 <= period[-1] <= 61, period
    assert np.all(np.diff(res["beats"]) > 0)


def test_double_time_folds_to_the_prior():
    """A 240 beats-per-minute train (period 25): the prior pulls the period to 50; every beat still lies on a click."""
    from piano_a2s_amd import beats
    env_full, env_low, clicks, _ = _train(3000, list(range(5, 3000, 25)), 4, 0)
    res = beats.track(env_full, env_low, 3000, bo.stages())
    assert (np.asarray(res["period_frames"]) == 50).all()
    inner = [int(b) for b in res["beats"] if EDGE <= b <= 3000 - EDGE]
    assert inner and set(inner) <= set(clicks.tolist()) and (np.diff(inner) == 50).all()


def test_forced_meter():
    from piano_a2s_amd import beats
    c = CASES["120 bpm in four"]
    env_full, env_low, clicks, accented = _train(c["n"], c["clicks"], c["meter"], c["first_accent"])
    res = beats.track(env_full, env_low, c["n"], bo.stages(), beats_per_bar=2)
    assert res["beats_per_bar"] == 2
    inner = [int(t) for t in res["downbeats"] if EDGE <= t <= c["n"] - EDGE]
    assert set(int(t) for t in accented if EDGE <= t <= c["n"] - EDGE) <= set(inner) and (np.diff(inner) == 100).all()
    with pytest.raises(ValueError):
        beats.downbeats([1, 2], env_low, env_full, beats_per_bar=5)


# ------------------------------------------------------------------------------------------- degenerate inputs
def test_tempo_path_degenerate():
    from piano_a2s_amd import beats
    assert beats.tempo_path(np.zeros((0, 181))).shape == (0,)
    assert beats.tempo_path(np.zeros((3, 181))).tolist() == [50, 50, 50]                # nothing but the prior
    assert beats.tempo_path(np.full((2, 181), np.nan)).tolist() == [50, 50]
    assert beats.tempo_path(np.zeros((2, 11)), lag_min=60).tolist() == [60, 60]          # the prior's centre lies outside: the nearest lag
    one = np.zeros((1, 181))
    one[0, 77 - 20] = 1.0
    assert beats.tempo_path(one).tolist() == [77]
    # a single block that disagrees with its neighbours does not move the path
    A = np.zeros((5, 181))
    A[:, 40 - 20] = 0.8
    A[2, 40 - 20], A[2, 120 - 20] = 0.0, 0.9
    assert beats.tempo_path(A).tolist() == [40] * 5
    with pytest.raises(ValueError):
        beats.tempo_path(np.zeros(5))
    with pytest.raises(ValueError):
        beats.tempo_path(np.zeros((2, 4)), lag_min=0)


def test_downbeats_degenerate():
    from piano_a2s_amd import beats
    env = np.zeros(100)
    none = beats.downbeats([], env, env)
    assert none["downbeats"].tolist() == [] and none["beats_per_bar"] == 4 and none["positions"].tolist() == []
    one = beats.downbeats([40], env, env)
    assert one["downbeats"].tolist() == [40] and one["beats_per_bar"] == 4
    flat = beats.downbeats([10, 20, 30, 40, 50, 60, 70, 80], env, env)                  # all accents equal: every meter ties, the largest wins
    assert flat["beats_per_bar"] == 4 and flat["downbeats"].tolist() == [40, 80] and flat["contrast"] == 0.0          # (equal paths: the last beat at 0)
    assert beats.downbeats([10, 20, 30, 40, 50, 60], env, env, beats_per_bar=3)["downbeats"].tolist() == [30, 60]
    # a beat at the very edge of the envelope
    assert beats.downbeats([0, 99], env, env)["positions"].tolist() == [3, 0]


def test_slips():
    """One missing beat in a bar of three: the path repeats or skips a position once and stays on the accents."""
    from piano_a2s_amd import beats
    a = np.tile([2.0, 0.0, 0.0], 12)
    a = np.delete(a, 16)                                                                # (a weak beat of the sixth bar is missing)
    a = (a - a.mean()) / a.std()
    pos, contrast = beats.bar_positions(a, 3, slip=4.0)
    assert (pos[a > 0] == 0).all() and (pos[a < 0] != 0).all()
    stiff, _ = beats.bar_positions(a, 3, slip=1e9)
    assert ((stiff[1:] - stiff[:-1]) % 3 == 1).all() and not (stiff[a > 0] == 0).all()


def test_all_zero_envelope_and_short_recordings():
    from piano_a2s_amd import beats
    for n in (0, 1, 9, 500):
        res = beats.track(np.zeros(n), np.zeros(n), n, bo.stages())
        assert len(res["period_frames"]) == max(1, -(-n // 100)) and set(res["period_frames"].tolist()) == {50}
        assert len(res["beats"]) == (0 if n == 0 else 1)                                # nothing to follow: the last beat alone
        assert res["beats_per_bar"] == 4 and len(res["downbeats"]) == len(res["beats"])
    with pytest.raises(ValueError):
        beats.track(np.zeros(5), np.zeros(5), 6, bo.stages())


# ------------------------------------------------------------------------------------------- the penalty table
def test_penalty_table():
    from piano_a2s_amd import beats
    pen = beats.penalty_table()
    assert pen.dtype == np.float32 and pen.shape == (181, 401)
    for tau in (20, 21, 50, 199, 200):
        row = pen[tau - 20]
        lo, hi = (tau + 1) // 2, 2 * tau
        assert row[tau] == 0.0 and (row[:lo] == 0).all() and (row[hi + 1:] == 0).all()
        d = np.arange(lo, hi + 1)
        want = (100.0 * np.log(d / float(tau)) ** 2).astype(np.float32)
        assert np.array_equal(row[lo:hi + 1], want)
        assert (np.diff(row[lo:tau + 1]) < 0).all() and (np.diff(row[tau:hi + 1]) > 0).all()
    assert abs(float(pen[50 - 20, 100]) - 100.0 * np.log(2.0) ** 2) < 1e-5 and abs(float(pen[50 - 20, 25]) - float(pen[50 - 20, 100])) < 1e-5
    small = beats.penalty_table(3, 5, 2.0)
    assert small.shape == (3, 11) and small[0, 2] == np.float32(2.0 * np.log(2.0 / 3.0) ** 2) and small[0, 1] == 0
    with pytest.raises(ValueError):
        beats.penalty_table(0, 5)
    with pytest.raises(ValueError):
        beats.penalty_table(6, 5)


def test_oracle_dp_small_by_hand():
    """Two impulses a period apart: the second links to the first at no price."""
    from piano_a2s_amd import beats
    ls = np.zeros((1, 12), dtype=np.float32)
    ls[0, [2, 6]] = 1.0
    S, back, bt, count = bo.beat_dp(ls, np.array([[4]], dtype=np.int32), beats.penalty_table(2, 4, 1.0), [12], 100, 2, 8)
    assert S[0, 2] == 1.0 and S[0, 6] == 2.0 and back[0, 6] == 2 and back[0, 2] == -1
    assert back[0, 10] == 6 and count[0] == 3 and bt[0, :3].tolist() == [2, 6, 10] and bt[0, 3] == -1


# ------------------------------------------------------------------------------------------- tiling of a recording
@pytest.mark.parametrize("n_frames,T,margin", [(0, 1201, 8), (1, 1201, 8), (1201, 1201, 8), (1202, 1201, 8), (2386, 1201, 8), (2387, 1201, 8), (60001, 1201, 8),
                                               (100, 20, 3), (101, 20, 0)])
def test_tile_plan(n_frames, T, margin):
    from piano_a2s_amd import beats
    starts, owner = beats.tile_plan(n_frames, T, margin)
    step = T - 2 * margin
    assert starts.tolist() == [w * step for w in range(len(starts))] and len(owner) == n_frames
    assert len(starts) == 1 or starts[-2] + T < n_frames <= starts[-1] + T, "as many windows as cover the recording, and no more"
    if n_frames:
        local = np.arange(n_frames) - starts[owner]
        assert (local >= 0).all() and (local < T).all() and (np.diff(owner) >= 0).all() and owner[0] == 0 and owner[-1] == len(starts) - 1
        left, right = local, T - 1 - local
        assert (left[owner > 0] >= margin).all(), "a frame is taken at least `margin` frames behind its window's start, but in the first window"
        assert (right[owner < len(starts) - 1] >= margin).all(), "... and at least `margin` frames before its end, but in the last window"
        for g in range(n_frames):                                                       # no other window holds the frame farther from its edges
            for w in range(len(starts)):
                lw = g - starts[w]
                if w != owner[g] and 0 <= lw < T:
                    here = min(left[g] if owner[g] > 0 else T, right[g] if owner[g] < len(starts) - 1 else T)
                    there = min(lw if w > 0 else T, T - 1 - lw if w < len(starts) - 1 else T)
                    assert here >= there, (g, w)


def test_tile_plan_refusals():
    from piano_a2s_amd import beats
    for args in ((-1, 20, 3), (10, 6, 3), (10, 20, -1)):
        with pytest.raises(ValueError):
            beats.tile_plan(*args)


# ------------------------------------------------------------------------------------------- the window plan from tracked downbeats
def test_plan_windows_from_tracked_downbeats(tracked):
    from piano_a2s_amd import audio
    c, clicks, accented, res = tracked["120 bpm in four"]
    downbeats_s = [float(f) * 160 / 16000 for f in res["downbeats"]]
    inner = [t for t in downbeats_s if EDGE / 100 <= t <= (c["n"] - EDGE) / 100]
    plan = audio.plan_windows(c["n"] * 160, 16000, inner, max_bars=5, max_samples=192000)
    assert plan and all(n_bars <= 5 and stop - start <= 192000 for start, stop, n_bars in plan)
    assert [p[0] for p in plan] == [int(round(t * 16000)) for t in inner[0::5]][:len(plan)]
    assert all((stop - start) == n_bars * 2 * 16000 for start, stop, n_bars in plan), "bars of four beats at 120 beats per minute last 2 s"
    assert sum(p[2] for p in plan) == len(inner) - 1


# ------------------------------------------------------------------------------------------- the command line
def _cli(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "transcribe.py")] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_command_line_argument_checks(tmp_path):
    hp = os.path.join(ROOT, "hparams", "finetune.yaml")
    base = [hp, "a.wav", "--checkpoint", str(tmp_path / "none.pt")]
    r = _cli(*base, "--track_downbeats", "--downbeats", "x.txt")
    assert r.returncode == 2 and "not allowed with" in r.stderr
    r = _cli(*base, "--beats_per_bar", "3")
    assert r.returncode == 2 and "--beats_per_bar" in r.stderr and "--track_downbeats" in r.stderr
    r = _cli(*base, "--track_downbeats", "--beats_per_bar", "5")
    assert r.returncode == 2 and "invalid choice" in r.stderr
    r = _cli(*base, "--track_downbeats", "--beats_per_bar", "3")                       # the arguments pass: the checkpoint is what is missing
    assert r.returncode != 2 and "no checkpoint" in r.stderr
    r = _cli("--help")
    assert r.returncode == 0 and "--track_downbeats" in r.stdout and "--beats_per_bar" in r.stdout


def test_transcribe_refuses_an_unknown_downbeats_word():
    from piano_a2s_amd import transcribe
    with pytest.raises(ValueError):
        transcribe.check_downbeats("follow", None)
    with pytest.raises(ValueError):
        transcribe.check_downbeats([1.0, 2.0], 3)
    with pytest.raises(ValueError):
        transcribe.check_downbeats("track", 5)
    assert transcribe.check_downbeats("track", 3) is None and transcribe.check_downbeats(None, None) is None
