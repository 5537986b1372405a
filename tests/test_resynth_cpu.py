"""Resynthesis of a decoded score, host side (piano_a2s_amd/resynth.py, audio.plan_bar_lines), without a GPU: the event round
trip through the tokens, the squeeze rule, lenient rows, truncation, the bar lines of a window plan, the correlation formula, and -- on the float64
chain tests/render_oracle.py -> oracle/vqt_ref.py -- that the agreement as defined puts a clip's own score above another clip's in every bar."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import vqt_ref
from piano_a2s_amd import audio, metrics, resynth, scoregen, spec
from tests import render_oracle, resynth_oracle

SIGS = scoregen.time_signatures()
LABELS = scoregen._LABELS


def _lines(clip, bars):
    bar_q = Fraction(scoregen._BAR_UNITS[clip["time_sig"]], 4)
    lines = [clip["lead"] + b * bar_q * clip["spq"] for b in range(bars + 1)]
    assert all(t.denominator == 1 for t in lines)
    return [int(t) for t in lines]


def _multiset(ev):
    return sorted((int(o), int(n), int(m)) for o, n, m in ev)


# ------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("ts", range(len(SIGS)))
def test_round_trip_of_the_generators_events(ts):
    cfg = spec.default_cfg()
    for s in range(6):
        clip = scoregen.make_clip(cfg, 1000 + 10 * ts + s, frames=1201, time_sig=ts)
        lines = _lines(clip, cfg["max_bars"])
        ev, truncated = resynth.score_events(clip["ids"]["upper"], clip["ids"]["lower"], [clip["time_sig"]] * cfg["max_bars"], lines)
        assert not truncated
        assert _multiset(ev) == _multiset(clip["events"]), (ts, s)
        assert ev.dtype == np.int64 and ev.shape == (len(clip["events"]), 3)
        assert np.all(np.diff(ev[:, 0]) >= 0), "in onset order, as a render program wants them"


# ------------------------------------------------------------------------------------------- squeeze rule
def test_an_overfull_bar_is_squeezed_into_its_bar():
    W = metrics.NOTE_W
    ticks = resynth.bar_ticks("2/4")
    assert ticks == W // 2
    row = LABELS.encode("1c\n4d")                                   # a whole note, then a quarter: 5/4 in a 2/4 bar
    notes, overflow = resynth.bar_events(row, ticks)
    assert not overflow
    assert notes == [(Fraction(0), Fraction(4, 5), 60), (Fraction(4, 5), Fraction(1, 5), 62)]
    ev, _ = resynth.score_events([row, LABELS.encode("4e")], [[], []], ["2/4", "2/4"], [100, 1100, 2100])
    first = ev[ev[:, 0] < 1100]
    assert _multiset(first) == [(100, 800, 60), (900, 200, 62)]
    assert np.all(ev[:, 0] + ev[:, 1] <= np.where(ev[:, 0] < 1100, 1100, 2100)), "nothing crosses its bar line"
    assert _multiset(ev[ev[:, 0] >= 1100]) == [(1100, 500, 64)], "a bar that is too short keeps its silence at the end"
    # a span of one sample still gives a note of one sample inside the bar
    ev, _ = resynth.score_events([row], [[]], ["2/4"], [7, 8])
    assert _multiset(ev) == [(7, 1, 60), (7, 1, 62)]


# ------------------------------------------------------------------------------------------- lenient rows
def test_lenient_rows():
    pad = LABELS.labels_map["<pad>"]
    ticks = resynth.bar_ticks("4/4")
    assert resynth.bar_events([], ticks) == ([], False)
    assert resynth.bar_events([pad] * 9, ticks) == ([], False)
    rest = LABELS.encode("1r")
    assert resynth.bar_events(rest, ticks) == ([], False)
    malformed = [LABELS.labels_map["c"], LABELS.labels_map["4"], LABELS.labels_map["\n"], 10 ** 6, -3] + LABELS.encode("8.e")
    want, overflow = metrics.note_events(malformed)
    got, got_overflow = resynth.bar_events(malformed, ticks)
    assert overflow == got_overflow
    assert [(o * ticks, n * ticks, m) for o, n, m in got] == [(on, dur, midi) for on, midi, dur, _ in want]
    ev, truncated = resynth.score_events([[], malformed], [[pad], rest], ["4/4", "3/8"], [0, 16000, 20000])
    assert not truncated and len(ev) == len(want)
    with pytest.raises(ValueError):
        resynth.score_events([[]], [[]], ["4/4"], [5, 5])
    with pytest.raises(ValueError):
        resynth.score_events([[]], [[]], ["4/4"], [0, 10, 20])


# ------------------------------------------------------------------------------------------- truncation
def test_truncation_keeps_the_earliest_and_says_so():
    row = LABELS.encode("\n".join(["16c 16e 16g"] * 16))            # 48 notes per bar and staff
    bars = 6
    ev, truncated = resynth.score_events([row] * bars, [row] * bars, ["4/4"] * bars, [1600 * b for b in range(bars + 1)])
    assert truncated and len(ev) == scoregen.MAX_EVENTS
    full, t2 = resynth.score_events([row] * bars, [row] * bars, ["4/4"] * bars, [1600 * b for b in range(bars + 1)], max_events=10 ** 6)
    assert not t2 and len(full) == 2 * 48 * bars
    assert np.array_equal(ev, full[:scoregen.MAX_EVENTS])
    p = resynth.program(ev, 9600)
    assert p.shape == (1 + scoregen.MAX_EVENTS, 8) and p[0, 1] == scoregen.MAX_EVENTS
    hd = render_oracle.header(p)
    assert hd["noise_level"] == 0.0 and hd["attack"] == resynth.RESYNTH_INSTRUMENT["attack"] and hd["n_samples"] == 9600


# ------------------------------------------------------------------------------------------- bar lines of a plan
PLANS = [
    ("plain", 16000 * 40, [0.5 + 2.0 * i for i in range(13)], {}),
    ("a repeated time", 16000 * 30, [1.0, 3.0, 3.0, 5.0, 7.5, 7.5, 7.5, 9.0, 12.0], {}),
    ("beyond the end", 16000 * 10, [1.0, 4.0, 8.0, 12.0, 16.0], {}),
    ("a group longer than the window", 16000 * 40, [0.0, 4.0, 8.0, 12.5, 16.0, 20.0, 24.0], {}),
    ("one bar longer than the window", 16000 * 40, [1.0, 15.0, 17.0, 19.0], {}),
    ("max_bars 1", 16000 * 20, [0.25 + 1.5 * i for i in range(9)], {"max_bars": 1}),
    ("a short window", 16000 * 20, [0.25 + 1.5 * i for i in range(9)], {"window_seconds": 4.0}),
]


@pytest.mark.parametrize("name,n,downbeats,kw", PLANS, ids=[p[0] for p in PLANS])
@pytest.mark.parametrize("max_bars", [1, 5])
def test_plan_bar_lines_against_plan_windows(name, n, downbeats, kw, max_bars):
    kw = dict({"max_bars": max_bars}, **kw)
    plan = audio.plan_windows(n, 16000, downbeats, **kw)
    flags = audio.plan_flags(n, 16000, downbeats, **kw)
    lines = audio.plan_bar_lines(n, 16000, downbeats, **kw)
    assert len(plan) == len(flags) == len(lines) > 0
    db = sorted({min(max(int(round(t * 16000)), 0), n) for t in downbeats})
    for (start, stop, n_bars), fl, ln in zip(plan, flags, lines):
        assert len(ln) == n_bars + 1 and ln[0] == 0 and ln[-1] == stop - start
        assert all(b > a for a, b in zip(ln, ln[1:])), "strictly ascending"
        if "bar_cut" in fl:
            assert n_bars == 1 and ln == [0, stop - start]
        else:
            assert [start + t for t in ln] == [t for t in db if start <= t <= stop], "the downbeats inside the window, each once"
    if name == "one bar longer than the window":
        assert flags[0] == ["bar_cut"]


def test_plan_bar_lines_without_downbeats_and_the_old_plans_unchanged():
    assert audio.plan_bar_lines(16000 * 30, 16000) == [None, None, None]
    assert audio.plan_windows(16000 * 30, 16000) == [(0, 192000, 5), (192000, 384000, 5), (384000, 480000, 5)]
    assert audio.plan_flags(16000 * 30, 16000) == [[], [], ["short"]]
    assert audio.plan_windows(16000 * 40, 16000, [1.0, 15.0, 17.0, 19.0]) == [(16000, 208000, 1), (240000, 304000, 2)]


# ------------------------------------------------------------------------------------------- the correlation
def test_agreement_formula():
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, size=(1, 7, 33))
    seg = [(0, 0, 7)]
    n = 7 * 33
    for a, b, want in ((2.5, 0.25, 1.0), (-0.75, 3.0, -1.0)):
        r = resynth.agreement(resynth_oracle.five_sums(x, a * x + b, seg)[0], n)
        assert abs(r - want) <= 1e-12
    const = np.full_like(x, 0.625)
    assert resynth.agreement(resynth_oracle.five_sums(const, x, seg)[0], n) is None
    assert resynth.agreement(resynth_oracle.five_sums(x, const, seg)[0], n) is None
    assert resynth.agreement(np.zeros(5), 0) is None
    y = rng.uniform(0.0, 1.0, size=x.shape)
    sums = resynth_oracle.five_sums(x, y, seg)[0]
    want = float(np.corrcoef(x.reshape(-1), y.reshape(-1))[0, 1])
    assert abs(resynth.agreement(sums, n) - want) <= 1e-12 and abs(resynth_oracle.correlation(sums, n) - want) <= 1e-12
    assert -1.0 <= resynth.agreement(sums, n) <= 1.0
    assert resynth.mean_agreement([None, 0.5, 0.25, None]) == 0.375 and resynth.mean_agreement([None]) is None


# ------------------------------------------------------------------------------------------- the definition separates scores
def test_own_score_agrees_better_than_the_next_clips_in_every_bar():
    cfg = spec.default_cfg(max_length=(200, 200))
    frames, hop, bars = 601, scoregen.HOP, cfg["max_bars"]
    clips = [scoregen.make_clip(cfg, seed, frames=frames) for seed in range(100, 104)]
    n_samples = clips[0]["n_samples"]

    def feats(prog):
        return vqt_ref.vqt_features_librosa(render_oracle.render(prog))

    gaps = []
    for i, clip in enumerate(clips):
        lines = _lines(clip, bars)
        x = feats(scoregen.pack_program(clip))[None]
        seg = [(0, lines[b] // hop, lines[b + 1] // hop) for b in range(bars)]
        cells = resynth_oracle.n_cells(seg, 1, x.shape[1], x.shape[2])
        r = []
        for other in (clip, clips[(i + 1) % len(clips)]):
            ev, truncated = resynth.score_events(other["ids"]["upper"], other["ids"]["lower"], [other["time_sig"]] * bars, lines)
            assert not truncated and len(ev) > 0
            y = feats(resynth.program(ev, n_samples))[None]
            assert y.shape == x.shape
            r.append([resynth.agreement(s, n) for s, n in zip(resynth_oracle.five_sums(x, y, seg), cells)])
        for b, (own, nxt) in enumerate(zip(*r)):
            print(f"seed {clip['seed']} bar {b}: own {own:.3f} next {nxt:.3f} gap {own - nxt:.3f}")
            assert own is not None and nxt is not None and own > nxt, (clip["seed"], b, own, nxt)
            gaps.append(own - nxt)
    print(f"smallest gap {min(gaps):.3f} over {len(gaps)} bars")
