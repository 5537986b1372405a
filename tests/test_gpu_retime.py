"""Resynthesis at the performed timing on the MI355X (csrc/a2s_retime.hip, piano_a2s_amd/resynth.py):

1. a2s_path_warp against the integer oracle (tests/retime_oracle.py) through the raw ABI, sentinels around every buffer: B = 3, segments of 0, 1, 2,
   17, 37 and 300 frames (a path longer than a workgroup), overlapping, repeated, out of order, one of negative length and one longer than n_max;
   paths: the diagonal, a vertical run followed by a horizontal run, the DTW oracle's path on random costs, a random walk, and corrupt ones
   (steps = 0, too many steps, a wrong end cell, cells outside [0, n), a step back).  warp2 and inverse2 EQUAL the oracle, the identity where the
   oracle says so; with inverse2 = NULL warp2 is the same and nothing else is written; two runs are bit-identical; a segment alone in another table
   equals itself in the big one;
2. a2s_retime_events on those warps: program_rows = 9, hop = 16.  Words 0 and 1 EQUAL the oracle; every other program word, every header and every
   sentinel is unchanged; bad rows (clip -1 and B, prog_row 0, program_rows, 2^31 - 1 and negative, seg -1 and S, an empty bar, a padding row) write
   nothing; an event alone in another table equals itself in the big one; the wrappers give the same bits;
3. refusals return -1, set a2s_last_error and launch nothing;
4. the loop on the eight rendered clips of tests/test_gpu_dtw.py's onset test (seeds 100 .. 107, |a| = 0.15): with the option off nothing of it is
   launched and resynthesise returns what it returns without it; with retime=1 the events EQUAL the oracle's retime through the first pass's own
   warps (read back by the existing keys); the onset errors and the plain agreement of the retimed render against what tools/retime_check.py gives on
   exactly these clips (profiles/retime.json); the note levels of dynamics=3 on the render retimed by two rounds, on the twelve
   clips of tools/dynamics_check.py --warp 0.15, against the float64 table of tools/retime_check.py --dynamics;
5. transcribe_waveform(performed_timing=R): the keys, parallel to "notes"; the MIDI notes are the retimed ones; every earlier key is unchanged."""
import numpy as np
import pytest
import torch

from piano_a2s_amd import scoregen, spec
from tests import dtw_oracle
from tests import retime_oracle as oracle

pytestmark = pytest.mark.gpu
SMALL = dict(conv_feature_size=32, hidden_size=32, max_length=(12, 8))
HP = dict(sample_rate=16000, hop_length=160, max_frame_num=1201, max_bars=5, bins_per_octave=60, n_octaves=8, gamma=20)
GUARD = 16
SENTINEL = -7
B, PROGRAM_ROWS, HOP, N_MAX = 3, 9, 16, 300
STRIDE = 2 * N_MAX - 1 + 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _diagonal(n):
    return [(k, k) for k in range(n)]


def _corner(n):
    """A vertical run followed by a horizontal run: 2 n - 1 cells."""
    return [(i, 0) for i in range(n)] + [(n - 1, j) for j in range(1, n)]


def _walk(n, rng):
    path = [(0, 0)]
    while path[-1] != (n - 1, n - 1):
        i, j = path[-1]
        steps = [(di, dj) for di, dj in ((1, 1), (1, 0), (0, 1)) if i + di < n and j + dj < n]
        di, dj = steps[int(rng.integers(0, len(steps)))]
        path.append((i + di, j + dj))
    return path


def _case():
    """-> (table (S, 4) int32, paths (S, STRIDE) int32 with garbage behind every row's steps, steps (S,) int32, what each row is)."""
    rng = np.random.default_rng(28)
    by_cost = lambda n: dtw_oracle.align(rng.uniform(0.0, 1.0, size=(n, n)))[0]
    back = _diagonal(17)
    back[9] = (7, 9)                                                            # a step back in i, then a step of two
    outside = _walk(37, rng)
    outside[20] = (40, outside[20][1])                                          # a cell outside [0, n)
    rows = [((0, 0, 17, 8), _diagonal(17), None, "diagonal"),
            ((1, 5, 42, 9), by_cost(37), None, "the oracle's path on random costs"),
            ((0, 10, 10, 8), [], None, "n = 0"),
            ((2, 3, 4, 8), [(0, 0)], None, "n = 1"),
            ((1, 40, 42, 8), _corner(2), None, "n = 2, vertical then horizontal"),
            ((0, 0, 17, 8), _corner(17), None, "the first segment again, vertical then horizontal"),
            ((2, 0, 300, 75), _walk(300, rng), None, "n = 300: a path longer than a workgroup"),
            ((1, 5, 42, 9), by_cost(37), 0, "corrupt: steps = 0"),
            ((0, 2, 19, 8), by_cost(17)[:-1], None, "corrupt: the wrong end cell"),
            ((2, 10, 47, 9), outside, None, "corrupt: a cell outside [0, n)"),
            ((0, 30, 13, 8), _diagonal(17), None, "f1 < f0: read as empty"),
            ((1, 0, 301, 8), _diagonal(300), None, "n > n_max: read as empty"),
            ((0, 0, 17, 8), by_cost(17), None, "the first segment a third time, the oracle's path"),
            ((2, 0, 37, 9), _diagonal(37), 80, "corrupt: more steps than 2 n - 1"),
            ((1, 7, 24, 4), back, None, "corrupt: a step back"),
            ((2, 100, 400, 75), _corner(300), None, "n = 300, vertical then horizontal: 599 cells"),
            ((0, 1, 2, 0), [(0, 0)], -3, "corrupt: negative steps"),
            ((1, 20, 57, 9), [(1, 1)] + _diagonal(37)[1:], None, "corrupt: the wrong first cell")]
    S = len(rows)
    table = np.array([r[0] for r in rows], dtype=np.int32)
    paths = rng.integers(-2 ** 31, 2 ** 31, size=(S, STRIDE), dtype=np.int64).astype(np.int32)
    steps = np.zeros(S, dtype=np.int32)
    for s, (_, path, forced, _) in enumerate(rows):
        paths[s, :len(path)] = dtw_oracle.pack(path)
        steps[s] = len(path) if forced is None else forced
    return table, paths, steps, [r[3] for r in rows]


@pytest.fixture(scope="module")
def case():
    return _case()


def _path_warp(dev, table, paths, steps, n_max=N_MAX, inverse=True, stride=STRIDE):
    """a2s_path_warp through the raw ABI, sentinels around the outputs -> (warp2, inverse2 or the untouched buffer) as int32 numpy (S, n_max + 1)."""
    from piano_a2s_amd import hip
    Lib = hip.lib()
    S, words = len(table), len(table) * (n_max + 1)
    td, pd, sd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (table, paths, steps))
    out = [torch.full((GUARD + words + GUARD,), SENTINEL, dtype=torch.int32, device=dev) for _ in range(2)]
    n0 = hip.retime_launches()
    rc = Lib.a2s_path_warp(hip.stream(), hip._p(pd), stride, hip._p(sd), hip._p(td), S, n_max, hip._p(out[0][GUARD:]), hip._p(out[1][GUARD:]) if inverse else None)
    assert rc == 0, Lib.a2s_last_error()
    assert hip.retime_launches() == n0 + 1, "one launch"
    host = [o.cpu().numpy() for o in out]
    for h in host:
        assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + words:] == SENTINEL).all(), "nothing outside the output is written"
    assert np.array_equal(pd.cpu().numpy(), paths) and np.array_equal(sd.cpu().numpy(), steps) and np.array_equal(td.cpu().numpy(), table), "the inputs are read only"
    return tuple(h[GUARD:GUARD + words].reshape(S, n_max + 1) for h in host)


# ------------------------------------------------------------------------------------------- 1. the warps
def test_path_warp_against_the_oracle(dev, case):
    table, paths, steps, what = case
    want_w, want_v = oracle.table_warps(paths, steps, table, N_MAX)
    ident = 2 * np.arange(N_MAX + 1)
    is_ident = [bool(np.array_equal(w, ident) and np.array_equal(v, ident)) for w, v in zip(want_w, want_v)]
    assert is_ident == [True, False, True, True, False, False, False, True, True, True, True, True, False, True, True, False, True, True], "the table covers what it says"
    assert want_w[5, :18].tolist() == [16] + [32] * 16 + [34] and want_v[5, :18].tolist() == [0] * 16 + [16, 18]
    got_w, got_v = _path_warp(dev, table, paths, steps)
    for s, name in enumerate(what):
        assert np.array_equal(got_w[s], want_w[s]) and np.array_equal(got_v[s], want_v[s]), (s, name)
    again = _path_warp(dev, table, paths, steps)
    assert again[0].tobytes() == got_w.tobytes() and again[1].tobytes() == got_v.tobytes(), "two runs are bit-identical"
    only_w, untouched = _path_warp(dev, table, paths, steps, inverse=False)
    assert only_w.tobytes() == got_w.tobytes() and (untouched == SENTINEL).all(), "inverse2 = NULL: warp2 alone"
    for s, name in enumerate(what):                                             # alone in another table, at another n_max where it fits
        n_max = 40 if table[s, 2] - table[s, 1] <= 40 and steps[s] <= 79 else N_MAX
        w1, v1 = _path_warp(dev, table[s:s + 1], paths[s:s + 1], steps[s:s + 1], n_max=n_max)
        assert np.array_equal(w1[0], got_w[s, :n_max + 1]) and np.array_equal(v1[0], got_v[s, :n_max + 1]), (s, name)
    w_short, _ = _path_warp(dev, table[[5, 6]], np.ascontiguousarray(paths[[5, 6], :40]), steps[[5, 6]], stride=40)
    assert np.array_equal(w_short[0], want_w[5]) and np.array_equal(w_short[1], ident), "a row shorter than a segment's steps: that path is not taken"


# ------------------------------------------------------------------------------------------- 2. the events
def _programs(rng):
    """(B, PROGRAM_ROWS, 8) int32 of a pattern no update writes: rows 1 .. 6 are notes with onsets near the segments, row 7 is a padding row (length
    0), row 8 has a negative length."""
    prog = rng.integers(-2 ** 31, 2 ** 31, size=(B, PROGRAM_ROWS, 8), dtype=np.int64).astype(np.int32)
    prog[:, 1:7, 0] = rng.integers(0, 45 * HOP, size=(B, 6))
    prog[:, 1:7, 1] = rng.integers(1, 6 * HOP, size=(B, 6))
    prog[2, 4:7, 0] = rng.integers(0, 400 * HOP, size=3)                        # inside the 300-frame segments
    prog[:, 7, 1], prog[:, 8, 1] = 0, -5
    return prog


def _event_case():
    """[clip, prog_row, seg, bar_start, bar_stop]: good rows over every kind of segment, no program row named twice among them; then the bad rows."""
    h = HOP
    good = [(0, 1, 0, 0, 17 * h), (0, 2, 5, 3, 17 * h - 5), (0, 3, 12, 2 * h, 12 * h), (0, 4, 8, 2 * h, 19 * h), (0, 5, 2, 0, 40 * h), (0, 6, 10, 100, 101),
            (1, 1, 1, 5 * h, 42 * h), (1, 2, 4, 40 * h, 42 * h), (1, 3, 7, 5 * h + 7, 42 * h - 3), (1, 4, 14, 7 * h, 24 * h), (1, 5, 1, 20 * h, 21 * h),
            (1, 6, 17, 0, 60 * h), (2, 1, 3, 3 * h, 4 * h), (2, 2, 9, 10 * h, 47 * h), (2, 3, 13, 0, 37 * h), (2, 4, 6, 0, 300 * h), (2, 5, 15, 100 * h, 400 * h),
            (2, 6, 6, 50 * h + 1, 250 * h - 1)]
    bad = [(-1, 1, 0, 0, 17 * h), (B, 1, 0, 0, 17 * h), (0, 0, 0, 0, 17 * h), (0, PROGRAM_ROWS, 0, 0, 17 * h), (0, 2 ** 31 - 1, 0, 0, 17 * h), (1, -PROGRAM_ROWS + 1, 0, 0, 17 * h),
           (1, -2 ** 31, 0, 0, 17 * h), (0, 1, -1, 0, 17 * h), (0, 1, 18, 0, 17 * h), (0, 1, 2 ** 31 - 1, 0, 17 * h), (0, 2, 0, 80, 80), (0, 2, 0, 90, 80), (1, 7, 1, 0, 60 * h),
           (2, 8, 6, 0, 300 * h), (2 ** 31 - 1, 1, 0, 0, 17 * h)]
    rows = np.zeros((len(good) + len(bad), 8), dtype=np.int64)
    order = np.random.default_rng(3).permutation(len(rows))                     # good and bad rows mixed: the kernel needs no order
    rows[order, :5] = np.array(good + bad, dtype=np.int64).astype(np.int32)     # (-2^31 and 2^31 - 1 are int32 values)
    is_good = np.zeros(len(rows), dtype=bool)
    is_good[order[:len(good)]] = True
    return rows.astype(np.int32), is_good


def _retime(dev, warp2, table, events, prog0, n_max=N_MAX, hop=HOP):
    """a2s_retime_events through the raw ABI on a copy of prog0 with sentinels around it -> the programs as int32 numpy."""
    from piano_a2s_amd import hip
    Lib = hip.lib()
    words = prog0.size
    pd = torch.full((GUARD + words + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    pd[GUARD:GUARD + words] = torch.from_numpy(prog0.reshape(-1)).to(dev)
    wd, td, ed = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev) for a in (warp2, table, events))
    n0 = hip.retime_launches()
    rc = Lib.a2s_retime_events(hip.stream(), hip._p(wd), n_max, hip._p(td), len(table), hip._p(ed), len(events), hop, hip._p(pd[GUARD:]), prog0.shape[0], prog0.shape[1])
    assert rc == 0, Lib.a2s_last_error()
    assert hip.retime_launches() == n0 + 1, "one launch"
    host = pd.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + words:] == SENTINEL).all(), "nothing outside the programs is written"
    assert np.array_equal(ed.cpu().numpy(), events) and np.array_equal(wd.cpu().numpy(), warp2), "the inputs are read only"
    return host[GUARD:GUARD + words].reshape(prog0.shape)


def test_retime_events_against_the_oracle(dev, case):
    from piano_a2s_amd import hip
    table, paths, steps, _ = case
    warp2, _ = _path_warp(dev, table, paths, steps)
    events, is_good = _event_case()
    prog0 = _programs(np.random.default_rng(5))
    want = oracle.retime_programs(prog0, events, warp2, table, N_MAX, HOP)
    moved = np.argwhere((want != prog0).any(axis=2))
    assert len(moved) >= 12 and (want[:, :, 2:] == prog0[:, :, 2:]).all() and (want[:, 0] == prog0[:, 0]).all() and (want[:, 7:] == prog0[:, 7:]).all()
    got = _retime(dev, warp2, table, events, prog0)
    assert np.array_equal(got, want), np.argwhere(got != want)
    assert _retime(dev, warp2, table, events, prog0).tobytes() == got.tobytes(), "two runs are bit-identical"
    assert np.array_equal(_retime(dev, warp2, table, np.ascontiguousarray(events[~is_good]), prog0), prog0), "the bad rows write nothing"
    assert np.array_equal(_retime(dev, warp2, table, np.ascontiguousarray(events[is_good]), prog0), want), "the good rows alone"
    for e, good in zip(events, is_good):                                        # an event alone, its segment alone in a table of one
        if not (0 <= e[0] < B and 1 <= e[1] < PROGRAM_ROWS and 0 <= e[2] < len(table)):
            continue
        alone = e.copy()
        alone[2] = 0
        one = _retime(dev, warp2[e[2]:e[2] + 1], table[e[2]:e[2] + 1], alone[None], prog0)
        assert np.array_equal(one[e[0], e[1]], want[e[0], e[1]] if good else prog0[e[0], e[1]]), e
        one[e[0], e[1]] = prog0[e[0], e[1]]
        assert np.array_equal(one, prog0), "no other row is touched"
    # the wrappers on fresh buffers: the same bits
    td = torch.from_numpy(table).to(dev)
    w2, v2 = hip.path_warp(torch.from_numpy(paths).to(dev), torch.from_numpy(steps).to(dev), td, N_MAX)
    assert np.array_equal(w2.cpu().numpy(), warp2) and v2 is not None and hip.path_warp(torch.from_numpy(paths).to(dev), torch.from_numpy(steps).to(dev), td, N_MAX, inverse=False)[1] is None
    pt = torch.from_numpy(prog0).to(dev)
    assert hip.retime_events(w2, td, torch.from_numpy(events).to(dev), HOP, pt) is pt and np.array_equal(pt.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_launch_nothing(dev, case):
    from piano_a2s_amd import hip
    Lib, st = hip.lib(), hip.stream()
    table, paths, steps, _ = case
    S = len(table)
    td, pd, sd = (torch.from_numpy(a).to(dev) for a in (table, paths, steps))
    w = torch.full((S, N_MAX + 1), SENTINEL, dtype=torch.int32, device=dev)
    v = torch.full((S, N_MAX + 1), SENTINEL, dtype=torch.int32, device=dev)
    events = torch.from_numpy(_event_case()[0]).to(dev)
    progs = torch.full((B, PROGRAM_ROWS, 8), SENTINEL, dtype=torch.int32, device=dev)
    n0, k0 = hip.retime_launches(), Lib.a2s_launch_count()
    ok = [hip._p(pd), STRIDE, hip._p(sd), hip._p(td), S, N_MAX, hip._p(w), hip._p(v)]
    for i, bad in ((0, None), (2, None), (3, None), (6, None), (4, -1), (5, 0), (5, -1), (5, 4097), (1, 0), (1, -5)):
        args = list(ok)
        args[i] = bad
        assert Lib.a2s_path_warp(st, *args) == -1, (i, bad)
        assert b"path_warp" in Lib.a2s_last_error()
    ok2 = [hip._p(w), N_MAX, hip._p(td), S, hip._p(events), events.shape[0], HOP, hip._p(progs), B, PROGRAM_ROWS]
    for i, bad in ((0, None), (2, None), (4, None), (7, None), (1, 0), (1, -1), (1, 4097), (3, -1), (5, -1), (8, -1), (9, -1), (6, 0), (6, -16), (6, 65536)):
        args = list(ok2)
        args[i] = bad
        assert Lib.a2s_retime_events(st, *args) == -1, (i, bad)
        assert b"retime_events" in Lib.a2s_last_error()
    for i in (3, 5):                                                            # S = 0 and E = 0 are fine and launch nothing
        args = list(ok2)
        args[i] = 0
        assert Lib.a2s_retime_events(st, *args) == 0
    args = list(ok)
    args[4] = 0
    assert Lib.a2s_path_warp(st, *args) == 0
    # the wrappers
    with pytest.raises(hip.A2SError, match="`n_max`"):
        hip.path_warp(pd, sd, td, 4097)
    with pytest.raises(hip.A2SError, match="`paths`"):
        hip.path_warp(pd[:2], sd, td, N_MAX)
    with pytest.raises(hip.A2SError, match="`steps`"):
        hip.path_warp(pd, sd.long(), td, N_MAX)
    with pytest.raises(hip.A2SError, match="`dev_table`"):
        hip.path_warp(pd, sd, table, N_MAX)
    with pytest.raises(hip.A2SError, match="`hop`"):
        hip.retime_events(w, td, events, 65536, progs)
    with pytest.raises(hip.A2SError, match="`programs`"):
        hip.retime_events(w, td, events, HOP, progs[:, :1])
    with pytest.raises(hip.A2SError, match="`events`"):
        hip.retime_events(w, td, events[:, :5], HOP, progs)
    with pytest.raises(hip.A2SError, match="`warp2`"):
        hip.retime_events(w[:2], td, events, HOP, progs)
    with pytest.raises(hip.A2SError, match="event_table"):
        hip.event_table([(0, PROGRAM_ROWS, 0, 0, 10)], B, PROGRAM_ROWS, table, dev)
    torch.cuda.synchronize()
    assert hip.retime_launches() == n0 and Lib.a2s_launch_count() == k0, "nothing was launched"
    assert (w == SENTINEL).all() and (v == SENTINEL).all() and (progs == SENTINEL).all()


# ------------------------------------------------------------------------------------------- 4. the loop on rendered clips
WARP_SEED = 25               # tests/test_gpu_dtw.py's onset test; tools/retime_check.py --amp 0.15 --seed 25 gives on exactly these clips (profiles/retime.json):
CHECK_LINEAR_MS = 174.5      # median onset error of linear placement,
CHECK_MEDIAN_MS = (1.96875, 1.875, 1.875)          # of the retimed notes after round 1, 2, 3 (the float performed_notes through the first warp: 1.97),
CHECK_AGREEMENT = (0.99226, 0.99317, 0.99316)      # the mean plain agreement of the retimed render after round 1, 2, 3,
STRAIGHT_AGREEMENT = 0.788   # and the project's baseline: the mean plain agreement of the straight render


@pytest.fixture(scope="module")
def scenario(dev):
    from piano_a2s_amd import render, resynth, transcribe
    cfg = spec.default_cfg(max_length=(200, 200))
    rng = np.random.default_rng(WARP_SEED)
    scns = [dtw_oracle.warped_clip(scoregen.make_clip(cfg, seed, frames=1201), cfg["max_bars"], 0.15, rng) for seed in range(100, 108)]
    n_samples = 1200 * scoregen.HOP
    vqt = transcribe._vqt(dev, HP)
    progs = np.stack([resynth.program(s["warped"], n_samples) for s in scns])
    x = vqt(render.render(torch.from_numpy(progs).to(dev), n_samples))
    truth = []
    for s in scns:                                                              # the true onsets, row for row with the straight events
        notes, true = (np.concatenate([bar[k] for bar in s["bars"]]).reshape(-1, 3) for k in ("notes", "true"))
        order = np.lexsort((notes[:, 2], notes[:, 0]))
        assert np.array_equal(notes[order], s["straight"])
        truth.append(true[order])
    return scns, truth, x, vqt, n_samples


def test_the_loop_on_rendered_clips(dev, scenario):
    from piano_a2s_amd import hip, resynth
    scns, truth, x, vqt, n_samples = scenario
    hop, ms = scoregen.HOP, 1e3 / scoregen.SR
    windows = [{"events": s["straight"], "bar_lines": s["lines"]} for s in scns]
    # off: nothing of it is launched, and the call returns what it returns without the parameter
    n0 = hip.retime_launches()
    off = resynth.resynthesise(windows, x, vqt, hop, align=True)
    assert len(off) == 3 and hip.retime_launches() == n0, "off: nothing of the retiming is launched or returned"
    waves0, plain0, aligned0 = off
    linear = np.concatenate([np.abs(s["straight"][:, 0] - t[:, 0]) for s, t in zip(scns, truth)])
    assert abs(np.median(linear) * ms - CHECK_LINEAR_MS) < 0.01 and len(linear) == 528
    first = np.concatenate([np.abs(resynth.performed_onsets(s["straight"], s["lines"], al, hop) - t[:, 0]) for s, al, t in zip(scns, aligned0, truth)])
    got = {}
    for R in (1, 2, 3):
        n0, r0, d0 = hip.retime_launches(), hip.render_launches(), hip.dtw_launches()
        waves, plain, aligned, retimed = resynth.resynthesise(windows, x, vqt, hop, align=True, retime=R)
        assert hip.retime_launches() == n0 + 2 * R, "two launches per round"
        assert hip.render_launches() == r0 + R + 1 and hip.dtw_launches() == d0 + 2 * R, "round 1 reads the alignment pass; one final render"
        assert plain == plain0, "the plain agreements are those of the straight pass"
        for a, b in zip(aligned, aligned0):
            assert all((p is None) == (q is None) and (p is None or (np.array_equal(p["warp"], q["warp"]) and p["agreement_warped"] == q["agreement_warped"]
                                                                   and p["total"] == q["total"] and np.array_equal(p["inverse"], q["inverse"]))) for p, q in zip(a, b))
        for s, w, rt in zip(scns, waves, retimed):
            ev = rt["events"]
            assert ev.shape == s["straight"].shape and ev.dtype == np.int64 and np.array_equal(ev[:, 2], s["straight"][:, 2])
            assert np.all(np.diff(ev[:, 0]) >= 0), "the onsets keep their order"
            assert len(rt["agreement"]) == 5 and w.shape == (n_samples,) and np.abs(w).max() < 1.0
            lines = np.asarray(s["lines"])
            bar = np.clip(np.searchsorted(lines, s["straight"][:, 0], side="right") - 1, 0, 4)
            assert np.all(ev[:, 0] >= lines[bar]) and np.all(ev[:, 0] + ev[:, 1] <= lines[bar + 1]) and np.all(ev[:, 1] >= 1), "every note stays in its bar"
        err = np.concatenate([np.abs(rt["events"][:, 0] - t[:, 0]) for rt, t in zip(retimed, truth)])
        agr = [a for rt in retimed for a in rt["agreement"] if a is not None]
        got[R] = (float(np.median(err) * ms), float(np.quantile(err, 0.9) * ms), float(np.mean(agr)), retimed, waves)
        print(f"R = {R}: {len(err)} notes, onset error median {got[R][0]:.3f} ms, 90 % {got[R][1]:.3f} ms (linear {np.median(linear) * ms:.1f}, first warp "
              f"{np.median(first) * ms:.3f}); mean agreement_retimed {got[R][2]:.5f} over {len(agr)} bars (float64: {CHECK_AGREEMENT[R - 1]})")
    assert not any(np.array_equal(a, b) for a, b in zip(got[2][4], waves0)), "the waves are the render at the performed timing"
    # round 1 EQUALS the integer definition applied to the first pass's own warps, as the existing keys read them back
    for s, al, rt in zip(scns, aligned0, got[1][3]):
        lines = s["lines"]
        for e, (onset, length, _) in enumerate(s["straight"]):
            b = min(max(int(np.searchsorted(lines, onset, side="right")) - 1, 0), 4)
            if al[b] is None:
                want = (onset, length)
            else:
                n = al[b]["frames"]
                w2 = np.rint(2 * np.concatenate([al[b]["warp"], [al[b]["warp"][-1] + 1.0]])).astype(np.int64)
                want = oracle.retime(onset, length, w2, al[b]["first_frame"], n, hop, lines[b], lines[b + 1])
            assert tuple(rt["events"][e, :2]) == want, (e, b)
    # Against the definition (tools/retime_check.py on exactly these clips), by the project's rule of the measured value plus half
    # its distance to the baseline.  R = 2 is the default: the definition gains from round 2 (1.969 -> 1.875 ms, 0.99226 -> 0.99317) and nothing from
    # round 3, so for round 3 only "no worse than round 2 by more than the definition's own difference" is asserted.
    R = resynth.RETIME_ROUNDS
    assert R == 2
    assert got[R][0] < 0.5 * (CHECK_MEDIAN_MS[R - 1] + CHECK_LINEAR_MS), "below the midpoint between the definition's median and linear placement"
    assert got[R][2] > 0.5 * (STRAIGHT_AGREEMENT + CHECK_AGREEMENT[R - 1]), "above the midpoint between the straight render's agreement and the definition's"
    assert got[R][0] <= np.median(first) * ms + abs(CHECK_MEDIAN_MS[1] - CHECK_MEDIAN_MS[0]), "not worse than the first-pass warp by more than the measured difference"
    assert got[3][0] <= got[2][0] + 0.1875, "round 3: the definition's worst move away from the truth is 0.1875 ms; no drift"


DYN_SEED = 26                # tools/retime_check.py --dynamics --seed 26 --clips 12 --rounds 2: tools/dynamics_check.py --warp 0.15's clips and phantoms; after
DYN_STRAIGHT_RMS = 1.75403   # three dynamics rounds the float64 definitions give an rms level error of 1.75403 dB without retiming,
DYN_RETIMED_RMS = 1.50350    # 1.50350 dB on the score retimed by two rounds (correlation 0.8449 -> 0.8751, AUC 0.9815 -> 0.9822)


def test_dynamics_on_the_retimed_render(dev):
    from piano_a2s_amd import render, resynth, transcribe
    from tests import dynamics_oracle
    cfg = spec.default_cfg(max_length=(200, 200))
    rng = np.random.default_rng(DYN_SEED)
    hop, n_samples = scoregen.HOP, 1200 * scoregen.HOP
    scns, progs = [], []
    for seed in range(100, 112):                                                # as tools/dynamics_check.py: warped_performance builds what is played
        clip = scoregen.make_clip(cfg, seed, frames=1201)
        scn = dynamics_oracle.scenario(clip, rng, 3)
        w = dtw_oracle.warped_clip(clip, cfg["max_bars"], 0.15, rng)
        amp_of = {(int(o), int(m)): float(a) for (o, _, m), a in zip(scn["events"], scn["amps"])}
        played = sorted((int(t[0]), int(t[2]), int(t[1]), amp_of[(int(s[0]), int(s[2]))]) for bar in w["bars"] for s, t in zip(bar["notes"], bar["true"]))
        progs.append(resynth.program(np.array([(o, ln, m) for o, m, ln, _ in played], dtype=np.int64), n_samples, amps=[a for *_, a in played]))
        scn["lines"] = w["lines"]
        scns.append(scn)
    vqt = transcribe._vqt(dev, HP)
    x = vqt(render.render(torch.from_numpy(np.stack(progs)).to(dev), n_samples))
    windows = [{"events": s["score"], "bar_lines": s["lines"]} for s in scns]

    def pooled(dyn):
        got = np.concatenate([d["level_db"].astype(np.float64) - d["level_db"].astype(np.float64)[s["real"]].mean() for d, s in zip(dyn, scns)])
        true = np.concatenate([s["true_db"] - s["true_db"][s["real"]].mean() for s in scns])
        real = np.concatenate([s["real"] for s in scns])
        err = got[real] - true[real]
        return float(np.sqrt(np.mean(err * err))), float(np.corrcoef(got[real], true[real])[0, 1]), dynamics_oracle.auc(got[real], got[~real])

    straight = pooled(resynth.resynthesise(windows, x, vqt, hop, align=True, dynamics=3)[3])
    *_, retimed, dyn = resynth.resynthesise(windows, x, vqt, hop, align=True, dynamics=3, retime=2)
    moved = pooled(dyn)
    print(f"rms level error {straight[0]:.4f} dB straight, {moved[0]:.4f} dB retimed (float64: {DYN_STRAIGHT_RMS}, {DYN_RETIMED_RMS}); correlation "
          f"{straight[1]:.4f} -> {moved[1]:.4f}, AUC {straight[2]:.4f} -> {moved[2]:.4f}")
    for s, d, rt in zip(scns, dyn, retimed):
        assert d["level_db"].shape == (len(s["score"]),) == (len(rt["events"]),) and d["agreement_warped"] == [None] * 5 and len(d["agreement"]) == 5
    assert int(sum(s["real"].sum() for s in scns)) == 809, "the clips of the definition's table"
    assert moved[0] < 0.5 * (DYN_RETIMED_RMS + DYN_STRAIGHT_RMS), "below the midpoint between the definition's value and the straight render's 1.75 dB"


# ------------------------------------------------------------------------------------------- 5. transcribe_waveform
@pytest.fixture(scope="module")
def state():
    return spec.procedural_state(spec.default_cfg(**SMALL), 11, eos_bias=3.0, lively=True)


@pytest.fixture(scope="module")
def recording(dev):
    """12 s at 16 kHz: a rendered clip below full scale; downbeats that cut it into one window of 5 bars."""
    from piano_a2s_amd.render import render
    w = render(torch.from_numpy(scoregen.pack_program(scoregen.make_clip(spec.default_cfg(), 2024, frames=1201))[None]).to(dev)).cpu().numpy()[0]
    return (w * (0.8 / np.abs(w).max())).astype(np.float32), [0.5, 2.75, 5.0, 7.25, 9.5, 11.75]


def test_transcribe_waveform_with_performed_timing(dev, state, recording):
    import models
    from piano_a2s_amd import audio, hip, transcribe
    x, downbeats = recording
    model = models.ScoreTranscription(**SMALL)
    model.load_state_dict(state)
    model = model.to(dev).eval()
    model.constrained_decoding = True                            # (an untrained model under the grammar still writes notes)
    kw = dict(downbeats=downbeats, hparams=HP, resynthesis=True, align_notes=True)
    n0 = hip.retime_launches()
    off = transcribe.transcribe_waveform(model, x, 16000, **kw)
    assert transcribe.transcribe_waveform(model, x, 16000, performed_timing=0, **kw)["windows"] == off["windows"]
    assert hip.retime_launches() == n0, "without the option nothing of it is launched"
    on = transcribe.transcribe_waveform(model, x, 16000, performed_timing=2, **kw)
    assert hip.retime_launches() == n0 + 2 * 2, "two rounds, two launches each"
    assert set(on) == set(off) and on["resynthesis"]["wave"].shape == off["resynthesis"]["wave"].shape and np.abs(on["resynthesis"]["wave"]).max() < 1.0
    some = 0
    for w_off, w_on in zip(off["windows"], on["windows"]):
        assert set(w_on) == set(w_off) | {"agreement_retimed"}
        assert {k: v for k, v in w_on.items() if k not in ("bars", "agreement_retimed")} == {k: v for k, v in w_off.items() if k != "bars"}
        for b_off, b_on in zip(w_off["bars"], w_on["bars"]):
            assert set(b_on) == set(b_off) | {"retimed", "agreement_retimed"} and {k: b_on[k] for k in b_off} == b_off, "every earlier key is unchanged"
            assert len(b_on["retimed"]) == len(b_on["notes"]) and (b_on["agreement_retimed"] is None) == (b_on["agreement"] is None)
            assert b_on["agreement_retimed"] is None or -1.0 <= b_on["agreement_retimed"] <= 1.0
            for note, moved in zip(b_on["notes"], b_on["retimed"]):
                assert moved[2] == note[2] and moved[1] > 0.0
                some += 1
        have = [b["agreement_retimed"] for b in w_on["bars"] if b["agreement_retimed"] is not None]
        assert (w_on["agreement_retimed"] is None) if not have else abs(w_on["agreement_retimed"] - sum(have) / len(have)) <= 1e-12
    assert some >= 5, "the seeded model decodes some notes"
    assert audio.result_notes(on) == [list(n) for w in on["windows"] for b in w["bars"] for n in b["retimed"]]
    both = transcribe.transcribe_waveform(model, x, 16000, performed_timing=1, dynamics=True, dynamics_rounds=1, **kw)
    assert hip.retime_launches() == n0 + 2 * 2 + 2
    for w in both["windows"]:
        for b in w["bars"]:
            assert len(b["dynamics"]) == len(b["retimed"]) == len(b["notes"]) and b.get("agreement_dynamics_warped") is None
