"""Bar-wise dynamic time warping on the MI355X (csrc/a2s_dtw.hip, piano_a2s_amd/resynth.py):

1. a2s_dtw_cost against the float64 oracle (tests/dtw_oracle.py) through the raw ABI: B = 3, T = 37, F = 24 (16-byte loads) and F = 23 (4-byte loads),
   clips T * F, T * F + 8 and T * F + 7 apart with NaN in the padding; segments of 0, 1, 2, 17 and 37 frames, overlapping, repeated, out of order,
   clamped, two with a clip outside [0, B); r in {-1, 0, 3, >= n}; dense blocks and a table whose blocks are all banded.  Inputs on a grid of 1/8
   with off = NULL are bit-equal to float64; random inputs with off != 0 stay inside the oracle's a-priori bound of an F-term fp32 FMA chain
   (derived in tests/dtw_oracle.py: per term two subtractions, |e^ - e| <= eta = u |x - y| + u (|e| + u |x - y|), an exact product, then recursive
   summation: sum (2 |e| eta + eta^2) + gamma(F) sum (|e| + eta)^2).  Nothing outside the band's cells is written;
2. a2s_dtw_path on the kernel's OWN costs read back: path, steps and total bit-equal to the float32 numpy DP; on grid inputs also equal to the
   float64 oracle; x = y gives the diagonal and total 0; empty segments give steps 0, total 0 and write nothing else;
3. n = 300 (an anti-diagonal longer than the workgroup, five tiles a side), F = 8, without a band and with r = 5;
4. a segment alone, in a tensor of another B and T, is bit-equal to the same segment inside the table; two runs are bit-identical;
5. refusals return -1, set a2s_last_error and launch nothing; the wrapper's checks;
6. end to end on eight rendered clips whose events are warped inside every bar by g(u) = u + a sin(pi u): with a = 0 nothing moves by a bit, with
   |a| = 0.15 the performed onsets are nearer to the true ones than linear placement (medians, pooled over all notes) and the warped agreement is
   at least the plain one in the mean;
7. transcribe_waveform(align_notes=True) adds its keys and changes nothing else; the command line writes NAME.mid.

Measured on the MI355X (the figures the tests print): on uniform inputs the largest |device - float64| of a cost is 0.16 (F = 24) and 0.19 (F = 23) of
its bound; test 6 at |a| = 0.15: 528 notes, median onset error 174.5 ms by linear placement and 1.97 ms through the warp (ratio 0.0113; the float64
definitions alone, tools/dtw_alignment_check.py, give the same), mean agreement 0.798, warped 0.991; see DESIGN.md section 25."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from piano_a2s_amd import scoregen, spec
from tests import dtw_oracle as oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(conv_feature_size=32, hidden_size=32, max_length=(12, 8))
HP = dict(sample_rate=16000, hop_length=160, max_frame_num=1201, max_bars=5, bins_per_octave=60, n_octaves=8, gamma=20)
LEAD = 8                                     # floats in front of a padded tensor: keeps the 16-byte alignment of the base
SENTINEL = -12345.5
GUARD = 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _padded(host, stride, dev):
    """host (B, T, F) float32 -> a device view of its shape whose clips lie `stride` floats apart, NaN everywhere else in its buffer."""
    B, T, F = host.shape
    flat = torch.full((LEAD + B * stride + 8,), float("nan"), dtype=torch.float32, device=dev)
    view = flat[LEAD:].as_strided((B, T, F), (stride, F, 1))
    view.copy_(torch.from_numpy(host))
    return view


def _raw(dev, xd, yd, stride, shape, table, off, n_max, r_max):
    """Both entry points through the raw ABI on buffers with sentinels around them -> (cost, ws, path (S, 2 n_max - 1), steps, total) as numpy;
    the sentinels are checked here."""
    from piano_a2s_amd import hip
    Lib, st = hip.lib(), hip.stream()
    B, T, F = shape
    table = np.asarray(table, dtype=np.int32).reshape(-1, 4)
    S = len(table)
    cb, wb = int(Lib.a2s_dtw_cost_bytes(S, n_max, r_max)), int(Lib.a2s_dtw_workspace_bytes(S, n_max, r_max))
    assert cb == 4 * wb
    cost = torch.full((GUARD + cb // 4 + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    ws = torch.full((GUARD + wb + GUARD,), 77, dtype=torch.uint8, device=dev)
    P = 2 * n_max - 1
    path = torch.full((GUARD + S * P + GUARD,), -7, dtype=torch.int32, device=dev)
    steps = torch.full((GUARD + S + GUARD,), -7, dtype=torch.int32, device=dev)
    total = torch.full((GUARD + S + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    sd = torch.from_numpy(table).to(dev)
    od = None if off is None else torch.from_numpy(np.asarray(off, dtype=np.float32)).to(dev)
    n0 = hip.dtw_launches()
    rc = Lib.a2s_dtw_cost(st, hip._p(xd), hip._p(yd), stride, B, T, F, hip._p(sd), S, None if od is None else hip._p(od), n_max, r_max, hip._p(cost[GUARD:]), cb)
    assert rc == 0, Lib.a2s_last_error()
    rc = Lib.a2s_dtw_path(st, hip._p(sd), S, B, T, n_max, r_max, hip._p(cost[GUARD:]), cb, hip._p(ws[GUARD:]), wb, hip._p(path[GUARD:]), hip._p(steps[GUARD:]),
                          hip._p(total[GUARD:]))
    assert rc == 0, Lib.a2s_last_error()
    assert hip.dtw_launches() == n0 + 2, "one launch each"
    out = []
    for t, fill, size in ((cost, SENTINEL, cb // 4), (ws, 77, wb), (path, -7, S * P), (steps, -7, S), (total, SENTINEL, S)):
        h = t.cpu().numpy()
        assert (h[:GUARD] == fill).all() and (h[GUARD + size:] == fill).all(), "nothing outside the buffers is written"
        out.append(h[GUARD:GUARD + size])
    out[2] = out[2].reshape(S, P)
    return out


def _check_paths(table, shape, n_max, w_max, cost, path, steps, total, want64=None):
    """Every segment of the raw outputs against the float32 DP on the device's own costs [and the float64 path and total]."""
    B, T, _ = shape
    for s, row in enumerate(table):
        sg = oracle.segment(row, B, T)
        if sg is None:
            assert steps[s] == 0 and total[s] == 0.0 and (path[s] == -7).all(), (s, row)
            continue
        _, _, n, r = sg
        d = oracle.unpack(cost, s, n, r, n_max, w_max)
        assert np.isfinite(d[oracle.band_mask(n, r)]).all() and np.isnan(d[~oracle.band_mask(n, r)]).all()
        want, tot = oracle.align(d, r, np.float32)
        assert steps[s] == len(want) <= 2 * n - 1, (s, row, steps[s], len(want))
        assert np.array_equal(path[s, :steps[s]], oracle.pack(want)), (s, row)
        assert (path[s, steps[s]:] == -7).all(), "entries behind steps are not written"
        assert total[s].tobytes() == np.float32(tot).tobytes(), (s, row, total[s], tot)
        if want64 is not None:
            p64, t64 = want64[s]
            assert np.array_equal(path[s, :steps[s]], oracle.pack(p64)) and float(total[s]) == t64, (s, row)


# segments of 0, 1, 2, 17 and 37 frames: overlapping, repeated, out of order, clamped, two with a clip outside [0, 3)
TABLE = [(2, 0, 37, 3), (0, 5, 5, -1), (1, 36, 37, 0), (0, 10, 27, 3), (3, 0, 37, -1), (2, 3, 5, 3), (0, 0, 37, -1), (1, 20, 99, -1), (0, 10, 27, 0),
         (1, 0, 37, 40), (2, 0, 37, 3), (-1, 0, 37, 2), (0, 12, 29, 17), (1, -4, 2, 1), (2, 0, 37, 0), (0, 9, 4, 2)]
BANDED = [(2, 0, 37, 3), (0, 10, 27, 3), (1, 20, 37, 0), (0, 5, 5, 1), (2, 0, 37, 2), (1, 3, 20, 3), (2, 0, 37, 3)]          # every block W < n: w_max = 7


# ------------------------------------------------------------------------------------------- 1, 2. cost and path against the oracle
@pytest.mark.parametrize("F", [24, 23])
def test_cost_and_path_against_the_oracle(dev, F):
    B, T = 3, 37
    rng = np.random.default_rng(F)
    worst = 0.0
    for table, (n_max, r_max, w_max) in ((TABLE, (37, -1, 37)), (BANDED, (37, 3, 7))):
        xg, yg = (rng.integers(0, 9, size=(B, T, F)).astype(np.float32) / 8.0 for _ in range(2))
        xu, yu = (rng.uniform(0.0, 1.0, size=(B, T, F)).astype(np.float32) for _ in range(2))
        off = rng.uniform(-0.3, 0.3, size=len(table)).astype(np.float32)
        for stride in (T * F, T * F + 8, T * F + 7):
            # on the grid, off = NULL: exact
            cost, _, path, steps, total = _raw(dev, _padded(xg, stride, dev), _padded(yg, stride, dev), stride, (B, T, F), table, None, n_max, r_max)
            want64 = {}
            for s, row in enumerate(table):
                sg = oracle.segment(row, B, T)
                if sg is None:
                    continue
                _, _, n, r = sg
                d64 = oracle.cost(xg, yg, row)
                got = oracle.unpack(cost, s, n, r, n_max, w_max)
                m = oracle.band_mask(n, r)
                assert np.array_equal(got[m].astype(np.float64), d64[m]), (F, stride, s, row)
                want64[s] = oracle.align(d64, r)
            assert (cost == SENTINEL).sum() == cost.size - sum(int(oracle.band_mask(sg[2], sg[3]).sum()) for sg in (oracle.segment(r, B, T) for r in table) if sg), \
                "exactly the cells inside the bands are written"
            _check_paths(table, (B, T, F), n_max, w_max, cost, path, steps, total, want64)
            assert np.array_equal(path[0], path[10] if table is TABLE else path[6]) and total[0] == (total[10] if table is TABLE else total[6]), "a segment listed twice"
            # uniform inputs, off != 0: inside the a-priori bound
            cost, _, path, steps, total = _raw(dev, _padded(xu, stride, dev), _padded(yu, stride, dev), stride, (B, T, F), table, off, n_max, r_max)
            for s, row in enumerate(table):
                sg = oracle.segment(row, B, T)
                if sg is None:
                    continue
                d64, bound = oracle.cost(xu, yu, row, off=float(off[s]), with_bound=True)
                got = oracle.unpack(cost, s, sg[2], sg[3], n_max, w_max)
                m = oracle.band_mask(sg[2], sg[3])
                err = np.abs(got[m].astype(np.float64) - d64[m])
                assert (err <= bound[m]).all(), (F, stride, s, row, float((err / bound[m]).max()))
                worst = max(worst, float((err / bound[m]).max()))
            _check_paths(table, (B, T, F), n_max, w_max, cost, path, steps, total)
    print(f"F = {F}: worst |device - float64| / bound = {worst:.3f}")


def test_equal_tensors_give_the_diagonal(dev):
    B, T, F = 3, 37, 24
    x = np.random.default_rng(7).uniform(0.0, 1.0, size=(B, T, F)).astype(np.float32)
    xd = _padded(x, T * F, dev)
    for table, (n_max, r_max, w_max) in ((TABLE, (37, -1, 37)), (BANDED, (37, 3, 7))):
        cost, _, path, steps, total = _raw(dev, xd, xd.clone(), T * F, (B, T, F), table, None, n_max, r_max)
        for s, row in enumerate(table):
            sg = oracle.segment(row, B, T)
            if sg is None:
                assert steps[s] == 0 and total[s] == 0.0
                continue
            n = sg[2]
            assert steps[s] == n and total[s] == 0.0 and np.array_equal(path[s, :n], oracle.pack([(k, k) for k in range(n)])), (s, row)


# ------------------------------------------------------------------------------------------- 3. a diagonal longer than the workgroup
@pytest.mark.parametrize("r", [-1, 5])
def test_three_hundred_frames(dev, r):
    B, T, F = 1, 300, 8
    rng = np.random.default_rng(300 + r)
    table = [(0, 0, 300, r)]
    n_max, r_max, w_max = oracle.geometry(table)
    assert (n_max, w_max) == (300, 300 if r < 0 else 11)
    # a performance that drifts: y is x read along a warp (inside the band where there is one), plus a little noise, on the grid of 1/8
    base = rng.integers(0, 9, size=(T, F)).astype(np.float32) / 8.0
    lag = np.clip(np.rint(np.arange(T) + (4.0 if r >= 0 else 25.0) * np.sin(np.arange(T) / 40.0)).astype(np.int64), 0, T - 1)
    y = base[lag].copy()
    flip = rng.uniform(size=y.shape) < 0.05
    y[flip] = rng.integers(0, 9, size=int(flip.sum())).astype(np.float32) / 8.0
    x, y = base[None], y[None]
    cost, _, path, steps, total = _raw(dev, _padded(x, T * F, dev), _padded(y, T * F, dev), T * F, (B, T, F), table, None, n_max, r_max)
    d64 = oracle.cost(x, y, table[0])
    m = oracle.band_mask(300, r)
    assert np.array_equal(oracle.unpack(cost, 0, 300, r, n_max, w_max)[m].astype(np.float64), d64[m])
    want = oracle.align(d64, r)
    _check_paths(table, (B, T, F), n_max, w_max, cost, path, steps, total, {0: want})
    assert steps[0] > 300, "the path leaves the diagonal"
    print(f"n = 300, r = {r}: {steps[0]} steps, total {total[0]}")


# ------------------------------------------------------------------------------------------- 4. independence, determinism
@pytest.mark.parametrize("F", [24, 23])
def test_a_segment_does_not_depend_on_its_table_or_tensor(dev, F):
    B, T = 3, 37
    rng = np.random.default_rng(40 + F)
    x, y = (rng.uniform(0.0, 1.0, size=(B, T, F)).astype(np.float32) for _ in range(2))
    off = rng.uniform(-0.3, 0.3, size=len(TABLE)).astype(np.float32)
    xd, yd = _padded(x, T * F, dev), _padded(y, T * F, dev)
    first = _raw(dev, xd, yd, T * F, (B, T, F), TABLE, off, 37, -1)
    again = _raw(dev, xd, yd, T * F, (B, T, F), TABLE, off, 37, -1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again)), "two runs are bit-identical"
    cost, _, path, steps, total = first
    for s, row in enumerate(TABLE):
        sg = oracle.segment(row, B, T)
        if sg is None:
            continue
        clip, f0, n, r = sg
        # alone: one clip of T' = n + 3 rows that holds the segment's rows from row 2 on, its own (smaller) blocks
        T2 = n + 3
        x2, y2 = np.zeros((1, T2, F), dtype=np.float32), np.zeros((1, T2, F), dtype=np.float32)
        x2[0, 2:2 + n], y2[0, 2:2 + n] = x[clip, f0:f0 + n], y[clip, f0:f0 + n]
        t2 = [(0, 2, 2 + n, row[3])]
        n_max, r_max, w_max = oracle.geometry(t2)
        c2, _, p2, s2, tot2 = _raw(dev, _padded(x2, T2 * F, dev), _padded(y2, T2 * F, dev), T2 * F, (1, T2, F), t2, off[s:s + 1], n_max, r_max)
        m = oracle.band_mask(n, r)
        assert oracle.unpack(c2, 0, n, r, n_max, w_max)[m].tobytes() == oracle.unpack(cost, s, n, r, 37, 37)[m].tobytes(), (s, row)
        assert s2[0] == steps[s] and np.array_equal(p2[0, :s2[0]], path[s, :steps[s]]) and tot2[0].tobytes() == total[s].tobytes(), (s, row)


# ------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_launch_nothing(dev):
    from piano_a2s_amd import hip
    Lib, st = hip.lib(), hip.stream()
    B, T, F, S = 2, 9, 24, 2
    x, y = torch.rand(B, T, F, device=dev), torch.rand(B, T, F, device=dev)
    seg = torch.tensor([[0, 0, T, 2], [1, 1, 4, -1]], dtype=torch.int32, device=dev)
    off = torch.zeros(S, device=dev)
    n_max, r_max = 9, -1
    cb, wb = int(Lib.a2s_dtw_cost_bytes(S, n_max, r_max)), int(Lib.a2s_dtw_workspace_bytes(S, n_max, r_max))
    assert (cb, wb) == (S * 81 * 4, S * 81) and int(Lib.a2s_dtw_workspace_bytes(5, 300, 5)) == 5 * 300 * 11 and int(Lib.a2s_dtw_cost_bytes(1, 9, 7)) == 81 * 4
    cost = torch.full((cb // 4,), SENTINEL, device=dev)
    ws = torch.full((wb,), 77, dtype=torch.uint8, device=dev)
    path = torch.full((S, 2 * n_max - 1), -7, dtype=torch.int32, device=dev)
    steps = torch.full((S,), -7, dtype=torch.int32, device=dev)
    total = torch.full((S,), SENTINEL, device=dev)
    n0, k0 = hip.dtw_launches(), Lib.a2s_launch_count()
    ok = [hip._p(x), hip._p(y), T * F, B, T, F, hip._p(seg), S, hip._p(off), n_max, r_max, hip._p(cost), cb]
    for i, bad in ((0, None), (1, None), (6, None), (11, None), (3, 0), (4, 0), (4, 4097), (5, 0), (5, -2), (7, -1), (2, T * F - 1), (9, 0), (9, T + 1), (12, cb - 1)):
        args = list(ok)
        args[i] = bad
        assert Lib.a2s_dtw_cost(st, *args) == -1, (i, bad)
        assert b"dtw_cost" in Lib.a2s_last_error()
    ok2 = [hip._p(seg), S, B, T, n_max, r_max, hip._p(cost), cb, hip._p(ws), wb, hip._p(path), hip._p(steps), hip._p(total)]
    for i, bad in ((0, None), (6, None), (8, None), (10, None), (11, None), (12, None), (1, -1), (2, 0), (3, 0), (3, 4097), (4, 0), (4, T + 1), (7, cb - 1), (9, wb - 1)):
        args = list(ok2)
        args[i] = bad
        assert Lib.a2s_dtw_path(st, *args) == -1, (i, bad)
        assert b"dtw_path" in Lib.a2s_last_error()
    args, args2 = list(ok), list(ok2)
    args[7], args2[1] = 0, 0
    assert Lib.a2s_dtw_cost(st, *args) == 0 and Lib.a2s_dtw_path(st, *args2) == 0, "S = 0 is fine"
    torch.cuda.synchronize()
    assert hip.dtw_launches() == n0 and Lib.a2s_launch_count() == k0, "nothing was launched"
    assert (cost == SENTINEL).all() and (ws == 77).all() and (path == -7).all() and (steps == -7).all() and (total == SENTINEL).all()
    args = list(ok)
    args[8] = None
    assert Lib.a2s_dtw_cost(st, *args) == 0 and Lib.a2s_dtw_path(st, *ok2) == 0, "off = NULL is allowed"
    torch.cuda.synchronize()
    assert hip.dtw_launches() == n0 + 2 and 9 <= int(steps[0]) <= 17 and 3 <= int(steps[1]) <= 5


def test_the_wrapper(dev):
    from piano_a2s_amd import hip
    Lib = hip.lib()
    rng = np.random.default_rng(9)
    B, T, F = 2, 37, 24
    x, y = (rng.integers(0, 9, size=(B, T, F)).astype(np.float32) / 8.0 for _ in range(2))
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    table = [(1, 0, 37, 9), (0, 4, 21, -1), (0, 7, 7, 0)]
    n0 = hip.dtw_launches()
    paths, steps, totals = hip.dtw_segments(xd[:, None], yd[:, None], table)
    assert hip.dtw_launches() == n0 + 2
    assert paths.dtype == torch.int32 and tuple(paths.shape) == (3, 73) and steps.dtype == torch.int32 and totals.dtype == torch.float32
    paths, steps, totals = paths.cpu().numpy(), steps.cpu().numpy(), totals.cpu().numpy()
    for s, row in enumerate(table[:2]):
        want, tot = oracle.align(oracle.cost(x, y, row), row[3])
        assert np.array_equal(paths[s, :steps[s]], oracle.pack(want)) and (paths[s, steps[s]:] == -1).all() and float(totals[s]) == tot
    assert steps[2] == 0 and totals[2] == 0.0 and (paths[2] == -1).all()
    # (S, 3): no band; off given
    p3, s3, t3 = hip.dtw_segments(xd, yd, [(0, 4, 21)], off=torch.zeros(1, device=dev))
    assert np.array_equal(p3.cpu().numpy()[0, :int(s3[0])], paths[1, :steps[1]]) and float(t3[0]) == float(totals[1])
    n0, k0 = hip.dtw_launches(), Lib.a2s_launch_count()
    empty = hip.dtw_segments(xd, yd, np.zeros((0, 4), dtype=np.int64))
    assert [tuple(t.shape)[0] for t in empty] == [0, 0, 0]
    for bad in ([(2, 0, 1, 0)], [(-1, 0, 1, 0)], [(0, 3, 2, 0)], [(0, 0, T + 1, 0)], [(0, 0.5, 2, 0)], [(0, 0)], "table"):
        with pytest.raises(hip.A2SError, match="`seg`"):
            hip.dtw_segments(xd, yd, bad)
    with pytest.raises(hip.A2SError, match="`seg`"):
        hip.dtw_segments(xd, yd, torch.tensor(table, device=dev))
    with pytest.raises(hip.A2SError, match="`y`"):
        hip.dtw_segments(xd, yd[:, :4], table)
    with pytest.raises(hip.A2SError, match="`x`"):
        hip.dtw_segments(xd.transpose(1, 2), yd.transpose(1, 2), [(0, 0, 1, 0)])
    with pytest.raises(hip.A2SError, match="`y`"):
        hip.dtw_segments(xd, yd.double(), table)
    with pytest.raises(hip.A2SError, match="`off`"):
        hip.dtw_segments(xd, yd, table, off=torch.zeros(2, device=dev))
    with pytest.raises(hip.A2SError, match="`x`"):
        hip.dtw_segments(torch.zeros(1, 4097, 4, device=dev), torch.zeros(1, 4097, 4, device=dev), [(0, 0, 5, 0)])
    torch.cuda.synchronize()
    assert hip.dtw_launches() == n0 and Lib.a2s_launch_count() == k0


# ------------------------------------------------------------------------------------------- 6. rendered clips, warped inside every bar
WARP_SEED = 25          # tools/dtw_alignment_check.py --amp 0.15 --seed 25: the float64 definition alone gives a ratio of medians of 0.011 on these clips


def _render_features(dev, vqt, events, n_samples):
    from piano_a2s_amd import render, resynth
    progs = np.stack([resynth.program(ev, n_samples) for ev in events])
    return vqt(render.render(torch.from_numpy(progs).to(dev), n_samples))


@pytest.fixture(scope="module")
def clips():
    cfg = spec.default_cfg(max_length=(200, 200))
    return cfg["max_bars"], [scoregen.make_clip(cfg, seed, frames=1201) for seed in range(100, 108)]


@pytest.mark.parametrize("amp", [0.0, 0.15])
def test_performed_onsets_on_warped_renders(dev, clips, amp):
    from piano_a2s_amd import hip, resynth, transcribe
    bars, clips = clips
    hop, n_samples = scoregen.HOP, 1200 * scoregen.HOP
    rng = np.random.default_rng(WARP_SEED)
    scns = [oracle.warped_clip(c, bars, amp, rng) for c in clips]
    vqt = transcribe._vqt(dev, HP)
    x = _render_features(dev, vqt, [s["warped"] for s in scns], n_samples)
    windows = [{"events": s["straight"], "bar_lines": s["lines"]} for s in scns]
    n0, a0 = hip.dtw_launches(), hip.agreement_launches()
    waves, plain, aligned = resynth.resynthesise(windows, x, vqt, hop, align=True)
    assert hip.dtw_launches() == n0 + 2 and hip.agreement_launches() == a0 + 4, "one DTW call and one more agreement call per batch"
    n0, a0 = hip.dtw_launches(), hip.agreement_launches()
    waves2, plain2 = resynth.resynthesise(windows, x, vqt, hop)
    assert plain2 == plain and all(np.array_equal(a, b) for a, b in zip(waves, waves2)), "the agreements and waves do not depend on the option"
    assert hip.dtw_launches() == n0 and hip.agreement_launches() == a0 + 2, "off: nothing of the alignment is launched"
    linear, moved, agr, agr_w = [], [], [], []
    for scn, p, al in zip(scns, plain, aligned):
        assert len(al) == bars and all((a is None) == (q is None) for a, q in zip(al, p))
        for b, (a, q) in enumerate(zip(al, p)):
            if a is None:
                continue
            f0, f1 = scn["lines"][b] // hop, scn["lines"][b + 1] // hop
            assert (a["first_frame"], a["frames"]) == (f0, f1 - f0) and a["warp"].shape == (f1 - f0,) and a["inverse"].shape == (f1 - f0,)
            assert np.all(np.diff(a["warp"]) >= 0) and 0 <= a["warp"][0] and a["warp"][-1] <= f1 - f0 - 1
            assert np.abs(a["warp"] - np.arange(f1 - f0)).max() <= resynth.dtw_band(f1 - f0), "inside the band"
            agr.append(q)
            agr_w.append(a["agreement_warped"])
            if amp == 0.0:
                assert np.array_equal(a["warp"], np.arange(f1 - f0)) and a["total"] == 0.0 and a["agreement_warped"] == q, (b, a["total"])
        lin, mov = oracle.onset_errors(scn, [None if a is None else (a["warp"], a["first_frame"]) for a in al], hop, resynth.performed_notes)
        linear += lin
        moved += mov
    assert len(linear) > 400 and len(agr) == 40
    ms = 1e3 / scoregen.SR
    print(f"|a| = {amp}: {len(linear)} notes, median onset error linear {np.median(linear) * ms:.2f} ms, aligned {np.median(moved) * ms:.2f} ms; "
          f"mean agreement {np.mean(agr):.4f}, warped {np.mean(agr_w):.4f}")
    if amp == 0.0:
        assert max(linear) == 0 and max(moved) == 0.0, "a straight performance: every performed onset IS its notes onset"
        assert agr_w == agr
    else:
        # measured (profiles/dtw_alignment.json, "test_scenario"): 1.97 ms against 174.5 ms, a ratio of 0.0113; the bound is that ratio plus half
        # its distance to 1
        assert np.median(moved) < 0.506 * np.median(linear), "the performed onsets are nearer to the truth than linear placement"
        assert np.mean(agr_w) >= np.mean(agr)


# ------------------------------------------------------------------------------------------- 7. transcribe_waveform, the command line
@pytest.fixture(scope="module")
def state():
    return spec.procedural_state(spec.default_cfg(**SMALL), 11, eos_bias=3.0, lively=True)


@pytest.fixture(scope="module")
def recording(dev):
    """20 s at 16 kHz: a rendered clip and then 8 s of a second one, below full scale; downbeats that cut it into windows of 5 and 3 bars."""
    from piano_a2s_amd.render import render
    cfg = spec.default_cfg()
    w = render(torch.from_numpy(np.stack([scoregen.pack_program(scoregen.make_clip(cfg, s, frames=1201)) for s in (2024, 2025)])).to(dev)).cpu().numpy()
    x = np.concatenate([w[0], w[1][:128000]])
    return (x * (0.8 / np.abs(x).max())).astype(np.float32), [0.5, 2.75, 5.0, 7.25, 9.5, 11.75, 14.0, 16.5, 19.0]


def test_align_notes_adds_its_keys_and_changes_nothing_else(dev, state, recording):
    import models
    from piano_a2s_amd import hip, transcribe
    x, downbeats = recording
    model = models.ScoreTranscription(**SMALL)
    model.load_state_dict(state)
    model = model.to(dev).eval()
    model.constrained_decoding = True                            # (an untrained model under the grammar still writes notes)
    n0 = hip.dtw_launches()
    off = transcribe.transcribe_waveform(model, x, 16000, downbeats=downbeats, hparams=HP, resynthesis=True)
    assert hip.dtw_launches() == n0, "without the option nothing of the alignment is launched"
    on = transcribe.transcribe_waveform(model, x, 16000, downbeats=downbeats, hparams=HP, resynthesis=True, align_notes=True)
    assert hip.dtw_launches() == n0 + 2, "both windows in one batch: one cost launch, one path launch"
    assert set(on) == set(off) and np.array_equal(on["resynthesis"]["wave"], off["resynthesis"]["wave"])
    assert {k: v for k, v in on.items() if k not in ("windows", "resynthesis")} == {k: v for k, v in off.items() if k not in ("windows", "resynthesis")}
    some = False
    for w_off, w_on in zip(off["windows"], on["windows"]):
        assert set(w_on) == set(w_off) | {"agreement_warped"}
        assert {k: v for k, v in w_on.items() if k not in ("bars", "agreement_warped")} == {k: v for k, v in w_off.items() if k != "bars"}
        for b_off, b_on in zip(w_off["bars"], w_on["bars"]):
            assert set(b_on) == set(b_off) | {"agreement_warped", "performed"}
            assert {k: b_on[k] for k in b_off} == b_off, "every earlier key is unchanged"
            assert (b_on["agreement_warped"] is None) == (b_on["agreement"] is None)
            assert b_on["agreement_warped"] is None or -1.0 <= b_on["agreement_warped"] <= 1.0
            assert len(b_on["performed"]) == len(b_on["notes"])
            for (o, ln, m), (o2, ln2, m2) in zip(b_on["notes"], b_on["performed"]):
                assert m2 == m and ln2 > 0 and w_on["start_s"] <= o2 and o2 + ln2 <= w_on["stop_s"] + 1e-9
                some = True
        have = [b["agreement_warped"] for b in w_on["bars"] if b["agreement_warped"] is not None]
        assert (w_on["agreement_warped"] is None) if not have else abs(w_on["agreement_warped"] - sum(have) / len(have)) <= 1e-12
    assert some, "the seeded model decodes some note"
    with pytest.raises(ValueError, match="align_notes"):
        transcribe.transcribe_waveform(model, x, 16000, downbeats=downbeats, hparams=HP, align_notes=True)


def test_command_line_writes_the_midi_file(tmp_path, state, recording):
    from piano_a2s_amd import audio
    x, downbeats = recording
    wav = tmp_path / "take.wav"
    audio.write_wav(wav, x[:96000], 16000, bits=16)
    ann = tmp_path / "downbeats.txt"
    ann.write_text("".join(f"{t}\n" for t in downbeats if t < 6.0))
    ck = tmp_path / "weights.pt"
    torch.save(state, ck)
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "transcribe.py"), os.path.join(ROOT, "hparams", "finetune.yaml"), "--checkpoint", str(ck), str(wav),
                        "--out", str(out), "--downbeats", str(ann), "--align_notes", "--constrained_decoding", "--conv_feature_size=32", "--hidden_size=32",
                        "--max_length=(12, 8)"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(out / "take.json") as f:
        res = json.load(f)
    assert res["performance"] == {"file": "take.mid"} and res["resynthesis"]["file"] == "take.resynth.wav", "--align_notes implies --resynthesis"
    bars = [b for w in res["windows"] for b in w["bars"]]
    assert all("agreement_warped" in b and "performed" in b for b in bars)
    assert (out / "take.mid").read_bytes() == audio.midi_bytes([n for b in bars for n in b["performed"]])
    assert (out / "take.mid").read_bytes()[:14] == b"MThd" + bytes([0, 0, 0, 6, 0, 0, 0, 1, 0x01, 0xF4])
