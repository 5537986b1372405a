"""Note dynamics on the MI355X (csrc/a2s_dynamics.hip, piano_a2s_amd/resynth.py):

1. a2s_note_levels against the float64 oracle (tests/dynamics_oracle.py) through the raw ABI: B = 3, T = 37, F = 24 and F = 23, clips T * F, T * F + 8
   and T * F + 7 apart with NaN in the padding; rows with n in {0, 1, 5, 12}, fx != fy, fx or fy negative or within n of T, bins -1, 0 and F - 1, clips
   outside [0, B), repeated and out of order.  On a grid of 1/8 the sums EQUAL float64; on uniform inputs they are within a relative 2^-40 (a double
   accumulation of at most 108 fp32 values rounds at most 107 times, 107 * 2^-53 < 2^-46; the oracle's own float64 sums the same; 2^-40 leaves both
   room).  A row alone in another table and in a one-clip tensor is bit-equal to itself in the big one; two runs are bit-identical;
2. a2s_note_amp_update on the levels kernel's OWN sums: clips of 5, 0, 300, 1 and 2 rows, a tie at the median, levels that hit both clamps, a row
   without cells (count = 0).  cum is bit-equal to the numpy float32 restatement; the amplitudes are within the a-priori bound of the float64
   definition; every program word but word 3 of the listed rows, and every header, is unchanged.
   The bound (tests/dynamics_oracle.py: amp_bound), relative to the amplitude base * 10^(cum / 20), u = 2^-24: the kernel forms a^ = fl(cum * K32)
   with K32 = fl(log2(10) / 20), so a^ is off by at most |a| (2 u + u^2), |a| <= 30 * 0.16610 < 4.99, which moves 2^a by at most the factor
   ln 2 * 2.0001 |a| u <= 6.92 u; the device's exp2f is within 1 ulp = 2 u (HIP's math tables; v_exp_f32); the product with base rounds once, u:
   9.92 u at |cum| = 30, 3 u at cum = 0, times 1.001 for the cross terms;
3. refusals return -1, set a2s_last_error and launch nothing; the wrappers' checks (a prog_row outside the program is refused by hip.note_table: the
   table lives on the device and the entry point reads nothing back); through the raw ABI such a row (-1, 0, program_stride, 2^31 - 1, a negative one
   that points into the clip before) still has its cum updated and writes no word: header and neighbouring programs stay as they were;
4. the loop on four rendered clips (seeds 100 .. 103, T = 1201, amplitudes 0.3 .. 1.0, a phantom beside every third note) on the GPU render and VQT:
   level_db after K = 3 against the float64 loop, the rms error against the true levels after round 3 below that after round 1, the AUC of real over
   phantom and the rms error against what tools/dynamics_check.py gives on exactly these clips; dynamics=0 launches and returns nothing new;
5. transcribe_waveform(dynamics=True): the keys, parallel to "notes"; the MIDI file carries the velocities; dynamics without resynthesis raises.

Measured on the MI355X (the figures the tests print) are recorded in DESIGN.md section 26."""
import numpy as np
import pytest
import torch

from piano_a2s_amd import scoregen, spec
from tests import dynamics_oracle as oracle

pytestmark = pytest.mark.gpu
SMALL = dict(conv_feature_size=32, hidden_size=32, max_length=(12, 8))
HP = dict(sample_rate=16000, hop_length=160, max_frame_num=1201, max_bars=5, bins_per_octave=60, n_octaves=8, gamma=20)
LEAD = 8
GUARD = 16
SENTINEL = -12345.5


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


def _levels(dev, xd, yd, stride, shape, rows):
    """a2s_note_levels through the raw ABI on an output with sentinels around it -> (S, 3) float64 numpy."""
    from piano_a2s_amd import hip
    Lib = hip.lib()
    B, T, F = shape
    rows = np.asarray(rows, dtype=np.int32).reshape(-1, 8)
    S = len(rows)
    out = torch.full((GUARD + 3 * S + GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    rd = torch.from_numpy(rows).to(dev)
    n0 = hip.dynamics_launches()
    rc = Lib.a2s_note_levels(hip.stream(), hip._p(xd), hip._p(yd), stride, B, T, F, hip._p(rd), S, hip._p(out[GUARD:]))
    assert rc == 0, Lib.a2s_last_error()
    assert hip.dynamics_launches() == n0 + 1, "one launch"
    h = out.cpu().numpy()
    assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + 3 * S:] == SENTINEL).all(), "nothing outside the output is written"
    return h[GUARD:GUARD + 3 * S].reshape(S, 3)


def _rows(F):
    """[clip, fx, fy, n, b1, b2, b3, prog_row]: n in {0, 1, 5, 12}; fx != fy; fx, fy negative and within n of T = 37; bins -1, 0, F - 1; clips outside
    [0, 3); repeated and out of order."""
    L = F - 1
    return [(2, 3, 3, 5, 0, 10, L, 1), (0, 0, 4, 12, 5, 11, 17, 2), (1, -3, 2, 5, 0, -1, L, 3), (0, 6, -2, 5, 1, 2, 3, 4), (1, 30, 20, 12, 7, L, -1, 5),
            (2, 20, 33, 12, L, 0, 9, 6), (3, 3, 3, 5, 0, 10, L, 7), (-1, 3, 3, 5, 0, 10, L, 8), (0, 5, 5, 0, 4, 5, 6, 9), (1, 36, 36, 1, L, -1, -1, 10),
            (2, 3, 3, 5, 0, 10, L, 1), (0, 36, 0, 5, 2, 8, 14, 11), (1, 9, 9, 1, -1, -1, -1, 12), (2, -20, 5, 12, 3, 4, 5, 13), (0, 0, 0, 12, 0, 1, 2, 14),
            (1, 12, 25, 12, F, F + 1, 4, 15), (0, 40, 40, 5, 4, 5, 6, 16), (2, 25, 25, 12, L, L, L, 17), (0, 0, 4, 12, 5, 11, 17, 2), (1, 2, 3, -4, 1, 2, 3, 18)]


# ------------------------------------------------------------------------------------------- 1. the level sums
@pytest.mark.parametrize("F", [24, 23])
def test_levels_against_the_oracle(dev, F):
    B, T = 3, 37
    rng = np.random.default_rng(F)
    rows = _rows(F)
    xg, yg = (rng.integers(0, 9, size=(B, T, F)).astype(np.float32) / 8.0 for _ in range(2))
    xu, yu = (rng.uniform(0.0, 1.0, size=(B, T, F)).astype(np.float32) for _ in range(2))
    want_g, want_u = oracle.levels(xg, yg, rows), oracle.levels(xu, yu, rows)
    assert want_g[0, 2] == 5 * 7 and want_g[14, 2] == 12 * 8 and want_g[1, 2] == 108 and not want_g[[6, 7, 8, 12, 16, 19]].any(), "the table covers what it says"
    assert want_g[2, 2] == 2 * 4 and want_g[3, 2] == 3 * 9 and want_g[4, 2] == 7 * 5 and want_g[5, 2] == 4 * 7 and want_g[13, 2] == 0
    worst, seen = 0.0, []
    for stride in (T * F, T * F + 8, T * F + 7):
        got = _levels(dev, _padded(xg, stride, dev), _padded(yg, stride, dev), stride, (B, T, F), rows)
        assert np.array_equal(got, want_g), (F, stride, np.nonzero(got != want_g))
        got = _levels(dev, _padded(xu, stride, dev), _padded(yu, stride, dev), stride, (B, T, F), rows)
        assert np.isfinite(got).all() and np.array_equal(got[:, 2], want_u[:, 2])
        err = np.abs(got[:, :2] - want_u[:, :2])
        assert (err <= 2.0 ** -40 * np.abs(want_u[:, :2])).all(), (F, stride, float((err / np.maximum(np.abs(want_u[:, :2]), 1e-300)).max()))
        worst = max(worst, float((err[want_u[:, :2] != 0] / np.abs(want_u[:, :2][want_u[:, :2] != 0])).max()))
        assert got[0].tobytes() == got[10].tobytes() and got[1].tobytes() == got[18].tobytes(), "a row listed twice"
        seen.append(got)
    assert all(s.tobytes() == seen[0].tobytes() for s in seen), "the clip stride does not reach the bits"
    print(f"F = {F}: worst relative |device - float64| on uniform inputs = 2^{np.log2(max(worst, 2.0 ** -60)):.1f}")


@pytest.mark.parametrize("F", [24, 23])
def test_a_row_does_not_depend_on_its_table_or_tensor(dev, F):
    B, T = 3, 37
    rng = np.random.default_rng(40 + F)
    x, y = (rng.uniform(0.0, 1.0, size=(B, T, F)).astype(np.float32) for _ in range(2))
    rows = _rows(F)
    xd, yd = _padded(x, T * F, dev), _padded(y, T * F, dev)
    first, again = _levels(dev, xd, yd, T * F, (B, T, F), rows), _levels(dev, xd, yd, T * F, (B, T, F), rows)
    assert first.tobytes() == again.tobytes(), "two runs are bit-identical"
    for s, row in enumerate(rows):
        alone = _levels(dev, xd, yd, T * F, (B, T, F), [row])
        assert alone[0].tobytes() == first[s].tobytes(), (s, row)
        if 0 <= row[0] < B:                                      # its clip as the only clip of another tensor
            c = row[0]
            one = _levels(dev, _padded(x[c:c + 1], T * F + 5, dev), _padded(y[c:c + 1], T * F + 5, dev), T * F + 5, (1, T, F), [(0,) + tuple(row[1:])])
            assert one[0].tobytes() == first[s].tobytes(), (s, row)


# ------------------------------------------------------------------------------------------- 2. the update
def _update_case(rng, F):
    """Clips of 5, 0, 300, 1 and 2 rows over features (5, 37, F): -> (rows (308, 8), first, cum0, E)."""
    L = F - 1
    sizes, E = [5, 0, 300, 1, 2], 300
    a, b, c = (0, 3, 3, 5, 0, 10, L), (0, 9, 20, 12, 4, 5, -1), (0, 30, 2, 5, 7, L, 3)
    rows = [a + (3,), a + (1,), b + (5,), a + (2,), c + (4,)]                       # three equal rows of five: the median is a tie whatever their value
    perm = rng.permutation(300) + 1
    for j in range(300):
        n = (1, 5, 12, 12)[j % 4]
        rows.append((2, int(rng.integers(-3, 36)), int(rng.integers(-3, 36)), n, int(rng.integers(0, F)), int(rng.integers(-1, F)), int(rng.integers(-1, F)),
                     int(perm[j])))
    rows[5 + 17] = (2, 5, 5, 12, -1, -1, -1, int(perm[17]))                         # count = 0: d = 0
    rows[5 + 40] = rows[5 + 41][:7] + (int(perm[40]),)                              # two equal rows next to each other
    rows += [(3, 4, 4, 5, 1, 2, 3, 300), (4, 6, 6, 5, 0, 8, L, 1), (4, 7, 2, 12, 9, 2, -1, 2)]
    first = np.concatenate([[0], np.cumsum(sizes)])
    cum0 = rng.uniform(-3.0, 3.0, size=len(rows)).astype(np.float32)
    cum0[[0, 1, 3]] = np.float32(0.625)                                            # the tie at the median
    cum0[5 + 40] = cum0[5 + 41]
    cum0[5 + 100:5 + 110] = rng.uniform(40.0, 90.0, size=10).astype(np.float32)    # far above the median: the upper clamp
    cum0[5 + 200:5 + 210] = rng.uniform(-90.0, -40.0, size=10).astype(np.float32)  # far below: the lower clamp
    return np.array(rows, dtype=np.int32), first, cum0, E


@pytest.mark.parametrize("F", [24, 23])
def test_update_against_the_restatement(dev, F):
    from piano_a2s_amd import hip
    Lib = hip.lib()
    rng = np.random.default_rng(70 + F)
    B, T = 5, 37
    rows, first, cum0, E = _update_case(rng, F)
    S = len(rows)
    x, y = (rng.uniform(0.0, 1.0, size=(B, T, F)).astype(np.float32) for _ in range(2))
    sums = _levels(dev, _padded(x, T * F, dev), _padded(y, T * F, dev), T * F, (B, T, F), rows)
    assert sums[5 + 17, 2] == 0 and sums[0].tobytes() == sums[1].tobytes() == sums[3].tobytes()
    # programs full of a pattern no update writes, sentinels around every buffer
    prog0 = rng.integers(-2 ** 31, 2 ** 31, size=(B, 1 + E, 8), dtype=np.int64).astype(np.int32)
    words = B * (1 + E) * 8
    pd = torch.full((GUARD + words + GUARD,), -7, dtype=torch.int32, device=dev)
    pd[GUARD:GUARD + words] = torch.from_numpy(prog0.reshape(-1)).to(dev)
    cd = torch.full((GUARD + S + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    cd[GUARD:GUARD + S] = torch.from_numpy(cum0).to(dev)
    sd, rd, fd = torch.from_numpy(sums).to(dev), torch.from_numpy(rows).to(dev), torch.from_numpy(first.astype(np.int32)).to(dev)
    base = 0.5
    n0 = hip.dynamics_launches()
    rc = Lib.a2s_note_amp_update(hip.stream(), hip._p(sd), hip._p(rd), hip._p(fd), B, hip._p(cd[GUARD:]), hip._p(pd[GUARD:]), 1 + E, base)
    assert rc == 0, Lib.a2s_last_error()
    assert hip.dynamics_launches() == n0 + 1, "one launch"
    ch, ph = cd.cpu().numpy(), pd.cpu().numpy()
    assert (ch[:GUARD] == SENTINEL).all() and (ch[GUARD + S:] == SENTINEL).all() and (ph[:GUARD] == -7).all() and (ph[GUARD + words:] == -7).all()
    cum, prog = ch[GUARD:GUARD + S], ph[GUARD:GUARD + words].reshape(B, 1 + E, 8)
    assert np.array_equal(sd.cpu().numpy(), sums) and np.array_equal(rd.cpu().numpy(), rows), "the inputs are read only"
    # cum: the float32 restatement, bit for bit
    want = oracle.update_f32(sums, first, cum0)
    assert cum.tobytes() == want.tobytes(), np.nonzero(cum != want)
    assert cum[0] == cum[1] == cum[3] == 0.0, "three equal rows of five: the median is one of them"
    assert (cum[5 + 100:5 + 110] == 12.0).all() and (cum[5 + 200:5 + 210] == -30.0).all() and cum[305] == 0.0 and cum[306:].min() == 0.0
    assert cum[5 + 40] == cum[5 + 41] and cum.min() == -30.0 and cum.max() == 12.0
    # the float64 definition of the same step agrees to fp32 rounding of c and of the median
    assert np.abs(oracle.update(sums, first, cum0.astype(np.float64)) - cum).max() < 1e-4
    # the programs: word 3 of the listed rows, within the a-priori bound of base * 10^(cum / 20); everything else untouched
    listed = np.zeros((B, 1 + E, 8), dtype=bool)
    listed[rows[:, 0], rows[:, 7], 3] = True
    assert listed.sum() == S and not listed[:, 0].any() and not listed[1].any()
    assert np.array_equal(prog[~listed], prog0[~listed]), "every other word, every header and the clip without rows are unchanged"
    amp = prog[rows[:, 0], rows[:, 7], 3].view(np.float32).astype(np.float64)
    err, bound = np.abs(amp - oracle.amplitudes_f64(cum, base)), oracle.amp_bound(cum, base)
    assert (err <= bound).all(), float((err / bound).max())
    print(f"F = {F}: worst |device amplitude - float64| / bound = {float((err / bound).max()):.3f}")
    # through the wrapper, on fresh buffers: the same bits
    rt, ft = hip.note_table(rows, first, B, 1 + E, dev)
    c2, p2 = torch.from_numpy(cum0).to(dev), torch.from_numpy(prog0).to(dev)
    s2 = hip.note_levels(_padded(x, T * F, dev), _padded(y, T * F, dev), rt)
    assert s2.cpu().numpy().tobytes() == sums.tobytes()
    hip.note_amp_update(s2, rt, ft, c2, p2, base)
    assert c2.cpu().numpy().tobytes() == cum.tobytes() and np.array_equal(p2.cpu().numpy(), prog)


# ------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_launch_nothing(dev):
    from piano_a2s_amd import hip
    Lib, st = hip.lib(), hip.stream()
    B, T, F, S, E = 2, 9, 24, 3, 4
    x, y = torch.rand(B, T, F, device=dev), torch.rand(B, T, F, device=dev)
    table = np.array([(0, 1, 1, 5, 0, 10, 23, 1), (0, 2, 3, 5, 1, 2, 3, 2), (1, 0, 0, 12, 4, 5, 6, 4)], dtype=np.int32)
    rows, first = torch.from_numpy(table).to(dev), torch.tensor([0, 2, 3], dtype=torch.int32, device=dev)
    out = torch.full((S, 3), SENTINEL, dtype=torch.float64, device=dev)
    cum = torch.full((S,), SENTINEL, dtype=torch.float32, device=dev)
    progs = torch.full((B, 1 + E, 8), -7, dtype=torch.int32, device=dev)
    n0, k0 = hip.dynamics_launches(), Lib.a2s_launch_count()
    ok = [hip._p(x), hip._p(y), T * F, B, T, F, hip._p(rows), S, hip._p(out)]
    for i, bad in ((0, None), (1, None), (6, None), (8, None), (3, 0), (3, -1), (4, 0), (5, 0), (5, -2), (7, -1), (2, T * F - 1)):
        args = list(ok)
        args[i] = bad
        assert Lib.a2s_note_levels(st, *args) == -1, (i, bad)
        assert b"note_levels" in Lib.a2s_last_error()
    ok2 = [hip._p(out), hip._p(rows), hip._p(first), B, hip._p(cum), hip._p(progs), 1 + E, 0.5]
    for i, bad in ((0, None), (1, None), (2, None), (4, None), (5, None), (3, 0), (3, -1), (3, 65536), (6, 1), (6, 0), (7, 0.0), (7, -0.5), (7, float("inf")),
                   (7, float("nan"))):
        args = list(ok2)
        args[i] = bad
        assert Lib.a2s_note_amp_update(st, *args) == -1, (i, bad)
        assert b"note_amp_update" in Lib.a2s_last_error()
    args = list(ok)
    args[7] = 0
    assert Lib.a2s_note_levels(st, *args) == 0, "S = 0 is fine"
    # the wrappers: a program row outside the program, rows of a clip apart, too many rows, wrong offsets, device tables, dtypes
    for bad_rows, bad_first in ((table + np.eye(8, dtype=np.int32)[7] * 4, [0, 2, 3]), (table * np.array([1, 1, 1, 1, 1, 1, 1, 0]), [0, 2, 3]), (table[[0, 2, 1]], [0, 2, 3]),
                                (table, [0, 2]), (table, [0, 3, 2]), (table, [1, 2, 3]), (table[:, :7], [0, 2, 3]), (table + 0.5, [0, 2, 3]),
                                (np.tile(table[:1], (hip.NOTE_ROWS_MAX + 1, 1)), [0, hip.NOTE_ROWS_MAX + 1, hip.NOTE_ROWS_MAX + 1])):
        with pytest.raises(hip.A2SError, match="note_table"):
            hip.note_table(bad_rows, bad_first, B, 1 + E, dev)
    with pytest.raises(hip.A2SError, match="`rows`"):
        hip.note_levels(x, y, table)
    with pytest.raises(hip.A2SError, match="`y`"):
        hip.note_levels(x, y[:, :4], rows)
    with pytest.raises(hip.A2SError, match="`x`"):
        hip.note_levels(x.transpose(1, 2), y.transpose(1, 2), rows)
    with pytest.raises(hip.A2SError, match="`out`"):
        hip.note_levels(x, y, rows, out=torch.zeros(S, 3, device=dev))
    with pytest.raises(hip.A2SError, match="`cum`"):
        hip.note_amp_update(out, rows, first, cum.double(), progs, 0.5)
    with pytest.raises(hip.A2SError, match="`first`"):
        hip.note_amp_update(out, rows, first[:2], cum, progs, 0.5)
    with pytest.raises(hip.A2SError, match="`programs`"):
        hip.note_amp_update(out, rows, first, cum, progs[:, :1], 0.5)
    with pytest.raises(hip.A2SError, match="`base_amp`"):
        hip.note_amp_update(out, rows, first, cum, progs, 0.0)
    assert tuple(hip.note_levels(x, y, rows[:0]).shape) == (0, 3)
    torch.cuda.synchronize()
    assert hip.dynamics_launches() == n0 and Lib.a2s_launch_count() == k0, "nothing was launched"
    assert (out == SENTINEL).all() and (cum == SENTINEL).all() and (progs == -7).all()
    rt, ft = hip.note_table(table, [0, 2, 3], B, 1 + E, dev)
    assert torch.equal(rt, rows) and torch.equal(ft, first)
    assert Lib.a2s_note_levels(st, *ok) == 0
    cum.zero_()
    assert Lib.a2s_note_amp_update(st, *ok2) == 0
    torch.cuda.synchronize()
    assert hip.dynamics_launches() == n0 + 2 and (progs[0, 1:3, 3] != -7).all() and (progs[1, 4, 3] != -7) and (progs[:, 0] == -7).all() and (progs[0, 3:] == -7).all()


def test_a_program_row_outside_the_program_writes_no_word(dev):
    """The table is on the device and the entry point reads nothing back, so a prog_row outside 1 .. program_stride - 1 cannot be refused there
    (include/a2s.h): the kernel's own guard is what keeps the header and the neighbouring program safe.  cum is still updated; no word is written."""
    from piano_a2s_amd import hip
    Lib = hip.lib()
    B, E, S = 2, 4, 7
    stride = 1 + E
    # clip 0: prog_row -1, 0 (the header), 5 = program_stride (the header of clip 1's program), 2 (valid), 2^31 - 1; clip 1: -5 (inside clip 0's program), 3 (valid)
    table = np.array([(0, 0, 0, 1, 0, -1, -1, -1), (0, 0, 0, 1, 0, -1, -1, 0), (0, 0, 0, 1, 0, -1, -1, stride), (0, 0, 0, 1, 0, -1, -1, 2),
                      (0, 0, 0, 1, 0, -1, -1, 2 ** 31 - 1), (1, 0, 0, 1, 0, -1, -1, -stride), (1, 0, 0, 1, 0, -1, -1, 3)], dtype=np.int32)
    first = np.array([0, 5, 7], dtype=np.int32)
    sums = np.array([(0.25 * s, 0.125, 2.0) for s in range(S)], dtype=np.float64)          # d = 80 (0.25 s - 0.125) / 2: 10 dB apart, every row distinct
    cum0 = np.linspace(-1.0, 1.0, S).astype(np.float32)
    words = B * stride * 8
    pd = torch.full((GUARD + words + GUARD,), -7, dtype=torch.int32, device=dev)
    cd = torch.full((GUARD + S + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    cd[GUARD:GUARD + S] = torch.from_numpy(cum0).to(dev)
    sd, rd, fd = torch.from_numpy(sums).to(dev), torch.from_numpy(table).to(dev), torch.from_numpy(first).to(dev)
    n0 = hip.dynamics_launches()
    rc = Lib.a2s_note_amp_update(hip.stream(), hip._p(sd), hip._p(rd), hip._p(fd), B, hip._p(cd[GUARD:]), hip._p(pd[GUARD:]), stride, 0.5)
    assert rc == 0, Lib.a2s_last_error()
    assert hip.dynamics_launches() == n0 + 1
    ch, ph = cd.cpu().numpy(), pd.cpu().numpy()
    assert (ch[:GUARD] == SENTINEL).all() and (ch[GUARD + S:] == SENTINEL).all() and (ph[:GUARD] == -7).all() and (ph[GUARD + words:] == -7).all()
    cum, prog = ch[GUARD:GUARD + S], ph[GUARD:GUARD + words].reshape(B, stride, 8)
    assert cum.tobytes() == oracle.update_f32(sums, first, cum0).tobytes(), "cum is updated for every row, listed in the program or not"
    written = prog != -7
    assert written.sum() == 2 and written[0, 2, 3] and written[1, 3, 3], "only the two rows inside their programs receive an amplitude"
    amp = prog[[0, 1], [2, 3], 3].view(np.float32).astype(np.float64)
    assert (np.abs(amp - oracle.amplitudes_f64(cum[[3, 6]], 0.5)) <= oracle.amp_bound(cum[[3, 6]], 0.5)).all()
    for bad in (-1, 0, stride):
        with pytest.raises(hip.A2SError, match="note_table"):
            hip.note_table(table[:1] * np.array([1, 1, 1, 1, 1, 1, 1, 0]) + np.eye(8, dtype=np.int32)[7] * bad, [0, 1, 1], B, stride, dev)


# ------------------------------------------------------------------------------------------- 4. the loop on rendered clips
CLIP_SEEDS = (100, 101, 102, 103)
PHANTOM_SEED = 26          # tools/dynamics_check.py --clips 4 (its default seed): the float64 definitions alone on exactly these clips and phantoms give,
CHECK_AUC = 0.98923        # after round 3, an AUC of real over phantom of 0.98923,
CHECK_RMS = 0.44405        # an rms level error of 0.44405 dB (0.83652 dB after round 1)
CHECK_SPREAD = 2.81308     # and the true levels, centred per clip, have a standard deviation of 2.81308 dB


@pytest.fixture(scope="module")
def scenarios():
    from tests import dtw_oracle
    cfg = spec.default_cfg(max_length=(200, 200))
    rng = np.random.default_rng(PHANTOM_SEED)
    out = []
    for seed in CLIP_SEEDS:
        clip = scoregen.make_clip(cfg, seed, frames=1201)
        scn = oracle.scenario(clip, rng, phantom_every=3)
        scn["lines"] = dtw_oracle.clip_lines(clip, cfg["max_bars"])
        out.append(scn)
    return out


@pytest.fixture(scope="module")
def float64_levels(scenarios):
    """The float64 loop of tools/dynamics_check.py on the same clips: per clip the levels after rounds 1, 2, 3.  Computed once."""
    from piano_a2s_amd import resynth
    n_samples = 1200 * scoregen.HOP
    return [oracle.loop64(oracle.features64(resynth.program(s["events"], n_samples, amps=s["amps"]), n_samples), s["score"], n_samples, scoregen.HOP, 3)
            for s in scenarios]


def _pooled(cums, scenarios):
    """(rms error in dB against the true levels over the real notes, both centred per clip; AUC of real over phantom), pooled as dynamics_check pools."""
    got, true, real = [], [], []
    for cum, s in zip(cums, scenarios):
        r = s["real"]
        got.append(np.asarray(cum, dtype=np.float64) - np.asarray(cum, dtype=np.float64)[r].mean())
        true.append(s["true_db"] - s["true_db"][r].mean())
        real.append(r)
    got, true, real = np.concatenate(got), np.concatenate(true), np.concatenate(real)
    err = got[real] - true[real]
    return float(np.sqrt(np.mean(err * err))), oracle.auc(got[real], got[~real])


def test_the_loop_on_rendered_clips(dev, scenarios, float64_levels):
    from piano_a2s_amd import hip, render, resynth, transcribe
    hop, n_samples = scoregen.HOP, 1200 * scoregen.HOP
    vqt = transcribe._vqt(dev, HP)
    progs = np.stack([resynth.program(s["events"], n_samples, amps=s["amps"]) for s in scenarios])
    x = vqt(render.render(torch.from_numpy(progs).to(dev), n_samples))
    windows = [{"events": s["score"], "bar_lines": s["lines"]} for s in scenarios]
    # the float64 side is what the tool reports
    rms64, auc64 = _pooled([c[2] for c in float64_levels], scenarios)
    assert abs(rms64 - CHECK_RMS) < 5e-5 and abs(auc64 - CHECK_AUC) < 5e-5 and abs(_pooled([c[0] for c in float64_levels], scenarios)[0] - 0.83652) < 5e-5
    # off: nothing new is launched or returned
    n0, r0, a0 = hip.dynamics_launches(), hip.render_launches(), hip.agreement_launches()
    off = resynth.resynthesise(windows, x, vqt, hop)
    assert len(off) == 2 and hip.dynamics_launches() == n0 and hip.render_launches() == r0 + 1 and hip.agreement_launches() == a0 + 2
    got = {}
    for K in (1, 3):
        n0, r0, a0 = hip.dynamics_launches(), hip.render_launches(), hip.agreement_launches()
        waves, agr, dyn = resynth.resynthesise(windows, x, vqt, hop, dynamics=K)
        assert hip.dynamics_launches() == n0 + 2 * K, "two launches per round"
        assert hip.render_launches() == r0 + K + 1 and hip.agreement_launches() == a0 + 4, "round 1 reads the unit pass; one final render and scoring"
        assert agr == off[1], "the plain agreements are those of the unit-amplitude pass"
        for s, d, w in zip(scenarios, dyn, waves):
            assert d["level_db"].shape == (len(s["score"]),) and d["level_db"].dtype == np.float32 and d["level_db"].min() >= -30.0 and d["level_db"].max() <= 12.0
            assert [resynth.velocity(v) for v in d["level_db"]] == d["velocity"].tolist() and len(d["agreement"]) == 5 and "agreement_warped" not in d
            assert np.abs(w).max() < 1.0 and w.shape == (n_samples,)
        got[K] = [d["level_db"] for d in dyn]
    # the levels against the float64 loop, over the real notes (a phantom's level is the difference of two noise floors)
    diff = np.concatenate([(g - c[2])[s["real"]] for g, c, s in zip(got[3], float64_levels, scenarios)])
    step = np.concatenate([(c[2] - c[1])[s["real"]] for c, s in zip(float64_levels, scenarios)])
    rms_diff, rms_step = float(np.sqrt(np.mean(diff * diff))), float(np.sqrt(np.mean(step * step)))
    (rms1, auc1), (rms3, auc3) = _pooled(got[1], scenarios), _pooled(got[3], scenarios)
    print(f"level_db after K = 3, device against float64 over {len(diff)} real notes: rms {rms_diff:.3e} dB, max {np.abs(diff).max():.3e} dB "
          f"(what round 3 itself moves in float64: rms {rms_step:.4f} dB)")
    print(f"rms error against the true levels: {rms1:.4f} dB after round 1, {rms3:.4f} dB after round 3 (float64: 0.83652, {CHECK_RMS}); "
          f"AUC {auc1:.5f}, {auc3:.5f} (float64: {CHECK_AUC})")
    # What the comparison guards against is a loop that is one round short or long: in float64 round 3 moves the real notes' levels by rms_step.
    # Measured on the MI355X: rms_diff = 1.26e-6 dB, max 6.7e-6 dB (the fp32 render and front end are that close to the float64
    # ones at the cells of a sounding note); rms_step = 0.1585 dB.  The bound is the measured value plus half its distance to rms_step.
    assert rms_diff < MEASURED_DIFF + 0.5 * (rms_step - MEASURED_DIFF), (rms_diff, rms_step)
    assert rms3 < rms1, "the iteration sorts out what the one-shot reading cannot"
    assert auc3 > 0.5 * (CHECK_AUC + 0.5), "above the midpoint between the float64 value and chance"
    assert rms3 < 0.5 * (CHECK_RMS + CHECK_SPREAD), "below the midpoint between the float64 value and knowing nothing (the spread of the true levels)"
    mean_plain = np.mean([a for w in off[1] for a in w if a is not None])
    mean_dyn = np.mean([a for d in dyn for a in d["agreement"] if a is not None])
    print(f"mean bar agreement {mean_plain:.4f} at unit amplitudes, {mean_dyn:.4f} at the estimated dynamics")


MEASURED_DIFF = 1.3e-6       # dB, measured on the MI355X (see the assertion that uses it)


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


def test_transcribe_waveform_with_dynamics(dev, state, recording, tmp_path):
    import models
    from piano_a2s_amd import audio, hip, transcribe
    x, downbeats = recording
    model = models.ScoreTranscription(**SMALL)
    model.load_state_dict(state)
    model = model.to(dev).eval()
    model.constrained_decoding = True                            # (an untrained model under the grammar still writes notes)
    n0 = hip.dynamics_launches()
    off = transcribe.transcribe_waveform(model, x, 16000, downbeats=downbeats, hparams=HP, resynthesis=True, align_notes=True)
    assert hip.dynamics_launches() == n0, "without the option nothing of it is launched"
    on = transcribe.transcribe_waveform(model, x, 16000, downbeats=downbeats, hparams=HP, resynthesis=True, align_notes=True, dynamics=True, min_level_db=-10.0)
    assert hip.dynamics_launches() == n0 + 2 * 3, "three rounds, two launches each"
    plain = transcribe.transcribe_waveform(model, x, 16000, downbeats=downbeats, hparams=HP, resynthesis=True, dynamics=True, dynamics_rounds=1)
    assert hip.dynamics_launches() == n0 + 2 * 3 + 2
    assert set(on) == set(off) and on["resynthesis"]["wave"].shape == off["resynthesis"]["wave"].shape and np.abs(on["resynthesis"]["wave"]).max() < 1.0
    assert not np.array_equal(on["resynthesis"]["wave"], off["resynthesis"]["wave"]), "the wave is the render at the estimated dynamics"
    some = 0
    for w_off, w_on, w_pl in zip(off["windows"], on["windows"], plain["windows"]):
        assert set(w_on) == set(w_off) | {"agreement_dynamics", "agreement_dynamics_warped"} and "agreement_dynamics_warped" not in w_pl
        assert {k: v for k, v in w_on.items() if k not in ("bars", "agreement_dynamics", "agreement_dynamics_warped")} == {k: v for k, v in w_off.items() if k != "bars"}
        for b_off, b_on, b_pl in zip(w_off["bars"], w_on["bars"], w_pl["bars"]):
            aligned = b_on["agreement_warped"] is not None
            assert set(b_on) == set(b_off) | {"dynamics", "agreement_dynamics", "quiet"} | ({"agreement_dynamics_warped"} if aligned else set())
            assert {k: b_on[k] for k in b_off} == b_off, "every earlier key is unchanged"
            assert set(b_pl) == (set(b_off) - {"agreement_warped", "performed"}) | {"dynamics", "agreement_dynamics"}
            assert len(b_on["dynamics"]) == len(b_on["notes"]) == len(b_on["quiet"]) == len(b_pl["dynamics"])
            assert (b_on["agreement_dynamics"] is None) == (b_on["agreement"] is None)
            for (level, vel), quiet in zip(b_on["dynamics"], b_on["quiet"]):
                assert -30.0 <= level <= 12.0 and 1 <= vel <= 127 and vel == oracle.velocity(level) and quiet == (level < -10.0)
                some += 1
            for v in (b_on["agreement_dynamics"], b_on.get("agreement_dynamics_warped")):
                assert v is None or -1.0 <= v <= 1.0
        have = [b["agreement_dynamics"] for b in w_on["bars"] if b["agreement_dynamics"] is not None]
        assert (w_on["agreement_dynamics"] is None) if not have else abs(w_on["agreement_dynamics"] - sum(have) / len(have)) <= 1e-12
    assert some >= 5, "the seeded model decodes some notes"
    # the MIDI file carries the velocities of the notes that are not quiet, at the performed times
    bars = [b for w in on["windows"] for b in w["bars"]]
    want = [list(n) + [d[1]] for b in bars for n, d, q in zip(b["performed"], b["dynamics"], b["quiet"]) if not q]
    assert audio.result_notes(on) == want and 0 < len(want) <= some
    audio.write_midi(tmp_path / "take.mid", on)
    data = (tmp_path / "take.mid").read_bytes()
    assert data == audio.midi_bytes(want) and (len(want) == 0 or data != audio.midi_bytes([n[:3] for n in want]) or all(n[3] == 64 for n in want))
    with pytest.raises(ValueError, match="dynamics"):
        transcribe.transcribe_waveform(model, x, 16000, downbeats=downbeats, hparams=HP, dynamics=True)
    with pytest.raises(ValueError, match="dynamics"):
        transcribe.transcribe_waveform(model, x, 16000, downbeats=downbeats, hparams=HP, resynthesis=True, min_level_db=-10.0)
