"""The device stages of the beat tracker (csrc/a2s_beat.hip) against tests/beat_oracle.py: onset strength (exact on a grid of
1/8, the a-priori fp32 bound on random inputs, alignment, NaN behind n_rows, batch independence), tempogram (the bound of its fp32 sums), the beat
dynamic programme (bit for bit), refusals and counters, and a rendered recording end to end through VQT, tracker and transcribe_waveform."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beat_oracle as bo  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 777.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------- 1. onset strength
def _onset_run(dev, x, n_rows, lag, f_split, aligned):
    """x (B, rows, F) float32 on the host.  The device copy holds NaN in every row at and behind n_rows[b] and between the rows and the clips; its row
    and clip strides are multiples of 16 bytes from a 16-byte aligned base (aligned) or break that.  The outputs have sentinels on both sides.
    -> (env_full, env_low) (B, rows) on the host."""
    from piano_a2s_amd import hip
    B, rows, F = x.shape
    rs = F + ((-F) % 4 + 4 if aligned else 1)
    if not aligned and rs % 4 == 0:
        rs += 1
    bs = rows * rs + (8 if aligned else 3)
    x_off = 0 if aligned else 1
    xbuf = torch.full((B * bs + 8,), float("nan"), dtype=torch.float32)
    xv = torch.as_strided(xbuf, (B, rows, F), (bs, rs, 1), x_off)
    for b in range(B):
        xv[b, :n_rows[b]] = torch.from_numpy(x[b, :n_rows[b]])
    xbuf = xbuf.to(dev)
    xd = torch.as_strided(xbuf, (B, rows, F), (bs, rs, 1), x_off)
    pad = 4 if aligned else 3
    es = pad + rows + pad
    es += (-es) % 4 if aligned else (1 if es % 4 == 0 else 0)
    ebuf = torch.full((2, B, es), SENT, dtype=torch.float32, device=dev)
    ef, el = ebuf[0, :, pad:pad + rows], ebuf[1, :, pad:pad + rows]
    assert (xd.data_ptr() % 16 == 0 and rs % 4 == 0 and bs % 4 == 0) == aligned and (ef.data_ptr() % 16 == 0 and el.data_ptr() % 16 == 0 and es % 4 == 0) == aligned
    out = hip.onset_strength(xd, torch.tensor(n_rows, dtype=torch.int32, device=dev), lag, f_split, env_full=ef, env_low=el)
    assert out[0].data_ptr() == ef.data_ptr() and out[1].data_ptr() == el.data_ptr()
    torch.cuda.synchronize()
    full = ebuf.cpu()
    assert (full[:, :, :pad] == SENT).all() and (full[:, :, pad + rows:] == SENT).all(), "the sentinels around the envelopes"
    return full[0, :, pad:pad + rows].clone().numpy(), full[1, :, pad:pad + rows].clone().numpy()


def _grid_clips(rng, B, rows, F):
    return (rng.integers(0, 9, size=(B, rows, F)) / 8.0).astype(np.float32)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("lag", [1, 2])
@pytest.mark.parametrize("F", [480, 7])
def test_onset_exact_on_a_grid_and_bounded_on_random_inputs(dev, F, lag, aligned):
    B, rows = 3, 37
    n_rows = [0, lag, rows]
    rng = np.random.default_rng(1000 * F + 10 * lag + aligned)
    grid = _grid_clips(rng, B, rows, F)
    rand = rng.uniform(0, 1, size=(B, rows, F)).astype(np.float32)
    worst = 0.0
    for f_split in (0, 3, F):
        ef, el = _onset_run(dev, grid, n_rows, lag, f_split, aligned)
        wf, wl = bo.onset_strength(grid, n_rows, lag, f_split)
        assert np.array_equal(ef, wf.astype(np.float32)) and np.array_equal(el, wl.astype(np.float32)), (f_split, "a grid of 1/8: exact")
        assert (ef[:2] == 0).all() and (el[:2] == 0).all() and ef[2, lag:].max() > 0 and (ef[2, :lag] == 0).all()
        assert (el[2] == 0).all() if f_split == 0 else el[2, lag:].max() > 0
        ef, el = _onset_run(dev, rand, n_rows, lag, f_split, aligned)
        wf, wl, bf, bl = bo.onset_strength(rand, n_rows, lag, f_split, with_bound=True)
        for got, want, bound in ((ef, wf, bf), (el, wl, bl)):
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= bound).all(), f"f_split {f_split}: {err.max():.3e}"
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        if f_split == F:
            assert np.array_equal(ef, el)
    print(f"onset strength F = {F}, lag = {lag}, aligned = {aligned}: at most {worst:.3f} of the bound (F + 1) u / (1 - (F + 1) u) * sum |terms|")


@pytest.mark.parametrize("F,lag", [(480, 2), (7, 3), (1028, 1), (300, 1)])
def test_onset_over_several_segments_and_column_tiles(dev, F, lag):
    """150 rows are three runs of 64 (the rows in front of a run come from memory, the others from LDS); 1028 and 300 columns are more than one column
    per thread on the 16-byte and on the 4-byte path; n_rows inside a run, at its edge and just behind it."""
    rows = 150
    n_rows = [150, 64, 65, 100, 1]
    rng = np.random.default_rng(F + lag)
    grid = _grid_clips(rng, len(n_rows), rows, F)
    for aligned in (True, False):
        ef, el = _onset_run(dev, grid, n_rows, lag, min(180, F), aligned)
        wf, wl = bo.onset_strength(grid, n_rows, lag, min(180, F))
        assert np.array_equal(ef, wf.astype(np.float32)) and np.array_equal(el, wl.astype(np.float32)), aligned
        assert ef[0, lag:].max() > 0 and ef[0, 128:].max() > 0


def test_onset_a_clips_bits_do_not_depend_on_the_batch(dev):
    rows, F, lag = 150, 480, 1
    rng = np.random.default_rng(3)
    clip = rng.uniform(0, 1, size=(1, rows, F)).astype(np.float32)
    others = rng.uniform(0, 1, size=(2, rows, F)).astype(np.float32)
    alone_f, alone_l = _onset_run(dev, clip, [rows], lag, 180, True)
    batch = np.concatenate([others[:1], clip, others[1:]])
    bf, bl = _onset_run(dev, batch, [40, rows, 150], lag, 180, True)
    assert np.array_equal(alone_f[0], bf[1]) and np.array_equal(alone_l[0], bl[1]) and alone_f.max() > 1
    short_f, _ = _onset_run(dev, clip, [77], lag, 180, True)                          # fewer rows of the same clip: the same bits where they exist
    assert np.array_equal(short_f[0, :77], alone_f[0, :77]) and (short_f[0, 77:] == 0).all()


def test_onset_front_door(dev):
    from piano_a2s_amd import hip
    x = torch.rand((2, 1, 20, 480), device=dev)
    n = torch.tensor([20, 7], dtype=torch.int32, device=dev)
    k0 = hip.beat_launches()
    ef, el = hip.onset_strength(x, n)                                                 # (B, 1, rows, F) as the VQT returns it; lag 1, f_split 180
    assert hip.beat_launches() == k0 + 1 and tuple(ef.shape) == (2, 20) == tuple(el.shape)
    wf, wl, bf, bl = bo.onset_strength(x[:, 0].cpu().numpy(), [20, 7], 1, 180, with_bound=True)
    assert (np.abs(ef.cpu().numpy() - wf) <= bf).all() and (np.abs(el.cpu().numpy() - wl) <= bl).all() and (ef[1, 7:] == 0).all()
    for bad in (dict(lag=0), dict(f_split=481), dict(lag=1.5), dict(lag=26)):
        with pytest.raises(hip.A2SError):
            hip.onset_strength(x, n, **bad)
    with pytest.raises(hip.A2SError):
        hip.onset_strength(x, n.long())
    with pytest.raises(hip.A2SError):
        hip.onset_strength(x.cpu(), n)
    empty = hip.onset_strength(x[:0], n[:0])
    assert tuple(empty[0].shape) == (0, 20) and hip.beat_launches() == k0 + 1


# ------------------------------------------------------------------------------------------- 2. tempogram
def _tempogram_check(dev, env, n, win, hop_b, lag_min, lag_max, J):
    from piano_a2s_amd import hip
    R = env.shape[0]
    nl = lag_max - lag_min + 1
    buf = torch.full((R * J * nl + 16,), SENT, dtype=torch.float32, device=dev)
    out = buf[8:8 + R * J * nl].view(R, J, nl)
    got = hip.tempogram(torch.from_numpy(env).to(dev), torch.tensor(n, dtype=torch.int32, device=dev), win, hop_b, lag_min, lag_max, J=J, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr() and (buf[:8] == SENT).all() and (buf[8 + R * J * nl:] == SENT).all()
    want, bound = bo.tempogram(env, n, win, hop_b, lag_min, lag_max, J, with_bound=True)
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(bound).all() and np.isfinite(got).all()
    err = np.abs(got - want)
    assert (err <= bound).all(), f"{err.max():.3e} against {bound[err > bound].min():.3e}"
    return got, want, float(err.max()), float((err / np.maximum(bound, 1e-300)).max())


def test_tempogram_small_geometry(dev):
    rng = np.random.default_rng(5)
    env = rng.uniform(0, 1, size=(3, 40)).astype(np.float32)
    env[:, ::5] += 2.0
    n = [0, 5, 37]
    got, want, worst, ratio = _tempogram_check(dev, env, n, 16, 4, 2, 7, 10)
    print(f"tempogram win 16: max |A - A64| = {worst:.3e}, at most {ratio:.3f} of the bound")
    assert (got[0] == 0).all(), "no frames: zeros"
    assert (got[1, 4:] == 0).all() and np.abs(got[1, :2]).max() > 0, "blocks whose window lies behind the recording's end are zero"
    assert got[2, 4, 5 - 2] > 0.2 and got[2, 4].argmax() == 5 - 2, "the period of 5 frames shows"
    flat = np.full((1, 40), 0.25, dtype=np.float32)                                  # a constant envelope: d = 0, the denominator vanishes
    from piano_a2s_amd import hip
    z = hip.tempogram(torch.from_numpy(flat).to(dev), torch.tensor([40], dtype=torch.int32, device=dev), 16, 4, 2, 7)
    assert tuple(z.shape) == (1, 10, 6) and (z == 0).all()


def test_tempogram_default_geometry(dev):
    rng = np.random.default_rng(6)
    env = rng.uniform(0, 0.3, size=(1, 1201)).astype(np.float32)
    env[0, 13::47] += 3.0
    got, want, worst, ratio = _tempogram_check(dev, env, [1201], 800, 100, 20, 200, 13)
    print(f"tempogram win 800, lags 20 .. 200, n = 1201: max |A - A64| = {worst:.3e}, at most {ratio:.3f} of the bound")
    assert got.shape == (1, 13, 181) and int(got[0, 6].argmax()) + 20 in (47, 94, 141, 188) and got[0, 6, 47 - 20] > 0.5


# ------------------------------------------------------------------------------------------- 3. the beat dynamic programme
def _dp_check(dev, ls, period, pen, n, hop_b, lag_min, max_beats):
    """Runs a2s_beat_dp into buffers with sentinels on both sides and compares all four outputs with the float32 oracle, written and unwritten parts."""
    from piano_a2s_amd import hip
    R, stride = ls.shape
    fills = (SENT, -7, -9, -11)

    def framed(shape, dtype, fill):
        k = int(np.prod(shape))
        buf = torch.full((k + 16,), fill, dtype=dtype, device=dev)
        return buf, buf[8:8 + k].view(*shape)

    (Sb, S), (Bb, back), (Tb, beats), (Cb, count) = (framed((R, stride), torch.float32, fills[0]), framed((R, stride), torch.int32, fills[1]),
                                                    framed((R, max_beats), torch.int32, fills[2]), framed((R,), torch.int32, fills[3]))
    hip.beat_dp(torch.from_numpy(ls).to(dev), torch.from_numpy(np.ascontiguousarray(period, dtype=np.int32)).to(dev), torch.from_numpy(pen).to(dev),
                torch.tensor(n, dtype=torch.int32, device=dev), hop_b, lag_min, max_beats, S=S, back=back, beats=beats, count=count)
    torch.cuda.synchronize()
    for buf, fill in zip((Sb, Bb, Tb, Cb), fills):
        assert (buf[:8] == fill).all() and (buf[-8:] == fill).all(), "the sentinels around the outputs"
    wS, wback, wbeats, wcount = bo.beat_dp(ls, period, pen, n, hop_b, lag_min, max_beats, sentinel=fills[:3])
    gS, gback, gbeats, gcount = S.cpu().numpy(), back.cpu().numpy(), beats.cpu().numpy(), count.cpu().numpy()
    assert np.array_equal(gS.view(np.int32), wS.view(np.int32)), f"S differs at {np.argwhere(gS.view(np.int32) != wS.view(np.int32))[:5].tolist()}"
    assert np.array_equal(gback, wback), f"back differs at {np.argwhere(gback != wback)[:5].tolist()}"
    assert np.array_equal(gcount, wcount) and np.array_equal(gbeats, wbeats)
    return gS, gback, gbeats, gcount


def _envelope(rng, R, stride, period=47):
    """An envelope over its standard deviation: noise and impulses every `period` frames, displaced by up to two frames."""
    env = rng.uniform(0, 0.5, size=(R, stride))
    for r in range(R):
        at = np.arange(7 + 3 * r, stride, period) + rng.integers(-2, 3, size=len(np.arange(7 + 3 * r, stride, period)))
        env[r, np.clip(at, 0, stride - 1)] += 3.0
    return (env / env.std()).astype(np.float32)


@pytest.fixture(scope="module")
def pen():
    from piano_a2s_amd import beats
    return beats.penalty_table()


def test_dp_constant_period_and_every_length(dev, pen):
    rng = np.random.default_rng(8)
    ls = _envelope(rng, 4, 500)
    n = [0, 1, 9, 500]
    for tau in (20, 47, 200):
        S, back, beats, count = _dp_check(dev, ls, np.full((4, 5), tau), pen, n, 100, 20, 60)
        assert count[0] == 0 and count[1] == 1 and beats[1, 0] == 0 and count[2] == 1 and count[3] >= 2
    S, back, beats, count = _dp_check(dev, ls, np.full((4, 5), 47), pen, n, 100, 20, 60)
    assert abs(float(np.diff(beats[3, :count[3]]).mean()) - 47) < 3, "the impulses are followed"


def test_dp_period_changes_per_block(dev, pen):
    """200 -> 20 and 20 -> 200 at block boundaries that fall inside a chunk: the chunk must follow the smallest half period of its frames."""
    rng = np.random.default_rng(9)
    ls = _envelope(rng, 3, 500, period=31)
    period = np.array([[200, 20, 200, 20, 50], [20, 200, 20, 200, 200], [50, 60, 70, 199, 21]])
    for hop_b in (100, 90, 7):                                                        # (7: the last period holds from frame 28 on)
        _dp_check(dev, ls, period, pen, [500, 123, 9], hop_b, 20, 80)
    _dp_check(dev, ls, np.array([[5, 300, 20, 20, 20]] * 3), pen, [500, 500, 500], 100, 20, 80)          # out of range: clamped to lag_min, lag_max


def test_dp_all_zero_envelope(dev, pen):
    ls = np.zeros((1, 500), dtype=np.float32)
    S, back, beats, count = _dp_check(dev, ls, np.full((1, 5), 50), pen, [500], 100, 20, 40)
    assert (back == -1).all() and (S == 0).all() and count[0] == 1 and beats[0, 0] == 450, "one beat: the first arg max of the last period"


def test_dp_ties_go_to_the_nearest(dev):
    from piano_a2s_amd import beats
    # two equal scores at the distances 25 and 100 of frame 200 at the period 50: ln(1/2)^2 = ln(2)^2, the nearer one wins
    ls = np.zeros((1, 500), dtype=np.float32)
    ls[0, [100, 175]] = 1.0
    soft = beats.penalty_table(20, 200, 0.01)
    assert soft[30, 25] == soft[30, 100]
    _dp_check(dev, ls, np.full((1, 5), 50), soft, [500], 100, 20, 40)
    # no price at all and one impulse at frame 10, period 20: the frames 20 .. 50 all score 1; frame 60 sees them in [20, 50] and takes the nearest
    free = np.zeros_like(soft)
    ls = np.zeros((1, 500), dtype=np.float32)
    ls[0, 10] = 1.0
    S, back, _, _ = _dp_check(dev, ls, np.full((1, 5), 20), free, [500], 100, 20, 60)
    assert (S[0, 20:51] == 1.0).all() and (back[0, 20:30] == 10).all() and back[0, 30] == 20 and back[0, 60] == 50 and back[0, 51] == 41 and S[0, 60] == 1.0
    # ... and equal impulses: plateaus of equal scores everywhere
    ls = np.zeros((2, 500), dtype=np.float32)
    ls[0, ::10] = 1.0
    ls[1, 3::25] = 0.5
    for tau in (20, 50, 200):
        _dp_check(dev, ls, np.full((2, 5), tau), free, [500, 499], 100, 20, 60)


def test_dp_more_beats_than_room(dev, pen):
    rng = np.random.default_rng(10)
    ls = _envelope(rng, 3, 500)
    S, back, beats, count = _dp_check(dev, ls, np.full((3, 5), 47), pen, [500, 300, 20], 100, 20, 3)
    assert count[0] > 3 and count[1] > 3 and count[2] == 1 and (np.diff(beats[0]) > 0).all(), "the true count, and the first beats that fit"
    from piano_a2s_amd import hip
    S2, back2, beats2, count2 = hip.beat_dp(torch.from_numpy(ls).to(dev), torch.full((3, 5), 47, dtype=torch.int32, device=dev), torch.from_numpy(pen).to(dev),
                                            torch.tensor([500, 300, 20], dtype=torch.int32, device=dev))
    assert tuple(beats2.shape) == (3, 500 // 10 + 1) and np.array_equal(count2.cpu().numpy(), count)
    assert np.array_equal(beats2[0, :3].cpu().numpy(), beats[0]) and (beats2[0, count[0]:] == -1).all()


# ------------------------------------------------------------------------------------------- 4. refusals and counters
def test_refusals_and_counters(dev, pen):
    from piano_a2s_amd import hip
    L = hip.lib()
    st = hip.stream()
    B, rows, F = 2, 10, 8
    x = torch.rand((B, rows, F), device=dev)
    n_rows = torch.tensor([10, 4], dtype=torch.int32, device=dev)
    ef, el = torch.zeros((B, rows), device=dev), torch.zeros((B, rows), device=dev)
    env = torch.rand((2, 40), device=dev)
    n = torch.tensor([40, 11], dtype=torch.int32, device=dev)
    tg = torch.zeros((2, 10, 6), device=dev)
    period = torch.full((2, 4), 30, dtype=torch.int32, device=dev)
    pen_d = torch.from_numpy(pen).to(dev)
    S, back = torch.zeros((2, 40), device=dev), torch.zeros((2, 40), dtype=torch.int32, device=dev)
    beats, count = torch.zeros((2, 5), dtype=torch.int32, device=dev), torch.zeros((2,), dtype=torch.int32, device=dev)
    p = hip._p
    calls = {
        # a2s_onset_strength(stream, x, x_bstride, x_rstride, n_rows, B, rows, F, lag, f_split, env_full, env_low, env_bstride)
        "a2s_onset_strength": ((p(x), rows * F, F, p(n_rows), B, rows, F, 1, 3, p(ef), p(el), rows), 4,
                               [(0, None), (3, None), (9, None), (10, None), (4, -1), (4, 65536), (7, 0), (7, -3), (7, 2000), (8, -1), (8, F + 1), (2, F - 1),
                                (1, rows * F - 1), (11, rows - 1), (5, 0), (6, 0)]),
        # a2s_tempogram(stream, env, stride, n, R, J, win, hop_b, lag_min, lag_max, out)
        "a2s_tempogram": ((p(env), 40, p(n), 2, 10, 16, 4, 2, 7, p(tg)), 3,
                          [(0, None), (2, None), (9, None), (3, -1), (3, 65536), (5, 0), (5, -16), (5, 8193), (6, 0), (7, 8), (7, -1), (8, 5000), (4, 0), (1, 0)]),
        # a2s_beat_dp(stream, ls, stride, period, J, hop_b, pen, lag_min, lag_max, n, R, S, back, beats, max_beats, count)
        "a2s_beat_dp": ((p(env), 40, p(period), 4, 10, p(pen_d), 20, 200, p(n), 2, p(S), p(back), p(beats), 5, p(count)), 9,
                        [(0, None), (2, None), (5, None), (8, None), (10, None), (11, None), (12, None), (14, None), (9, -1), (9, 65536), (6, 0), (6, 201),
                         (7, 4097), (13, 0), (4, 0), (3, 0), (1, 0)]),
    }
    torch.cuda.synchronize()
    for name, (ok, count_at, bad) in calls.items():
        fn = getattr(L, name)
        k0, l0 = hip.beat_launches(), L.a2s_launch_count()
        for i, v in bad:
            args = list(ok)
            args[i] = v
            assert fn(st, *args) == -1, (name, i, v)                                  # A2S_ERR_ARG
            assert name[4:].encode() in L.a2s_last_error()
        args = list(ok)
        args[count_at] = 0
        assert fn(st, *args) == 0, name                                               # B = 0, R = 0: fine, and nothing to launch
        assert hip.beat_launches() == k0 and L.a2s_launch_count() == l0, f"{name}: nothing was launched"
        assert fn(st, *ok) == 0
        torch.cuda.synchronize()
        assert hip.beat_launches() == k0 + 1 and L.a2s_launch_count() == l0 + 1, f"{name}: one launch per call"
    k0 = hip.beat_launches()
    for call in (lambda: hip.tempogram(env, n, win=0), lambda: hip.tempogram(env, n, lag_min=9, lag_max=8), lambda: hip.tempogram(env, n.long()),
                 lambda: hip.tempogram(env.cpu(), n), lambda: hip.beat_dp(env, period, pen_d, n, lag_min=21), lambda: hip.beat_dp(env, period.long(), pen_d, n),
                 lambda: hip.beat_dp(env, period, pen_d, n, max_beats=0), lambda: hip.beat_dp(env, period, pen_d, n, hop_b=0)):
        with pytest.raises(hip.A2SError):
            call()
    assert hip.beat_launches() == k0


# ------------------------------------------------------------------------------------------- 5. a recording, end to end
HP = dict(sample_rate=16000, hop_length=160, max_frame_num=1201, max_bars=5, bins_per_octave=60, n_octaves=8, gamma=20)
SMALL = dict(conv_feature_size=32, hidden_size=32, max_length=(12, 8))
TOLERANCE_S = 0.070          # the tolerance window of the field's standard beat F-measure
FIRST_S, BEAT_S, SECONDS = 0.25, 0.5, 20.0


def _bursts():
    """20 s at 16 kHz: a short decaying tone burst every 0.5 s (120 beats per minute), every fourth with an added bass tone.
    -> (wave (320000,) float32, burst times, bass burst times)."""
    sr = 16000
    rng = np.random.default_rng(12)
    x = np.zeros(int(SECONDS * sr))
    tt = np.arange(int(0.4 * sr)) / sr
    shape = np.minimum(tt / 0.004, 1.0) * np.exp(-tt / 0.08)
    times = np.arange(FIRST_S, SECONDS - 0.45, BEAT_S)
    for k, t in enumerate(times):
        f = 440.0 * 2.0 ** (rng.integers(0, 13) / 12.0)
        note = 0.3 * shape * (np.sin(2 * np.pi * f * tt) + 0.5 * np.sin(4 * np.pi * f * tt))
        if k % 4 == 2:
            note = note + 0.5 * shape * (np.sin(2 * np.pi * 55.0 * tt) + 0.7 * np.sin(2 * np.pi * 110.0 * tt))
        i0 = int(round(t * sr))
        x[i0:i0 + len(tt)] += note
    return x.astype(np.float32), times, times[2::4]


@pytest.fixture(scope="module")
def recording(dev):
    """The burst recording tracked once on the device and once with the oracle's stages on the same device features."""
    from piano_a2s_amd import beats
    wave, times, bass = _bursts()
    w = torch.from_numpy(wave).to(dev)
    return dict(wave=wave, times=times, bass=bass, device=beats.track_recording(w, HP), oracle=beats.track_recording(w, HP, stages=bo.stages()))


def _inner(a):
    return np.array([t for t in a if 2.0 <= t <= SECONDS - 2.0])


def test_recording_beats_and_downbeats(recording):
    got, want = recording["device"], recording["oracle"]
    assert set(got) == {"beats_s", "downbeats_s", "beats_per_bar", "period_frames"}
    assert got["beats_s"] == want["beats_s"] and got["downbeats_s"] == want["downbeats_s"] and got["period_frames"] == want["period_frames"]
    beats_s, times = np.asarray(got["beats_s"]), _inner(recording["times"])
    offsets = np.array([beats_s[np.abs(beats_s - t).argmin()] - t for t in times])
    print(f"beat - burst over {len(times)} interior bursts: mean {1e3 * offsets.mean():+.1f} ms, worst {1e3 * np.abs(offsets).max():.1f} ms; periods {got['period_frames']}")
    assert len(times) >= 30 and (np.abs(offsets) <= TOLERANCE_S).all()
    assert len(got["period_frames"]) == 21 and all(48 <= p <= 52 for p in got["period_frames"])
    assert got["beats_per_bar"] == 4
    down, bass = _inner(got["downbeats_s"]), _inner(recording["bass"])
    assert len(down) == len(bass) >= 7 and (np.abs(down - bass) <= TOLERANCE_S).all(), (down, bass)


def test_transcribe_with_tracked_downbeats(dev, recording):
    import models
    from piano_a2s_amd import audio, spec, transcribe
    model = models.ScoreTranscription(**SMALL)
    model.load_state_dict(spec.procedural_state(spec.default_cfg(**SMALL), 11, eos_bias=3.0, lively=True))
    model = model.to(dev).eval()
    x = recording["wave"][:, None]
    res = transcribe.transcribe_waveform(model, x, 16000, downbeats="track", hparams=HP)
    assert set(res) == {"sample_rate_in", "sample_rate", "frames_per_second", "windows", "tracking"}
    assert res["tracking"] == recording["device"], "the tracker's result as it stands"
    down = res["tracking"]["downbeats_s"]
    plan = audio.plan_windows(len(x), 16000, down, max_bars=5, max_samples=192000)
    assert len(res["windows"]) == len(plan) >= 2
    for win, (start, stop, n_bars) in zip(res["windows"], plan):
        assert win["start_s"] == start / 16000 and win["stop_s"] == stop / 16000 and win["n_bars"] == n_bars <= 5 and len(win["bars"]) == n_bars
        assert min(abs(win["start_s"] - d) for d in down) < 1e-4, "a window starts at a tracked downbeat"
    forced = transcribe.transcribe_waveform(model, x, 16000, downbeats="track", beats_per_bar=2, hparams=HP)
    assert forced["tracking"]["beats_per_bar"] == 2 and forced["tracking"]["beats_s"] == res["tracking"]["beats_s"]
    plain = transcribe.transcribe_waveform(model, x, 16000, hparams=HP)
    assert set(plain) == {"sample_rate_in", "sample_rate", "frames_per_second", "windows"} and len(plain["windows"]) == 2
    with pytest.raises(ValueError):
        transcribe.transcribe_waveform(model, x, 16000, downbeats=[1.0, 3.0], beats_per_bar=4, hparams=HP)
