"""The tuning kernels (csrc/a2s_tuning.hip) on the GPU, through the raw C ABI with sentinels around every output.

1. a2s_tuning_profile EQUALS tests/tuning_oracle.py integer for integer: strided clips and rows with NaN in the padding, 16-byte and 4-byte loads,
   every n_rows, every kind of cell; a clip alone gives the row it gives in the batch; two runs are identical; sums beyond 2^32 in one cell.
2. a2s_tuning_estimate is bit-equal to piano_a2s_amd.tuning.estimate_host (and the definition): crafted histograms and profile's own output.
3. Refusals return -1, name the entry point and launch nothing; the wrappers refuse a `first` that does not ascend from 0 to B.
4. The chain on the GPU render and the GPU VQT: the estimate against the detuning of the render, the correlation before and after the Tuner.
5. transcribe_waveform(tuning=...) on the small model, and a recipe stage with --tuning_correction=true."""
import os

import numpy as np
import pytest
import torch

from piano_a2s_amd import scoregen, spec, tuning
from tests import tuning_oracle as oracle
from tests.test_tuning_cpu import ERROR_BOUND

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(conv_feature_size=32, hidden_size=32, max_length=(12, 8))
HP = dict(sample_rate=16000, hop_length=160, max_frame_num=1201, max_bars=5, bins_per_octave=60, n_octaves=8, gamma=20)
H = oracle.H
GUARD = 16
SENT_I = -7777777
SENT_F = -12345.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _laid_out(host, layout, dev):
    """host (B, T, F) float32 -> a device view of its shape: "contiguous"; "padded4": rows F + 4 and clips a further 8 floats apart, 16-byte aligned
    where F % 4 == 0; "padded1": rows F + 1 apart, clips 3 more, starting one float into the buffer (never 16-byte loads).  NaN in all padding."""
    B, T, F = host.shape
    lead, rs, extra = {"contiguous": (8, F, 0), "padded4": (8, F + 4, 8), "padded1": (1, F + 1, 3)}[layout]
    bs = T * rs + extra
    flat = torch.full((lead + B * bs + 8,), float("nan"), dtype=torch.float32, device=dev)
    view = flat[lead:].as_strided((B, T, F), (bs, rs, 1))
    view.copy_(torch.from_numpy(host))
    return view


def _profile(dev, xd, n_rows, thr=0.5, S=5, launches=1):
    """a2s_tuning_profile through the raw ABI on an output with sentinels around it -> (B, H + 1) int64 numpy."""
    from piano_a2s_amd import hip
    Lib = hip.lib()
    B, T, F = xd.shape
    out = torch.full((GUARD + B * (H + 1) + GUARD,), SENT_I, dtype=torch.int64, device=dev)
    nd = torch.tensor(list(n_rows), dtype=torch.int32, device=dev)
    n0 = hip.tuning_launches()
    rc = Lib.a2s_tuning_profile(hip.stream(), hip._p(xd), xd.stride(0) if B > 1 else max(xd.stride(0), (T - 1) * xd.stride(1) + F), xd.stride(1),
                                hip._p(nd), B, T, F, S, thr, hip._p(out[GUARD:]))
    assert rc == 0, Lib.a2s_last_error()
    assert hip.tuning_launches() == n0 + launches
    h = out.cpu().numpy()
    assert (h[:GUARD] == SENT_I).all() and (h[GUARD + B * (H + 1):] == SENT_I).all(), "nothing outside hist is written"
    return h[GUARD:GUARD + B * (H + 1)].reshape(B, H + 1)


# ------------------------------------------------------------------------------------------- 1. the profile
@pytest.mark.parametrize("layout", ["contiguous", "padded4", "padded1"])
@pytest.mark.parametrize("F", [24, 23, 3, 2])
def test_profile_equals_the_oracle(dev, F, layout):
    rng = np.random.default_rng(100 + F)
    T = 37
    for name, x in oracle.feature_cases(rng, B=3, T=T, F=F).items():
        xd = _laid_out(x, layout, dev)
        for n_rows in ([T, 5, 0], [-3, T + 9, T]):
            for thr in (0.0, 0.5, 1.0):
                got = _profile(dev, xd, n_rows, thr, launches=1 if F >= 3 else 0)
                assert np.array_equal(got, oracle.profile(x, n_rows, thr)), (name, n_rows, thr)
        got = _profile(dev, xd, [T, T, T], 0.5, launches=1 if F >= 3 else 0)
        assert np.array_equal(got, _profile(dev, xd, [T, T, T], 0.5, launches=1 if F >= 3 else 0)), "two runs are identical"
        alone = _profile(dev, xd[1:2], [T], 0.5, launches=1 if F >= 3 else 0)
        assert np.array_equal(alone[0], got[1]), "a clip alone gives the row it gives inside the batch"
        if name == "uniform" and F > 3:
            assert got[:, H].min() > 0
        other = _profile(dev, xd, [T, T, T], 0.5, S=2, launches=1 if F >= 3 else 0)
        assert np.array_equal(other, oracle.profile(x, [T, T, T], 0.5, 2)), (name, "two bins per semitone")


def test_profile_of_one_wide_clip(dev):
    rng = np.random.default_rng(480)
    for name, x in oracle.feature_cases(rng, B=1, T=5, F=480).items():
        for layout in ("contiguous", "padded4", "padded1"):
            got = _profile(dev, _laid_out(x, layout, dev), [5], 0.5)
            assert np.array_equal(got, oracle.profile(x, [5], 0.5)), (name, layout)
            if name == "uniform":
                assert got[0, H] > 200, "both column steps of a row and the cells between them carry peaks"


@pytest.mark.parametrize("T, F, value", [(21900, 480, 1.0), (64, 330000, 2.0)])
def test_profile_sums_beyond_32_bits(dev, T, F, value):
    """x = value where f mod 5 == 0, else 0: every peak falls into one cell.  21 900 x 480 at value 1 (weight 2049) is the largest sum a recording of
    some minutes gives, 4.26e9, just below 2^32, spread over many workgroups.  64 x 330 000 at value 2 (weight 4097) is one workgroup whose every
    wave adds 16 x 65 999 x 4097 = 4.33e9 > 2^32 to one cell: without the flush inside the loop the low 32 bits alone would arrive.  All rows are
    equal, so the oracle's row, times T, is the expectation."""
    row = np.zeros((1, 1, F), dtype=np.float32)
    row[0, 0, ::5] = value
    want = oracle.profile(row, [1], 0.5) * T
    cell = int(np.argmax(want[0, :H]))
    assert want[0, H] == T * ((F - 2) // 5) and want[0, cell] == want[0, H] * (1 + int(min(value - 0.5, 1.0) * oracle.Q)) and want[0, :H].sum() == want[0, cell]
    if F > 480:
        assert want[0, cell] // 4 > 2 ** 32, "a wave's share exceeds 32 bits"
    xd = torch.zeros((1, T, F), dtype=torch.float32, device=dev)
    xd[:, :, ::5] = value
    assert np.array_equal(_profile(dev, xd, [T], 0.5), want)


# ------------------------------------------------------------------------------------------- 2. the estimate
def _estimate(dev, hist, first, min_conf, min_peaks, S=5):
    """a2s_tuning_estimate through the raw ABI, sentinels around both outputs -> (est (G, 3) float64, eff (B,) float32) numpy."""
    from piano_a2s_amd import hip
    Lib = hip.lib()
    hist = np.ascontiguousarray(hist, dtype=np.int64).reshape(-1, H + 1)
    B, G = hist.shape[0], len(first) - 1
    hd, fd = torch.from_numpy(hist).to(dev), torch.tensor(list(first), dtype=torch.int32, device=dev)
    est = torch.full((GUARD + 3 * G + GUARD,), SENT_F, dtype=torch.float64, device=dev)
    eff = torch.full((GUARD + B + GUARD,), SENT_F, dtype=torch.float32, device=dev)
    n0 = hip.tuning_launches()
    rc = Lib.a2s_tuning_estimate(hip.stream(), hip._p(hd), hip._p(fd), G, B, S, float(min_conf), int(min_peaks), hip._p(est[GUARD:]), hip._p(eff[GUARD:]))
    assert rc == 0, Lib.a2s_last_error()
    assert hip.tuning_launches() == n0 + 1, "one launch"
    e, f = est.cpu().numpy(), eff.cpu().numpy()
    assert (e[:GUARD] == SENT_F).all() and (e[GUARD + 3 * G:] == SENT_F).all() and (f[:GUARD] == SENT_F).all() and (f[GUARD + B:] == SENT_F).all()
    return e[GUARD:GUARD + 3 * G].reshape(G, 3), f[GUARD:GUARD + B]


def _crafted():
    """308 histograms in G = 6 groups of 5, 0, 300, 1, 2 and 0 clips."""
    rng = np.random.default_rng(6)
    first = [0, 5, 5, 305, 306, 308, 308]
    hist = np.zeros((308, H + 1), dtype=np.int64)
    hist[0:5, 99], hist[0:5, 0], hist[0:5, 98], hist[0:5, H] = [700, 650, 600, 0, 500], [500, 640, 600, 0, 700], 90, 40        # the wrap (one clip of zeros)
    hist[5:305, :H] = rng.integers(0, 1000, (300, H))                                                                        # cells near 2^45
    hist[5:305, 41:44] += (1 << 45) + (rng.integers(0, 1 << 30, (300, 3)).astype(np.int64) << 14)
    hist[5:305, H] = rng.integers(0, 1 << 31, 300)
    hist[305, 20], hist[305, 70], hist[305, H] = 300, 300, 200                                                               # a tie: the first wins
    hist[306:308, :H] = rng.integers(0, 40, (2, H))                                                                          # the group at the gates
    hist[306:308, 61:64] += [[900, 2000, 700]]
    hist[306:308, H] = [60, 65]
    return hist, first


def test_estimate_is_bit_equal_to_the_restatement(dev):
    hist, first = _crafted()
    ref = oracle.estimate(hist, first, 0.0, 0)[0]
    assert ref[0, 0] >= 49.0 or ref[0, 0] < -49.0, "group 0 peaks at the wrap"
    assert ref[3, 0] == 20.5 - 50 and ref[2, 1] > 10 and ref[2, 2] > 2 ** 31 and ref[1].tolist() == [-49.5, 0.0, 0.0]
    conf, peaks = float(ref[4, 1]), int(ref[4, 2])
    assert peaks == 125
    for S in (5, 2):
        for min_conf, min_peaks in ((tuning.MIN_CONF, tuning.MIN_PEAKS), (conf, peaks), (np.nextafter(conf, np.inf), peaks), (conf, peaks + 1), (0.0, 0), (1e300, 0)):
            got_est, got_eff = _estimate(dev, hist, first, min_conf, min_peaks, S)
            want_est, want_eff = tuning.estimate_host(hist, first, min_conf, min_peaks, S)
            def_est, def_eff, det = oracle.estimate(hist, first, min_conf, min_peaks, S)
            assert _same(want_est, def_est) and _same(want_eff, def_eff), "the restatement is the definition"
            assert _same(got_est, want_est), (S, min_conf, min_peaks, got_est, want_est)
            assert _same(got_eff, want_eff), (S, min_conf, min_peaks)
            assert bool(det[4]) == (min_conf <= conf and min_peaks <= peaks) and bool(got_eff[306] != 0) == bool(det[4])
    # profile's own output, every clip a group and all clips one group
    rng = np.random.default_rng(124)
    x = oracle.feature_cases(rng, B=3, T=37, F=24)["uniform"]
    h = _profile(dev, _laid_out(x, "contiguous", dev), [37, 37, 20], 0.5)
    for f in ([0, 1, 2, 3], [0, 3], [0, 0, 2, 3]):
        got_est, got_eff = _estimate(dev, h, f, 1.0, 10)
        want_est, want_eff = tuning.estimate_host(h, f, 1.0, 10)
        assert _same(got_est, want_est) and _same(got_eff, want_eff) and (want_est[:, 2] > 0).any()


# ------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_launch_nothing(dev):
    from piano_a2s_amd import hip
    Lib, st = hip.lib(), hip.stream()
    B, T, F, G = 2, 9, 24, 2
    x = torch.rand(B, T, F, device=dev)
    n_rows = torch.full((B,), T, dtype=torch.int32, device=dev)
    hist = torch.full((B, H + 1), SENT_I, dtype=torch.int64, device=dev)
    first = torch.tensor([0, 1, 2], dtype=torch.int32, device=dev)
    est = torch.full((G, 3), SENT_F, dtype=torch.float64, device=dev)
    eff = torch.full((B,), SENT_F, dtype=torch.float32, device=dev)
    n0, k0 = hip.tuning_launches(), Lib.a2s_launch_count()
    ok = [hip._p(x), T * F, F, hip._p(n_rows), B, T, F, 5, 0.5, hip._p(hist)]
    for i, bad in ((0, None), (3, None), (9, None), (4, -1), (4, 65536), (5, 0), (6, 0), (6, -3), (7, 0), (7, 65), (8, -0.01), (8, 1.01), (8, float("nan")),
                   (8, float("inf")), (2, F - 1), (1, (T - 1) * F + F - 1)):
        args = list(ok)
        args[i] = bad
        assert Lib.a2s_tuning_profile(st, *args) == -1, (i, bad)
        assert b"tuning_profile" in Lib.a2s_last_error()
    ok2 = [hip._p(hist), hip._p(first), G, B, 5, 3.0, 100, hip._p(est), hip._p(eff)]
    for i, bad in ((0, None), (1, None), (7, None), (8, None), (2, -1), (2, 65536), (3, -1), (4, 0), (4, 65), (5, float("nan")), (5, float("inf")), (6, -1)):
        args = list(ok2)
        args[i] = bad
        assert Lib.a2s_tuning_estimate(st, *args) == -1, (i, bad)
        assert b"tuning_estimate" in Lib.a2s_last_error()
    args = list(ok)
    args[4] = 0
    assert Lib.a2s_tuning_profile(st, *args) == 0, "B = 0 is fine"
    args = list(ok2)
    args[2] = 0
    assert Lib.a2s_tuning_estimate(st, *args) == 0, "G = 0 is fine"
    # the wrappers
    good = torch.zeros((B, H + 1), dtype=torch.int64, device=dev)
    for bad in ([0, 2, 1, 2], [0, 1], [1, 2], [0, 1, 3], [0, 0.5, 2], [], [[0, 2]]):
        with pytest.raises(hip.A2SError, match="`first`|first"):
            hip.tuning_estimate(good, bad, 3.0, 100)
    with pytest.raises(hip.A2SError, match="`hist`"):
        hip.tuning_estimate(good.to(torch.int32), [0, 2], 3.0, 100)
    with pytest.raises(hip.A2SError, match="`min_conf`"):
        hip.tuning_estimate(good, [0, 2], float("nan"), 100)
    with pytest.raises(hip.A2SError, match="`min_peaks`"):
        hip.tuning_estimate(good, [0, 2], 3.0, -1)
    with pytest.raises(hip.A2SError, match="`x`"):
        hip.tuning_profile(x.transpose(1, 2), n_rows)
    with pytest.raises(hip.A2SError, match="`x`"):
        hip.tuning_profile(x.double(), n_rows)
    with pytest.raises(hip.A2SError, match="`n_rows`"):
        hip.tuning_profile(x, n_rows.long())
    with pytest.raises(hip.A2SError, match="`thr`"):
        hip.tuning_profile(x, n_rows, thr=1.5)
    with pytest.raises(hip.A2SError, match="`bins_per_semitone`"):
        hip.tuning_profile(x, n_rows, bins_per_semitone=0)
    with pytest.raises(hip.A2SError, match="`out`"):
        hip.tuning_profile(x, n_rows, out=torch.zeros((B, H), dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="multiple of 12"):
        tuning.Tuner(dev, bins_per_octave=50)
    assert tuple(hip.tuning_estimate(good[:0], [0], 3.0, 100)[0].shape) == (0, 3)
    torch.cuda.synchronize()
    assert hip.tuning_launches() == n0 and Lib.a2s_launch_count() == k0, "nothing was launched"
    assert (hist == SENT_I).all() and (est == SENT_F).all() and (eff == SENT_F).all()
    assert Lib.a2s_tuning_profile(st, *ok) == 0 and Lib.a2s_tuning_estimate(st, *ok2) == 0
    torch.cuda.synchronize()
    assert hip.tuning_launches() == n0 + 2 and (hist >= 0).all() and (est != SENT_F).all() and (eff != SENT_F).all()
    h2 = hip.tuning_profile(x, n_rows)
    assert torch.equal(h2, hist) and np.array_equal(h2.cpu().numpy(), oracle.profile(x.cpu().numpy(), [T, T], 0.5))


# ------------------------------------------------------------------------------------------- 4. the chain on the GPU render and the GPU VQT
SEEDS = (100, 101, 102, 103)
CENTS = (-40, -20, 0, 13, 30)
FRAMES = 301


@pytest.fixture(scope="module")
def float64_estimates():
    """The float64 chain on the same renders (resynth's instrument), computed once: {(seed, cents): estimated cents}."""
    return {(s, c): float(oracle.chain(s, c, FRAMES, "resynth")[0]) for s in SEEDS for c in CENTS}


def test_the_chain_on_rendered_clips(dev, float64_estimates):
    from piano_a2s_amd import hip, render, resynth, transcribe
    vqt = transcribe._vqt(dev, HP)
    progs, truth = [], []
    for s in SEEDS:
        p, n_samples = oracle.clip_program(s, FRAMES, "resynth")
        for c in CENTS:
            progs.append(scoregen.detune_program(p, c))
            truth.append((s, c))
    n0 = hip.tuning_launches()
    x = vqt(render.render(torch.from_numpy(np.stack(progs)).to(dev), n_samples))
    assert hip.tuning_launches() == n0, "with the tuner unused nothing of it is launched"
    B = len(truth)
    tuner = tuning.Tuner(dev, bins_per_octave=60)
    y, est, eff = tuner(x)
    assert hip.tuning_launches() == n0 + 2, "profile and estimate, one launch each"
    assert y.shape == x.shape and tuple(est.shape) == (B, 3) and tuple(eff.shape) == (B,) and est.is_cuda and eff.is_cuda
    est_h, eff_h = est.cpu().numpy(), eff.cpu().numpy()
    worst = gap = 0.0
    for (s, c), row in zip(truth, est_h):
        err = oracle.cents_error(row[0], c)
        worst, gap = max(worst, abs(err)), max(gap, abs(oracle.cents_error(row[0], float64_estimates[(s, c)])))
        print(f"seed {s} c {c:4d}: estimate {row[0]:8.3f} (float64 chain {float64_estimates[(s, c)]:8.3f}) confidence {row[1]:6.3f} peaks {int(row[2])}")
        assert abs(err) <= ERROR_BOUND, (s, c, row)
        assert row[1] >= tuning.MIN_CONF and row[2] >= tuning.MIN_PEAKS, (s, c, row)
    print(f"GPU chain over {B} clips: worst error {worst:.4f} cent (bound {ERROR_BOUND:.3f}); largest difference to the float64 chain's estimate {gap:.2e} cent")
    # Measured on the MI355X: worst error 0.280 cent; 1.9e-6 cent at the most between this estimate and the float64 chain's
    # (the fp32 render and front end move a peak's three cells that little); the difference is recorded, not asserted.
    assert _same(eff_h, (-est_h[:, 0] * 5.0 / 100.0).astype(np.float32)), "eff_bins is what a2s_shift_bins reads"
    assert torch.equal(y, hip.shift_bins(x, eff))
    # the correlation with the in-tune clip's features over the whole clip, before and after
    ref = torch.cat([x[i - i % len(CENTS) + CENTS.index(0)][None] for i in range(B)])
    seg = [(i, 0, x.shape[-2]) for i in range(B)]
    cells = x.shape[-2] * x.shape[-1]
    before = [resynth.agreement(r, cells) for r in hip.segment_agreement(x, ref, seg).cpu().numpy()]
    after = [resynth.agreement(r, cells) for r in hip.segment_agreement(y, ref, seg).cpu().numpy()]
    for (s, c), b, a in zip(truth, before, after):
        print(f"seed {s} c {c:4d}: correlation with the in-tune features {b:.4f} -> {a:.4f}")
        if abs(c) >= 13:
            assert a > b, (s, c, b, a)
    # a given tuning launches neither kernel
    n1 = hip.tuning_launches()
    y2, est2, eff2 = tuner(x, cents=12.5)
    assert hip.tuning_launches() == n1 and (eff2 == np.float32(-12.5 * 5 / 100.0)).all() and (est2[:, 0] == 12.5).all() and (est2[:, 1:] == 0).all()
    assert torch.equal(y2, hip.shift_bins(x, eff2))
    # one group of all clips of one detuning: the recording's tuning
    idx = [i for i, (s, c) in enumerate(truth) if c == 30]
    _, est3, eff3 = tuner(x[idx].contiguous(), first=[0, len(idx)])
    assert tuple(est3.shape) == (1, 3) and abs(float(est3[0, 0]) - 30.0) <= ERROR_BOUND and (eff3 == eff3[0]).all() and float(est3[0, 2]) == est_h[idx, 2].sum()


# ------------------------------------------------------------------------------------------- 5. transcribe_waveform and the recipes
@pytest.fixture(scope="module")
def state():
    return spec.procedural_state(spec.default_cfg(**SMALL), 11, eos_bias=3.0, lively=True)


def test_transcribe_waveform_with_tuning(dev, state):
    import models
    from piano_a2s_amd import hip, transcribe
    from piano_a2s_amd.render import render
    prog = scoregen.detune_program(scoregen.pack_program(scoregen.make_clip(spec.default_cfg(), 2024, frames=1201)), 25)
    w = render(torch.from_numpy(prog[None]).to(dev)).cpu().numpy()[0]
    x, downbeats = (w * (0.8 / np.abs(w).max())).astype(np.float32), [0.5, 2.75, 5.0, 7.25, 9.5, 11.75]
    model = models.ScoreTranscription(**SMALL)
    model.load_state_dict(state)
    model = model.to(dev).eval()
    model.constrained_decoding = True
    n0 = hip.tuning_launches()
    off = transcribe.transcribe_waveform(model, x, 16000, downbeats=downbeats, hparams=HP)
    assert "tuning" not in off and hip.tuning_launches() == n0, "without the option there is no key and no launch"
    on = transcribe.transcribe_waveform(model, x, 16000, downbeats=downbeats, hparams=HP, tuning="auto")
    assert hip.tuning_launches() == n0 + 2
    t = on["tuning"]
    print("transcribe_waveform(tuning='auto') on a clip rendered 25 cents sharp:", t)
    assert set(t) == {"cents", "confidence", "peaks", "determined", "a4_hz"} and set(on) == set(off) | {"tuning"}
    assert abs(t["cents"] - 25.0) <= ERROR_BOUND and t["determined"] is True and t["confidence"] >= tuning.MIN_CONF and t["peaks"] >= tuning.MIN_PEAKS
    assert t["a4_hz"] == 440.0 * 2.0 ** (t["cents"] / 1200.0) and len(on["windows"]) == len(off["windows"])
    given = transcribe.transcribe_waveform(model, x, 16000, downbeats=downbeats, hparams=HP, tuning=12.5)
    assert hip.tuning_launches() == n0 + 2, "a given tuning launches no profile"
    assert given["tuning"] == {"cents": 12.5, "confidence": None, "peaks": None, "determined": True, "a4_hz": 440.0 * 2.0 ** (12.5 / 1200.0)}
    for bad in ("x", "", "Auto", float("nan"), True):
        with pytest.raises(ValueError, match="tuning"):
            transcribe.transcribe_waveform(model, x, 16000, downbeats=downbeats, hparams=HP, tuning=bad)
    assert hip.tuning_launches() == n0 + 2


def test_recipe_with_tuning_correction(dev, tmp_path):
    """One epoch of the small synthetic model with --tuning_correction=true: TRAIN, VALID and TEST correct their features on the device and report the
    two stats; the same run without the switch launches nothing of it and reports neither."""
    import pretrain
    from piano_a2s_amd import hip
    args = [os.path.join(ROOT, "hparams", "pretrain.yaml"), "--device=cuda:0", "--soundfont_folder=/none",
            "--synthetic_clips=8", "--hidden_size=32", "--conv_feature_size=32", "--bins_per_octave=24", "--n_octaves=1", "--max_length=(12, 8)",
            "--synthetic_frames=41", "--synthetic_lengths=[[3, 10], [2, 7]]", "--batch_size=4", "--number_of_epochs=1", "--seed=1234"]
    n0 = hip.tuning_launches()
    brain = pretrain.main(args + [f"--workspace={tmp_path / 'on'}", "--tuning_correction=true"])
    launched = hip.tuning_launches() - n0
    assert launched >= 2 * (2 + 1 + 1) and launched % 2 == 0, "two TRAIN batches, VALID and TEST: profile and estimate for every batch"
    for stats in (brain.train_stats, brain.last_stats):
        assert 0.0 <= stats["tuning_determined"] <= 1.0 and 0.0 <= stats["tuning_abs_cents"] <= 50.0, stats
    n1 = hip.tuning_launches()
    brain = pretrain.main(args + [f"--workspace={tmp_path / 'off'}"])
    assert hip.tuning_launches() == n1 and "tuning_determined" not in brain.train_stats and "tuning_abs_cents" not in brain.last_stats
