"""The tuning estimate without a GPU: the float64 definition of tests/tuning_oracle.py against a brute-force loop, the numpy
restatement piano_a2s_amd.tuning.estimate_host against the definition, scoregen.detune_program, and the float64 chain on rendered clips."""
import numpy as np
import pytest

from piano_a2s_amd import scoregen, tuning
from tests import tuning_oracle as oracle

H = oracle.H
# tools/tuning_check.py (144 cases: seeds 100 .. 105 at 301 frames and 100, 101 at 1201 frames, nine detunings, both instruments) measured a worst
# error of 0.30602 cent, a smallest confidence of 5.0716 on the rendered clips and a largest of 1.5492 on its noise tensors.  Ten cents is half a
# feature bin, the size at which a correction stops paying: the bound is the measured worst plus half its distance to ten cents.
CHECK_WORST = 0.30602
ERROR_BOUND = CHECK_WORST + 0.5 * (10.0 - CHECK_WORST)


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


@pytest.mark.parametrize("F", [24, 23, 3, 2])
@pytest.mark.parametrize("thr", [0.0, 0.5, 1.0])
def test_profile_against_the_brute_force_loop(F, thr):
    rng = np.random.default_rng(27 + F)
    for S in (5, 2):
        for name, x in oracle.feature_cases(rng, F=F).items():
            n_rows = [x.shape[1], 3, -2]
            got, want = oracle.profile(x, n_rows, thr, S), oracle.profile_loops(x, n_rows, thr, S)
            assert np.array_equal(got, want), (name, S)
            assert (got[2] == 0).all() and got.dtype == np.int64
            if name == "constant rows" or F < 3:
                assert not got.any(), "a plateau gives no peak"
            if name == "uniform" and F > 3 and thr == 0.0:
                assert got[0, H] > 0 and got[0, :H].sum() >= got[0, H]


def test_profile_places_a_parabola_where_it_peaks():
    """Samples of one parabola whose vertex sits d bins beside column f land in the cell of (f mod S + d) * 100 / S cents; weight 1 + rint(.. * Q)."""
    for f, d, S in ((10, 0.0, 5), (11, 0.3, 5), (14, -0.45, 5), (12, 0.49, 5), (7, -0.2, 2)):
        x = np.zeros((1, 1, 24), dtype=np.float64)
        for k in (-1, 0, 1):
            x[0, 0, f + k] = 0.9 - 0.05 * (k - d) ** 2
        hist = oracle.profile(x.astype(np.float32), [1], 0.5, S)[0]
        u = (f % S + d + S / 2.0) % S
        assert hist[H] == 1 and hist[int(np.floor(u * H / S))] == 1 + int(np.rint((float(np.float32(0.9 - 0.05 * d * d)) - 0.5) * oracle.Q))


def _one(hist, **kw):
    est, eff, det = oracle.estimate(np.asarray(hist, dtype=np.int64)[None], [0, 1], kw.pop("min_conf", 0.0), kw.pop("min_peaks", 0), **kw)
    return est[0], eff[0], det[0]


def test_estimate_one_cell_at_every_position():
    for k in range(H):
        hist = np.zeros(H + 1, dtype=np.int64)
        hist[k], hist[H] = 1000, 500
        est, eff, det = _one(hist)
        assert est[0] == k + 0.5 - 50 and est[1] == 7 * H / 49 and est[2] == 500 and det
        assert eff == np.float32(-(k + 0.5 - 50) * 5 / 100.0)


def test_estimate_wrap_ties_zeros():
    hist = np.zeros(H + 1, dtype=np.int64)
    hist[99], hist[0], hist[H] = 600, 600, 400
    est, _, _ = _one(hist)                                            # sm[99] == sm[0]: the first arg max is 0, its neighbours pull it to the wrap
    assert est[0] == -50.0, est
    hist[99], hist[0] = 700, 500                                      # the peak sits in cell 99, pulled towards 0 across the wrap: still below 50
    est, _, _ = _one(hist)
    assert 49.5 < est[0] < 50.0
    hist[99], hist[0] = 500, 700
    est, _, _ = _one(hist)
    assert -50.0 <= est[0] < -49.5
    hist[:] = 0
    hist[20], hist[70], hist[H] = 300, 300, 200                       # two equal peaks: the first wins
    assert _one(hist)[0][0] == 20.5 - 50
    est, eff, det = _one(np.zeros(H + 1, dtype=np.int64), min_peaks=1)
    assert est.tolist() == [-49.5, 0.0, 0.0] and eff == 0 and not det
    assert not _one(np.zeros(H + 1, dtype=np.int64), min_conf=1e-9)[2], "either gate keeps a group of zeros undetermined"
    flat = np.full(H + 1, 3, dtype=np.int64)                          # a flat histogram: confidence 1, den == 0, no refinement
    est, _, _ = _one(flat)
    assert est[0] == -49.5 and est[1] == 1.0


def test_estimate_gates_and_groups():
    rng = np.random.default_rng(5)
    hist = rng.integers(0, 50, (9, H + 1)).astype(np.int64)
    hist[:, 37] += 4000
    hist[4] = 0
    hist[:, H] = [150, 99, 100, 101, 0, 1000, 1000, 1000, 1000]
    first = [0, 0, 1, 2, 3, 4, 5, 9, 9]                                # empty groups at both ends, one-clip groups, a group of four
    est, eff, det = oracle.estimate(hist, first, 3.0, 100)
    assert det.tolist() == [False, True, False, True, True, False, True, False]
    assert est[0].tolist() == [-49.5, 0.0, 0.0] and est[7].tolist() == [-49.5, 0.0, 0.0] and est[6, 2] == 4000
    assert eff[1] == 0 and eff[4] == 0 and eff[0] != 0 and (eff[5:9] == eff[5]).all() and eff[5] == np.float32(-est[6, 0] * 5 / 100.0)
    conf = est[1, 1]
    assert oracle.estimate(hist, first, conf, 100)[2][1] and not oracle.estimate(hist, first, np.nextafter(conf, np.inf), 100)[2][1], "conf >= min_conf"
    assert oracle.estimate(hist, first, 3.0, 150)[2][1] and not oracle.estimate(hist, first, 3.0, 151)[2][1], "peaks >= min_peaks"
    # the numpy restatement: the same bits, on these and on cells near 2^45
    big = hist.copy()
    big[:, :H] += (rng.integers(0, 1 << 20, (9, H)).astype(np.int64) << 25) + (1 << 45)
    for h in (hist, big):
        for S in (5, 2):
            want_est, want_eff, _ = oracle.estimate(h, first, 3.0, 100, S)
            got_est, got_eff = tuning.estimate_host(h, first, 3.0, 100, S)
            assert _same(got_est, want_est) and _same(got_eff, want_eff)
    for bad in ([0, 5], [1, 9], [0, 4, 3, 9], [0.5, 9], []):
        with pytest.raises(ValueError, match="first"):
            tuning.estimate_host(hist, bad)
    with pytest.raises(ValueError, match="multiple of 12"):
        tuning.bins_per_semitone(50)
    assert tuning.bins_per_semitone(60) == 5 and tuning.H == H and tuning.Q == oracle.Q and tuning.HALF_WINDOW == oracle.HALF_WINDOW


def test_detune_program():
    prog, _ = oracle.clip_program(100, 301, "own")
    same = scoregen.detune_program(prog, 0)
    assert same is not prog and np.array_equal(same, prog) and same.dtype == np.int32
    inc = prog[1:, 2].view(np.uint32).astype(np.int64)
    assert (inc > 0).any() and (inc == 0).any(), "events and padding rows"
    up, down = scoregen.detune_program(prog, 1200), scoregen.detune_program(prog, -1200)
    assert np.array_equal(up[1:, 2].view(np.uint32).astype(np.int64), 2 * inc)
    assert np.array_equal(down[1:, 2].view(np.uint32).astype(np.int64), np.rint(inc / 2.0).astype(np.int64))
    for p in (up, down, scoregen.detune_program(prog, 13)):
        assert np.array_equal(p[0], prog[0]) and np.array_equal(np.delete(p, 2, axis=1), np.delete(prog, 2, axis=1)), "only word 2 of the event rows"
    c13 = scoregen.detune_program(prog, 13)[1:, 2].view(np.uint32).astype(np.float64)
    assert np.array_equal(c13, np.rint(inc * 2.0 ** (13 / 1200.0)))
    batch = scoregen.detune_program(np.stack([prog, prog]), 13)
    assert np.array_equal(batch[1], scoregen.detune_program(prog, 13))


@pytest.fixture(scope="module")
def chain_results():
    """The float64 chain, computed once: {(instrument, seed, cents): [estimate, confidence, peaks]}."""
    return {(inst, seed, c): oracle.chain(seed, c, 301, inst) for inst in ("resynth", "own") for seed in range(100, 104) for c in (-49, -20, 0, 13, 45)}


def test_the_float64_chain_on_rendered_clips(chain_results):
    worst, low = 0.0, np.inf
    for (inst, seed, c), est in chain_results.items():
        err = oracle.cents_error(est[0], c)
        worst, low = max(worst, abs(err)), min(low, est[1])
        assert abs(err) <= ERROR_BOUND, (inst, seed, c, est)
        assert est[1] > tuning.MIN_CONF and est[2] >= tuning.MIN_PEAKS, (inst, seed, c, est)
    print(f"float64 chain over {len(chain_results)} cases: worst error {worst:.4f} cent (bound {ERROR_BOUND:.3f}), smallest confidence {low:.3f}")


def test_noise_stays_below_the_confidence_gate():
    for x in oracle.noise_tensors():
        est = oracle.estimate(oracle.profile(x[None], [x.shape[0]]), [0, 1], tuning.MIN_CONF, tuning.MIN_PEAKS)
        assert est[0][0, 1] < tuning.MIN_CONF and not est[2][0] and est[1][0] == 0, est[0]
