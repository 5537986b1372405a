"""The room acoustics without a GPU (piano_a2s_amd/room.py, piano_a2s_amd/recipe.py, tests/room_oracle.py):

1. Room.params: reproducible, inside its ranges, pre >= 1, equal to the oracle's scalar restatement;
2. the closed form of the tail's energy;
3. the oracle's FIR against np.convolve;
4. the switch: --synthetic_room without the rendered corpus, bad values and bad ranges raise; off builds nothing."""
import types

import numpy as np
import pytest
import torch

from piano_a2s_amd import recipe, scoregen
from piano_a2s_amd.room import Room, check_stages, room_seeds
from tests import room_oracle

SEEDS = (np.arange(1000, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xFFFFFFFF)


def _f32(words):
    return np.ascontiguousarray(words).view(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------- 1. the parameter table
def test_params_are_reproducible_and_inside_their_ranges():
    room = Room()
    assert room.L_max == 10_000 == room_oracle.default_L_max()
    table = room.params(SEEDS)
    assert table.shape == (1000, 4) and table.dtype == np.int32
    assert np.array_equal(table, Room().params(SEEDS.copy())), "the same seeds give the same table"
    assert np.array_equal(table[17:18], room.params(SEEDS[17:18])), "a clip's row does not depend on the batch"
    rt60, drr, pre = room.draws(SEEDS)
    assert (rt60 >= 0.2).all() and (rt60 < 0.6).all() and (drr >= 0).all() and (drr < 12).all()
    assert (pre >= 1).all() and (pre >= 80).all() and (pre <= 400).all() and np.array_equal(pre, table[:, 0])
    assert (table[:, 1] > table[:, 0]).all() and (table[:, 1] <= room.L_max).all()
    assert np.array_equal(table[:, 1], np.minimum(room.L_max, pre + np.ceil(rt60 * 16000).astype(np.int64)))
    wet, decay = _f32(table[:, 2]), _f32(table[:, 3])
    assert np.allclose(decay, np.log(1000.0) / (rt60 * 16000), rtol=1e-7, atol=0) and (wet > 0).all()
    assert (wet <= np.sqrt(3.0 * (1.0 - np.exp(-2.0 * np.log(1000.0) / 3200)))).all(), "at 0 dB and the shortest RT60"
    # the draws spread over their ranges and are not the same draw three times
    assert rt60.max() - rt60.min() > 0.39 and drr.max() - drr.min() > 11.8 and pre.max() - pre.min() > 310
    assert abs(np.corrcoef(rt60, drr)[0, 1]) < 0.1 and abs(np.corrcoef(rt60, pre)[0, 1]) < 0.1


def test_params_equal_the_oracles_scalar_restatement():
    room, short = Room(), Room(rt60=(0.3, 1.2), drr_db=(-3, 6), predelay_ms=(1, 2.5), sample_rate=22050, L_max=5000)
    for seed in (0, 1, 0xFFFFFFFF, 0x524F4F4D, *SEEDS[:40].tolist()):
        assert np.array_equal(room.params([seed])[0], room_oracle.table_row(room_oracle.params(seed))), seed
        p = room_oracle.params(seed, rt60=(0.3, 1.2), drr_db=(-3, 6), predelay_ms=(1, 2.5), sr=22050, L_max=5000)
        assert np.array_equal(short.params([seed])[0], room_oracle.table_row(p)) and p["pre"] >= 1 and p["L"] == 5000, seed


def test_room_seed_is_the_noise_seed_xor_the_constant():
    progs = np.stack([scoregen.pack_rows(100, [], noise_seed=s, rows=3) for s in (0, 0x80000001, 0xFFFFFFFF)])
    want = np.array([0x524F4F4D, 0x80000001 ^ 0x524F4F4D, 0xFFFFFFFF ^ 0x524F4F4D], dtype=np.uint32)
    assert np.array_equal(room_seeds(progs), want) and np.array_equal(room_seeds(torch.from_numpy(progs)), want)


# ------------------------------------------------------------------------------------------- 2. the tail's energy
def test_closed_form_of_the_tail_energy():
    """E[h[k]^2] = wet^2 / 3 * exp(-2 decay (k - pre)) for k >= pre (u has variance 1/3); summed over the tail it is
    10^(-drr / 10) * (1 - exp(-2 decay (L - pre))): the direct-to-reverberant ratio, short of it only by what L truncates."""
    worst = 0.0
    for seed in SEEDS[:50].tolist():
        for L_max in (None, 3000):
            p = room_oracle.params(seed, L_max=L_max)
            k = np.arange(p["pre"], p["L"], dtype=np.float64)
            lhs = np.sum(p["wet64"] ** 2 * np.exp(-2.0 * p["decay64"] * (k - p["pre"])) / 3.0)
            rhs = 10.0 ** (-p["drr_db"] / 10.0) * (1.0 - np.exp(-2.0 * p["decay64"] * (p["L"] - p["pre"])))
            worst = max(worst, abs(lhs - rhs))
            assert abs(lhs - rhs) <= 1e-12, (seed, L_max, lhs, rhs)
            if L_max is None:                                          # the whole tail: -60 dB at RT60, energy 1e-12 of the ratio is missing
                assert rhs > 10.0 ** (-p["drr_db"] / 10.0) * (1 - 2e-6)
    print(f"closed form: largest |sum - closed form| {worst:.2e}")


def test_impulse_response_shape_and_energy():
    seed = 0xC0FFEE
    p = room_oracle.params(seed)
    h = room_oracle.impulse_response(seed, p["pre"], p["L"], p["wet"], p["decay"], L_max=10_000)
    assert h.shape == (10_000,) and h[0] == 1.0 and (h[1:p["pre"]] == 0).all() and (h[p["L"]:] == 0).all() and (h[p["pre"]:p["L"]] != 0).mean() > 0.99
    tail = np.sum(h[p["pre"]:] ** 2)
    assert abs(tail / 10.0 ** (-p["drr_db"] / 10.0) - 1.0) < 0.1, "the realised tail energy is the ratio's, within the spread of a few thousand draws"
    env = np.abs(h[p["pre"]:p["L"]])
    assert env[:200].max() <= p["wet"] and env[-1] <= 1.001e-3 * p["wet"] * np.exp(p["decay"]), "-60 dB at the end of the tail"


# ------------------------------------------------------------------------------------------- 3. the FIR
def test_oracle_fir_is_the_convolution():
    rng = np.random.default_rng(5)
    for N, L in ((1, 1), (7, 1), (50, 9), (50, 50), (40, 77), (300, 120)):
        x, h = rng.standard_normal(N), rng.standard_normal(L)
        want = np.convolve(x, h)[:N]
        assert np.allclose(room_oracle.fir(x, h), want, rtol=0, atol=1e-12), (N, L)
        cut = max(1, L // 2)
        assert np.allclose(room_oracle.fir(x, h, L=cut), np.convolve(x, h[:cut])[:N], rtol=0, atol=1e-12), "taps behind L are not used"
    xi, hi = rng.integers(-3, 4, 200).astype(np.float64), rng.integers(-2, 3, 90).astype(np.float64)
    assert np.array_equal(room_oracle.fir(xi, hi), np.convolve(xi, hi)[:200]), "integers: exact"
    y, p = room_oracle.apply(xi, 99, L_max=64)
    assert p["L"] == 64 and np.array_equal(y[:p["pre"]], xi[:p["pre"]]), "before the pre-delay only the direct path sounds"


# ------------------------------------------------------------------------------------------- 4. the switch
def _brain(**hparams):
    brain = recipe.ASR.__new__(recipe.ASR)
    brain.device = "cpu"
    brain.hparams = types.SimpleNamespace(seed=1234, **hparams)
    return brain


def test_switch_values_and_the_rendered_corpus():
    assert check_stages(None) == "none" and check_stages(" Train ") == "train" and check_stages("eval") == "eval" and check_stages("ALL") == "all"
    for bad in ("valid", "", "true", 1):
        with pytest.raises(ValueError, match="synthetic_room"):
            check_stages(bad)
    assert recipe.synthetic_room({}) is None and recipe.synthetic_room({"synthetic_room": "none", "room_rt60": "(9, 1)"}) is None
    for hp in ({"synthetic_room": "all"}, {"synthetic_room": "train", "synthetic_clips": 8}, {"synthetic_room": "eval", "synthetic_clips": 8, "synthetic_scores": "random"},
               {"synthetic_room": "all", "synthetic_scores": "rendered"}):
        with pytest.raises(ValueError, match="synthetic_scores=rendered"):
            recipe.synthetic_room(hp)
    with pytest.raises(ValueError, match="synthetic_scores=rendered"):
        _brain(synthetic_room="train")._room(recipe.sb.Stage.TRAIN)          # refused from the values alone: no module, no device is touched
    with pytest.raises(ValueError, match="synthetic_room"):
        _brain(synthetic_room="sometimes", synthetic_clips=8, synthetic_scores="rendered")._room(recipe.sb.Stage.TRAIN)
    ok = {"synthetic_clips": 8, "synthetic_scores": "rendered", "sample_rate": 16000}
    mode, room = recipe.synthetic_room({**ok, "synthetic_room": "eval", "room_rt60": "(0.3, 0.5)", "room_drr_db": (-2, 3.5), "room_predelay_ms": "[10,12]"})
    assert mode == "eval" and room.rt60 == (0.3, 0.5) and room.drr_db == (-2.0, 3.5) and room.predelay_ms == (10.0, 12.0) and room.L_max == 192 + 8000
    with pytest.raises(ValueError, match="room_rt60"):
        recipe.synthetic_room({**ok, "synthetic_room": "all", "room_rt60": "(0.5, 0.3)"})


def test_stages():
    S = recipe.sb.Stage
    hp = dict(synthetic_clips=8, synthetic_scores="rendered")
    for mode, want in (("train", (True, False, False)), ("eval", (False, True, True)), ("all", (True, True, True))):
        brain = _brain(synthetic_room=mode, **hp)
        got = tuple(brain._room(s) is not None for s in (S.TRAIN, S.VALID, S.TEST))
        assert got == want, mode
        assert brain._room(S.TRAIN) is brain._room(S.TRAIN) or not want[0], "one Room per run"
    brain = _brain(**hp)
    assert all(brain._room(s) is None for s in (S.TRAIN, S.VALID, S.TEST)) and brain._synthetic_room is None


def test_bad_ranges_raise():
    for kw in (dict(rt60=(0.6, 0.2)), dict(rt60=(0.0, 0.5)), dict(rt60=(0.2, 11.0)), dict(rt60="(a, b)"), dict(rt60=(0.2,)), dict(rt60=0.3),
               dict(drr_db=(3, float("nan"))), dict(drr_db=(-50, 0)), dict(drr_db=(0, float("inf"))), dict(predelay_ms=(0.0, 5.0)), dict(predelay_ms=(30, 20)),
               dict(predelay_ms=(5, 2000)), dict(sample_rate=0)):
        with pytest.raises(ValueError, match="room"):
            Room(**kw)
    with pytest.raises(ValueError, match="L_max"):
        Room(L_max=0)
    with pytest.raises(ValueError, match="L_max"):
        Room(L_max=10_001)
    assert Room(rt60="(0.2, 0.2)", predelay_ms=(1, 1), sample_rate=1000).params([5])[0, 0] == 1, "the smallest pre-delay still leaves pre >= 1"


def test_off_leaves_the_features_path_as_it_was():
    batch = [torch.rand(2, 1, 7, 480), torch.zeros(2, 5, dtype=torch.long)]
    out = recipe._features(list(batch), "cpu")
    assert all(o is b for o, b in zip(out, batch))
    out = recipe._features(list(batch), "cpu", room=Room())              # features that are no render programs pass a room untouched
    assert all(o is b for o, b in zip(out, batch))
    with pytest.raises(recipe_error()):
        Room().apply(torch.zeros(2, 100), [1, 2])                        # a CPU waveform


def recipe_error():
    from piano_a2s_amd.hip import A2SError
    return A2SError
