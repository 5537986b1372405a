"""The spectrogram augmentation without a GPU (piano_a2s_amd/augment.py, piano_a2s_amd/recipe.py, tests/specaug_oracle.py):

1. the flags' ranges and the messages that name them;
2. the draws: reproducible per (seed, rank, epoch), a stream of their own, no global generator advances, a component switched off moves no other;
3. the table: |g_k| <= E, v_k against its closed form, the augmenter's table against the oracle's;
4. the mask plan's properties over 10 000 draws per shape;
5. the definition on hand-built clips;
6. the physics check of the definition: a two-tap filter of the waveform against its gain table on the feature rows;
7. the recipe: nothing is built when every flag is off; transposition, tempo, then this, on both training paths."""
import random
import types

import numpy as np
import pytest
import torch

from piano_a2s_amd import recipe, scoregen, spec
from piano_a2s_amd.augment import SpecAugment, TempoAugment, TransposeAugment, check_specaug, specaug_table
from tests import specaug_oracle as oracle

CFG = spec.default_cfg()


# ------------------------------------------------------------------------------------------- 1. ranges
def test_flag_values_and_messages():
    assert check_specaug() == (0.0, None, 0, 0, 2)
    assert check_specaug("6", "(30, 50)", "20", 10.0, 4) == (6.0, (30.0, 50.0), 20, 10, 4)
    assert check_specaug(12, [20, 80], 100, 60, 1) == (12.0, (20.0, 80.0), 100, 60, 1)
    assert check_specaug(0, "[40,40]")[1] == (40.0, 40.0)
    bad = {"eq_augment_db": [dict(eq_db=v) for v in (-0.1, 12.5, "x", None, float("nan"), float("inf"))],
           "noise_augment_db": [dict(noise_db=v) for v in ("(10, 50)", "(30, 90)", "(50, 30)", "30", (30,), "(a, b)", (float("nan"), 50), 40)],
           "mask_time": [dict(mask_time=v) for v in (-1, 101, 2.5, "x", None)],
           "mask_freq": [dict(mask_freq=v) for v in (-1, 61, 0.5, "many")],
           "mask_count": [dict(mask_count=v) for v in (0, 5, 1.5, "x")]}
    for flag, cases in bad.items():
        for kw in cases:
            with pytest.raises(ValueError, match=flag):
                check_specaug(**kw)
    with pytest.raises(ValueError, match="eq_augment_db"):
        SpecAugment(CFG, eq_db=13, seed=1)
    with pytest.raises(ValueError, match="mask_count"):
        _brain(mask_time=10, mask_count=9)._spec_augment()          # refused from the values alone: no module, no device is touched
    with pytest.raises(ValueError, match="noise_augment_db"):
        _brain(noise_augment_db="(5, 10)")._spec_augment()


# ------------------------------------------------------------------------------------------- 2. the draws
def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_draws_are_reproducible_and_of_their_own_stream():
    kw = dict(eq_db=6, noise_db=(30, 50), mask_time=20, mask_freq=10)
    a, b = SpecAugment(CFG, seed=5, **kw), SpecAugment(CFG, seed=5, **kw)
    first = a.draw(8)
    assert first[0].dtype == np.float32 and first[0].shape == (8, 2, 480) and first[1].dtype == np.uint32 and first[1].shape == (8, 16)
    assert _same(first, b.draw(8)) and not _same(a.draw(8), first)
    a.reseed(0)
    assert _same(a.draw(8), first), "reseeding repeats the epoch"
    seen = {first[1].tobytes()}
    for k in (dict(seed=6), dict(seed=5, rank=1)):
        seen.add(SpecAugment(CFG, **kw, **k).draw(8)[1].tobytes())
    a.reseed(1)
    seen.add(a.draw(8)[1].tobytes())
    a.reseed(0, rank=2)
    seen.add(a.draw(8)[1].tobytes())
    assert len(seen) == 5, "seed, rank and epoch each change the draws"
    # neither the transposer's stream nor the tempo generator's: generators seeded as theirs give other numbers
    a.reseed(0, rank=0)
    mine = a.draw_raw(8)[0]
    for words in ([5, 0, 0], [5, 0, 0, 0x74656D70]):
        other = np.random.Generator(np.random.PCG64(np.random.SeedSequence(words))).uniform(-1.0, 1.0, size=(8, 3))
        assert not np.array_equal(other, mine)


def test_the_other_augmenters_draw_what_they_draw_alone_and_no_global_generator_advances():
    alone_t, alone_s = TransposeAugment(CFG, 3, 1.5, seed=5, device="cpu"), TempoAugment(CFG, 0.2, seed=5, device="cpu")
    want = [(alone_t.draw(8), alone_s.draw(8)) for _ in range(3)]
    random.seed(1), np.random.seed(2), torch.manual_seed(3)
    state = (random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state().clone())
    t, s, c = TransposeAugment(CFG, 3, 1.5, seed=5, device="cpu"), TempoAugment(CFG, 0.2, seed=5, device="cpu"), SpecAugment(CFG, 6, (30, 50), 20, 10, seed=5)
    for (ws, wd), wu in want:
        c.draw(8)
        s2, d2 = t.draw(8)
        c.draw(3)
        assert np.array_equal(ws, s2) and np.array_equal(wd, d2) and np.array_equal(wu, s.draw(8))
    c.reseed(4)
    c.draw(2)
    assert random.getstate() == state[0] and np.array_equal(np.random.get_state()[1], state[1]) and torch.equal(torch.get_rng_state(), state[2])


def test_switching_a_component_off_leaves_the_others_draws_unchanged():
    full = dict(eq_db=6, noise_db=(30, 50), mask_time=20, mask_freq=10)
    t_all, d_all = SpecAugment(CFG, seed=9, **full).draw(6)
    for off in ("eq_db", "noise_db", "mask_time", "mask_freq"):
        kw = dict(full)
        kw[off] = None if off == "noise_db" else 0
        aug = SpecAugment(CFG, seed=9, **kw)
        t, d = aug.draw(6)
        assert np.array_equal(d, d_all), off
        assert np.array_equal(t[:, 0], t_all[:, 0]) or off == "eq_db"
        assert np.array_equal(t[:, 1], t_all[:, 1]) or off == "noise_db"
        if off == "eq_db":
            assert (t[:, 0] == 1).all()
        if off == "noise_db":
            assert (t[:, 1] == 0).all()
        t2, d2 = aug.draw(6)                      # and the batch after it
        assert not np.array_equal(d2, d)
    raw_a, raw_b = SpecAugment(CFG, seed=9, **full).draw_raw(6), SpecAugment(CFG, seed=9, mask_time=5).draw_raw(6)
    assert _same(raw_a, raw_b), "what leaves the generator does not depend on the components"
    assert not SpecAugment(CFG, seed=9).active and SpecAugment(CFG, seed=9, mask_freq=1).active


# ------------------------------------------------------------------------------------------- 3. the table
@pytest.mark.parametrize("F", [1, 37, 480])
def test_table_bounds_and_closed_forms(F):
    rng = np.random.default_rng(F)
    E, bpo = 12.0, 60
    for _ in range(50):
        e, phi = rng.uniform(-1, 1, 3) * E / 3, rng.random(2)
        L, tilt = rng.uniform(20, 80), rng.uniform(-3, 3)
        tab = oracle.table(F, e, phi, L, tilt, bpo)
        assert tab.dtype == np.float32 and tab.shape == (2, F)
        g = 10 * np.log10(tab[0].astype(np.float64))
        assert np.abs(g).max() <= E + 1e-5, "|g_k| <= E"
        k = np.arange(F)
        want = 10.0 ** ((-L + tilt * (k - (F - 1) / 2) / bpo) / 10)
        assert np.allclose(tab[1], want, rtol=1e-6, atol=0)
        assert np.allclose(tab, specaug_table(F, e, phi, L, tilt, bpo), rtol=2.0 ** -22, atol=0), "the augmenter's table is the oracle's (vectorised against scalar float64: one fp32 ulp)"
        off = specaug_table(F, e, phi, L, tilt, bpo, eq=False, noise=False)
        assert (off[0] == 1).all() and (off[1] == 0).all() and np.array_equal(off, oracle.table(F, e, phi, L, tilt, bpo, eq=False, noise=False))
    # the extremes: every e at its bound, the phases where the cosines peak together
    tab = oracle.table(F, np.full(3, E / 3), (0.0, 0.0), 20, 3, bpo)
    assert np.abs(10 * np.log10(tab[0].astype(np.float64))).max() <= E + 1e-5
    # the noise level in the middle of the range is L dB below the peak
    if F > 1:
        assert abs(10 * np.log10(float(oracle.table(F, e, phi, 40.0, 0.0, bpo)[1, F // 2])) + 40.0) < 1e-5


def test_augmenter_table_follows_its_draws():
    aug = SpecAugment(CFG, 6, (30, 50), seed=3)
    e, phi, ul, ut, words = aug.draw_raw(4)
    aug.reseed(0)
    tab, d = aug.draw(4)
    assert np.array_equal(d, words)
    for b in range(4):
        assert np.allclose(tab[b], oracle.table(480, e[b] * 2.0, phi[b], 30 + ul[b] * 20, ut[b] * 3.0, 60), rtol=2.0 ** -22, atol=0)
    assert (np.abs(10 * np.log10(tab[:, 0].astype(np.float64))) <= 6 + 1e-5).all()
    lev = -10 * np.log10(tab[:, 1, [0, 479]].astype(np.float64))
    assert (lev >= 30 - 3 * 4 - 1e-4).all() and (lev <= 50 + 3 * 4 + 1e-4).all(), "the level stays in the range up to the tilt over +- 4 octaves"


# ------------------------------------------------------------------------------------------- 4. the mask plan
@pytest.mark.parametrize("F", [1, 37, 480])
@pytest.mark.parametrize("n", [0, 1, 4, 5, 6, 400, 1201])
def test_mask_plan_properties(n, F):
    rng = np.random.default_rng(1000 * n + F)
    draws = rng.integers(0, 2 ** 32, size=(10000, 16), dtype=np.uint32)
    draws[0], draws[1] = 0, 0xFFFFFFFF                                     # the two extreme words
    widest_t = widest_f = 0
    for i, d in enumerate(draws):
        Wt, Wf, m = (100, 60, 4) if i < 2 else (int(rng.integers(0, 101)), int(rng.integers(0, 61)), int(rng.integers(0, 5)))
        p = oracle.mask_plan(n, F, d, Wt, Wf, m)
        assert len(p) == 16
        for j in range(4):
            t0, w, k0, wk = p[2 * j], p[2 * j + 1], p[8 + 2 * j], p[9 + 2 * j]
            assert 0 <= t0 and 0 <= w and t0 + w <= n and 0 <= k0 and 0 <= wk and k0 + wk <= F, (n, F, p)
            assert w <= min(Wt, n // 5) and wk <= min(Wf, F // 5)
            if j >= m:
                assert (t0, w, k0, wk) == (0, 0, 0, 0)
            widest_t, widest_f = max(widest_t, w), max(widest_f, wk)
    assert widest_t == min(100, n // 5) and widest_f == min(60, F // 5), "the largest width is reached (by the all-ones word)"


# ------------------------------------------------------------------------------------------- 5. the definition on hand-built clips
def _clip(rows=12, F=9, n=9, seed=0):
    """n rows of content in [0.45, 1] with a third of the cells at one floor value and one cell at 1.0, padding behind."""
    rng = np.random.default_rng(seed)
    x = np.zeros((rows, F), dtype=np.float32)
    c = (0.5 + 0.5 * rng.random((n, F))).astype(np.float32)
    c[rng.random((n, F)) < 0.35] = np.float32(0.4531)
    c[n // 2, F // 3] = 1.0
    c[0, 0] = np.float32(0.4531)
    c[n - 1, F - 1] = 0.75
    x[:n] = c
    return x


NEUTRAL = lambda F: np.stack([np.ones(F), np.zeros(F)]).astype(np.float32)


def test_neutral_parameters_return_the_input():
    for seed in range(5):
        x = _clip(seed=seed)
        r = oracle.apply(x, NEUTRAL(9))
        assert r["n"] == 9 and r["M"] == 1.0 and r["x_min"] == np.float32(0.4531)
        assert np.abs(r["out"] - x.astype(np.float64)).max() <= 1e-12
        assert (r["out"][9:] == 0).all()


def test_floor_cells_stay_and_nothing_falls_below_the_floor():
    x = _clip(seed=1)
    rng = np.random.default_rng(7)
    for trial in range(20):
        tab = NEUTRAL(9)
        tab[0] = 10 ** (rng.uniform(-12, 12, 9) / 10)                       # any gain, cuts and boosts
        r = oracle.apply(x, tab)
        n, out, floor = r["n"], r["out"], r["floor"]
        assert floor.any() and not floor.all()
        image = out[:n][floor]
        assert (image == image[0]).all(), "every floor cell has the same image"
        # the floor cell's power relative to the new peak: p_min / M; where the peak did not move, the cell did not either
        assert abs(image[0] - np.clip(1 + np.log10(oracle.power(r["x_min"]) / r["M"]) / 8, 0, 1)) < 1e-15
        assert (out[:n] >= image[0]).all(), "no cell comes out below the floor's image"
        assert out[:n].max() == 1.0 and (out[n:] == 0).all()
    # a cut of every bin by the same 10 dB: the peak cell is still the peak, the floor cells rise by 10 dB / 80 against it
    tab = NEUTRAL(9)
    tab[0] = 0.1
    r = oracle.apply(x, tab)
    assert abs(r["out"][:9][r["floor"]][0] - (0.4531 + 0.125)) < 1e-6
    # cells within 2^-18 of the minimum are floor cells, cells further above are not
    y = x.copy()
    y[1, 1], y[1, 2] = np.float32(0.4531) + np.float32(2.0 ** -19), np.float32(0.4531) + np.float32(2.0 ** -16)
    f = oracle.apply(y, NEUTRAL(9))["floor"]
    assert f[1, 1] and not f[1, 2]


def test_noise_lifts_the_floor_and_masks_and_padding_are_zero():
    x = _clip(rows=40, F=37, n=33, seed=2)
    tab = oracle.table(37, (1.0, -2.0, 0.5), (0.3, 0.8), 30.0, 1.5, 60)
    plan = oracle.mask_plan(33, 37, np.arange(16, dtype=np.uint64) * 0x10000000 + 12345, 5, 6, 3)
    r = oracle.apply(x, tab, plan)
    out, m = r["out"], r["masked"]
    assert m.any() and (out[m] == 0).all() and (out[33:] == 0).all() and not m[33:, :].all()
    free = ~m[:33]
    assert (out[:33][free] > 0).all()
    # a floor cell under noise: its power is max(p_min, v_k), never less than without noise
    quiet = oracle.apply(x, np.stack([tab[0], np.zeros(37, dtype=np.float32)]), plan)
    assert (r["y"] >= quiet["y"]).all()
    if not m[:33][np.unravel_index(np.argmax(r["y"]), r["y"].shape)]:
        assert out.max() == 1.0
    zero = oracle.apply(np.zeros((5, 37), dtype=np.float32), tab, plan)
    assert zero["n"] == 0 and (zero["out"] == 0).all()
    neg = np.zeros((5, 37), dtype=np.float32)
    neg[:] = -0.0
    assert oracle.apply(neg, tab)["n"] == 0
    nan = np.zeros((5, 37), dtype=np.float32)
    nan[2, 3] = np.nan
    assert oracle.content_rows(nan) == 3


# ------------------------------------------------------------------------------------------- 6. physics
FILTERS = (-0.9, -0.5, 0.5, 0.9)

@pytest.mark.parametrize("seed", [3, 7, 11])
def test_a_filter_on_the_waveform_is_the_gain_table_on_the_feature_rows(seed):
    """mean |augmented dry features - features of the filtered waveform| < 0.5 * mean |dry features - features of the filtered waveform| for
    y[n] = x[n] + c x[n - 1], c in {-0.9, -0.5, 0.5, 0.9}, host renderer and direct-form VQT.  Measured: 0.006 - 0.253 (the boosts
    are the larger ones: what is hidden under the floor cannot rise out of it); 0.5 is twice the worst."""
    from oracle.vqt_ref import vqt_direct
    from tests.render_oracle import render
    clip = scoregen.make_clip(spec.default_cfg(max_bars=2), seed, frames=301)
    wave = render(scoregen.pack_program(clip, rows=len(clip["events"])))
    dry = vqt_direct(wave).astype(np.float32)
    at_floor = float((dry - dry.min() <= oracle.FLOOR_EPS).mean())
    print(f"seed {seed}: {dry.shape[0]} frames, {100 * at_floor:.1f} % of the cells at the floor value {dry.min():.4f}")
    for c in FILTERS:
        filtered = wave.copy()
        filtered[1:] += c * wave[:-1]
        wet = vqt_direct(filtered)
        aug = oracle.apply(dry, oracle.filter_gain_table(c))["out"]
        with_aug, without = float(np.abs(aug - wet).mean()), float(np.abs(dry.astype(np.float64) - wet).mean())
        print(f"seed {seed}, c = {c}: mean |augmented - filtered| = {with_aug:.5f}, mean |dry - filtered| = {without:.5f}, ratio {with_aug / without:.3f}")
        assert with_aug < 0.5 * without, (seed, c, with_aug, without)


# ------------------------------------------------------------------------------------------- 7. the switch and the recipe
def _brain(**hparams):
    brain = recipe.ASR.__new__(recipe.ASR)
    brain.device = "cpu"
    brain.hparams = types.SimpleNamespace(seed=1234, **hparams)
    brain.teacher_forcing_ratio = 0.5
    return brain


def _batch():
    return [torch.rand(2, 1, 7, 480), torch.zeros(2, 5, dtype=torch.long), torch.full((2, 5), 6), torch.ones(2, 5, 9, dtype=torch.long), torch.ones(2, 5),
            torch.ones(2, 5, 6, dtype=torch.long), torch.ones(2, 5), ["a", "b"], torch.zeros(2)]


def test_off_builds_nothing_and_hands_on_the_same_tensors():
    for hp in ({}, dict(eq_augment_db=0, mask_time="0", mask_freq=0, mask_count=3), dict(eq_augment_db="0.0", noise_augment_db=None)):
        brain = _brain(**hp)
        assert brain._spec_augment() is None and brain._specaug is None
        assert not hasattr(brain, "_augment") and not hasattr(brain, "_tempo"), "the switch has an attribute of its own"
        batch = _batch()
        out = brain._train_features(batch)
        assert all(o is b for o, b in zip(out, batch)), "the tensors that reach the step are the ones that reach it without the feature"


def test_any_one_component_builds_the_augmenter():
    class Model:
        cfg = CFG

    for hp in (dict(eq_augment_db=3), dict(noise_augment_db="(30, 40)"), dict(mask_time=10), dict(mask_freq=5)):
        brain = _brain(**hp)
        brain.modules = types.SimpleNamespace(transcription=Model())
        aug = brain._spec_augment()
        assert isinstance(aug, SpecAugment) and aug.active and aug.m == 2 and aug.seed == 1234
    brain = _brain(mask_time=10)
    brain.modules = types.SimpleNamespace(transcription=object())
    with pytest.raises(ValueError, match="freq_bins"):
        brain._spec_augment()


class _Stage:
    """Stands in for an augmenter: features -> features * a + b (so that the order shows); the transposer's also rewrites the targets in place."""

    def __init__(self, log, name, a, b, targets=False):
        self.log, self.name, self.a, self.b, self.targets = log, name, a, b, targets

    def __call__(self, batch):
        self.log.append(self.name)
        batch = list(batch)
        batch[0] = batch[0] * self.a + self.b
        if self.targets:
            for i in (2, 3, 5):
                batch[i] += 100
        return batch

    def reseed(self, epoch):
        self.log.append((self.name, epoch))


@pytest.mark.parametrize("others", [True, False], ids=["after_transposition_and_tempo", "alone"])
def test_both_training_paths_apply_it_last(monkeypatch, others):
    seen = {}

    class Fused:
        def __call__(self, batch, tf):
            seen["fused"] = batch

        def report(self):
            return [0.1, 0.2, 0.3, 0.4, 1.0]

    monkeypatch.setattr(recipe.sb.Brain, "fit_batch", lambda self, batch: seen.__setitem__("generic", batch) or torch.tensor(0.0))
    for path in ("fused", "generic"):
        log = []
        brain = _brain()
        brain._augment = _Stage(log, "transpose", 1, 1, targets=True) if others else None
        brain._tempo = _Stage(log, "tempo", 2, 0) if others else None
        brain._specaug = _Stage(log, "specaug", 3, 5)
        brain._fused = Fused() if path == "fused" else False
        brain.time_losses, brain.key_losses, brain.upper_losses, brain.lower_losses = [], [], [], []
        batch = _batch()
        keep = [t.clone() if torch.is_tensor(t) else t for t in batch]
        brain.fit_batch(batch)
        got = seen[path]
        if others:
            assert log == ["transpose", "tempo", "specaug"]
            assert torch.equal(got[0], ((keep[0] + 1) * 2) * 3 + 5) and all(torch.equal(got[i], keep[i] + 100) for i in (2, 3, 5))
        else:
            assert log == ["specaug"]
            assert torch.equal(got[0], keep[0] * 3 + 5) and all(got[i] is batch[i] for i in (2, 3, 5)), "no target is touched, none is copied"
        assert all(torch.equal(batch[i], keep[i]) for i in (0, 2, 3, 5)), "the caller's tensors are as they were"
        again = recipe._features(got, "cpu")
        assert all(a is g for a, g in zip(again, got))
