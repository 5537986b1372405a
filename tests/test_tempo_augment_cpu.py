"""The tempo augmentation without a GPU (piano_a2s_amd/augment.py, piano_a2s_amd/recipe.py, tests/tempo_oracle.py):

1. the definition: identity at step 65536, at most three taps, weights that sum to W, and the kernel's closed form of the tap rows;
2. the plan never loses the last content frame;
3. the draws: reproducible, a stream of their own, no global generator advances;
4. the switch is parsed and refused as documented; nothing is built when it is off; transposition runs first, then tempo, on both training paths."""
import random
import types

import numpy as np
import pytest
import torch

from piano_a2s_amd import recipe, spec
from piano_a2s_amd.augment import TempoAugment, TransposeAugment, check_tempo
from tests import tempo_oracle as oracle

STEPS = [52429, 60000, 65535, 65536, 65537, 75000, 87381]
ROWS = 37


# ------------------------------------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("step", STEPS)
def test_oracle_properties(step):
    x = np.random.default_rng(step).random((ROWS, 5))
    y = oracle.stretch(x, step)
    if step == oracle.ONE:
        assert np.array_equal(y, x), "step 65536 is the identity"
    h = max(oracle.ONE, step)
    for t in range(ROWS + 8):          # (+ 8: the rows a thread of the last workgroup computes positions for)
        ks, ws, W = oracle.taps(step, t)
        assert 1 <= len(ks) <= 3 and W == sum(ws) and all(w > 0 for w in ws)
        assert ks == list(range(ks[0], ks[0] + len(ks))), "the taps are neighbours"
        if step <= oracle.ONE:
            assert W == oracle.ONE and ks[0] == (t * step) >> 16 and len(ks) <= 2
        # the closed form csrc/a2s_tempo.hip uses: the first tap is floor((pos - h + 65536) / 65536), the last floor((pos + h - 1) / 65536)
        pos = t * step
        assert ks[0] == (pos - h + oracle.ONE) >> 16 and ks[-1] == (pos + h - 1) >> 16
    assert np.array_equal(oracle.stretch(x, 0), np.zeros_like(x)) and np.array_equal(oracle.stretch(x, 200000), np.zeros_like(x))


def test_a_thread_of_the_kernel_never_needs_more_than_13_source_rows():
    """8 consecutive output rows, the first at any row of a 16384-row clip: first tap of the first to last tap of the last, at the two extreme steps
    and around 65536 (the kernel keeps 13 rows in registers and compiles, for its r-th row, the offsets floor(r * 52429 / 65536) .. ceil(r * 87381 / 65536))."""
    for step in (52429, 65535, 65536, 65537, 87380, 87381):
        h = max(oracle.ONE, step)
        t0 = np.arange(0, 16384, dtype=np.int64)
        first = (t0 * step - h + oracle.ONE) >> 16
        for r in range(8):
            pos = (t0 + r) * step
            d = ((pos - h + oracle.ONE) >> 16) - first
            assert d.min() >= (r * 52429) >> 16 and d.max() <= (r * 87381 + 65535) >> 16, (step, r)
            assert (((pos + h - 1) >> 16) - first).max() <= 12, (step, r)
        assert int(((t0 + 8) * step + h).max()) < 2 ** 31


# ------------------------------------------------------------------------------------------- 2. the plan
def test_the_plan_keeps_the_last_content_frame():
    cases = 0
    for rows in (37, 201, 1201):
        min_frames = min(400, rows // 3)
        contents = sorted({1, 2, rows // 3 - 1, rows // 3, rows // 3 + 1, rows // 2, (3 * rows) // 4, (4 * rows) // 5, rows - rows // 8, rows - 2, rows - 1, rows})
        for R in (0.15, 0.25):
            for n in contents:
                for u in (0.0, 0.5, 0.999999):
                    step, kept = oracle.plan(n, rows, u, R, min_frames)
                    assert oracle.MIN_STEP <= step <= oracle.MAX_STEP and (step == oracle.ONE or not kept)
                    h, k = max(oracle.ONE, step), (n - 1) * oracle.ONE
                    t = np.arange(rows, dtype=np.int64)
                    assert (h - np.abs(k - t * step) > 0).any(), (rows, n, u, R, step)
                    cases += 1
    assert cases == 3 * 2 * 12 * 3
    assert oracle.plan(0, 37, 0.5, 0.25, 12) == (oracle.ONE, True), "an all-zero clip is kept"
    assert oracle.plan(37, 37, 0.999999, 0.25, 12)[0] >= oracle.ONE, "a clip that fills its window is only ever compressed"
    assert oracle.plan(5, 37, 0.0, 0.25, 12) == (oracle.ONE, True), "less content than min_frames could be stretched to: no feasible interval"


# ------------------------------------------------------------------------------------------- 3. the draws
def test_draws_are_reproducible_and_of_their_own_stream():
    cfg = spec.default_cfg()
    a, b = TempoAugment(cfg, 0.15, seed=5, device="cpu"), TempoAugment(cfg, 0.15, seed=5, device="cpu")
    ua = a.draw(16)
    assert ua.dtype == np.float32 and ua.shape == (16,) and (ua >= 0).all() and (ua < 1).all()
    assert np.array_equal(ua, b.draw(16)) and not np.array_equal(a.draw(16), ua)
    a.reseed(0)
    assert np.array_equal(a.draw(16), ua), "reseeding repeats the epoch"
    seen = {ua.tobytes()}
    for kw in (dict(seed=6), dict(seed=5, rank=1)):
        seen.add(TempoAugment(cfg, 0.15, device="cpu", **kw).draw(16).tobytes())
    a.reseed(1)
    seen.add(a.draw(16).tobytes())
    a.reseed(0, rank=2)
    seen.add(a.draw(16).tobytes())
    assert len(seen) == 5, "seed, rank and epoch each change the draws"
    # not the transposer's stream: a generator seeded as the transposer's gives other numbers
    like_transposer = np.random.Generator(np.random.PCG64(np.random.SeedSequence([5, 0, 0]))).random(size=16, dtype=np.float32)
    assert not np.array_equal(like_transposer, ua)


def test_the_transposer_draws_what_it_draws_alone_and_no_global_generator_advances():
    cfg = spec.default_cfg()
    alone = TransposeAugment(cfg, 3, 1.5, seed=5, device="cpu")
    want = [alone.draw(8) for _ in range(3)]
    random.seed(1), np.random.seed(2), torch.manual_seed(3)
    state = (random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state().clone())
    beside, tempo = TransposeAugment(cfg, 3, 1.5, seed=5, device="cpu"), TempoAugment(cfg, 0.2, seed=5, device="cpu")
    for s, d in want:
        tempo.draw(8)
        s2, d2 = beside.draw(8)
        tempo.draw(3)
        assert np.array_equal(s, s2) and np.array_equal(d, d2)
    tempo.reseed(4)
    assert random.getstate() == state[0] and np.array_equal(np.random.get_state()[1], state[1]) and torch.equal(torch.get_rng_state(), state[2])


# ------------------------------------------------------------------------------------------- 4. the switch and the recipe
def _brain(**hparams):
    brain = recipe.ASR.__new__(recipe.ASR)
    brain.device = "cpu"
    brain.hparams = types.SimpleNamespace(seed=1234, **hparams)
    brain.teacher_forcing_ratio = 0.5
    return brain


def _batch():
    return [torch.rand(2, 1, 7, 480), torch.zeros(2, 5, dtype=torch.long), torch.full((2, 5), 6), torch.ones(2, 5, 9, dtype=torch.long), torch.ones(2, 5),
            torch.ones(2, 5, 6, dtype=torch.long), torch.ones(2, 5), ["a", "b"], torch.zeros(2)]


def test_switch_values():
    assert check_tempo(0) == 0.0 and check_tempo("0.15") == 0.15 and check_tempo(0.25) == 0.25
    for R in (0.4, "0.4", -0.1, 0.2500001, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="tempo_augment"):
            check_tempo(R)
    with pytest.raises(ValueError, match="tempo_augment"):
        TempoAugment(spec.default_cfg(), 0.3, seed=1, device="cpu")
    with pytest.raises(ValueError, match="min_frames"):
        TempoAugment(spec.default_cfg(), 0.1, seed=1, device="cpu", min_frames=0)
    with pytest.raises(ValueError, match="tempo_augment"):
        _brain(tempo_augment="0.4")._tempo_augment()          # refused from the value alone: no module, no device is touched


def test_off_builds_nothing_and_hands_on_the_same_tensors():
    brain = _brain()
    assert brain._tempo_augment() is None and brain._tempo is None
    assert not hasattr(brain, "_augment"), "the tempo switch has an attribute of its own"
    batch = _batch()
    out = brain._train_features(batch)
    assert all(o is b for o, b in zip(out, batch)), "the tensors that reach the step are the ones that reach it without the feature"
    assert _brain(tempo_augment=0)._tempo_augment() is None and _brain(tempo_augment="0.0")._tempo_augment() is None


class _Transposer:
    """Stands in for augment.TransposeAugment: features + 1, targets + 100 in place."""

    def __init__(self, log):
        self.log = log

    def __call__(self, batch):
        self.log.append("transpose")
        batch = list(batch)
        batch[0] = batch[0] + 1
        for i in (2, 3, 5):
            batch[i] += 100
        return batch

    def reseed(self, epoch):
        self.log.append(("transpose", epoch))


class _Stretcher:
    """Stands in for augment.TempoAugment: features * 2 (so that the order shows), targets untouched."""

    def __init__(self, log):
        self.log = log

    def __call__(self, batch):
        self.log.append("tempo")
        batch = list(batch)
        batch[0] = batch[0] * 2
        return batch

    def reseed(self, epoch):
        self.log.append(("tempo", epoch))


@pytest.mark.parametrize("both", [True, False], ids=["with_transposition", "tempo_alone"])
def test_both_training_paths_get_the_batch_transposed_first_then_stretched(monkeypatch, both):
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
        brain._augment = _Transposer(log) if both else None
        brain._tempo = _Stretcher(log)
        brain._fused = Fused() if path == "fused" else False
        brain.time_losses, brain.key_losses, brain.upper_losses, brain.lower_losses = [], [], [], []
        batch = _batch()
        keep = [t.clone() if torch.is_tensor(t) else t for t in batch]
        brain.fit_batch(batch)
        got = seen[path]
        if both:
            assert log == ["transpose", "tempo"]
            assert torch.equal(got[0], (keep[0] + 1) * 2) and all(torch.equal(got[i], keep[i] + 100) for i in (2, 3, 5))
        else:
            assert log == ["tempo"]
            assert torch.equal(got[0], keep[0] * 2) and all(got[i] is batch[i] for i in (2, 3, 5)), "no target is touched, none is copied"
        assert all(torch.equal(batch[i], keep[i]) for i in (0, 2, 3, 5)), "the caller's tensors are as they were"
        again = recipe._features(got, "cpu")
        assert all(a is g for a, g in zip(again, got))
