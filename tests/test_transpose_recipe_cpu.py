"""The recipe's side of the transposition augmentation, without a GPU (piano_a2s_amd/recipe.py): the switches are parsed and
refused as documented, nothing is built when they are off, and both training paths hand the augmented batch on."""
import types

import pytest
import torch

from piano_a2s_amd import recipe
from piano_a2s_amd.augment import check_range


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
    assert check_range(0, 0) == (0, 0.0) and check_range("3", "1.5") == (3, 1.5) and check_range(6, 2.5) == (6, 2.5)
    for K, D in ((9, 0), ("9", 0), (-1, 0), (7, 0), ("2.5", 0), (1, 2.6), (1, -0.5), ("x", 0), (1, "y")):
        with pytest.raises(ValueError, match="transpose_augment|detune_bins"):
            check_range(K, D)
    with pytest.raises(ValueError, match="transpose_augment"):
        _brain(transpose_augment="9")._transpose_augment()          # refused from the values alone: no module, no device is touched


def test_off_builds_nothing_and_hands_on_the_same_tensors():
    brain = _brain()
    assert brain._transpose_augment() is None and brain._augment is None
    batch = _batch()
    out = brain._train_features(batch)
    assert all(o is b for o, b in zip(out, batch)), "the tensors that reach the step are the ones that reach it without the feature"


class _Stub:
    """Stands in for augment.TransposeAugment: marks what it was given, as the kernels would (features replaced, targets rewritten in place)."""

    def __init__(self):
        self.calls, self.epochs = 0, []

    def __call__(self, batch):
        self.calls += 1
        batch = list(batch)
        batch[0] = batch[0] + 1
        for i in (2, 3, 5):
            batch[i] += 100
        return batch

    def reseed(self, epoch):
        self.epochs.append(epoch)


def test_both_training_paths_get_the_augmented_batch(monkeypatch):
    seen = {}

    class Fused:
        def __call__(self, batch, tf):
            seen["fused"] = batch

        def report(self):
            return [0.1, 0.2, 0.3, 0.4, 1.0]

    monkeypatch.setattr(recipe.sb.Brain, "fit_batch", lambda self, batch: seen.__setitem__("generic", batch) or torch.tensor(0.0))
    for path in ("fused", "generic"):
        brain = _brain()
        brain._augment = _Stub()
        brain._fused = Fused() if path == "fused" else False
        brain.time_losses, brain.key_losses, brain.upper_losses, brain.lower_losses = [], [], [], []
        batch = _batch()
        keep = [t.clone() if torch.is_tensor(t) else t for t in batch]
        brain.fit_batch(batch)
        got = seen[path]
        assert brain._augment.calls == 1
        assert torch.equal(got[0], keep[0] + 1) and all(torch.equal(got[i], keep[i] + 100) for i in (2, 3, 5))
        assert all(torch.equal(batch[i], keep[i]) for i in (0, 2, 3, 5)), "targets that were on the device already are the caller's: copied, not rewritten"
        # what the generic path's compute_forward / compute_objectives do with it: a device batch passes through as it is
        again = recipe._features(got, "cpu")
        assert all(a is g for a, g in zip(again, got))
