"""The augmentation chain on the MI355X (piano_a2s_amd/recipe.py over piano_a2s_amd/augment.py; DESIGN.md sections 16, 18, 20): what ASR._train_features
hands to the training step with all three augmenters on is, bit for bit, what the six wrappers give when they are called directly, in the order of
recipe.AUGMENTERS, with the draws of three augmenters of the same seed.  Both sides run the same kernels on the same inputs: there is no tolerance."""
import types

import numpy as np
import pytest
import torch

from data_processing.humdrum import LabelsMultiple
from piano_a2s_amd import kern_transpose as kt
from piano_a2s_amd import recipe
from piano_a2s_amd.augment import SpecAugment, TempoAugment, TransposeAugment

pytestmark = pytest.mark.gpu
LABELS = LabelsMultiple(extended=True)
PAD, EOS = LABELS.labels_map["<pad>"], LABELS.labels_map["<eos>"]
SEED, B, ROWS, CONTENT = 1234, 3, 37, 20          # 37 rows: three row tiles of 16, the last partial; clip 1 is zero behind row 20
K, D, R, E, NOISE, WT, WF, M = 2, 1.0, 0.2, 6.0, (30.0, 50.0), 7, 10, 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _row(text, length):
    ids = LABELS.encode(text)
    assert len(ids) < length
    return ids + [EOS] + [PAD] * (length - len(ids) - 1)


def _batch(F, dev):
    """Three clips of scores that can be respelled (C major, one bar in G major), features (B, 1, ROWS, F)."""
    x = torch.rand(B, 1, ROWS, F, generator=torch.Generator().manual_seed(F))
    x[1, :, CONTENT:] = 0
    key = torch.tensor([[6, 6, 6], [6, 6, 7], [6, 6, 6]], dtype=torch.long)
    upper = torch.tensor([[_row(t, 9) for t in bars] for bars in (["4c 4e", "8d\n8g", "2b-"], ["4c 4e", "8d\n8g", "4f# 4a"], ["4c 4e", "8d\n8g", "4f 4a"])])
    lower = torch.tensor([[_row(t, 6) for t in bars] for bars in (["2C", "4r", "1GG"], ["2C", "4E", "2D"], ["2C", "4E", "2G"])])
    lens = torch.ones(B, 3)
    return [t.to(dev) for t in (x, torch.zeros(B, 3, dtype=torch.long), key, upper, lens, lower, lens)] + [["a", "b", "c"], torch.zeros(B)]


def _brain(F, dev):
    class Model:
        cfg = {"freq_bins": F}

    brain = recipe.ASR.__new__(recipe.ASR)
    brain.device = dev
    brain.hparams = types.SimpleNamespace(seed=SEED, transpose_augment=K, detune_bins=D, tempo_augment=R, eq_augment_db=E, noise_augment_db=str(NOISE),
                                          mask_time=WT, mask_freq=WF, mask_count=M)
    brain.modules = types.SimpleNamespace(transcription=Model())
    return brain


def _by_hand(F, batch, dev):
    """The six wrappers in the chain's order on copies of the batch -> (features, key, upper, lower, the three counter tensors)."""
    from piano_a2s_amd import hip
    cfg = {"freq_bins": F}
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    counters = [torch.zeros(3, dtype=torch.int32, device=dev) for _ in range(3)]
    x, key, upper, lower = batch[0].clone(), batch[2].clone(), batch[3].clone(), batch[5].clone()
    s, d = TransposeAugment(cfg, K, D, SEED, dev).draw(B)
    eff = torch.empty(B, device=dev)
    hip.transpose_targets(*(torch.from_numpy(np.array(t)).to(dev) for t in kt.tables()), torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev), key, upper, lower,
                          5, eff, counters[0])          # (60 bins per octave: 5 per semitone)
    x = hip.shift_bins(x, eff)
    u = TempoAugment(cfg, R, SEED, dev).draw(B)
    content, step = i32(B), i32(B)
    hip.tempo_plan(x, torch.from_numpy(u).to(dev), R, min(400, ROWS // 3), content, step, counters[1])
    x = hip.stretch_frames(x, step)
    table, words = SpecAugment(cfg, E, NOISE, WT, WF, M, seed=SEED, device=dev).draw(B)
    table = torch.from_numpy(table).to(dev)
    content, plan, stats = i32(B), i32(B, 16), torch.empty((B, 2), device=dev)
    hip.specaug_plan(x, table, torch.from_numpy(words.view(np.int32)).to(dev), WT, WF, M, content, plan, stats, counters[2])
    x = hip.specaug_apply(x, table, content, plan, stats)
    return x, key, upper, lower, counters


@pytest.mark.parametrize("F", [60, 65], ids=["four_wide", "scalar"])          # F % 4 == 0: four floats per thread; 65 = 13 semitones of 5 bins: one
def test_train_features_are_the_six_wrappers_in_order(dev, F):
    from piano_a2s_amd import hip
    batch = _batch(F, dev)
    keep = [t.clone() if torch.is_tensor(t) else t for t in batch]
    want_x, want_key, want_upper, want_lower, counters = _by_hand(F, batch, dev)
    brain = _brain(F, dev)
    launches = lambda: (hip.augment_launches(), hip.tempo_launches(), hip.specaug_launches())
    before = launches()
    out = brain._train_features(batch)
    torch.cuda.synchronize()
    assert launches() == tuple(n + 2 for n in before), "two launches per augmenter, each on its own counter"
    assert out[0].shape == (B, 1, ROWS, F) and torch.equal(out[0], want_x), "bit for bit"
    assert torch.equal(out[2], want_key) and torch.equal(out[3], want_upper) and torch.equal(out[5], want_lower)
    assert not torch.equal(out[3], keep[3]), "some clip was transposed: the comparison is not of untouched targets"
    assert all(torch.equal(batch[i], keep[i]) for i in (0, 1, 2, 3, 4, 5, 6)), "the caller's tensors are as they were"
    assert all(out[i] is batch[i] for i in (1, 4, 6)) and all(out[i] is not batch[i] for i in (0, 2, 3, 5))
    assert brain._tempo.last_plan[0].tolist() == [ROWS, CONTENT, ROWS], "the content scan saw the padding (a shift along the bins leaves a zero row zero)"
    for cls, c in zip(recipe.AUGMENTERS, counters):
        assert list(getattr(brain, cls.cache).counts().values()) == c.tolist() and c[0].item() == B
