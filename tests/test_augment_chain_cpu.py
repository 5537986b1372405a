"""The augmentation chain without a GPU (piano_a2s_amd/augment.py, piano_a2s_amd/recipe.py; DESIGN.md sections 16, 18, 20):
(a) the host draws of the three augmenters are the ones recorded before they got a common base class;
(b) recipe.AUGMENTERS is the only wiring: reseeding, the train stats and run_summary.json follow from the table, for all three and for each alone."""
import hashlib
import json
import types

import numpy as np
import pytest

from piano_a2s_amd import recipe
from piano_a2s_amd.augment import SpecAugment, TempoAugment, TransposeAugment

CFG = {"freq_bins": 480}


def _digest(arrays):
    sha = hashlib.sha256()
    for a in arrays if isinstance(arrays, tuple) else (arrays,):
        a = np.ascontiguousarray(a)
        sha.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return sha.hexdigest()[:16]


# ------------------------------------------------------------------------------------------- (a) the draws
def test_draws_after_a_reseed_are_the_recorded_ones():
    """seed 1234, rank 1, reseed(3), then two consecutive draws of 5 clips."""
    aug = TransposeAugment(CFG, 3, 1.5, seed=1234, device="cpu", rank=1)
    aug.reseed(3)
    first = aug.draw(5)
    assert first[0].tolist() == [3, -2, 0, -1, -1]
    assert (_digest(first), _digest(aug.draw(5))) == ("777e8e38d87e38db", "f1ad058188c5da73")
    aug = TempoAugment(CFG, 0.15, seed=1234, device="cpu", rank=1)
    aug.reseed(3)
    assert (_digest(aug.draw(5)), _digest(aug.draw(5))) == ("c3383f108a36348c", "a43831a85f5fef26")
    # draw_raw, not draw: the table goes through float64 cos / pow, which need not be bit-stable across machines
    aug = SpecAugment(CFG, 6, "(30, 50)", 20, 10, 2, seed=1234, device="cpu", rank=1)
    aug.reseed(3)
    first = aug.draw_raw(5)
    assert first[4][0, :3].tolist() == [1315846728, 3649631396, 3020310524]
    assert (_digest(first), _digest(aug.draw_raw(5))) == ("f626c28c3ae230bd", "3fa354cb30cb2e42")


def test_draws_of_a_fresh_augmenter_are_the_recorded_ones():
    """rank and epoch defaulted: a constructor seeds as reseed(0, 0) does."""
    assert _digest(TransposeAugment(CFG, 3, 1.5, 7, "cpu").draw(4)) == "a1a3d28d8114096d"
    assert _digest(TempoAugment(CFG, 0.25, 7, "cpu").draw(4)) == "2ad935703bf0d499"
    assert _digest(SpecAugment(CFG, mask_time=10, seed=7).draw_raw(4)) == "fdd397836d12dc9d"


# ------------------------------------------------------------------------------------------- (b) the table
FLAGS = {"_augment": dict(transpose_augment=3, detune_bins=1.5), "_tempo": dict(tempo_augment=0.15),
         "_specaug": dict(eq_augment_db=6, noise_augment_db="(30, 50)", mask_time=20, mask_freq=10, mask_count=2)}
STATS = {"_augment": ("augmented_clips", "transposed_clips", "not_representable_clips"), "_tempo": ("tempo_clips", "tempo_stretched_clips", "tempo_kept_clips"),
         "_specaug": ("specaug_clips", "specaug_time_masked_clips", "specaug_freq_masked_clips")}
BLOCKS = {"_augment": ("transpose_augment", dict(max_semitones=3, detune_bins=1.5, clips=0, transposed=0, not_representable=0)),
          "_tempo": ("tempo_augment", dict(max_change=0.15, clips=0, stretched=0, kept=0)),
          "_specaug": ("spec_augment", dict(eq_db=6.0, noise_db=[30.0, 50.0], mask_time=20, mask_freq=10, mask_count=2, clips=0, time_masked=0, freq_masked=0))}


def _brain(**hparams):
    class Model:
        cfg = CFG

    brain = recipe.ASR.__new__(recipe.ASR)
    brain.device = "cpu"
    brain.hparams = types.SimpleNamespace(seed=1234, teacher_forcing_ratio=0.5, teacher_forcing_decay=0.9, **hparams)
    brain.modules = types.SimpleNamespace(transcription=Model())
    return brain


def _train_stage(brain, epoch):
    brain.on_stage_start(recipe.sb.Stage.TRAIN, epoch)
    for losses in (brain.time_losses, brain.key_losses, brain.upper_losses, brain.lower_losses):
        losses.append(0.25)
    brain.on_stage_end(recipe.sb.Stage.TRAIN, 1.0, epoch)


def _summary(brain, tmp_path):
    recipe.write_run_summary(brain, {"output_folder": str(tmp_path)})
    return json.loads((tmp_path / "run_summary.json").read_text())


class _Stage:
    """Stands in for the augmenter kept in `cache`: counts base, base + 1, base + 2 under its class's count names."""

    def __init__(self, cls, base, log):
        self.cls, self.base, self.log = cls, base, log

    def reseed(self, epoch):
        self.log.append((self.cls.cache, epoch))

    def counts(self):
        return {name: self.base + i for i, name in enumerate(self.cls.count_names)}

    def settings(self):
        return {"setting": self.base}


def test_the_table_names_the_three_in_the_order_they_are_applied():
    assert recipe.AUGMENTERS == (TransposeAugment, TempoAugment, SpecAugment)
    assert [cls.cache for cls in recipe.AUGMENTERS] == ["_augment", "_tempo", "_specaug"]
    assert [cls.rewrites_targets for cls in recipe.AUGMENTERS] == [True, False, False]


def test_all_three_on_stub_stages(tmp_path):
    log = []
    brain = _brain(**{k: v for flags in FLAGS.values() for k, v in flags.items()})
    for i, cls in enumerate(recipe.AUGMENTERS):
        setattr(brain, cls.cache, _Stage(cls, 100 * (i + 1), log))
    _train_stage(brain, 5)
    assert log == [("_augment", 5), ("_tempo", 5), ("_specaug", 5)]
    want = {stat: 100 * (i + 1) + j for i, cache in enumerate(("_augment", "_tempo", "_specaug")) for j, stat in enumerate(STATS[cache])}
    assert len(want) == 9 and {k: v for k, v in brain.train_stats.items() if k.endswith("_clips")} == want
    summary = _summary(brain, tmp_path)
    assert summary["transpose_augment"] == dict(setting=100, clips=100, transposed=101, not_representable=102)
    assert summary["tempo_augment"] == dict(setting=200, clips=200, stretched=201, kept=202)
    assert summary["spec_augment"] == dict(setting=300, clips=300, time_masked=301, freq_masked=302)


def test_all_three_built_from_the_flags(tmp_path):
    brain = _brain(**{k: v for flags in FLAGS.values() for k, v in flags.items()})
    _train_stage(brain, 5)
    built = [getattr(brain, cls.cache) for cls in recipe.AUGMENTERS]
    assert [type(a) for a in built] == list(recipe.AUGMENTERS) and all(a.seed == 1234 and a.rank == 0 and a.freq_bins == 480 for a in built)
    assert built == [brain._transpose_augment(), brain._tempo_augment(), brain._spec_augment()]
    for aug in built:                                     # on_stage_start reseeded each with the epoch: the draws are those of a fresh one after reseed(5)
        fresh = type(aug)(CFG, seed=1234, device="cpu", **type(aug).read(brain.hparams))
        fresh.reseed(5)
        draw = "draw_raw" if isinstance(aug, SpecAugment) else "draw"
        assert _digest(getattr(aug, draw)(3)) == _digest(getattr(fresh, draw)(3))
    assert {k: v for k, v in brain.train_stats.items() if k.endswith("_clips")} == {stat: 0 for stats in STATS.values() for stat in stats}
    summary = _summary(brain, tmp_path)
    for name, block in BLOCKS.values():
        assert summary[name] == block


@pytest.mark.parametrize("cache", ["_augment", "_tempo", "_specaug"])
def test_one_flag_wires_that_one_alone(tmp_path, cache):
    brain = _brain(**FLAGS[cache])
    _train_stage(brain, 2)
    for other in FLAGS:
        assert (getattr(brain, other) is not None) == (other == cache)
    assert {k for k in brain.train_stats if k.endswith("_clips")} == set(STATS[cache])
    summary = _summary(brain, tmp_path)
    assert {name for name, _ in BLOCKS.values() if name in summary} == {BLOCKS[cache][0]}
    assert summary[BLOCKS[cache][0]] == BLOCKS[cache][1]
