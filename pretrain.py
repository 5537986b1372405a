#!/usr/bin/env python3
"""Pre-training entry point: ``python pretrain.py hparams/pretrain.yaml --workspace=... --soundfont_folder=...`` or
``torchrun --nproc_per_node=N pretrain.py hparams/pretrain.yaml ...`` (one process per GPU, RCCL).

Same command line, yaml keys and recipe hooks as the reference's pretrain.py (:251-305); the recipe class lives in
piano_a2s_amd/recipe.py.  ``--synthetic_clips=N`` trains on N seeded synthetic clips instead of a rendered corpus; with
``--synthetic_scores=rendered`` their audio is the sound of their (well-formed) score, synthesised on the GPU.  Optional overrides of the
VALID / TEST decoder: ``--constrained_decoding=true`` (kern grammar), ``--metrical_decoding=true`` (the grammar and the metre of each bar's predicted time signature; the stats gain ``complete_bars``), ``--beam_size=K [--beam_length_penalty=A]`` (beam search, K in 1 .. 4); of their scoring: ``--note_metrics=true`` (note-level F1 beside the WER).  Optional override of the TRAIN stage:
``--transpose_augment=K [--detune_bins=D]`` (every clip transposed by -K .. K semitones, K in 0 .. 6, and detuned by up to D feature bins, D <= 2.5, on the GPU),
``--tempo_augment=R`` (every clip played 1 - R .. 1 + R times as slowly, R <= 0.25, its content kept inside the window; the features are time-stretched on the GPU, the score stays),
``--eq_augment_db=E --noise_augment_db="(lo, hi)" --mask_time=Wt --mask_freq=Wf [--mask_count=m]`` (the colour of the recording, each part on its own: an equaliser curve of at most
E <= 12 dB per clip that leaves the front end's floor where it is, a noise floor lo .. hi dB below the clip's peak with 20 <= lo <= hi <= 80, and m in 1 .. 4 SpecAugment masks of up to
Wt <= 100 frames and Wf <= 60 bins; the features are re-normalised to their new peak on the GPU, after transposition and tempo; the score stays).
Optional override of the rendered corpus: ``--synthetic_room=none|train|eval|all [--room_rt60="(lo, hi)" --room_drr_db="(lo, hi)" --room_predelay_ms="(lo, hi)"]``
(with ``--synthetic_scores=rendered`` only: every clip is heard in a synthetic room of its own -- direct path, pre-delay, decaying diffuse tail, drawn from the
clip's seed and applied to the waveform on the GPU -- in the TRAIN stage, in VALID and TEST, or in all three; the default is none).
Optional override of all three stages: ``--tuning_correction=true`` (every clip's tuning against A4 = 440 Hz is estimated on the GPU and its features are shifted
back onto the grid, in TRAIN in front of the augmenters; the stage stats gain ``tuning_abs_cents`` and ``tuning_determined``)."""
import sys

from piano_a2s_amd.recipe import ASR, sb, synthetic_sets, write_run_summary

try:
    from hyperpyyaml import load_hyperpyyaml
except Exception:  # noqa: BLE001
    from piano_a2s_amd.hyperyaml import load_hyperpyyaml


def main(argv):
    hparams_file, run_opts, overrides = sb.parse_arguments(argv)
    sb.utils.distributed.ddp_init_group(run_opts)
    with open(hparams_file) as fin:
        hparams = load_hyperpyyaml(fin, overrides)
    sb.create_experiment_directory(experiment_directory=hparams["output_folder"], hyperparams_to_save=hparams_file, overrides=overrides)

    n_syn = int(hparams.get("synthetic_clips", 0) or 0)
    if n_syn:
        train_set, valid_set, test_set = synthetic_sets(hparams, n_syn)
    else:
        from datasets.syn import TestDataset, TrainDataset
        test_versions = range(4) if hparams["midi_syn"] == "epr" else [0]      # score + 3 composers' renderings for "epr"
        train_set = TrainDataset(hparams, "train", run_opts["device"], range(10))
        valid_set = TestDataset(hparams, "valid", run_opts["device"], test_versions)
        test_set = TestDataset(hparams, "test", run_opts["device"], test_versions)

    brain = ASR(modules=hparams["modules"], opt_class=hparams["opt_class"], hparams=hparams, run_opts=run_opts,
                checkpointer=hparams["checkpointer"])
    brain.fit(brain.hparams.epoch_counter, train_set, valid_set,
              train_loader_kwargs=hparams["train_dataloader_opts"], valid_loader_kwargs=hparams["valid_dataloader_opts"])
    brain.evaluate(test_set, test_loader_kwargs=hparams["test_dataloader_opts"], min_key="WER")
    write_run_summary(brain, hparams)
    return brain


if __name__ == "__main__":
    main(sys.argv[1:])
