#!/usr/bin/env python3
"""Fine-tuning entry point (real-audio clips, ASAP layout): ``python finetune.py hparams/finetune.yaml --workspace=... ...``.

As the reference's finetune.py (:230-294): starts from the pre-training checkpoints by copying ``<pretrain>/save`` into the new
output folder and resetting their recorded WER so that the first fine-tuned epoch is kept; fixed teacher-forcing ratio; the test
split doubles as validation split.  ``--constrained_decoding=true``, ``--metrical_decoding=true``, ``--beam_size=K [--beam_length_penalty=A]``, ``--note_metrics=true``, ``--synthetic_scores=rendered`` and
``--transpose_augment=K [--detune_bins=D]`` as in pretrain.py;
``--tempo_augment=R`` likewise: the one variation a fine-tuning corpus of recordings otherwise lacks, each clip being heard at exactly one tempo;
``--eq_augment_db=E --noise_augment_db="(lo, hi)" --mask_time=Wt --mask_freq=Wf [--mask_count=m]`` likewise: microphone and instrument response, noise floor and missing stretches
of time or frequency, applied to the precomputed feature files' rows on the GPU (TRAIN batches only).
Optional override of the rendered corpus: ``--synthetic_room=none|train|eval|all [--room_rt60="(lo, hi)" --room_drr_db="(lo, hi)" --room_predelay_ms="(lo, hi)"]``
(with ``--synthetic_scores=rendered`` only: every clip is heard in a synthetic room of its own -- direct path, pre-delay, decaying diffuse tail, drawn from the
clip's seed and applied to the waveform on the GPU -- in the TRAIN stage, in VALID and TEST, or in all three; the default is none).
``--tuning_correction=true`` as in pretrain.py: recordings of pianos that do not sit at A4 = 440 Hz are shifted back onto the grid, clip by clip, in all three stages."""
import os
import shutil
import sys

from piano_a2s_amd.recipe import ASR, sb, synthetic_sets, write_run_summary
from utilities import load, save

try:
    from hyperpyyaml import load_hyperpyyaml
except Exception:  # noqa: BLE001
    from piano_a2s_amd.hyperyaml import load_hyperpyyaml


class FinetuneASR(ASR):
    finetune = True


def seed_from_pretraining(pretrained_output_folder, output_folder):
    src, dst = os.path.join(pretrained_output_folder, "save"), os.path.join(output_folder, "save")
    if os.path.isdir(src):
        shutil.copytree(src, dst, dirs_exist_ok=True)
    if os.path.isdir(dst):
        for folder in os.listdir(dst):
            meta_file = os.path.join(dst, folder, "CKPT.yaml")
            if os.path.exists(meta_file):
                meta = load(meta_file)
                meta["WER"] = 100                     # any fine-tuned epoch beats it
                save(meta, meta_file)


def main(argv):
    hparams_file, run_opts, overrides = sb.parse_arguments(argv)
    sb.utils.distributed.ddp_init_group(run_opts)
    with open(hparams_file) as fin:
        hparams = load_hyperpyyaml(fin, overrides)
    sb.create_experiment_directory(experiment_directory=hparams["output_folder"], hyperparams_to_save=hparams_file, overrides=overrides)
    # rank 0 copies, every rank waits: the others must not look for checkpoints in a half-copied save/ (the reference runs the cp
    # synchronously on every rank, finetune.py:251-258); Brain.on_fit_start then broadcasts rank 0's recovered parameters
    sb.utils.distributed.run_on_main(seed_from_pretraining, args=[hparams["pretrained_output_folder"], hparams["output_folder"]])

    n_syn = int(hparams.get("synthetic_clips", 0) or 0)
    if n_syn:
        train_set, valid_set, test_set = synthetic_sets(hparams, n_syn, test_offset=None, online_vqt=False)
    else:
        from datasets.asap import ASAPDataset
        train_set = ASAPDataset(hparams, "train", run_opts["device"])
        valid_set = test_set = ASAPDataset(hparams, "test", run_opts["device"])

    brain = FinetuneASR(modules=hparams["modules"], opt_class=hparams["opt_class"], hparams=hparams, run_opts=run_opts,
                        checkpointer=hparams["checkpointer"])
    brain.fit(brain.hparams.epoch_counter, train_set, valid_set,
              train_loader_kwargs=hparams["train_dataloader_opts"], valid_loader_kwargs=hparams["valid_dataloader_opts"])
    brain.evaluate(test_set, test_loader_kwargs=hparams["test_dataloader_opts"], min_key="WER")
    write_run_summary(brain, hparams)
    return brain


if __name__ == "__main__":
    main(sys.argv[1:])
