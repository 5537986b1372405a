"""Inputs shared by the note-level metric's tests (tests/test_note_metrics_cpu.py, tests/test_gpu_note_metrics.py): the hand-written bars and a recipe stage driven without a model."""
import os
import types

from data_processing.humdrum import LabelsMultiple

LABELS = LabelsMultiple(extended=True)
IDS = LABELS.labels_map
V = len(LABELS.labels)
EOS, PAD, SOS = IDS["<eos>"], IDS["<pad>"], IDS["<sos>"]
enc = LABELS.encode

# (target, prediction) as kern text: every hand bar of the definition
HAND_PAIRS = [
    ("4c 4e\n4d\n2r", "4c 4e\n8d\n8r\n2r"),
    ("4c\t8e\n.\t8f\n4d\t4g", "4c\t8e\n.\t8f\n4d\t4g"),
    ("4c 4e 4g\n2.r", "4g 4c 4e\n2.r"),                              # a chord in another order
    ("4c\t8e\n.\t8f\n4d\t4g", "8e\t4c\n8f\t.\n4g\t4d"),               # the two spines swapped
    ("[4c\n4c]", "4c\n4c"),                                           # a tie: the continuation is no note
    ("[4c\n4c_\n4c;]", "[4c\n4c_\n4c;]"),
    ("4c#", "4d-"),                                                    # same key of the piano, another spelling
    ("2c\n2d", "4c\n4d\n2r"),                                          # a shortened first note moves the second one's onset
    ("", ""),
    ("4c", ""),
    ("", "4c"),
]

def hand_rows():
    """[(target ids, prediction ids)] of HAND_PAIRS; an empty text is an empty row."""
    return [(enc(r) if r else [], enc(h) if h else []) for r, h in HAND_PAIRS]


class _Logger:
    def __init__(self):
        self.valid_stats = None

    def log_stats(self, stats_meta, train_stats=None, valid_stats=None):
        self.valid_stats = dict(valid_stats)


def run_valid_stage(output_folder, corpus, **hparams):
    """One VALID stage's on_stage_end of the recipe over recorded rows (corpus: synthetic.make_note_corpus), without a model: -> (stats, {clip id: record})."""
    import torch
    from piano_a2s_amd import recipe
    from piano_a2s_amd.recipe import load
    brain = recipe.ASR.__new__(recipe.ASR)
    brain.device = "cpu"
    logger = _Logger()
    brain.hparams = types.SimpleNamespace(output_folder=str(output_folder), feature_folder="/none", lr_annealing=lambda wer: (1.0, 1.0), train_logger=logger,
                                          **hparams)
    brain.optimizer = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    brain.checkpointer = types.SimpleNamespace(save_and_keep_only=lambda **kw: None)
    brain._fused = False
    brain.on_stage_start(recipe.sb.Stage.VALID, 1)
    brain.upper_target, brain.upper_pred = corpus["upper"]
    brain.lower_target, brain.lower_pred = corpus["lower"]
    for cid, rows in brain.upper_pred.items():
        brain.key_pred[cid] = brain.key_target[cid] = [6] * len(rows)
        brain.time_sig_pred[cid] = brain.time_sig_target[cid] = [0] * len(rows)
    for store in (brain.time_losses, brain.key_losses, brain.upper_losses, brain.lower_losses):
        store.append(0.5)
    brain.on_stage_end(recipe.sb.Stage.VALID, 2.0, 1)
    records = {cid: load(os.path.join(str(output_folder), "results", "valid", f"{cid}.json")) for cid in brain.upper_pred}
    return logger.valid_stats, records
