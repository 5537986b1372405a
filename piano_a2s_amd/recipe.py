"""The training recipe: a Brain subclass with the reference's hooks (reference pretrain.py:31-214 / finetune.py:30-193).

Shared by pretrain.py and finetune.py (they differ in the teacher-forcing schedule, the clip id and the result record).
`fit_batch` keeps the reference's semantics (forward, 4-term NLL, backward, check_gradients, optimizer step, zero_grad) but, when the
transcription module is the HIP model, runs them as the fused step of piano_a2s_amd.train (loss terms stay on the device)."""
import os

import numpy as np
import torch

try:                                    # the real thing when present, the compat slice otherwise
    import speechbrain as sb
except Exception:                       # noqa: BLE001
    from piano_a2s_amd import sb_compat as sb

from data_processing.humdrum import LabelsMultiple
from piano_a2s_amd import augment, metrics
from utilities import load, mkdirs, save

labels = LabelsMultiple(extended=True)

# the augmenters of a TRAIN batch in the order they are applied (DESIGN.md sections 16, 18, 20).  This table is all the wiring there is: every class states
# its switches, the attribute that keeps it, its stat keys and its run_summary.json block itself (piano_a2s_amd/augment.py)
AUGMENTERS = _TRANSPOSE, _TEMPO, _SPECAUG = (augment.TransposeAugment, augment.TempoAugment, augment.SpecAugment)


def _to_device(batch, device):
    return [t.to(device, non_blocking=True) if torch.is_tensor(t) else t for t in batch]


_VQT = {}


def _features(batch, device, room=None):
    """Online front-end: when the loader yields raw 16 kHz waveforms (B, N) instead of cached spectrograms
    (B, 1, T, F), the VQT runs on the GPU in front of the model (piano_a2s_amd.vqt; the reference caches librosa features offline).  When it yields
    render programs (B, 1 + E, 8) int32, the waveforms are synthesised on the GPU first (piano_a2s_amd.render) and, with a `room`
    (piano_a2s_amd.room.Room, --synthetic_room), convolved with every clip's own impulse response before the VQT."""
    rendered = torch.is_tensor(batch[0]) and batch[0].dim() == 3 and batch[0].dtype == torch.int32
    if rendered:
        # rendered synthetic corpus (datasets.syn.RenderedClips): render programs (B, 1 + E, 8) -> waveforms, synthesised on the GPU; the clip length
        # and the room seeds are taken from the headers while the programs are still on the host (nothing is read back from the device)
        from piano_a2s_amd.render import program_samples, render
        n_samples = program_samples(batch[0])
        if room is not None:
            from piano_a2s_amd.room import room_seeds
            seeds = room_seeds(batch[0])
    batch = _to_device(batch, device)
    if rendered:
        batch[0] = render(batch[0], n_samples)
        if room is not None:
            batch[0] = room.apply(batch[0], seeds)
    if torch.is_tensor(batch[0]) and batch[0].dim() == 2:
        from piano_a2s_amd.vqt import VQT
        if device not in _VQT:
            _VQT[device] = VQT(torch.device(device))
        batch[0] = _VQT[device](batch[0])
    return batch


def _hp(hparams, key, default=None):
    return hparams.get(key, default) if isinstance(hparams, dict) else getattr(hparams, key, default)


def synthetic_room(hparams):
    """--synthetic_room=none|train|eval|all [--room_rt60="(lo, hi)" --room_drr_db="(lo, hi)" --room_predelay_ms="(lo, hi)"] (optional overrides, like
    --synthetic_scores): the clips of the rendered corpus are heard in a synthetic room of their own in the TRAIN stage, in VALID and TEST, or in all
    three (piano_a2s_amd.room).  -> (mode, Room), or None for none (the default: nothing is built, nothing is launched).  A value
    out of range, or a room without --synthetic_scores=rendered, raises ValueError."""
    from piano_a2s_amd import room
    mode = room.check_stages(_hp(hparams, "synthetic_room"))
    if mode == "none":
        return None
    if str(_hp(hparams, "synthetic_scores") or "random").strip().lower() != "rendered" or not int(_hp(hparams, "synthetic_clips", 0) or 0):
        raise ValueError(f"--synthetic_room={mode} needs the rendered corpus (--synthetic_clips=N --synthetic_scores=rendered): only its clips have a waveform "
                         "that is made on the device")
    ranges = {k: _hp(hparams, "room_" + k) for k in ("rt60", "drr_db", "predelay_ms")}
    return mode, room.Room(sample_rate=int(_hp(hparams, "sample_rate", 16000)), **{k: v for k, v in ranges.items() if v is not None})


def synthetic_sets(hparams, n_syn, test_offset=20_000, online_vqt=True):
    """--synthetic_clips=N: the (train, valid, test) sets of N / N // 8 / N // 8 seeded clips at disjoint seed offsets.  --synthetic_scores=rendered
    (an optional override, like --synthetic_frames): clips whose audio is the GPU-synthesised sound of their score (datasets.syn.RenderedClips);
    without it the random clips (--online_vqt, where the caller honours it: with random waveforms) as before.  Rendered clips take neither
    --synthetic_lengths (their bars are as long as the drawn score; --max_length caps them) nor --online_vqt (they always go through the GPU VQT): both
    are ignored with them.  test_offset None: the test set is the
    validation set (finetune.py)."""
    from datasets.syn import RenderedClips, SyntheticClips, SyntheticWaveClips
    cfg = hparams["transcription"].cfg
    syn = dict(frames=int(hparams.get("synthetic_frames") or hparams["max_frame_num"]))
    scores = str(hparams.get("synthetic_scores") or "random").strip().lower()
    if scores == "rendered":
        cls = RenderedClips
    elif scores == "random":
        cls = SyntheticWaveClips if online_vqt and hparams.get("online_vqt") else SyntheticClips
        if hparams.get("synthetic_lengths"):
            syn.update(upper_range=tuple(hparams["synthetic_lengths"][0]), lower_range=tuple(hparams["synthetic_lengths"][1]))
    else:
        raise ValueError(f"--synthetic_scores must be 'random' or 'rendered' (got {scores!r})")
    synthetic_room(hparams)                   # (a --synthetic_room that is out of range or lacks the rendered corpus is refused before any set is made)
    train_set = cls(cfg, n_syn, seed=hparams["seed"], **syn)
    valid_set = cls(cfg, max(1, n_syn // 8), seed=hparams["seed"] + 10_000, **syn)
    test_set = valid_set if test_offset is None else cls(cfg, max(1, n_syn // 8), seed=hparams["seed"] + test_offset, **syn)
    return train_set, valid_set, test_set


class ASR(sb.Brain):
    finetune = False

    # ------------------------------------------------------------------ forward / objective
    def compute_forward(self, batch, stage):
        batch = _features(batch, self.device, room=self._room(stage))
        if stage != sb.Stage.TRAIN:
            batch = self._correct_tuning(batch)       # (a TRAIN batch was corrected in _train_features, in front of the augmenters)
        spectrogram, ts_t, key_t, up_t, up_len, lo_t, lo_len = batch[:7]
        if stage == sb.Stage.TRAIN:
            return self.modules.transcription(spectrogram=spectrogram, inference=False,
                                              ground_truth=[ts_t, key_t, up_t, up_len, lo_t, lo_len],
                                              teacher_forcing_ratio=self.teacher_forcing_ratio, device=self.device)
        self._set_constrained_decoding()
        return self.modules.transcription(spectrogram=spectrogram, inference=True, ground_truth=None,
                                          teacher_forcing_ratio=0., device=self.device)

    def _constrained(self):
        """--constrained_decoding=true (an optional override, not a key of the yaml files): VALID / TEST decode under the kern token grammar."""
        v = getattr(self.hparams, "constrained_decoding", False)
        return v.strip().lower() in ("1", "true", "yes") if isinstance(v, str) else bool(v)

    def _metrical(self):
        """--metrical_decoding=true (an optional override as --constrained_decoding, which it implies): VALID / TEST decode under the kern token grammar
        AND the metre of the time signature predicted for each bar."""
        v = getattr(self.hparams, "metrical_decoding", False)
        return v.strip().lower() in ("1", "true", "yes") if isinstance(v, str) else bool(v)

    def _beam_size(self):
        """--beam_size=K (an optional override as --constrained_decoding): VALID / TEST decode by beam search with K hypotheses per clip; 1 = greedy."""
        return int(getattr(self.hparams, "beam_size", 1))

    def _set_beam(self):
        K = self._beam_size()
        if not 1 <= K <= 4:
            raise ValueError(f"--beam_size must be in 1 .. 4 (got {K})")
        if K == 1:
            return
        model = self.modules.transcription
        model = getattr(model, "module", model)                      # (a DistributedDataParallel wrapper)
        if not hasattr(model, "beam_size"):
            raise ValueError(f"--beam_size needs a transcription module that decodes by beam search; {type(model).__name__} has no `beam_size` attribute")
        model.beam_size, model.beam_length_penalty = K, float(getattr(self.hparams, "beam_length_penalty", 0.0))

    def _alignment(self):
        """--alignment=true (an optional override as --constrained_decoding): VALID / TEST also record where in the audio every decoded bar and token lies."""
        v = getattr(self.hparams, "alignment", False)
        return v.strip().lower() in ("1", "true", "yes") if isinstance(v, str) else bool(v)

    def _note_metrics(self):
        """--note_metrics=true (an optional override as --constrained_decoding): VALID / TEST also score the decoded bars note by note
        (metrics.corpus_note_f1).  Off by default: no key is added and nothing of it runs."""
        v = getattr(self.hparams, "note_metrics", False)
        return v.strip().lower() in ("1", "true", "yes") if isinstance(v, str) else bool(v)

    def _tuning_correction(self):
        """--tuning_correction=true (an optional override as --constrained_decoding): in all three stages every clip's tuning is estimated on the
        device and its features are shifted back onto the grid at A4 = 440 Hz (piano_a2s_amd.tuning), every clip a group of
        its own; in TRAIN in front of the augmenters.  Off by default: nothing is built, nothing is launched, no stat is added."""
        v = getattr(self.hparams, "tuning_correction", False)
        return v.strip().lower() in ("1", "true", "yes") if isinstance(v, str) else bool(v)

    def _correct_tuning(self, batch):
        """The batch of `_features` with its features corrected, or as it is when the switch is off.  [sum of |cents| over the determined clips, the
        determined clips, the clips] grow on the device; on_stage_end reads them once."""
        if not self._tuning_correction():
            return batch
        if not hasattr(self, "_tuner"):
            from piano_a2s_amd.tuning import Tuner
            self._tuner = Tuner(self.device, bins_per_octave=int(getattr(self.hparams, "bins_per_octave", 60)))
            self._tuning_sums = torch.zeros(3, dtype=torch.float64, device=self.device)
        batch = list(batch)
        batch[0], est, _ = self._tuner(batch[0])
        determined = ((est[:, 2] >= self._tuner.min_peaks) & (est[:, 1] >= self._tuner.min_conf)).to(torch.float64)
        self._tuning_sums += torch.stack([(est[:, 0].abs() * determined).sum(), determined.sum(), determined.new_tensor(float(est.shape[0]))])
        return batch

    def _tuning_stats(self):
        """{"tuning_abs_cents": the mean |cents| over the stage's determined clips (0 without one), "tuning_determined": their share of the clips},
        or {} when the switch is off: one small D2H per stage; the sums start again."""
        if not self._tuning_correction() or not hasattr(self, "_tuning_sums"):
            return {}
        total, determined, clips = self._tuning_sums.tolist()
        self._tuning_sums.zero_()
        return {"tuning_abs_cents": total / determined if determined else 0.0, "tuning_determined": determined / clips if clips else 0.0}

    def _set_alignment(self):
        if not self._alignment():
            return
        model = self.modules.transcription
        model = getattr(model, "module", model)                      # (a DistributedDataParallel wrapper)
        if not hasattr(model, "alignment"):
            raise ValueError(f"--alignment needs a transcription module that reports the attention alignment; {type(model).__name__} has no `alignment` attribute")
        model.alignment = True                                       # (takes effect in evaluation mode only: a training forward does not align)

    def _set_constrained_decoding(self):
        self._set_beam()
        self._set_alignment()
        if self._metrical():
            model = self.modules.transcription
            model = getattr(model, "module", model)                  # (a DistributedDataParallel wrapper)
            if not hasattr(model, "metrical_decoding"):
                raise ValueError(f"--metrical_decoding needs a transcription module that decodes under the metre; {type(model).__name__} has no "
                                 "`metrical_decoding` attribute")
            if self._beam_size() >= 2 or self._alignment():
                raise ValueError("--metrical_decoding decodes greedily: it does not combine with --beam_size >= 2 or --alignment")
            model.metrical_decoding = True
            return
        if not self._constrained():
            return
        model = self.modules.transcription
        model = getattr(model, "module", model)                      # (a DistributedDataParallel wrapper)
        if not hasattr(model, "constrained_decoding"):
            raise ValueError(f"--constrained_decoding needs a transcription module that decodes under the kern grammar; {type(model).__name__} has no "
                             "`constrained_decoding` attribute")
        model.constrained_decoding = True

    def _augmenter(self, cls):
        """The augmenter of class `cls` (one of AUGMENTERS) that the run's switches ask for, built on first use and kept in the attribute `cls.cache`, or
        None when its switches are off (the default: nothing is built, nothing is launched).  Values out of range raise ValueError, from the values
        alone: no module, no device is touched before."""
        if not hasattr(self, cls.cache):
            settings = cls.read(self.hparams)
            setattr(self, cls.cache, None)
            if settings is not None:
                model = self.modules.transcription
                model = getattr(model, "module", model)                  # (a DistributedDataParallel wrapper)
                if not isinstance(getattr(model, "cfg", None), dict) or "freq_bins" not in model.cfg:
                    raise ValueError(f"{cls.needs} a transcription module that states its `cfg['freq_bins']`; {type(model).__name__} does not")
                import torch.distributed as dist
                rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
                setattr(self, cls.cache, cls(model.cfg, **settings, seed=getattr(self.hparams, "seed", 0), device=self.device, rank=rank))
        return getattr(self, cls.cache)

    def _augmenters(self):
        """[(class, augmenter)] of the augmenters that are on, in the order of AUGMENTERS."""
        return [(cls, aug) for cls, aug in ((cls, self._augmenter(cls)) for cls in AUGMENTERS) if aug is not None]

    def _transpose_augment(self):
        """--transpose_augment=K [--detune_bins=D] (optional overrides as --constrained_decoding): every TRAIN batch is transposed on the device by a
        whole number of semitones in -K .. K per clip (features shifted, score respelled) and detuned by up to D feature bins."""
        return self._augmenter(_TRANSPOSE)

    def _tempo_augment(self):
        """--tempo_augment=R: every TRAIN batch is time-stretched on the device, each clip by a factor drawn in 1 - R .. 1 + R and narrowed so that its
        content stays inside the window (the targets stay)."""
        return self._augmenter(_TEMPO)

    def _spec_augment(self):
        """--eq_augment_db=E, --noise_augment_db="(lo, hi)", --mask_time=Wt, --mask_freq=Wf [--mask_count=m]: every TRAIN batch gets, per clip, an
        equaliser curve of at most E dB, a noise floor lo .. hi dB below its peak and m masks of up to Wt frames and Wf bins, and is re-normalised as
        the front end does (the targets stay)."""
        return self._augmenter(_SPECAUG)

    def _room(self, stage):
        """--synthetic_room (`synthetic_room` above): the Room the batches of `stage` go through, or None.  Built on first use and kept: its count of
        clips and its device buffers belong to the run."""
        if not hasattr(self, "_synthetic_room"):
            self._synthetic_room = synthetic_room(self.hparams)
        if self._synthetic_room is None:
            return None
        from piano_a2s_amd.room import STAGES
        mode, room = self._synthetic_room
        name = {sb.Stage.TRAIN: "train", sb.Stage.VALID: "valid", sb.Stage.TEST: "test"}[stage]
        return room if name in STAGES[mode] else None

    def _train_features(self, batch):
        """`_features` of a TRAIN batch, augmented when the run asks for it, in the order of AUGMENTERS: transposed first, then time-stretched, then
        coloured and masked.  Where an augmenter rewrites the targets in place, a tensor that was on the device before (and so is the caller's own) is
        copied first."""
        out = self._correct_tuning(_features(batch, self.device, room=self._room(sb.Stage.TRAIN)))      # (--detune_bins then acts on a normalised clip)
        for cls, aug in self._augmenters():
            if cls.rewrites_targets:
                for i in (2, 3, 5):
                    if out[i] is batch[i]:
                        out[i] = out[i].clone()
            out = aug(out)
        return out

    def compute_objectives(self, predictions, batch, stage):
        batch = _to_device(batch, self.device)
        _, ts_t, key_t, up_t, _, lo_t, _, names, versions = batch
        ts_o, key_o, up_o, lo_o = predictions
        hp = self.hparams
        time_loss = hp.loss_time_sig(ts_o.permute(0, 2, 1), ts_t)
        key_loss = hp.loss_key(key_o.permute(0, 2, 1), key_t)
        flat = lambda o, t: (o.reshape(o.shape[0] * o.shape[1], -1, o.shape[3]).permute(0, 2, 1), t.reshape(t.shape[0] * t.shape[1], -1))
        upper_loss = hp.loss_score(*flat(up_o, up_t))
        lower_loss = hp.loss_score(*flat(lo_o, lo_t))
        self._record_losses(time_loss, key_loss, upper_loss, lower_loss)
        if stage != sb.Stage.TRAIN:
            self._record_predictions(predictions, (ts_t, key_t, up_t, lo_t), names, versions)
        return time_loss + key_loss + upper_loss + lower_loss

    def _record_losses(self, *terms):
        for store, t in zip((self.time_losses, self.key_losses, self.upper_losses, self.lower_losses), terms):
            store.append(float(t.detach()))

    def _clip_id(self, name, version):
        return name if self.finetune else "~".join([str(int(version)), name])

    def _record_predictions(self, predictions, targets, names, versions):
        ts_o, key_o, up_o, lo_o = predictions
        ts_t, key_t, up_t, lo_t = targets
        if self._constrained() or self._metrical() or self._beam_size() >= 2:
            # the ids the constrained / beam decoder EMITTED (the log-probabilities stay the unconstrained ones, their argmax is not what was decoded)
            model = self.modules.transcription
            decoded = getattr(model, "module", model).last_decoded
            up_ids, lo_ids = decoded["up"][0].cpu().numpy(), decoded["lo"][0].cpu().numpy()
        else:
            up_ids, lo_ids = up_o.argmax(-1).cpu().numpy(), lo_o.argmax(-1).cpu().numpy()
        ts_ids, key_ids = ts_o.argmax(-1).cpu().numpy(), key_o.argmax(-1).cpu().numpy()
        up_t, lo_t, ts_t, key_t = up_t.cpu().numpy(), lo_t.cpu().numpy(), ts_t.cpu().numpy(), key_t.cpu().numpy()
        al = None
        if self._alignment():
            model = self.modules.transcription
            al = {k: {f: t.cpu().numpy() for f, t in v.items()} for k, v in getattr(model, "module", model).last_alignment.items()}
        for b, name in enumerate(names):
            cid = self._clip_id(name, versions[b])
            if al is not None:
                # per bar one centroid (in frames), per staff and bar one per KEPT token: trimmed exactly as metrics.unpad trims the ids
                kept = {k: [len(metrics.unpad(r)) for r in ids[b]] for k, ids in (("up", up_ids), ("lo", lo_ids))}
                rec = {"frames_per_second": self.hparams.sample_rate / self.hparams.hop_length,
                       "bar": al["bar"]["centroid"][b].tolist(), "bar_weight": al["bar"]["weight"][b].tolist()}
                for key, k in (("upper", "up"), ("lower", "lo")):
                    rec[key] = [al[k]["centroid"][b, i, :n].tolist() for i, n in enumerate(kept[k])]
                    rec[key + "_weight"] = [al[k]["weight"][b, i, :n].tolist() for i, n in enumerate(kept[k])]
                self.alignment_records[cid] = rec
            self.upper_pred[cid] = [metrics.unpad(r).tolist() for r in up_ids[b]]
            self.upper_target[cid] = [metrics.unpad(r).tolist() for r in up_t[b]]
            self.lower_pred[cid] = [metrics.unpad(r).tolist() for r in lo_ids[b]]
            self.lower_target[cid] = [metrics.unpad(r).tolist() for r in lo_t[b]]
            self.key_pred[cid], self.key_target[cid] = key_ids[b].tolist(), key_t[b].tolist()
            self.time_sig_pred[cid], self.time_sig_target[cid] = ts_ids[b].tolist(), ts_t[b].tolist()

    # ------------------------------------------------------------------ training step
    def _fused_step(self):
        """The fused HIP step needs the HIP model, Adadelta and the yaml's NLL objective; otherwise fall back to the generic path."""
        if getattr(self, "_fused", None) is None:
            model = self.modules.transcription
            opt = getattr(self, "optimizer", None)
            if opt is None:
                return False              # no optimizer yet (evaluate() before fit()): decide once there is one, do not cache "no"
            self._fused = False
            if hasattr(model, "flatten_") and isinstance(opt, torch.optim.Adadelta) and str(self.device).startswith("cuda"):
                from piano_a2s_amd import train
                g = opt.param_groups[0]
                self._fused = train.TrainStep(model, lr=g["lr"], rho=g["rho"], eps=g["eps"], max_grad_norm=self.max_grad_norm)
        return self._fused

    def init_optimizers(self):
        """As sb.Brain.init_optimizers (the optimizer becomes the checkpointer's `optimizer` recoverable) -- but when the fused HIP step
        is the one that trains, ITS Adadelta accumulators are the optimizer state: FusedAdadelta is registered instead of the idle
        torch object (same optimizer.ckpt format), before on_fit_start recovers, so a resumed run continues with the saved
        square_avg / acc_delta instead of silently restarting them from zero."""
        super().init_optimizers()
        fused = self._fused_step()
        if fused and self.checkpointer is not None:
            self.checkpointer.add_recoverable("optimizer", fused.opt)

    def on_fit_start(self):
        """Recovery restores the learning rate with the optimizer state (optimizer.ckpt holds the NewBob-annealed lr, as in the
        reference, whose torch optimizer IS the recoverable).  When the fused step trains, the recoverable is fused.opt: its recovered
        lr is the truth, and the idle torch optimizer (which update_learning_rate also addresses) is brought in line with it -- without
        this, the first epoch after a resume, or after finetune.py's copy of the pretraining save/, ran at the yaml's initial lr."""
        self._augmenters()                        # (an augmentation switch out of range is refused before anything else happens)
        self._room(sb.Stage.TRAIN)                # (and a --synthetic_room)
        if self._tuning_correction():             # (and a --tuning_correction on features whose bins do not divide the semitone)
            from piano_a2s_amd.tuning import bins_per_semitone
            bins_per_semitone(getattr(self.hparams, "bins_per_octave", 60))
        super().on_fit_start()
        self._set_constrained_decoding()          # (a module that cannot decode under the grammar is refused before the first epoch, not after it)
        fused = self._fused_step()
        if fused and self.optimizer is not None:
            for g in self.optimizer.param_groups:
                g["lr"] = fused.opt.lr

    def fit_batch(self, batch):
        fused = self._fused_step()
        if not fused:
            if self._augmenters() or self._tuning_correction():
                # the generic path reads the batch twice (compute_forward, compute_objectives): both see the augmented device batch, which
                # `_features` and `_to_device` pass through as it is
                batch = self._train_features(batch)
            return super().fit_batch(batch)
        fused(self._train_features(batch), self.teacher_forcing_ratio)
        *terms, applied = fused.report()                              # one small D2H per step (the reference does four)
        self._record_losses(*[torch.tensor(t) for t in terms])
        loss = torch.tensor(sum(terms))
        if not applied:
            # the device skipped the update (non-finite loss on some rank or non-finite gradient norm): SpeechBrain's check_gradients
            # counts these and gives up after `nonfinite_patience` of them (reference pretrain.py:126)
            self.nonfinite_count += 1
            if self.nonfinite_count > self.nonfinite_patience:
                raise ValueError("Loss is not finite and patience is exhausted. To debug, wrap `fit()` with autograd's "
                                 "`detect_anomaly()`.")
        return loss

    def evaluate_batch(self, batch, stage):
        with torch.no_grad():
            predictions = self.compute_forward(batch, stage=stage)
            loss = self.compute_objectives(predictions, batch, stage=stage)
        return loss.detach()

    # ------------------------------------------------------------------ stage hooks
    def on_stage_start(self, stage, epoch):
        self.time_losses, self.key_losses, self.upper_losses, self.lower_losses = [], [], [], []
        if stage != sb.Stage.TRAIN:
            self.upper_pred, self.upper_target, self.lower_pred, self.lower_target = {}, {}, {}, {}
            self.key_pred, self.key_target, self.time_sig_pred, self.time_sig_target = {}, {}, {}, {}
            self.alignment_records = {}
            for split in ("valid", "test"):
                mkdirs(os.path.join(self.hparams.output_folder, "results", split))
        self.time_sig_list = load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                               "data_processing", "metadata", "time_signature_list.json"))
        if stage == sb.Stage.TRAIN:
            for _, aug in self._augmenters():
                aug.reseed(epoch)                     # the draws of an epoch depend on (seed, rank, epoch) alone: a resumed run repeats them
        if stage != sb.Stage.TRAIN:
            self.teacher_forcing_ratio = 0.
        elif self.finetune:
            self.teacher_forcing_ratio = self.hparams.teacher_forcing_ratio
        else:                                                          # exponential decay per epoch (pretrain.py:151)
            self.teacher_forcing_ratio = self.hparams.teacher_forcing_ratio * self.hparams.teacher_forcing_decay ** epoch

    def on_stage_end(self, stage, stage_loss, epoch):
        stats = {"loss": stage_loss, "time_loss": np.mean(self.time_losses), "key_loss": np.mean(self.key_losses),
                 "upper_loss": np.mean(self.upper_losses), "lower_loss": np.mean(self.lower_losses)}
        if not self.finetune:
            stats["teacher_forcing_ratio"] = self.teacher_forcing_ratio
        stats.update(self._tuning_stats())
        if stage == sb.Stage.TRAIN:
            self.train_stats = stats
            for cls, aug in self._augmenters():
                counts = aug.counts()                                 # one small D2H per epoch each; cumulative over the run, logged with the train stats
                stats.update({stat: counts[name] for stat, name in zip(cls.stats, cls.count_names)})
            return
        if not hasattr(self, "train_stats"):
            self.train_stats = {"loss": -1}
        inv = labels.labels_map_inv
        wer_up, wer_up_d = metrics.corpus_wer(self.upper_pred, self.upper_target, inv)
        wer_lo, wer_lo_d = metrics.corpus_wer(self.lower_pred, self.lower_target, inv)
        key_f1, key_f1_d = metrics.corpus_f1(self.key_pred, self.key_target)
        time_f1, time_f1_d = metrics.corpus_f1(self.time_sig_pred, self.time_sig_target)
        stats.update(key_f1=key_f1, time_f1=time_f1, WER_upper=wer_up, WER_lower=wer_lo, WER=(wer_up + wer_lo) / 2)
        if hasattr(self.hparams, "metrical_decoding"):
            # share of the decoded bars (both staves) that are complete under the time signature predicted for them -- for whatever decoder ran:
            # --metrical_decoding=false reports it for the run's other settings (host side; without the override the stats are as before)
            from piano_a2s_amd import kern_grammar
            if not hasattr(self, "_kern_metre"):
                self._kern_metre = kern_grammar.KernMetre()
            both = {(cid, staff): rows for staff, pred in (("up", self.upper_pred), ("lo", self.lower_pred)) for cid, rows in pred.items()}
            stats["complete_bars"] = kern_grammar.complete_share(both, {k: self.time_sig_pred[k[0]] for k in both}, self._kern_metre)
        notes_d = None
        if self._note_metrics():
            notes_up, notes_up_d = metrics.corpus_note_f1(self.upper_pred, self.upper_target)
            notes_lo, notes_lo_d = metrics.corpus_note_f1(self.lower_pred, self.lower_target)
            for staff, m in (("upper", notes_up), ("lower", notes_lo)):
                stats.update({f"note_f1_{level}_{staff}": m[f"f1_{level}"] for level in ("pitch", "onset", "value")})
            stats["note_f1"] = (notes_up["f1_onset"] + notes_lo["f1_onset"]) / 2
            notes_d = {cid: {"upper": notes_up_d[cid], "lower": notes_lo_d[cid]} for cid in self.upper_pred}
        old_lr, new_lr = self.hparams.lr_annealing(stats["WER"])
        sb.nnet.schedulers.update_learning_rate(self.optimizer, new_lr)
        fused = self._fused_step()
        if fused:                                                      # the lr the fused step uses AND the one optimizer.ckpt saves below
            sb.nnet.schedulers.update_learning_rate(fused.opt, new_lr)
        self.hparams.train_logger.log_stats(stats_meta={"epoch": epoch, "lr": old_lr}, train_stats=self.train_stats, valid_stats=stats)
        self.checkpointer.save_and_keep_only(meta={"loss": stats["loss"], "WER": stats["WER"]}, min_keys=["WER"])
        self.last_stats = stats
        split = "test" if stage == sb.Stage.TEST else "valid"
        for cid in self.upper_pred:
            pred = [[self.key_pred[cid][i] - 6, self.time_sig_list[self.time_sig_pred[cid][i]], self.lower_pred[cid][i], self.upper_pred[cid][i]]
                    for i in range(len(self.upper_pred[cid]))]
            record = {"pred": pred, "wer_upper": wer_up_d[cid], "wer_lower": wer_lo_d[cid], "key_f1": key_f1_d[cid], "time_f1": time_f1_d[cid]}
            record.update(self._clip_record(cid, split))
            if cid in self.alignment_records:
                record["alignment"] = self.alignment_records[cid]
            if notes_d is not None:
                record["notes"] = notes_d[cid]
            save(record, os.path.join(self.hparams.output_folder, "results", split, f"{cid}.json"))

    def _clip_record(self, cid, split):
        ff = self.hparams.feature_folder
        if self.finetune:
            return {"target_path": os.path.join(ff, "test", "target", f"{cid}.pkl")}
        version, chunk, soundfont = (cid.split("~") + ["", ""])[:3]
        info_path = os.path.join(ff, split, version, "info", f"{chunk}.json")
        composer = load(info_path).get("composer") if os.path.exists(info_path) else None
        return {"style": "classical" if chunk[:1].islower() else "pop", "soundfont": soundfont, "composer": composer,
                "target_path": os.path.join(ff, split, version, "target", f"{chunk}.pkl")}


def write_run_summary(brain, hparams):
    """<output_folder>/run_summary.json (rank 0): how the run executed -- which training step, how many ranks over which backend, how many
    optimizer steps and gradient all-reduces.  Not part of the reference's artefacts; it is what lets a launch under torchrun be
    checked end to end (tests/test_gpu_recipe.py)."""
    import torch.distributed as dist
    if not sb.utils.distributed.if_main_process():
        return
    fused = getattr(brain, "_fused", None)
    inited = dist.is_available() and dist.is_initialized()
    extra = {}
    for cls in AUGMENTERS:
        aug = getattr(brain, cls.cache, None)
        if aug is not None:
            extra[cls.summary] = dict(**aug.settings(), **aug.counts())
    room = getattr(brain, "_synthetic_room", None)
    if room is not None:
        extra["room"] = dict(stages=room[0], clips=room[1].clips, **room[1].describe())
    save({**extra, "fused_hip_step": bool(fused), "world_size": dist.get_world_size() if inited else 1, "backend": dist.get_backend() if inited else None,
          "optimizer_steps": int(getattr(brain, "step", 0)), "gradient_allreduces": int(fused.collectives) if fused else 0,
          "nonfinite_steps": int(getattr(brain, "nonfinite_count", 0)), "device": str(brain.device)},
         os.path.join(hparams["output_folder"], "run_summary.json"))
