"""From a recording to decoded kern bars: resample (piano_a2s_amd.audio, csrc/a2s_resample.hip), cut into the clips the model
takes, GPU VQT, the model exactly as the recipe's evaluation runs it, ids -> kern text per bar and staff.

A joined two-staff Humdrum file is out of scope: it needs spine-split bookkeeping across bars, which the reference leaves to humextra.  The result is a
dict per recording; the command line (transcribe.py at the root of the repository) writes it as JSON."""
import json
import os

import numpy as np
import torch
import yaml

from data_processing.humdrum import LabelsMultiple

from . import audio, metrics

labels = LabelsMultiple(extended=True)
_VQT = {}
_TIME_SIGNATURES = []


def time_signatures():
    if not _TIME_SIGNATURES:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data_processing", "metadata", "time_signature_list.json")
        with open(path) as f:
            _TIME_SIGNATURES.extend(json.load(f))
    return _TIME_SIGNATURES


def _hp(hparams, key, default=None):
    return hparams.get(key, default) if isinstance(hparams, dict) else getattr(hparams, key, default)


def _vqt(device, hparams):
    key = (str(device), int(_hp(hparams, "sample_rate", 16000)), int(_hp(hparams, "hop_length", 160)), int(_hp(hparams, "bins_per_octave", 60)),
           int(_hp(hparams, "n_octaves", 8)), float(_hp(hparams, "gamma", 20)))
    if key not in _VQT:
        from .vqt import VQT
        _VQT[key] = VQT(device, sr=key[1], hop=key[2], n_bins=key[3] * key[4], bins_per_octave=key[3], gamma=key[5])
    return _VQT[key]


def to_16k(x, sr, device, hparams):
    """x: (frames,) or (frames, channels) samples at the rate sr, numpy or torch -> (wave (n,) float32 on the device at the hparams' rate, its rate)."""
    x = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x).to(torch.float32)
    if x.dim() == 1:
        x = x[:, None]
    if x.dim() != 2:
        raise ValueError(f"transcribe: the samples must be (frames,) or (frames, channels) (got {tuple(x.shape)})")
    rate = int(_hp(hparams, "sample_rate", 16000))
    y, n_out = audio.Resampler(device, sr, rate)(x.to(device)[None].contiguous())
    return y[0], rate


def check_downbeats(downbeats, beats_per_bar):
    """What transcribe_waveform takes as `downbeats`: None, times in seconds, or the word "track"; beats_per_bar (2, 3 or 4) only with "track"."""
    if isinstance(downbeats, str) and downbeats != "track":
        raise ValueError(f'transcribe: downbeats must be None, a list of times in seconds or "track" (got {downbeats!r})')
    tracking = isinstance(downbeats, str)
    if beats_per_bar is not None and not tracking:
        raise ValueError('transcribe: beats_per_bar belongs to downbeats="track"')
    if beats_per_bar is not None and beats_per_bar not in (2, 3, 4):
        raise ValueError(f"transcribe: beats_per_bar must be 2, 3 or 4 (got {beats_per_bar!r})")


def check_tuning(tuning):
    """What transcribe_waveform takes as `tuning`: None, the word "auto", or a finite number of cents -> None, "auto" or a float."""
    if tuning is None or tuning == "auto":
        return tuning
    if isinstance(tuning, (str, bool)) or not isinstance(tuning, (int, float, np.integer, np.floating)) or not np.isfinite(tuning):
        raise ValueError(f'transcribe: tuning must be None, "auto" or a number of cents (got {tuning!r})')
    return float(tuning)


def transcribe_waveform(model, x, sr, *, downbeats=None, beats_per_bar=None, window_seconds=12.0, hop_seconds=None, batch_size=16, hparams, resynthesis=False, align_notes=False,
                        dynamics=False, dynamics_rounds=None, min_level_db=None, tuning=None, performed_timing=None):
    """Decode the recording x ((frames,) or (frames, channels) at the rate sr) with `model` (models.ScoreTranscription on the GPU), run in evaluation
    mode exactly as the recipe's VALID / TEST stages run it; `constrained_decoding`, `beam_size` (with `beam_length_penalty`) and `alignment` are
    honoured as the caller set them on the module.  hparams: the yaml's geometry (sample_rate, hop_length, max_frame_num, max_bars, VQT keys).
    Windows: audio.plan_windows -- with `downbeats` (seconds) groups of max_bars bars as in the reference's test protocol, without them fixed windows
    every hop_seconds (the model was trained on bar-aligned clips: expect less of the second).  downbeats="track": the downbeats are tracked on the
    recording's own features (piano_a2s_amd.beats; beats_per_bar 2, 3 or 4 fixes the meter) and then used as if they had been
    given; the result gains "tracking": {"beats_s", "downbeats_s", "beats_per_bar", "period_frames"}.
    -> {"sample_rate_in", "sample_rate", "frames_per_second", "windows": [{"start_s", "stop_s", "n_bars", "flags", "time_signature", "key",
        "bars": [{"upper", "lower", "upper_ids", "lower_ids", ["complete": with `metrical_decoding`]}], ["alignment"]}]};  time_signature and key hold one entry per kept bar (key as in the
        recipe's result files: class - 6), bars the first n_bars decoded bars.
    resynthesis=True (needs downbeats, given or tracked: without them the bars have no position, ValueError): the decoded score is played back on
    piano_a2s_amd.resynth's instrument and compared with the recording bar by bar, whatever the decoding mode -- only the
    emitted ids and the predicted time signatures are read.  Every bar gains "agreement" (the Pearson correlation of the recording's and the
    resynthesis's features over the bar's frames, in [-1, 1]; None for a window without a note and for a bar in which nothing sounds) and "notes" ([[onset_s, length_s, midi]] in
    recording time), every window "agreement" (the mean over its bars that have one, or None) and the flag "notes_truncated" where its notes did not
    fit a render program; the result gains "resynthesis": {"sample_rate", "wave": float32 numpy (N,)}, the windows' renders overlap-added at their
    starts (release tails included up to the render length), as long as the recording at the model's rate.  Off, nothing of this is allocated,
    launched or returned.
    align_notes=True (needs resynthesis, ValueError without): inside every bar the resynthesis is warped onto the recording (banded dynamic time
    warping of the two feature tensors).  Every bar gains "agreement_warped" (the agreement with the resynthesis read along the
    warp: timing no longer counts; None where "agreement" is None) and "performed" ([[onset_s, length_s, midi]]: the bar's "notes" with onset and end
    moved through the bar's warp, clamped to the bar, at least one frame long), every window "agreement_warped" (the mean over its bars).
    dynamics=True (needs resynthesis, ValueError without; with or without align_notes): every note's loudness is estimated from the recording by
    analysis by synthesis (dynamics_rounds rounds, default resynth.DYNAMICS_ROUNDS).  Every bar gains "dynamics" ([[level_db,
    velocity]] parallel to "notes": dB relative to the window's median note in -30 .. 12, and the MIDI velocity 64 * 10^(level_db / 40) in 1 .. 127;
    [None, None] for a note that did not fit the render program) and "agreement_dynamics" (the agreement with the resynthesis at those dynamics),
    where the bar was aligned also "agreement_dynamics_warped"; every window the means of those; "resynthesis" is the render at the estimated
    dynamics.  min_level_db=L: every bar also gains "quiet", one flag per note, True where the level is below L (audio.result_notes leaves those
    out; the decoded bars keep them).  A level is relative to its window: loudness across windows is not recovered.
    tuning="auto": the recording's tuning is estimated on the device from the features of all its windows as one group (piano_a2s_amd.tuning, DESIGN.md
    section 27) and the features are shifted back onto the grid at A4 = 440 Hz before the model and the resynthesis comparison see them (a tracker
    keeps the uncorrected ones); tuning=CENTS (a number): the features are shifted by that much and nothing is estimated.  The result gains "tuning":
    {"cents", "confidence", "peaks", "determined", "a4_hz"} (a4_hz = 440 * 2^(cents / 1200); with a given number confidence and peaks are None); an
    estimate that is not determined leaves the features as they are.  One read-back of three doubles per recording.  The resynthesis and the MIDI
    file stay at 440 Hz.  Any other string: ValueError.  Off, the result has no such key and neither tuning kernel runs.
    performed_timing=R (needs align_notes, ValueError without; 0 or None: off; R < 0: ValueError): the resynthesis itself is moved to the performed
    timing: R rounds on the device move every note through the warp of its bar and render and align again.  Every bar gains
    "retimed" ([[onset_s, length_s, midi]] parallel to "notes": where the notes stand after the last round; a note that did not fit the render
    program keeps its "performed" entry) and "agreement_retimed" (the PLAIN agreement of the recording with the render at that timing), every window
    the mean; "resynthesis" is that render, and audio.result_notes and the MIDI file take "retimed" before "performed".  "performed",
    "agreement" and "agreement_warped" keep their values: they describe the first, straight pass.  With dynamics=True the dynamics keys are measured
    on the retimed render, every note read at the same frames of the recording and the render, and "agreement_dynamics_warped" is None: that render
    is at the performed timing already."""
    check_downbeats(downbeats, beats_per_bar)
    tuning = check_tuning(tuning)
    if resynthesis and downbeats is None:
        raise ValueError("transcribe: resynthesis needs downbeats (given or tracked): in fixed windows the decoded bars have no position in the audio")
    if align_notes and not resynthesis:
        raise ValueError("transcribe: align_notes aligns the resynthesis with the recording: it needs resynthesis=True")
    if dynamics and not resynthesis:
        raise ValueError("transcribe: dynamics sets the amplitudes of the resynthesis from the recording: it needs resynthesis=True")
    if (dynamics_rounds is not None or min_level_db is not None) and not dynamics:
        raise ValueError("transcribe: dynamics_rounds and min_level_db belong to dynamics=True")
    if dynamics_rounds is not None and int(dynamics_rounds) < 1:
        raise ValueError(f"transcribe: dynamics_rounds must be at least 1 (got {dynamics_rounds!r})")
    performed_timing = int(performed_timing or 0)
    if performed_timing < 0:
        raise ValueError(f"transcribe: performed_timing counts rounds: it must not be negative (got {performed_timing!r})")
    if performed_timing and not align_notes:
        raise ValueError("transcribe: performed_timing moves the notes through the warps of align_notes: it needs align_notes=True")
    core = getattr(model, "module", model)
    device = next(core.parameters()).device
    hop = int(_hp(hparams, "hop_length", 160))
    max_bars = int(_hp(hparams, "max_bars", 5))
    length = (int(_hp(hparams, "max_frame_num", 1201)) - 1) * hop
    wave, rate = to_16k(x, sr, device, hparams)
    fps = rate / hop
    tracking = None
    if isinstance(downbeats, str):
        from . import beats
        tracking = beats.track_recording(wave, hparams, beats_per_bar=beats_per_bar)
        downbeats = tracking["downbeats_s"]
    plan = audio._plan(wave.shape[0], rate, downbeats, window_seconds, hop_seconds, max_bars, length)
    result = {"sample_rate_in": int(sr), "sample_rate": rate, "frames_per_second": fps, "windows": []}
    if tracking is not None:
        result["tracking"] = tracking
    if resynthesis:
        from . import resynth
        result["resynthesis"] = {"sample_rate": rate, "wave": np.zeros(wave.shape[0], dtype=np.float32)}
    if not plan:
        return result
    feats = _vqt(device, hparams)(audio.cut_windows(wave, plan, length))
    if tuning is not None:
        from . import tuning as tuning_
        tuner = tuning_.Tuner(device, bins_per_octave=int(_hp(hparams, "bins_per_octave", 60)))
        feats, est, _ = tuner(feats, first=[0, len(plan)], cents=None if tuning == "auto" else tuning)            # all windows: one group
        if tuning == "auto":
            result["tuning"] = tuning_.describe(est[0].cpu().numpy(), tuner.min_conf, tuner.min_peaks)
        else:
            result["tuning"] = {"cents": tuning, "confidence": None, "peaks": None, "determined": True, "a4_hz": tuning_.a4_hz(tuning)}
    inv, ts_list = labels.labels_map_inv, time_signatures()
    was_training = core.training
    model.eval()
    try:
        for w0 in range(0, len(plan), int(batch_size)):
            with torch.no_grad():
                ts_o, key_o, up_o, lo_o = model(spectrogram=feats[w0:w0 + int(batch_size)], inference=True, ground_truth=None, teacher_forcing_ratio=0.,
                                                device=device)
            metrical = bool(getattr(core, "metrical_decoding", False))
            if getattr(core, "constrained_decoding", False) or metrical or int(getattr(core, "beam_size", 1)) >= 2:
                # the ids the constrained / beam decoder EMITTED (the log-probabilities stay the unconstrained ones)
                up_ids, lo_ids = core.last_decoded["up"][0].cpu().numpy(), core.last_decoded["lo"][0].cpu().numpy()
            else:
                up_ids, lo_ids = up_o.argmax(-1).cpu().numpy(), lo_o.argmax(-1).cpu().numpy()
            ts_ids, key_ids = ts_o.argmax(-1).cpu().numpy(), key_o.argmax(-1).cpu().numpy()
            al = None
            if getattr(core, "alignment", False) and core.last_alignment is not None:
                al = {k: {f: t.cpu().numpy() for f, t in v.items()} for k, v in core.last_alignment.items()}
            batch = []
            for b, (start, stop, n_bars, flags, lines) in enumerate(plan[w0:w0 + int(batch_size)]):
                n_bars = min(n_bars, up_ids.shape[1])
                up = [metrics.unpad(r) for r in up_ids[b][:n_bars]]
                lo = [metrics.unpad(r) for r in lo_ids[b][:n_bars]]
                win = {"start_s": start / rate, "stop_s": stop / rate, "n_bars": n_bars, "flags": list(flags),
                       "time_signature": [ts_list[int(i)] for i in ts_ids[b][:n_bars]], "key": [int(i) - 6 for i in key_ids[b][:n_bars]],
                       "bars": [{"upper": metrics.ids_to_text([u], inv), "lower": metrics.ids_to_text([l], inv), "upper_ids": u.tolist(), "lower_ids": l.tolist()}
                                for u, l in zip(up, lo)]}
                if metrical:
                    # both staves of the bar end in <eos> with every spine at the length of the bar's time signature
                    km, eos = core._kern_metre(), core._kern_grammar().eos
                    for i, bar in enumerate(win["bars"]):
                        rows = (up_ids[b][i].tolist(), lo_ids[b][i].tolist())
                        bar["complete"] = all(eos in r and km.complete(r, int(ts_ids[b][i])) for r in rows)
                if al is not None:
                    win["alignment"] = _alignment_record(al, b, start / rate, fps, up, lo)
                result["windows"].append(win)
                batch.append((win, start, lines, up, lo))
            if resynthesis:
                _resynthesise_batch(resynth, batch, feats[w0:w0 + int(batch_size)], _vqt(device, hparams), hop, rate, result["resynthesis"]["wave"],
                                    align=align_notes, dynamics=(int(dynamics_rounds or resynth.DYNAMICS_ROUNDS) if dynamics else 0), min_level_db=min_level_db,
                                    retime=performed_timing)
    finally:
        model.train(was_training)
    return result


def _resynthesise_batch(resynth, batch, feats, vqt, hop, rate, total, align=False, dynamics=0, min_level_db=None, retime=0):
    """The resynthesis of one batch of windows [(window dict, start sample, bar lines, upper rows, lower rows)]: fills the windows' and bars' new keys
    and adds the renders into `total` (the recording-long waveform) at the windows' starts.  align: also the keys of align_notes; dynamics: the
    rounds of the dynamics estimate (0: off) and its keys; retime: the rounds of performed_timing (0: off) and its keys."""
    windows, bar_notes = [], []
    for win, start, lines, up, lo in batch:
        lines = lines[:win["n_bars"] + 1]
        events, truncated = resynth.score_events(up, lo, win["time_signature"], lines)
        if truncated:
            win["flags"].append("notes_truncated")
        for i, bar in enumerate(win["bars"]):
            notes, _ = resynth.score_events(up[i:i + 1], lo[i:i + 1], win["time_signature"][i:i + 1], lines[i:i + 2], max_events=1 << 30)
            bar["notes"] = [[(start + int(o)) / rate, int(n) / rate, int(m)] for o, n, m in notes]
            bar_notes.append(notes)
        windows.append({"events": events, "bar_lines": lines})
    waves, agreements, *more = resynth.resynthesise(windows, feats, vqt, hop, align=align, dynamics=dynamics, retime=retime)
    alignments, levels, retimed = more[0] if align else None, more[-1] if dynamics else None, more[1] if retime else None
    bar_notes = iter(bar_notes)
    for k, ((win, start, lines, *_), w, agr) in enumerate(zip(batch, waves, agreements)):
        for i, (bar, a) in enumerate(zip(win["bars"], agr)):
            bar["agreement"] = a
            if align:
                al = alignments[k][i]
                bar["agreement_warped"] = None if al is None else al["agreement_warped"]
                moved = resynth.performed_notes(next(bar_notes), None if al is None else al["warp"], 0 if al is None else al["first_frame"], hop,
                                                lines[i], lines[i + 1])
                bar["performed"] = [[(start + o) / rate, n / rate, m] for o, n, m in moved]
        win["agreement"] = resynth.mean_agreement(agr)
        if align:
            win["agreement_warped"] = resynth.mean_agreement([bar["agreement_warped"] for bar in win["bars"]])
        if retime:
            _retimed_keys(resynth, win, retimed[k], start, rate)
        if dynamics:
            _dynamics_keys(resynth, win, levels[k], align, min_level_db)
        if w is not None and start < len(total):
            n = min(len(w), len(total) - start)
            total[start:start + n] += w[:n]


def _retimed_keys(resynth, win, rt, start, rate):
    """The keys of performed_timing of one window: rt is the window's entry of resynthesise's retimed (None for a window without a note).  The window's
    events are its bars' notes in order, cut at the render program's length."""
    at = 0
    for i, bar in enumerate(win["bars"]):
        n = len(bar["notes"])
        have = 0 if rt is None else max(0, min(n, len(rt["events"]) - at))
        bar["retimed"] = [[(start + int(o)) / rate, int(ln) / rate, int(m)] for o, ln, m in (rt["events"][at:at + have] if have else [])] + [list(p) for p in bar["performed"][have:]]
        bar["agreement_retimed"] = None if rt is None else rt["agreement"][i]
        at += n
    win["agreement_retimed"] = resynth.mean_agreement([bar["agreement_retimed"] for bar in win["bars"]])


def _dynamics_keys(resynth, win, lv, align, min_level_db):
    """The keys of dynamics=True of one window: lv is the window's entry of resynthesise's dynamics (None for a window without a note).  The window's
    events are its bars' notes in order, cut at the render program's length."""
    at = 0
    for i, bar in enumerate(win["bars"]):
        n = len(bar["notes"])
        have = 0 if lv is None else max(0, min(n, len(lv["level_db"]) - at))
        bar["dynamics"] = [[float(lv["level_db"][at + j]), int(lv["velocity"][at + j])] for j in range(have)] + [[None, None]] * (n - have)
        bar["agreement_dynamics"] = None if lv is None else lv["agreement"][i]
        if align and bar.get("agreement_warped") is not None:
            bar["agreement_dynamics_warped"] = lv["agreement_warped"][i]
        if min_level_db is not None:
            bar["quiet"] = [d[0] is not None and d[0] < float(min_level_db) for d in bar["dynamics"]]
        at += n
    win["agreement_dynamics"] = resynth.mean_agreement([bar["agreement_dynamics"] for bar in win["bars"]])
    if align:
        win["agreement_dynamics_warped"] = resynth.mean_agreement([bar.get("agreement_dynamics_warped") for bar in win["bars"]])


def _alignment_record(al, b, start_s, fps, up, lo):
    """The record of the recipe's result files for one window, its frame positions as seconds in the recording (None where no
    step ran), trimmed to the kept bars and tokens."""
    sec = lambda v: [None if f < 0 else start_s + float(f) / fps for f in v]
    n_bars = len(up)
    rec = {"unit": "seconds", "bar": sec(al["bar"]["centroid"][b][:n_bars]), "bar_weight": al["bar"]["weight"][b][:n_bars].tolist()}
    for key, k, rows in (("upper", "up", up), ("lower", "lo", lo)):
        rec[key] = [sec(al[k]["centroid"][b, i, :len(r)]) for i, r in enumerate(rows)]
        rec[key + "_weight"] = [al[k]["weight"][b, i, :len(r)].tolist() for i, r in enumerate(rows)]
    return rec


def read_downbeats(path):
    """One time per line, the first whitespace-separated column (ASAP's annotation files: time, time, label); where a third column exists only the
    lines whose third column starts with `db` count."""
    out = []
    with open(path) as f:
        for line in f:
            cols = line.split()
            if not cols or cols[0].startswith("#"):
                continue
            if len(cols) >= 3 and not cols[2].startswith("db"):
                continue
            out.append(float(cols[0]))
    return out


def load_model(hparams_file, checkpoint, device, overrides=None):
    """(model on the device in evaluation mode, the geometry keys of the yaml).  The model is the yaml's `transcription`; `checkpoint` is a state_dict
    file or a checkpoint directory holding transcription.ckpt."""
    from .hyperyaml import load_keys
    keys = ("transcription", "sample_rate", "hop_length", "max_frame_num", "max_bars", "bins_per_octave", "n_octaves", "gamma")
    with open(hparams_file) as f:
        hp = load_keys(f, keys, overrides)
    path = os.path.join(checkpoint, "transcription.ckpt") if os.path.isdir(checkpoint) else checkpoint
    if not os.path.isfile(path):
        raise FileNotFoundError(f"no checkpoint at {path}")
    model = hp.pop("transcription")
    model.load_state_dict(torch.load(path, map_location="cpu"))
    return model.to(device).eval(), hp


HELP = """Transcribe WAV recordings (any sample rate, any number of channels) into kern bars, one JSON file per recording.

With --downbeats the recording is cut into groups of max_bars bars, the reference's test protocol.  With --track_downbeats the tool finds the downbeats
itself, on the recording's own features (metres of 2, 3 and 4 beats; --beats_per_bar fixes the metre), and cuts at them in the same way.  With neither the
tool works on fixed windows, but the model was trained on bar-aligned clips: expect less.  The output holds the decoded bars of every window per staff; a joined two-staff Humdrum file is out
of scope (it needs spine-split bookkeeping across bars, which the reference leaves to humextra)."""


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(prog="transcribe.py", description=HELP, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("hparams", help="hparams yaml (hparams/finetune.yaml): the model is its `transcription` key")
    ap.add_argument("audio", nargs="+", help="WAV files: PCM 8/16/24/32 bits, IEEE float 32/64 bits, extensible headers")
    ap.add_argument("--checkpoint", required=True, help="a state_dict file, or a checkpoint directory holding transcription.ckpt")
    where = ap.add_mutually_exclusive_group()
    where.add_argument("--downbeats", help="one downbeat time (s) per line, first column; with a third column only lines whose third column starts with `db`")
    where.add_argument("--track_downbeats", action="store_true", help="track beats and downbeats on the recording itself and cut at the tracked downbeats")
    ap.add_argument("--beats_per_bar", type=int, choices=(2, 3, 4), default=None, help="with --track_downbeats: the metre, instead of the tracker's choice")
    ap.add_argument("--out", default=".", help="output folder: DIR/NAME.json per recording")
    ap.add_argument("--window_seconds", type=float, default=12.0)
    ap.add_argument("--hop_seconds", type=float, default=None)
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--constrained_decoding", action="store_true", help="decode under the kern token grammar")
    ap.add_argument("--metrical_decoding", action="store_true", help="decode under the grammar and the metre of each bar's predicted time signature; "
                    'every bar of the output gains "complete"')
    ap.add_argument("--beam_size", type=int, default=1, help="1 .. 4 hypotheses per clip, 1 = greedy")
    ap.add_argument("--beam_length_penalty", type=float, default=0.0)
    ap.add_argument("--alignment", action="store_true", help="also report where in the recording every decoded bar and token lies")
    ap.add_argument("--resynthesis", action="store_true", help="play the decoded score back and compare it with the recording bar by bar: every bar gains "
                    '"agreement" and "notes", and DIR/NAME.resynth.wav holds the recording (left) beside the resynthesis (right), 16 bits, for A/B listening; '
                    "needs --downbeats or --track_downbeats")
    ap.add_argument("--align_notes", action="store_true", help="implies --resynthesis: warp the resynthesis onto the recording inside every bar; every bar "
                    'gains "agreement_warped" and "performed" (its notes where they are heard), and DIR/NAME.mid holds the performed notes as a '
                    "Standard MIDI File (format 0, 1 ms ticks, velocity 64)")
    ap.add_argument("--performed_timing", type=int, nargs="?", const=2, default=0, metavar="R", help="implies --align_notes: move the resynthesis itself to "
                    'the performed timing in R rounds (default 2) of warp, retime, render and align on the device; every bar gains "retimed" and '
                    '"agreement_retimed", DIR/NAME.resynth.wav plays the score in time with the recording and DIR/NAME.mid holds the retimed notes')
    ap.add_argument("--dynamics", action="store_true", help="implies --resynthesis: estimate every note's loudness from the recording by analysis by "
                    'synthesis; every bar gains "dynamics" ([level_db, velocity] per note, relative to the window\'s median note) and '
                    '"agreement_dynamics", DIR/NAME.resynth.wav plays the score at those dynamics and DIR/NAME.mid carries the velocities')
    ap.add_argument("--dynamics_rounds", type=int, default=None, help="with --dynamics: rounds of render, measure, update (default 3)")
    ap.add_argument("--min_level_db", type=float, default=None, help="with --dynamics: notes whose level is below this are left out of DIR/NAME.mid and "
                    'marked in the bar\'s "quiet"; nothing is dropped from the decoded bars.  No default: the gap between notes that are not in the '
                    "audio and quiet real notes has only been seen on renders")
    ap.add_argument("--tuning", default=None, metavar="auto|CENTS", help="auto: estimate how far the recording sits from A4 = 440 Hz (in -50 .. 50 cents, "
                    "one value per recording) and shift the features back before the model sees them; a number: shift by that many cents without "
                    'estimating; the output gains "tuning".  The resynthesis and the MIDI file stay at 440 Hz')
    ap.add_argument("--device", default="cuda:0")
    a, extra = ap.parse_known_args(argv)
    overrides = {}
    for item in extra:                                                     # hparams overrides as the recipes take them: --key=value
        if not item.startswith("--") or "=" not in item:
            ap.error(f"unrecognised argument {item!r} (hparams overrides are written --key=value)")
        k, v = item[2:].split("=", 1)
        overrides[k] = yaml.safe_load(v)
    if not 1 <= a.beam_size <= 4:
        ap.error(f"--beam_size must be in 1 .. 4 (got {a.beam_size})")
    if a.metrical_decoding and (a.beam_size >= 2 or a.alignment):
        ap.error("--metrical_decoding decodes greedily: it does not combine with --beam_size >= 2 or --alignment")
    if len(a.audio) > 1 and a.downbeats:
        ap.error("--downbeats belongs to one recording")
    if a.beats_per_bar is not None and not a.track_downbeats:
        ap.error("--beats_per_bar belongs to --track_downbeats")
    if (a.dynamics_rounds is not None or a.min_level_db is not None) and not a.dynamics:
        ap.error("--dynamics_rounds and --min_level_db belong to --dynamics")
    if a.dynamics_rounds is not None and a.dynamics_rounds < 1:
        ap.error(f"--dynamics_rounds must be at least 1 (got {a.dynamics_rounds})")
    if a.tuning is not None and a.tuning != "auto":
        try:
            a.tuning = float(a.tuning)
        except ValueError:
            ap.error(f"--tuning takes `auto` or a number of cents (got {a.tuning!r})")
    if a.performed_timing < 0:
        ap.error(f"--performed_timing counts rounds: it must not be negative (got {a.performed_timing})")
    a.align_notes = a.align_notes or a.performed_timing > 0
    a.resynthesis = a.resynthesis or a.align_notes or a.dynamics
    if a.resynthesis and not (a.downbeats or a.track_downbeats):
        ap.error("--resynthesis needs --downbeats or --track_downbeats: in fixed windows the decoded bars have no position in the audio")
    model, hp = load_model(a.hparams, a.checkpoint, torch.device(a.device), overrides or None)
    model.constrained_decoding, model.alignment = bool(a.constrained_decoding), bool(a.alignment)
    model.metrical_decoding = bool(a.metrical_decoding)
    model.beam_size, model.beam_length_penalty = a.beam_size, a.beam_length_penalty
    downbeats = read_downbeats(a.downbeats) if a.downbeats else ("track" if a.track_downbeats else None)
    os.makedirs(a.out, exist_ok=True)
    for path in a.audio:
        x, sr = audio.read_wav(path)
        result = transcribe_waveform(model, x, sr, downbeats=downbeats, beats_per_bar=a.beats_per_bar, window_seconds=a.window_seconds,
                                     hop_seconds=a.hop_seconds, batch_size=a.batch_size, hparams=hp, resynthesis=a.resynthesis, align_notes=a.align_notes,
                                     dynamics=a.dynamics, dynamics_rounds=a.dynamics_rounds, min_level_db=a.min_level_db, tuning=a.tuning,
                                     performed_timing=a.performed_timing)
        result["audio"] = os.path.basename(path)
        out = os.path.join(a.out, os.path.splitext(os.path.basename(path))[0] + ".json")
        if a.resynthesis:
            # the wave goes to a file of its own, not into the JSON: left the recording at the model's rate, right the resynthesis
            res = result.pop("resynthesis")
            rec = to_16k(x, sr, torch.device(a.device), hp)[0].cpu().numpy()
            wav = out[:-len(".json")] + ".resynth.wav"
            audio.write_wav(wav, np.stack([rec, res["wave"][:len(rec)]], axis=1), res["sample_rate"], bits=16)
            result["resynthesis"] = {"sample_rate": res["sample_rate"], "file": os.path.basename(wav)}
        if a.align_notes or a.dynamics:
            mid = out[:-len(".json")] + ".mid"
            audio.write_midi(mid, result)
            result["performance"] = {"file": os.path.basename(mid)}
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
        print(f"{path}: {len(result['windows'])} windows -> {out}")
    return 0
