"""Is the rendered synthetic corpus learnable, and what do the decoders make of it?  (needs the GPU.)

    python tools/rendered_corpus_eval.py --model small|full --steps N [--batch B] [--frames F] [--eval_clips M] [--note_metrics] [--resynthesis]
                                         [--out profiles/rendered_corpus.json]

1. trains on rendered clips (datasets.syn.RenderedClips, fresh clips every step) for N fused optimizer steps -- once with every clip's own audio and
   once, as the control, from the same initial weights with the audio permuted among the clips of each batch (uninformative audio);
2. on held-out rendered clips reports per-staff WER and key / time-signature F1 of greedy, grammar-constrained and beam (K = 2, 4) decoding with the
   share of well-formed bars, for both models; with --note_metrics also the note-level F1 (pitch / onset / value, metrics.corpus_note_f1: DESIGN.md
   section 17) of every decoding mode beside its WER; with --resynthesis also the mean bar agreement (piano_a2s_amd.resynth) of the
   decoded scores with the audio they were decoded from, beside that of the ground-truth scores of that audio (the ceiling); the control run gives the
   agreement of scores decoded from uninformative audio;
3. reports the mean absolute difference between the forced-alignment centroids (teacher-forced forward over the true score) and the true onsets;
4. writes the JSON.
No threshold is applied to anything: the file records what the run shows.

    python tools/rendered_corpus_eval.py --room [--model small --steps 200 --batch 32 ...] [--out profiles/rendered_corpus_room.json]

--room replaces 1 to 3: from the same initial weights and on the same training clips one model is trained dry and one with every
clip in its own synthetic room (piano_a2s_amd.room.Room, the default ranges); each model is then scored on the same held-out clips, once dry and
once in their rooms: the teacher-forced loss (its four terms summed, evaluation mode) and the key F1 of greedy decoding."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _batches(ds, batch, workers):
    from torch.utils.data import DataLoader
    return DataLoader(ds, batch_size=batch, shuffle=False, num_workers=workers, drop_last=True)


def _features(batch, dev, front, permute=False, room=None):
    from piano_a2s_amd.render import render
    wave = render(batch[0].to(dev))
    if room is not None:
        from piano_a2s_amd.room import room_seeds
        wave = room.apply(wave, room_seeds(batch[0]))
    x = front(wave)
    if permute:
        x = torch.roll(x, 1, dims=0)                                       # clip b hears clip b - 1
    return [x] + [t.to(dev) for t in batch[1:7]]


def _train(model, ds, args, dev, front, permute, room=None, tag=None):
    from piano_a2s_amd import train
    model.train()
    step = train.TrainStep(model)
    rng = random.Random(args.seed)
    curve, t0 = [], time.perf_counter()
    for k, batch in enumerate(_batches(ds, args.batch, args.workers)):
        terms = step(_features(batch, dev, front, permute, room), args.teacher_forcing, rng=rng)
        if k % args.log_every == 0 or k == args.steps - 1:
            t = terms[:, 0].tolist()
            curve.append({"step": k, "time_sig": t[0], "key": t[1], "upper": t[2], "lower": t[3], "loss": sum(t)})
            print(f"{tag or ('control' if permute else 'matched')} step {k}: loss {sum(t):.4f} (ts {t[0]:.3f} key {t[1]:.3f} up {t[2]:.3f} lo {t[3]:.3f})", flush=True)
    torch.cuda.synchronize()
    return curve, time.perf_counter() - t0


def _unpad_rows(ids):
    from piano_a2s_amd import metrics
    return [metrics.unpad(r).tolist() for r in ids]


def _bar_lines(clip, bars):
    from fractions import Fraction
    from piano_a2s_amd import scoregen
    bar_q = Fraction(scoregen._BAR_UNITS[clip["time_sig"]], 4)
    return [int(clip["lead"] + b * bar_q * clip["spq"]) for b in range(bars + 1)]


def _batch_agreement(ds, first, heard, feats, front, up_ids, lo_ids, ts_ids):
    """Bar agreements of one evaluation batch: clip b of the batch was decoded from the audio of clip first + heard[b] of `ds` (features feats[b]), so
    its decoded bars are laid on THAT clip's bar lines -> (agreements of the decoded scores, of the heard clips' own scores, warped agreements of the
    decoded scores, plain agreements of the decoded scores rendered at the performed timing (section 28)), one entry per bar,
    None where a bar has none."""
    from piano_a2s_amd import resynth, scoregen
    sigs = scoregen.time_signatures()
    dec, gt = [], []
    for b, h in enumerate(heard):
        clip = ds.clip(first + h)
        bars = len(clip["ids"]["upper"])
        lines = _bar_lines(clip, bars)
        ev = resynth.score_events(_unpad_rows(up_ids[b]), _unpad_rows(lo_ids[b]), [sigs[int(t)] for t in ts_ids[b]], lines)[0]
        dec.append({"events": ev, "bar_lines": lines})
        gt.append({"events": resynth.score_events(clip["ids"]["upper"], clip["ids"]["lower"], [clip["time_sig"]] * bars, lines)[0], "bar_lines": lines})
    _, plain, aligned, retimed = resynth.resynthesise(dec, feats, front, scoregen.HOP, align=True, retime=resynth.RETIME_ROUNDS)
    flat = lambda rows: [a for row in rows for a in row]
    moved = flat([[None] * len(p) if r is None else r["agreement"] for p, r in zip(plain, retimed)])
    return (flat(plain), flat(resynth.resynthesise(gt, feats, front, scoregen.HOP)[1]), [None if a is None else a["agreement_warped"] for a in flat(aligned)],
            moved)


def _decode(model, ds, args, dev, front, permute, constrained, K):
    from data_processing.humdrum import LabelsMultiple
    from piano_a2s_amd import kern_grammar, metrics
    inv = LabelsMultiple(extended=True).labels_map_inv
    model.eval()
    model.constrained_decoding, model.beam_size, model.alignment = constrained, K, False
    pred = {k: {} for k in ("up", "lo", "key", "ts")}
    target = {k: {} for k in ("up", "lo", "key", "ts")}
    agr_dec, agr_gt, agr_warped, agr_retimed, first = [], [], [], [], 0
    with torch.no_grad():
        for batch in _batches(ds, args.eval_batch, 0):
            f = _features(batch, dev, front, permute)
            ts_o, key_o, up_o, lo_o = model(f[0], inference=True)
            if constrained or K >= 2:
                up_ids, lo_ids = model.last_decoded["up"][0].cpu().numpy(), model.last_decoded["lo"][0].cpu().numpy()
            else:
                up_ids, lo_ids = up_o.argmax(-1).cpu().numpy(), lo_o.argmax(-1).cpu().numpy()
            if args.resynthesis:
                n = len(batch[7])
                heard = [(b - 1) % n if permute else b for b in range(n)]          # (_features rolls the audio by one clip)
                d, g, w, r = _batch_agreement(ds, first, heard, f[0], front, up_ids, lo_ids, ts_o.argmax(-1).cpu().numpy())
                agr_retimed += r
                agr_dec += d
                agr_gt += g
                agr_warped += w
                first += n
            for b, name in enumerate(batch[7]):
                pred["up"][name], target["up"][name] = _unpad_rows(up_ids[b]), _unpad_rows(batch[3][b].numpy())
                pred["lo"][name], target["lo"][name] = _unpad_rows(lo_ids[b]), _unpad_rows(batch[5][b].numpy())
                pred["key"][name], target["key"][name] = key_o[b].argmax(-1).cpu().tolist(), batch[2][b].tolist()
                pred["ts"][name], target["ts"][name] = ts_o[b].argmax(-1).cpu().tolist(), batch[1][b].tolist()
    model.constrained_decoding, model.beam_size = False, 1
    out = {"WER_upper": metrics.corpus_wer(pred["up"], target["up"], inv)[0], "WER_lower": metrics.corpus_wer(pred["lo"], target["lo"], inv)[0],
           "key_f1": metrics.corpus_f1(pred["key"], target["key"])[0], "time_f1": metrics.corpus_f1(pred["ts"], target["ts"])[0],
           "legal_share_upper": kern_grammar.legal_share(pred["up"]), "legal_share_lower": kern_grammar.legal_share(pred["lo"])}
    if args.note_metrics:
        for staff, k in (("upper", "up"), ("lower", "lo")):
            means = metrics.corpus_note_f1(pred[k], target[k])[0]
            out.update({f"note_f1_{level}_{staff}": means[f"f1_{level}"] for level in ("pitch", "onset", "value")})
            out[f"spelled_share_{staff}"], out[f"overflow_rows_{staff}"] = means["spelled_share"], means["overflow_rows"]
        out["note_f1"] = (out["note_f1_onset_upper"] + out["note_f1_onset_lower"]) / 2
    if args.resynthesis:
        from piano_a2s_amd import resynth
        out["bar_agreement_decoded"], out["bar_agreement_ground_truth"] = resynth.mean_agreement(agr_dec), resynth.mean_agreement(agr_gt)
        out["bar_agreement_warped_decoded"] = resynth.mean_agreement(agr_warped)
        out["bar_agreement_retimed_decoded"] = resynth.mean_agreement(agr_retimed)
        out["bars"], out["bars_without_agreement_decoded"] = len(agr_dec), sum(a is None for a in agr_dec)
    return out


def _alignment_error(model, ds, args, dev, front):
    """Forced alignment of the true score (teacher-forced forward in evaluation mode) against the true onsets: mean |centroid - onset| in seconds."""
    model.eval()
    model.alignment = True
    err = {"bar": [], "upper": [], "lower": []}
    idx = 0
    with torch.no_grad():
        for batch in _batches(ds, args.eval_batch, 0):
            f = _features(batch, dev, front)
            model(f[0], inference=False, ground_truth=f[1:7], teacher_forcing_ratio=1.0)
            al = {k: v["centroid"].cpu().numpy() for k, v in model.last_alignment.items()}
            for b in range(len(batch[7])):
                on = ds.onsets(idx)
                idx += 1
                err["bar"] += [abs(al["bar"][b, i] / 100.0 - t) for i, t in enumerate(on["bar"]) if al["bar"][b, i] >= 0]
                for key, k in (("upper", "up"), ("lower", "lo")):
                    err[key] += [abs(al[k][b, i, j] / 100.0 - t) for i, row in enumerate(on[key]) for j, t in enumerate(row) if al[k][b, i, j] >= 0]
    model.alignment = False
    return {k: (float(np.mean(v)) if v else None) for k, v in err.items()} | {"tokens": len(err["upper"]) + len(err["lower"])}


def _room_score(model, ds, args, dev, front, room):
    """Teacher-forced loss (mean over the batches of the four NLL terms summed, evaluation mode) and key F1 of greedy decoding on the clips of `ds`,
    dry (room None) or each in its own room."""
    import torch.nn.functional as F
    from piano_a2s_amd import metrics
    model.eval()
    model.constrained_decoding, model.beam_size, model.alignment = False, 1, False
    losses, pred, target = [], {}, {}
    flat = lambda o, t: (o.reshape(-1, o.shape[-1]), t.reshape(-1))
    with torch.no_grad():
        for batch in _batches(ds, args.eval_batch, 0):
            f = _features(batch, dev, front, room=room)
            outs = model(f[0], inference=False, ground_truth=f[1:7], teacher_forcing_ratio=1.0)
            targets = (f[1], f[2], f[3], f[5])
            # the recipe's objective (hparams/pretrain.yaml): NLL of the four outputs, the score terms without their padding (id 147)
            losses.append(sum(float(F.nll_loss(*flat(o, t), ignore_index=pad)) for o, t, pad in zip(outs, targets, (-100, -100, 147, 147))))
            key_o = model(f[0], inference=True)[1]
            for b, name in enumerate(batch[7]):
                pred[name], target[name] = key_o[b].argmax(-1).cpu().tolist(), batch[2][b].tolist()
    return {"teacher_forced_loss": float(np.mean(losses)), "key_f1": metrics.corpus_f1(pred, target)[0]}


def _room_runs(args, cfg, init, train_set, held_out, dev, front, res):
    import models
    from piano_a2s_amd import hip
    from piano_a2s_amd.room import Room
    res["room"] = Room().describe()
    for name, trained_in_rooms in (("trained_dry", False), ("trained_in_rooms", True)):
        model = models.ScoreTranscription(**cfg)
        model.load_state_dict(init)
        model = model.to(dev)
        curve, seconds = _train(model, train_set, args, dev, front, False, room=Room() if trained_in_rooms else None, tag=name)
        run = {"loss_curve": curve, "train_seconds": seconds}
        for cond, room in (("held_out_dry", None), ("held_out_in_rooms", Room())):
            run[cond] = _room_score(model, held_out, args, dev, front, room)
            print(name, cond, json.dumps(run[cond]), flush=True)
        res["runs"][name] = run
    res["room_launches"] = hip.room_launches()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("small", "full"), default="small")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--eval_batch", type=int, default=16)
    ap.add_argument("--eval_clips", type=int, default=32)
    ap.add_argument("--frames", type=int, default=1201)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--teacher_forcing", type=float, default=1.0)
    ap.add_argument("--log_every", type=int, default=10)
    ap.add_argument("--no_control", action="store_true")
    ap.add_argument("--note_metrics", action="store_true")
    ap.add_argument("--resynthesis", action="store_true")
    ap.add_argument("--room", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import models
    from datasets.syn import RenderedClips
    from piano_a2s_amd import hip, spec
    from piano_a2s_amd.vqt import VQT
    dev = torch.device("cuda:0")
    cfg = spec.default_cfg() if args.model == "full" else spec.default_cfg(hidden_size=64, conv_feature_size=64)
    front = VQT(dev)
    train_set = RenderedClips(cfg, args.steps * args.batch, seed=args.seed, frames=args.frames)
    held_out = RenderedClips(cfg, args.eval_clips, seed=args.seed + 10_000_000, frames=args.frames)
    res = {"model": args.model, "cfg": {k: cfg[k] for k in ("hidden_size", "conv_feature_size", "max_length", "max_bars")}, "steps": args.steps,
           "batch": args.batch, "frames": args.frames, "eval_clips": args.eval_clips, "teacher_forcing": args.teacher_forcing, "note_metrics": args.note_metrics, "resynthesis": args.resynthesis, "runs": {}}
    torch.manual_seed(args.seed)
    init = {k: v.clone() for k, v in models.ScoreTranscription(**cfg).state_dict().items()}
    if args.room:
        _room_runs(args, cfg, init, train_set, held_out, dev, front, res)
    for name, permute in () if args.room else (("matched", False),) + (() if args.no_control else (("control_permuted_audio", True),)):
        model = models.ScoreTranscription(**cfg)
        model.load_state_dict(init)
        model = model.to(dev)
        curve, seconds = _train(model, train_set, args, dev, front, permute)
        run = {"loss_curve": curve, "train_seconds": seconds, "decoding": {}}
        for tag, constrained, K in (("greedy", False, 1), ("constrained", True, 1), ("beam2", False, 2), ("beam4", False, 4)):
            run["decoding"][tag] = _decode(model, held_out, args, dev, front, permute, constrained, K)
            print(name, tag, json.dumps(run["decoding"][tag]), flush=True)
        if not permute:
            run["forced_alignment_abs_error_s"] = _alignment_error(model, held_out, args, dev, front)
            print(name, "alignment", json.dumps(run["forced_alignment_abs_error_s"]), flush=True)
        res["runs"][name] = run
    res["render_launches"] = hip.render_launches()
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
