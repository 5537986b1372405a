"""Note dynamics by analysis by synthesis, measured on the MI355X: python tools/dynamics_bench.py [out.json] [quick]

1. one round on 256 windows (rendered clips of 1201 frames, a phantom beside every third note), split into render, VQT, a2s_note_levels and
   a2s_note_amp_update: the four take turns call by call in one process, 3 warm-up + 10 timed calls each between device events (median / min / max);
2. the device-side loop of K = 3 (resynth.estimate_dynamics: no host work, no read-back) beside a host-side loop that does the same through a
   read-back of the sums, the numpy float32 update, scoregen.pack_program and an upload per round, taking turns (host clock around work that ends
   in a synchronise): the comparison the update kernel exists for, reported whichever way it comes out;
3. a 10-minute recording (tone bursts, the shipped model size on seeded procedural weights: the cost, not a score): transcribe_waveform with
   resynthesis=True without and with dynamics=True;
4. the table of tools/dynamics_check.py through the GPU path: 12 rendered clips (seeds 100 .. 111), the performance on resynth's instrument and on
   each clip's own drawn one, per round the correlation and rms error against 20 log10(amp), the AUC of real over phantom, the phantoms' median and
   the real notes' 5 % quantile.
Nothing here is a pass / fail number.  `quick`: every section at a small size (a rehearsal of the script, not a measurement)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dtw_oracle, dynamics_oracle as oracle                                          # noqa: E402
from tools.beat_bench import HP, bursts                                                          # noqa: E402
from tools.dynamics_check import performance_program                                             # noqa: E402
from tools.resynth_bench import _clock                                                           # noqa: E402
from tools.transpose_augment_bench import _alternating, _stats                                   # noqa: E402


def _scenarios(n_clips, frames, first_clip=100, seed=26):
    from piano_a2s_amd import scoregen, spec
    cfg = spec.default_cfg(max_length=(200, 200))
    rng = np.random.default_rng(seed)
    out = []
    for s in range(first_clip, first_clip + n_clips):
        clip = scoregen.make_clip(cfg, s, frames=frames)
        scn = oracle.scenario(clip, rng, 3)
        scn["clip"], scn["lines"] = clip, dtw_oracle.clip_lines(clip, cfg["max_bars"])
        out.append(scn)
    return out


def _setup(dev, scns, frames, instrument="resynth"):
    """-> (vqt, x3 the performances' features, the score programs on the host (B, 512, 8), the host note table and offsets, n_samples)."""
    from piano_a2s_amd import render, resynth, scoregen, transcribe
    n_samples = (frames - 1) * scoregen.HOP
    vqt = transcribe._vqt(dev, dict(HP, max_frame_num=frames))
    perf = np.stack([performance_program(s["events"], s["amps"], n_samples, s["clip"], instrument) for s in scns])
    x = vqt(render.render(torch.from_numpy(perf).to(dev), n_samples))
    x3 = (x[:, 0] if x.dim() == 4 else x).contiguous()
    progs = np.stack([resynth.program(s["score"], n_samples) for s in scns])
    table = np.concatenate([resynth.note_rows(s["score"], None, scoregen.HOP, frames, x3.shape[2], clip=i) for i, s in enumerate(scns)])
    first = np.concatenate([[0], np.cumsum([len(s["score"]) for s in scns])])
    return vqt, x3, progs, table, first, n_samples


def round_split(dev, scns, frames):
    from piano_a2s_amd import hip, render, resynth
    vqt, x3, progs, table, first, n_samples = _setup(dev, scns, frames)
    pd = torch.from_numpy(progs).to(dev)
    rows, fd = hip.note_table(table, first, len(scns), progs.shape[1], dev)
    wave = render.render(pd, n_samples)
    y = vqt(wave)
    y3 = y[:, 0] if y.dim() == 4 else y
    sums = hip.note_levels(x3, y3, rows)
    cum = torch.zeros(len(table), device=dev)
    fns = [lambda: hip.render_notes(pd, n_samples, wave), lambda: vqt(wave), lambda: hip.note_levels(x3, y3, rows, out=sums),
           lambda: hip.note_amp_update(sums, rows, fd, cum, pd, resynth.RESYNTH_AMP)]
    ms = [_stats(m) for m in _alternating(fns)]
    cells = float(sums[:, 2].sum())
    res = {"windows": len(scns), "frames": frames, "freq_bins": int(x3.shape[2]), "note_rows": len(table), "cells": cells,
           "render_ms": ms[0], "vqt_ms": ms[1], "note_levels_ms": ms[2], "note_amp_update_ms": ms[3],
           "note_levels_bytes_read": 2 * 4 * cells + 32 * len(table), "round_ms_sum_of_medians": sum(m["median"] for m in ms)}
    return res


def loops(dev, scns, frames, rounds=3):
    from piano_a2s_amd import hip, render, resynth
    vqt, x3, progs, table, first, n_samples = _setup(dev, scns, frames)
    rows, fd = hip.note_table(table, first, len(scns), progs.shape[1], dev)

    def device_loop():
        return resynth.estimate_dynamics(torch.from_numpy(progs).to(dev), x3, vqt, n_samples, rows, fd, rounds).cpu().numpy()

    def host_loop():
        cum, p = np.zeros(len(table), dtype=np.float32), progs
        for _ in range(rounds):
            y = vqt(render.render(torch.from_numpy(p).to(dev), n_samples))
            sums = hip.note_levels(x3, y[:, 0] if y.dim() == 4 else y, rows).cpu().numpy()
            cum = oracle.update_f32(sums, first, cum)
            amps = resynth.RESYNTH_AMP * 10.0 ** (cum.astype(np.float64) / 20.0)
            p = np.stack([resynth.program(s["score"], n_samples, amps=amps[first[i]:first[i + 1]]) for i, s in enumerate(scns)])
        return cum

    a, b = device_loop(), host_loop()                                                            # untimed
    dev_ms, host_ms = [], []
    for _ in range(5):
        dev_ms.append(_clock(device_loop)[1])
        host_ms.append(_clock(host_loop)[1])
    return {"windows": len(scns), "rounds": rounds, "note_rows": len(table), "device_loop_ms": _stats(dev_ms), "host_loop_ms": _stats(host_ms),
            "host_over_device": float(np.median(host_ms) / np.median(dev_ms)), "largest_level_difference_db": float(np.abs(a - b).max()),
            "note": "both include the upload of the first programs and one read-back of the levels; the host loop packs with pack_program's gain rule "
                    "every round, the device loop keeps the first pack's gain (the features are normalised to the window's peak)"}


def recording(dev, seconds):
    import models
    from piano_a2s_amd import spec, transcribe
    wave, _, _ = bursts(seconds)
    downbeats = [float(t) for t in np.arange(0.25, seconds - 1.0, 2.0)]
    model = models.ScoreTranscription()
    model.load_state_dict(spec.procedural_state(spec.default_cfg(), 11, eos_bias=3.0, lively=True))
    model = model.to(dev).eval()
    model.constrained_decoding = True                                                            # (untrained weights write notes only under the grammar)
    short = [d for d in downbeats if d < 24]
    transcribe.transcribe_waveform(model, wave[:16000 * 24], 16000, downbeats=short, hparams=HP, resynthesis=True, dynamics=True)      # untimed
    off, on = [], []
    for _ in range(3):
        _, ms0 = _clock(lambda: transcribe.transcribe_waveform(model, wave, 16000, downbeats=downbeats, hparams=HP, resynthesis=True))
        r1, ms1 = _clock(lambda: transcribe.transcribe_waveform(model, wave, 16000, downbeats=downbeats, hparams=HP, resynthesis=True, dynamics=True))
        off.append(ms0)
        on.append(ms1)
    bars = [b for w in r1["windows"] for b in w["bars"]]
    agr = [(b["agreement"], b["agreement_dynamics"]) for b in bars if b["agreement"] is not None and b["agreement_dynamics"] is not None]
    out = {"seconds": seconds, "windows": len(r1["windows"]), "bars": len(bars), "notes": sum(len(b["notes"]) for b in bars), "decoding": "constrained greedy, batch 16",
           "transcribe_with_resynthesis_ms": _stats(off), "transcribe_with_dynamics_ms": _stats(on),
           "mean_agreement": float(np.mean([a for a, _ in agr])) if agr else None, "mean_agreement_dynamics": float(np.mean([d for _, d in agr])) if agr else None}
    out["dynamics_extra_ms_median"] = out["transcribe_with_dynamics_ms"]["median"] - out["transcribe_with_resynthesis_ms"]["median"]
    return out


def check_table(dev, n_clips, frames, rounds=3):
    """tools/dynamics_check.py's table with the GPU render, VQT and kernels in place of the float64 definitions."""
    from piano_a2s_amd import resynth, scoregen
    scns = _scenarios(n_clips, frames)
    out = []
    for instrument in ("resynth", "own"):
        vqt, x3, _, _, _, _ = _setup(dev, scns, frames, instrument)
        windows = [{"events": s["score"], "bar_lines": s["lines"]} for s in scns]
        for K in range(1, rounds + 1):
            dyn = resynth.resynthesise(windows, x3, vqt, scoregen.HOP, dynamics=K)[2]
            got, true, real = [], [], []
            for d, s in zip(dyn, scns):
                r, cum = s["real"], d["level_db"].astype(np.float64)
                got.append(cum - cum[r].mean())
                true.append(s["true_db"] - s["true_db"][r].mean())
                real.append(r)
            got, true, real = np.concatenate(got), np.concatenate(true), np.concatenate(real)
            err = got[real] - true[real]
            out.append({"instrument": instrument, "rounds": K, "notes": int(real.sum()), "phantoms": int((~real).sum()),
                        "correlation": float(np.corrcoef(got[real], true[real])[0, 1]), "rms_error_db": float(np.sqrt(np.mean(err * err))),
                        "auc_real_over_phantom": oracle.auc(got[real], got[~real]), "phantom_median_db": float(np.median(got[~real])),
                        "real_quantile_05_db": float(np.quantile(got[real], 0.05))})
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dynamics.json")
    quick = len(sys.argv) > 2 and sys.argv[2] == "quick"
    if not torch.cuda.is_available():
        raise SystemExit("dynamics_bench: needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    B, frames, seconds, n_clips = (8, 301, 30.0, 4) if quick else (256, 1201, 600.0, 12)
    res = {"device": torch.cuda.get_device_name(0), "quick": quick}
    scns = _scenarios(B, frames)
    res["one_round"] = round_split(dev, scns, frames)
    res["loops"] = loops(dev, scns, frames)
    del scns
    res["check_table"] = check_table(dev, n_clips, 1201)
    res["recording"] = recording(dev, seconds)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
