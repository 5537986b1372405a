"""Resynthesis and bar agreement, measured on the MI355X: python tools/resynth_bench.py [out.json] [quick]

1. kernel: a2s_segment_agreement (the two launches of one call, table already on the device) on 256 windows x 5 bars of 1201 x 480 features, ALTERNATING
   in one process with a2s_onset_strength on one of the two tensors and with a plain-torch restatement (slice, multiply, sum) on the same tensors
   (3 warm-up + 10 timed calls each between device events; median / min / max; bytes the algorithm needs, TB/s, share of the 8 TB/s roof); the same
   call on ONE window's 5 bars (what a short recording gives), and hip.segment_agreement as the host calls it (table check and upload included);
2. a 10-minute recording (tone bursts, the shipped model size on seeded procedural weights: the cost, not a score): transcribe_waveform with given
   downbeats without and with resynthesis=True (host clock around work that ends in a read-back), and resynth.resynthesise alone on the windows of one
   batch (render + VQT + agreement);
3. the own / other / mutated table on the device: N rendered clips of scoregen at 1201 frames; per bar the agreement of the clip's features with the
   resynthesis of its OWN score, of the NEXT clip's score on the same bar grid, and of its own score with 25 % of the notes moved by +-1 .. 2 semitones.
Nothing here is a pass / fail number.  `quick`: every section at a small size (a rehearsal of the script, not a measurement)."""
import json
import os
import sys
import time
from fractions import Fraction

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.beat_bench import HP, bursts                                                          # noqa: E402
from tools.transpose_augment_bench import HBM_ROOF_GBS, _alternating, _stats, _timed          # noqa: E402


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def kernel_times(dev, B, rows, bars=5, F=480):
    from piano_a2s_amd import hip
    Lib = hip.lib()
    x = torch.rand(B, rows, F, device=dev).clamp_(min=0.33)
    y = torch.rand(B, rows, F, device=dev)
    per = (rows - 1) // bars
    table = np.array([(b, i * per, (i + 1) * per, 0) for b in range(B) for i in range(bars)], dtype=np.int32)
    seg = torch.from_numpy(table).to(dev)
    out = torch.empty((len(table), 5), dtype=torch.float64, device=dev)
    n_rows = torch.full((B,), rows, dtype=torch.int32, device=dev)
    ef, el = torch.empty((B, rows), device=dev), torch.empty((B, rows), device=dev)

    def agree(S=len(table)):
        hip.check(Lib.a2s_segment_agreement(hip.stream(), hip._p(x), hip._p(y), rows * F, B, rows, F, hip._p(seg), S, hip._p(out)), "a2s_segment_agreement")

    def plain():
        xs, ys = x[:, :bars * per].reshape(B, bars, -1), y[:, :bars * per].reshape(B, bars, -1)
        return torch.stack([xs.sum(-1), ys.sum(-1), (xs * xs).sum(-1), (ys * ys).sum(-1), (xs * ys).sum(-1)], dim=-1)

    a, o, p = (_stats(ms) for ms in _alternating([agree, lambda: hip.onset_strength(x, n_rows, 1, 180, env_full=ef, env_low=el), plain]))
    cells = B * bars * per * F
    need = {"segment_agreement": 2 * cells * 4 + len(table) * (16 + 40), "onset_strength": x.numel() * 4 + 2 * B * rows * 4, "plain_torch": 2 * cells * 4}
    res = {"windows": B, "rows": rows, "freq_bins": F, "bars_per_window": bars, "frames_per_bar": per, "segments": len(table), "feature_bytes_both": 2 * x.numel() * 4,
           "partial_cells": hip.agreement_partial_cells()}
    for name, ms in (("segment_agreement", a), ("onset_strength", o), ("plain_torch", p)):
        tbs = need[name] / (ms["median"] * 1e-3) / 1e12
        res[name] = {"ms": ms, "bytes_needed": need[name], "tb_per_s": tbs, "share_of_8tb_roof": tbs * 1e3 / HBM_ROOF_GBS}
    res["plain_torch"]["note"] = "bytes_needed counts one read of the cells; the restatement reads them several times and writes three products"
    got = out.cpu().numpy()
    ref = plain().double().cpu().numpy().reshape(-1, 5)
    res["max_rel_diff_kernel_vs_plain_torch_fp32"] = float((np.abs(got - ref) / np.maximum(np.abs(got), 1e-300)).max())
    res["one_window_5_segments"] = {"ms": _stats(_timed(lambda: agree(bars))), "bytes_needed": 2 * bars * per * F * 4}
    res["wrapper_with_table_upload"] = {"ms": _stats(_timed(lambda: hip.segment_agreement(x, y, table)))}
    return res


def recording(dev, seconds):
    import models
    from piano_a2s_amd import resynth, spec, transcribe
    wave, times, bass = bursts(seconds)
    downbeats = [float(t) for t in np.arange(0.25, seconds - 1.0, 2.0)]
    model = models.ScoreTranscription()
    model.load_state_dict(spec.procedural_state(spec.default_cfg(), 11, eos_bias=3.0, lively=True))
    model = model.to(dev).eval()
    model.constrained_decoding = True                                                            # (untrained weights write notes only under the grammar)
    short = [d for d in downbeats if d < 24]
    transcribe.transcribe_waveform(model, wave[:16000 * 24], 16000, downbeats=short, hparams=HP, resynthesis=True)          # untimed: banks, first launches
    off, on = [], []
    for _ in range(3):
        r0, ms0 = _clock(lambda: transcribe.transcribe_waveform(model, wave, 16000, downbeats=downbeats, hparams=HP))
        r1, ms1 = _clock(lambda: transcribe.transcribe_waveform(model, wave, 16000, downbeats=downbeats, hparams=HP, resynthesis=True))
        off.append(ms0)
        on.append(ms1)
    out = {"seconds": seconds, "windows": len(r1["windows"]), "bars": sum(len(w["bars"]) for w in r1["windows"]),
           "notes": sum(len(b["notes"]) for w in r1["windows"] for b in w["bars"]),
           "bars_with_an_agreement": sum(b["agreement"] is not None for w in r1["windows"] for b in w["bars"]),
           "decoding": "constrained greedy, batch 16", "transcribe_ms": _stats(off), "transcribe_with_resynthesis_ms": _stats(on)}
    out["resynthesis_extra_ms_median"] = out["transcribe_with_resynthesis_ms"]["median"] - out["transcribe_ms"]["median"]
    # one batch of 16 windows alone: render + VQT + agreement + read-back
    vqt = transcribe._vqt(dev, HP)
    feats = torch.rand(16, 1, 1201, 480, device=dev)
    rng = np.random.default_rng(3)
    windows = []
    for _ in range(16):
        on_ = np.sort(rng.integers(0, 150000, size=60))
        ev = np.stack([on_, rng.integers(2000, 16000, size=60), rng.integers(36, 96, size=60)], axis=1).astype(np.int64)
        windows.append({"events": ev, "bar_lines": [0, 32000, 64000, 96000, 128000, 160000]})
    resynth.resynthesise(windows, feats, vqt, 160)
    out["resynthesise_one_batch_of_16_ms"] = _stats([_clock(lambda: resynth.resynthesise(windows, feats, vqt, 160))[1] for _ in range(5)])
    return out


def _lines(clip, bars):
    from piano_a2s_amd import scoregen
    bar_q = Fraction(scoregen._BAR_UNITS[clip["time_sig"]], 4)
    return [int(clip["lead"] + b * bar_q * clip["spq"]) for b in range(bars + 1)]


def own_other_mutated(dev, n_clips, frames=1201):
    from piano_a2s_amd import render, resynth, scoregen, spec, transcribe
    cfg = spec.default_cfg(max_length=(200, 200))
    bars = cfg["max_bars"]
    clips = [scoregen.make_clip(cfg, 100 + i, frames=frames) for i in range(n_clips)]
    hp = dict(HP, max_frame_num=frames)
    vqt = transcribe._vqt(dev, hp)
    x = vqt(render.render(torch.from_numpy(np.stack([scoregen.pack_program(c) for c in clips])).to(dev)))
    rng = np.random.default_rng(9)
    agr, touched = {}, []
    for which in ("own", "other", "mutated"):
        windows = []
        for i, clip in enumerate(clips):
            src = clips[(i + 1) % n_clips] if which == "other" else clip
            ev, _ = resynth.score_events(src["ids"]["upper"], src["ids"]["lower"], [src["time_sig"]] * bars, _lines(clip, bars))
            if which == "mutated":
                ev = ev.copy()
                pick = rng.random(len(ev)) < 0.25
                ev[pick, 2] += rng.choice([-2, -1, 1, 2], size=int(pick.sum()))
                lines = _lines(clip, bars)
                touched.append([bool(((ev[pick, 0] >= lines[b]) & (ev[pick, 0] < lines[b + 1])).any()) for b in range(bars)])
            windows.append({"events": ev, "bar_lines": _lines(clip, bars)})
        agr[which] = np.array(resynth.resynthesise(windows, x, vqt, scoregen.HOP)[1], dtype=np.float64)
    own, other, mut, touched = agr["own"], agr["other"], agr["mutated"], np.array(touched)
    drop = own.mean(axis=1) - mut.mean(axis=1)
    return {"clips": n_clips, "frames": frames, "seeds": [100, 100 + n_clips - 1], "bars": int(own.size), "instrument": dict(resynth.RESYNTH_INSTRUMENT, amp=resynth.RESYNTH_AMP),
            "own": {"min": float(own.min()), "max": float(own.max()), "mean": float(own.mean())},
            "other": {"min": float(other.min()), "max": float(other.max()), "mean": float(other.mean())},
            "bars_where_own_beats_other": int((own > other).sum()), "smallest_gap_own_minus_other": float((own - other).min()),
            "mutated": {"share_of_notes_moved": 0.25, "semitones": [-2, -1, 1, 2], "clips_whose_mean_drops": int((drop > 0).sum()), "smallest_drop_of_a_clip_mean": float(drop.min()),
                        "mean_drop_of_a_clip_mean": float(drop.mean()), "touched_bars": int(touched.sum()),
                        "touched_bars_that_drop": int(((own - mut > 0) & touched).sum()),
                        "largest_change_of_an_untouched_bar": float(np.abs(own - mut)[~touched].max()) if (~touched).any() else None}}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "resynthesis.json")
    quick = len(sys.argv) > 2 and sys.argv[2] == "quick"
    if not torch.cuda.is_available():
        raise SystemExit("resynth_bench: needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    B, rows, seconds, n_clips = (8, 201, 30.0, 4) if quick else (256, 1201, 600.0, 24)
    res = {"device": torch.cuda.get_device_name(0), "quick": quick}
    res["kernel"] = kernel_times(dev, B, rows)
    res["own_other_mutated"] = own_other_mutated(dev, n_clips)
    res["recording"] = recording(dev, seconds)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
