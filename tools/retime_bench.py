"""Resynthesis at the performed timing, measured on the MI355X: python tools/retime_bench.py [out.json] [quick]

1. one timing round on 256 windows x 5 bars of 240 frames (rendered clips of 1201 frames, every bar warped by u + 0.15 sin(pi u)), split into render,
   VQT, agreement, DTW, a2s_path_warp and a2s_retime_events: the six take turns call by call in one process, 3 warm-up + 10 timed calls each between
   device events (median / min / max);
2. the device loop of R rounds (resynth.refine_timing: no per-note host work, one read-back) beside the host route that does the same through a
   read-back of the paths, resynth.warp_from_path per bar, resynth.performed_notes per note, resynth.program and an upload per round, taking turns
   (host clock around work that ends in a synchronise), reported whichever way it comes out;
3. a 10-minute recording (tone bursts, the shipped model size on seeded procedural weights: the cost, not a score): transcribe_waveform with
   align_notes=True without and with performed_timing=2;
4. the table of tools/retime_check.py through the GPU path: the eight clips of tests/test_gpu_retime.py, per round the median and 90 % onset error of
   the retimed notes and the mean plain agreement of the retimed render.
The result is written under the key "gpu" of the JSON file, whose other keys (the float64 table of tools/retime_check.py under "definition") stay.
Nothing here is a pass / fail number.  `quick`: every section at a small size (a rehearsal of the script, not a measurement)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dtw_oracle                                                                     # noqa: E402
from tools.beat_bench import HP, bursts                                                          # noqa: E402
from tools.resynth_bench import _clock                                                           # noqa: E402
from tools.retime_check import paired                                                            # noqa: E402
from tools.transpose_augment_bench import _alternating, _stats                                   # noqa: E402


def _scenarios(n_clips, frames, first_clip=100, seed=25, amp=0.15):
    from piano_a2s_amd import scoregen, spec
    cfg = spec.default_cfg(max_length=(200, 200))
    rng = np.random.default_rng(seed)
    return [dtw_oracle.warped_clip(scoregen.make_clip(cfg, s, frames=frames), cfg["max_bars"], amp, rng) for s in range(first_clip, first_clip + n_clips)]


def _setup(dev, scns, frames):
    """-> (vqt, x3 the performances' features, the straight programs on the host, the aligned bars' host table, the host event rows, n_samples)."""
    from piano_a2s_amd import render, resynth, scoregen, transcribe
    n_samples = (frames - 1) * scoregen.HOP
    vqt = transcribe._vqt(dev, dict(HP, max_frame_num=frames))
    x = vqt(render.render(torch.from_numpy(np.stack([resynth.program(s["warped"], n_samples) for s in scns])).to(dev), n_samples))
    x3 = (x[:, 0] if x.dim() == 4 else x).contiguous()
    progs = np.stack([resynth.program(s["straight"], n_samples) for s in scns])
    seg, where = resynth.bar_segments([{"events": s["straight"], "bar_lines": s["lines"]} for s in scns], scoregen.HOP, frames)
    table = np.array([[c, f0, f1, resynth.dtw_band(f1 - f0)] for c, f0, f1 in seg], dtype=np.int64)
    seg_of = {w: k for k, w in enumerate(where)}
    rows = np.concatenate([resynth.event_rows(s["straight"], s["lines"], [seg_of[(i, b)] for b in range(len(s["lines"]) - 1)], clip=i) for i, s in enumerate(scns)])
    return vqt, x3, progs, table, rows, n_samples


def _first_pass(x3, y3, table):
    from piano_a2s_amd import hip
    sums = hip.segment_agreement(x3, y3, table)
    cells = torch.from_numpy(((table[:, 2] - table[:, 1]) * x3.shape[2]).astype(np.float64)).to(x3.device)
    return hip.dtw_segments(x3, y3, table, ((sums[:, 0] - sums[:, 1]) / cells).to(torch.float32))


def round_split(dev, scns, frames):
    from piano_a2s_amd import hip, render, scoregen
    vqt, x3, progs, table, rows, n_samples = _setup(dev, scns, frames)
    pd = torch.from_numpy(progs).to(dev)
    events = hip.event_table(rows, len(scns), progs.shape[1], table, dev)
    td = torch.from_numpy(table.astype(np.int32)).to(dev)
    n_max = int((table[:, 2] - table[:, 1]).max())
    wave = render.render(pd, n_samples)
    y = vqt(wave)
    y3 = (y[:, 0] if y.dim() == 4 else y).contiguous()
    paths, steps, _ = _first_pass(x3, y3, table)
    warp2, _ = hip.path_warp(paths, steps, td, n_max, inverse=False)
    scratch = pd.clone()                                                                         # (retiming moves the events it is given: a copy per call keeps the work the same)
    fns = [lambda: hip.render_notes(pd, n_samples, wave), lambda: vqt(wave), lambda: hip.segment_agreement(x3, y3, table), lambda: hip.dtw_segments(x3, y3, table),
           lambda: hip.path_warp(paths, steps, td, n_max, inverse=False), lambda: hip.retime_events(warp2, td, events, scoregen.HOP, scratch.copy_(pd))]
    ms = [_stats(m) for m in _alternating(fns)]
    return {"windows": len(scns), "frames": frames, "segments": int(len(table)), "segment_frames_max": n_max, "events": int(len(rows)),
            "path_cells": int(steps.sum()), "render_ms": ms[0], "vqt_ms": ms[1], "agreement_ms": ms[2], "dtw_ms": ms[3], "path_warp_ms": ms[4],
            "retime_events_with_program_copy_ms": ms[5], "round_ms_sum_of_medians": sum(m["median"] for m in ms),
            "note": "agreement and dtw include the upload of their host table; retime_events includes a device copy of the programs (B x 512 x 8 int32)"}


def loops(dev, scns, frames, rounds):
    from piano_a2s_amd import hip, render, resynth, scoregen
    vqt, x3, progs, table, rows, n_samples = _setup(dev, scns, frames)
    hop = scoregen.HOP
    bar_of = [np.clip(np.searchsorted(np.asarray(s["lines"]), s["straight"][:, 0], side="right") - 1, 0, len(s["lines"]) - 2) for s in scns]
    seg_at = {(int(c), int(f0)): k for k, (c, f0, _, _) in enumerate(table)}

    def start():
        pd = torch.from_numpy(progs).to(dev)
        y = vqt(render.render(pd, n_samples))
        return pd, (y[:, 0] if y.dim() == 4 else y).contiguous()

    def device_loop():
        pd, y3 = start()
        paths, steps, _ = _first_pass(x3, y3, table)
        events = hip.event_table(rows, len(scns), progs.shape[1], table, dev)
        return resynth.refine_timing(pd, x3, vqt, n_samples, hop, table, events, paths, steps, rounds)[:, :, 0]

    def host_loop():
        pd, y3 = start()
        events = [s["straight"].copy() for s in scns]
        for k in range(rounds):
            if k:
                y = vqt(render.render(torch.from_numpy(np.stack([resynth.program(ev, n_samples) for ev in events])).to(dev), n_samples))
                y3 = (y[:, 0] if y.dim() == 4 else y).contiguous()
            paths, steps, _ = (t.cpu().numpy() for t in _first_pass(x3, y3, table))
            for i, s in enumerate(scns):
                lines = s["lines"]
                for b in range(len(lines) - 1):
                    t = seg_at[(i, lines[b] // hop)]
                    warp, _ = resynth.warp_from_path(paths[t, :steps[t]], int(table[t, 2] - table[t, 1]))
                    sel = np.nonzero(bar_of[i] == b)[0]
                    moved = resynth.performed_notes(events[i][sel], warp, int(table[t, 1]), hop, lines[b], lines[b + 1])
                    events[i][sel, 0] = [int(np.floor(m[0])) for m in moved]
                    events[i][sel, 1] = [max(1, int(np.floor(m[0] + m[1])) - int(np.floor(m[0]))) for m in moved]
        out = np.zeros((len(scns), progs.shape[1]), dtype=np.int64)
        for i, ev in enumerate(events):
            out[i, 1:1 + len(ev)] = ev[:, 0]
        return out

    a, b = device_loop(), host_loop()                                                            # untimed
    n = [len(s["straight"]) for s in scns]
    diff = max(int(np.abs(a[i, 1:1 + n[i]] - b[i, 1:1 + n[i]]).max()) for i in range(len(scns)))
    dev_ms, host_ms = [], []
    for _ in range(5):
        dev_ms.append(_clock(device_loop)[1])
        host_ms.append(_clock(host_loop)[1])
    return {"windows": len(scns), "rounds": rounds, "events": int(sum(n)), "device_loop_ms": _stats(dev_ms), "host_loop_ms": _stats(host_ms),
            "host_over_device": float(np.median(host_ms) / np.median(dev_ms)), "largest_onset_difference_samples": diff,
            "note": "both include the upload of the first programs, their render and VQT, the first alignment pass and one read-back of the onsets; the "
                    "host route floors the float performed_notes, the device rounds in integers: onsets may differ by a sample per round"}


def recording(dev, seconds, rounds):
    import models
    from piano_a2s_amd import spec, transcribe
    wave, _, _ = bursts(seconds)
    downbeats = [float(t) for t in np.arange(0.25, seconds - 1.0, 2.0)]
    model = models.ScoreTranscription()
    model.load_state_dict(spec.procedural_state(spec.default_cfg(), 11, eos_bias=3.0, lively=True))
    model = model.to(dev).eval()
    model.constrained_decoding = True                                                            # (untrained weights write notes only under the grammar)
    kw = dict(hparams=HP, resynthesis=True, align_notes=True)
    transcribe.transcribe_waveform(model, wave[:16000 * 24], 16000, downbeats=[d for d in downbeats if d < 24], performed_timing=rounds, **kw)      # untimed
    off, on = [], []
    for _ in range(3):
        _, ms0 = _clock(lambda: transcribe.transcribe_waveform(model, wave, 16000, downbeats=downbeats, **kw))
        r1, ms1 = _clock(lambda: transcribe.transcribe_waveform(model, wave, 16000, downbeats=downbeats, performed_timing=rounds, **kw))
        off.append(ms0)
        on.append(ms1)
    bars = [b for w in r1["windows"] for b in w["bars"]]
    agr = [(b["agreement"], b["agreement_warped"], b["agreement_retimed"]) for b in bars if b["agreement_retimed"] is not None and b["agreement_warped"] is not None]
    out = {"seconds": seconds, "rounds": rounds, "windows": len(r1["windows"]), "bars": len(bars), "notes": sum(len(b["notes"]) for b in bars),
           "decoding": "constrained greedy, batch 16", "transcribe_with_align_notes_ms": _stats(off), "transcribe_with_performed_timing_ms": _stats(on)}
    for k, name in enumerate(("mean_agreement", "mean_agreement_warped", "mean_agreement_retimed")):
        out[name] = float(np.mean([a[k] for a in agr])) if agr else None
    out["performed_timing_extra_ms_median"] = out["transcribe_with_performed_timing_ms"]["median"] - out["transcribe_with_align_notes_ms"]["median"]
    return out


def check_table(dev, n_clips, frames, rounds=3):
    """tools/retime_check.py's table with the GPU render, VQT and kernels in place of the float64 definitions."""
    from piano_a2s_amd import render, resynth, scoregen, transcribe
    scns = _scenarios(n_clips, frames)
    n_samples, ms = (frames - 1) * scoregen.HOP, 1e3 / scoregen.SR
    vqt = transcribe._vqt(dev, dict(HP, max_frame_num=frames))
    x = vqt(render.render(torch.from_numpy(np.stack([resynth.program(s["warped"], n_samples) for s in scns])).to(dev), n_samples))
    windows = [{"events": s["straight"], "bar_lines": s["lines"]} for s in scns]
    truth = [paired(s)[1] for s in scns]
    out = []
    for R in range(1, rounds + 1):
        _, plain, aligned, retimed = resynth.resynthesise(windows, x, vqt, scoregen.HOP, align=True, retime=R)
        err = np.concatenate([np.abs(rt["events"][:, 0] - t[:, 0]) for rt, t in zip(retimed, truth)])
        out.append({"rounds": R, "notes": int(len(err)), "median_error_ms": float(np.median(err) * ms), "p90_error_ms": float(np.quantile(err, 0.9) * ms),
                    "mean_error_ms": float(err.mean() * ms), "mean_agreement_retimed": float(np.mean([a for rt in retimed for a in rt["agreement"] if a is not None])),
                    "mean_agreement_straight": float(np.mean([a for w in plain for a in w if a is not None])),
                    "mean_agreement_warped": float(np.mean([a["agreement_warped"] for w in aligned for a in w if a is not None]))})
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "retime.json")
    quick = len(sys.argv) > 2 and sys.argv[2] == "quick"
    if not torch.cuda.is_available():
        raise SystemExit("retime_bench: needs the GPU (there is no CPU path to time)")
    from piano_a2s_amd import resynth
    dev = torch.device("cuda:0")
    B, frames, seconds, n_clips = (8, 1201, 30.0, 2) if quick else (256, 1201, 600.0, 8)
    res = {"device": torch.cuda.get_device_name(0), "quick": quick}
    res["check_table"] = check_table(dev, n_clips, 1201)
    scns = _scenarios(B, frames)
    res["one_round"] = round_split(dev, scns, frames)
    res["loops"] = loops(dev, scns, frames, resynth.RETIME_ROUNDS)
    del scns
    res["recording"] = recording(dev, seconds, resynth.RETIME_ROUNDS)
    print(json.dumps(res))
    whole = {}
    if os.path.exists(path):
        with open(path) as f:
            whole = json.load(f)
    whole["gpu"] = res
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(whole, f, indent=1)


if __name__ == "__main__":
    main()
