"""Bar-wise alignment of the resynthesis, measured on the MI355X: python tools/dtw_bench.py [out.json] [quick]

1. kernels: a2s_dtw_cost on 256 windows x 5 bars of 240 frames x 480 bins (T = 1201), with the band the host uses (r = 60) and without one, ALTERNATING in
   one process with a torch.cdist restatement (squared) of the unbanded costs (3 warm-up + 10 timed calls each between device events; median / min /
   max); the FMAs of the definition (cells inside the band x F), FLOP/s at 2 per FMA and the share of the 157.3 TFLOP/s fp32 vector roof -- the kernel
   issues three vector operations per term (two subtractions and the FMA), so a third of the roof is its ceiling in these units; a2s_dtw_path on the
   same tables and on ONE segment of 1201 frames (2401 anti-diagonals, one barrier each);
2. a 10-minute recording (tone bursts, the shipped model size on seeded procedural weights: the cost, not a score): transcribe_waveform with
   resynthesis=True without and with align_notes=True (host clock around work that ends in a read-back);
3. the own / other / mutated table of section 24 with the plain and the warped agreement, on straight renders and on renders warped inside every bar
   by g(u) = u + a sin(pi u), |a| = 0.15;
4. the onset errors of linear placement and of the warp on warped renders, |a| = 0.05, 0.10, 0.15 (medians and 90th percentiles over all notes, and
   the ratio of the medians).
Nothing here is a pass / fail number.  `quick`: every section at a small size (a rehearsal of the script, not a measurement)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import dtw_oracle as oracle                                                          # noqa: E402
from tools.beat_bench import HP, bursts                                                          # noqa: E402
from tools.resynth_bench import _clock                                                           # noqa: E402
from tools.transpose_augment_bench import _alternating, _stats, _timed                           # noqa: E402

FP32_ROOF = 157.3e12


def kernel_times(dev, B, rows, bars=5, F=480):
    from piano_a2s_amd import hip, resynth
    Lib, st = hip.lib(), hip.stream()
    x, y = torch.rand(B, rows, F, device=dev), torch.rand(B, rows, F, device=dev)
    per = (rows - 1) // bars
    r = resynth.dtw_band(per)
    res = {"windows": B, "rows": rows, "freq_bins": F, "bars_per_window": bars, "frames_per_bar": per, "segments": B * bars, "band": r}
    runs = {}
    for name, band in (("banded", r), ("unbanded", -1)):
        table = np.array([(b, i * per, (i + 1) * per, band) for b in range(B) for i in range(bars)], dtype=np.int64)
        n_max, r_max = hip.dtw_geometry(table)
        S = len(table)
        seg = torch.from_numpy(table.astype(np.int32)).to(dev)
        off = torch.full((S,), 0.01, device=dev)
        cb, wb = int(Lib.a2s_dtw_cost_bytes(S, n_max, r_max)), int(Lib.a2s_dtw_workspace_bytes(S, n_max, r_max))
        cost, ws = torch.zeros(cb // 4, device=dev), torch.zeros(wb, dtype=torch.uint8, device=dev)
        paths = torch.zeros((S, 2 * n_max - 1), dtype=torch.int32, device=dev)
        steps, total = torch.zeros(S, dtype=torch.int32, device=dev), torch.zeros(S, device=dev)

        def run_cost(seg=seg, S=S, off=off, n_max=n_max, r_max=r_max, cost=cost, cb=cb):
            hip.check(Lib.a2s_dtw_cost(st, hip._p(x), hip._p(y), rows * F, B, rows, F, hip._p(seg), S, hip._p(off), n_max, r_max, hip._p(cost), cb), "a2s_dtw_cost")

        def run_path(seg=seg, S=S, n_max=n_max, r_max=r_max, cost=cost, cb=cb, ws=ws, wb=wb, paths=paths, steps=steps, total=total):
            hip.check(Lib.a2s_dtw_path(st, hip._p(seg), S, B, rows, n_max, r_max, hip._p(cost), cb, hip._p(ws), wb, hip._p(paths), hip._p(steps), hip._p(total)), "a2s_dtw_path")

        cells = int(oracle.band_mask(per, band).sum()) * S
        runs[name] = (run_cost, run_path, cells, cb, steps)

    def cdist():
        xs, ys = x[:, :bars * per].reshape(B * bars, per, F), y[:, :bars * per].reshape(B * bars, per, F)
        return torch.cdist(xs, ys + 0.01) ** 2

    cb_ms, cu_ms, cd_ms = (_stats(ms) for ms in _alternating([runs["banded"][0], runs["unbanded"][0], cdist]))
    for name, ms in (("banded", cb_ms), ("unbanded", cu_ms)):
        fma = runs[name][2] * F
        tf = 2.0 * fma / (ms["median"] * 1e-3)
        res["cost_" + name] = {"ms": ms, "cells": runs[name][2], "fma": fma, "tflops_at_2_per_fma": tf / 1e12, "share_of_fp32_roof": tf / FP32_ROOF,
                               "vector_ops_per_term": 3, "share_of_roof_counting_the_three_ops": 3.0 * fma / (ms["median"] * 1e-3) / (FP32_ROOF / 2.0),
                               "cost_buffer_bytes": runs[name][3]}
    # each alone, back to back: what follows a kernel in the alternation (the restatement streams 0.9 GB through the caches) is part of its time there
    res["cost_banded"]["ms_alone"], res["cost_unbanded"]["ms_alone"] = _stats(_timed(runs["banded"][0])), _stats(_timed(runs["unbanded"][0]))
    res["torch_cdist_squared_unbanded"] = {"ms": cd_ms, "note": "cdist(x, y + off) ** 2 on the same segments; a GEMM formulation, not the chain of the definition"}
    pb_ms, pu_ms = (_stats(ms) for ms in _alternating([runs["banded"][1], runs["unbanded"][1]]))
    for name, ms in (("banded", pb_ms), ("unbanded", pu_ms)):
        res["path_" + name] = {"ms": ms, "anti_diagonals": 2 * per - 1, "cells": runs[name][2], "mean_steps": float(runs[name][4].float().mean())}
    # one long segment: the whole window
    table = np.array([(0, 0, rows, -1)], dtype=np.int64)
    n_max, r_max = hip.dtw_geometry(table)
    seg = torch.from_numpy(table.astype(np.int32)).to(dev)
    cb, wb = int(Lib.a2s_dtw_cost_bytes(1, n_max, r_max)), int(Lib.a2s_dtw_workspace_bytes(1, n_max, r_max))
    cost, ws = torch.zeros(cb // 4, device=dev), torch.zeros(wb, dtype=torch.uint8, device=dev)
    paths, steps, total = torch.zeros((1, 2 * n_max - 1), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, device=dev)
    one_cost = lambda: hip.check(Lib.a2s_dtw_cost(st, hip._p(x), hip._p(y), rows * F, B, rows, F, hip._p(seg), 1, None, n_max, r_max, hip._p(cost), cb), "a2s_dtw_cost")
    one_path = lambda: hip.check(Lib.a2s_dtw_path(st, hip._p(seg), 1, B, rows, n_max, r_max, hip._p(cost), cb, hip._p(ws), wb, hip._p(paths), hip._p(steps), hip._p(total)), "a2s_dtw_path")
    res["one_segment_of_the_whole_window"] = {"frames": rows, "anti_diagonals": 2 * rows - 1, "cost_ms": _stats(_timed(one_cost)), "path_ms": _stats(_timed(one_path)),
                                              "steps": int(steps[0])}
    res["wrapper_with_table_upload_banded"] = {"ms": _stats(_timed(lambda: hip.dtw_segments(x, y, np.array([(b, i * per, (i + 1) * per, r) for b in range(B) for i in range(bars)]))))}
    return res


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
    transcribe.transcribe_waveform(model, wave[:16000 * 24], 16000, downbeats=short, hparams=HP, resynthesis=True, align_notes=True)      # untimed
    off, on = [], []
    for _ in range(3):
        _, ms0 = _clock(lambda: transcribe.transcribe_waveform(model, wave, 16000, downbeats=downbeats, hparams=HP, resynthesis=True))
        r1, ms1 = _clock(lambda: transcribe.transcribe_waveform(model, wave, 16000, downbeats=downbeats, hparams=HP, resynthesis=True, align_notes=True))
        off.append(ms0)
        on.append(ms1)
    bars = [b for w in r1["windows"] for b in w["bars"]]
    out = {"seconds": seconds, "windows": len(r1["windows"]), "bars": len(bars), "notes": sum(len(b["notes"]) for b in bars),
           "bars_with_a_warp": sum(b["agreement_warped"] is not None for b in bars), "decoding": "constrained greedy, batch 16",
           "transcribe_with_resynthesis_ms": _stats(off), "transcribe_with_align_notes_ms": _stats(on)}
    out["align_notes_extra_ms_median"] = out["transcribe_with_align_notes_ms"]["median"] - out["transcribe_with_resynthesis_ms"]["median"]
    return out


def _features(dev, vqt, events, n_samples):
    from piano_a2s_amd import render, resynth
    return vqt(render.render(torch.from_numpy(np.stack([resynth.program(ev, n_samples) for ev in events])).to(dev), n_samples))


def _summary(a):
    a = np.array([v for v in a if v is not None], dtype=np.float64)
    return {"min": float(a.min()), "max": float(a.max()), "mean": float(a.mean())}


def rendered(dev, n_clips, amps, frames=1201):
    """Sections 3 and 4: the performance is the clip's own score rendered on resynth's instrument, straight or warped inside every bar."""
    from piano_a2s_amd import resynth, scoregen, spec, transcribe
    cfg = spec.default_cfg(max_length=(200, 200))
    bars, hop, n_samples = cfg["max_bars"], scoregen.HOP, (frames - 1) * scoregen.HOP
    clips = [scoregen.make_clip(cfg, 100 + i, frames=frames) for i in range(n_clips)]
    vqt = transcribe._vqt(dev, dict(HP, max_frame_num=frames))
    out = {"clips": n_clips, "frames": frames, "seeds": [100, 100 + n_clips - 1], "warp_seed": 25, "onset_errors": [], "agreements": {}}
    ms = 1e3 / scoregen.SR
    for amp in amps:
        rng = np.random.default_rng(25)
        scns = [oracle.warped_clip(c, bars, amp, rng) for c in clips]
        x = _features(dev, vqt, [s["warped"] for s in scns], n_samples)
        if amp > 0.0:
            windows = [{"events": s["straight"], "bar_lines": s["lines"]} for s in scns]
            _, _, aligned = resynth.resynthesise(windows, x, vqt, hop, align=True)
            linear, moved = [], []
            for scn, al in zip(scns, aligned):
                lin, mov = oracle.onset_errors(scn, [None if a is None else (a["warp"], a["first_frame"]) for a in al], hop, resynth.performed_notes)
                linear += lin
                moved += mov
            out["onset_errors"].append({"amp": amp, "notes": len(linear), "linear_ms": {"median": float(np.median(linear) * ms), "p90": float(np.percentile(linear, 90) * ms)},
                                        "dtw_ms": {"median": float(np.median(moved) * ms), "p90": float(np.percentile(moved, 90) * ms)},
                                        "ratio_of_medians": float(np.median(moved) / np.median(linear))})
        if amp in (0.0, max(amps)):
            mut_rng = np.random.default_rng(9)
            table = {}
            for which in ("own", "other", "mutated"):
                windows = []
                for i, scn in enumerate(scns):
                    ev = scn["straight"]
                    if which == "other":                                                       # the next clip's score on THIS clip's bar grid
                        src = clips[(i + 1) % n_clips]
                        ev = resynth.score_events(src["ids"]["upper"], src["ids"]["lower"], [src["time_sig"]] * bars, scn["lines"])[0]
                    if which == "mutated":
                        ev = ev.copy()
                        pick = mut_rng.random(len(ev)) < 0.25
                        ev[pick, 2] += mut_rng.choice([-2, -1, 1, 2], size=int(pick.sum()))
                    windows.append({"events": ev, "bar_lines": scn["lines"]})
                _, plain, aligned = resynth.resynthesise(windows, x, vqt, hop, align=True)
                table[which] = (np.array([[np.nan if v is None else v for v in row] for row in plain]),
                                np.array([[np.nan if a is None else a["agreement_warped"] for a in row] for row in aligned]))
            rec = {}
            for k, key in enumerate(("agreement", "agreement_warped")):
                own, other, mut = (table[w][k] for w in ("own", "other", "mutated"))
                drop = np.nanmean(own, axis=1) - np.nanmean(mut, axis=1)
                rec[key] = {"own": _summary(own.ravel()), "other": _summary(other.ravel()), "mutated": _summary(mut.ravel()),
                            "bars_where_own_beats_other": int(np.nansum(own > other)), "smallest_gap_own_minus_other": float(np.nanmin(own - other)),
                            "smallest_drop_of_a_clip_mean_when_mutated": float(drop.min()), "mean_drop_of_a_clip_mean_when_mutated": float(drop.mean())}
            out["agreements"]["straight" if amp == 0.0 else f"warped_{amp}"] = rec
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dtw_alignment.json")
    quick = len(sys.argv) > 2 and sys.argv[2] == "quick"
    if not torch.cuda.is_available():
        raise SystemExit("dtw_bench: needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    B, rows, seconds, n_clips = (8, 201, 30.0, 4) if quick else (256, 1201, 600.0, 24)
    res = {"device": torch.cuda.get_device_name(0), "quick": quick}
    res["kernels"] = kernel_times(dev, B, rows)
    res["rendered"] = rendered(dev, n_clips, [0.0, 0.05, 0.10, 0.15])
    # the clips, the seed and the amplitude of tests/test_gpu_dtw.py: the ratio its assertion (b) compares with 1
    res["test_scenario"] = rendered(dev, 4 if quick else 8, [0.15])["onset_errors"][0]
    res["recording"] = recording(dev, seconds)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
