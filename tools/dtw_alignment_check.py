"""The bar-wise alignment of DESIGN.md section 25 on rendered clips, WITHOUT the GPU: the float64 definitions alone (tests/render_oracle.py renders,
oracle/vqt_ref.py makes the features, tests/dtw_oracle.py aligns).  It answers one question before a seed is fixed in tests/test_gpu_dtw.py: does the
definition itself, on the chosen clips, place the notes of a warped performance better than linear placement does, and does the warped agreement
stay at or above the plain one?

    python tools/dtw_alignment_check.py [--amp 0.15] [--seed 25] [--first_clip 100] [--clips 8] [--out FILE.json]

Every bar's events are moved by g(u) = u + a sin(pi u), a = +-amp with the sign drawn per bar from the seeded generator; the performance is the moved
events rendered, the score side the straight events rendered, both on resynth's instrument.  Prints and (with --out) writes the pooled median onset
errors of linear placement and of the warp, their ratio, and the mean agreement and warped agreement over the bars.  Minutes of CPU time."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import vqt_ref                                                                       # noqa: E402
from piano_a2s_amd import resynth, scoregen, spec                                                 # noqa: E402
from tests import dtw_oracle as oracle, render_oracle, resynth_oracle                             # noqa: E402


def features(events, n_samples):
    return vqt_ref.vqt_features_librosa(render_oracle.render(resynth.program(events, n_samples), n_samples))


def check(amp, seed, first_clip, n_clips, frames=1201):
    cfg = spec.default_cfg(max_length=(200, 200))
    bars, hop = cfg["max_bars"], scoregen.HOP
    n_samples = (frames - 1) * hop
    rng = np.random.default_rng(seed)
    linear, moved, plain, warped = [], [], [], []
    for clip_seed in range(first_clip, first_clip + n_clips):
        scn = oracle.warped_clip(scoregen.make_clip(cfg, clip_seed, frames=frames), bars, amp, rng)
        x, y = features(scn["warped"], n_samples)[None], features(scn["straight"], n_samples)[None]
        seg, _ = resynth.bar_segments([{"events": scn["straight"], "bar_lines": scn["lines"]}], hop, frames)
        warps = []
        for _, f0, f1 in seg:
            n = int(f1 - f0)
            sums = resynth_oracle.five_sums(x, y, [(0, f0, f1)])[0]
            a = resynth_oracle.correlation(sums, n * x.shape[2])
            if a is None:
                warps.append(None)
                continue
            r = resynth.dtw_band(n)
            d = oracle.cost(x, y, (0, f0, f1, r), off=(sums[0] - sums[1]) / (n * x.shape[2]))
            path, _ = oracle.align(d, r)
            warp, inverse = oracle.warp_from_path(path, n)
            heard = y.copy()
            heard[0, f0:f1] = y[0, f0 + np.floor(inverse + 0.5).astype(np.int64)]
            plain.append(a)
            warped.append(resynth_oracle.correlation(resynth_oracle.five_sums(x, heard, [(0, f0, f1)])[0], n * x.shape[2]))
            warps.append((warp, int(f0)))
        lin, mov = oracle.onset_errors(scn, warps, hop, resynth.performed_notes)
        linear += lin
        moved += mov
        print(f"clip {clip_seed}: {len(lin)} notes, median error linear {np.median(lin) / scoregen.SR * 1e3:.1f} ms, warped {np.median(mov) / scoregen.SR * 1e3:.1f} ms", flush=True)
    ms = 1e3 / scoregen.SR
    return {"amp": amp, "seed": seed, "clips": [first_clip, first_clip + n_clips - 1], "notes": len(linear), "bars": len(plain),
            "median_error_linear_ms": float(np.median(linear) * ms), "median_error_dtw_ms": float(np.median(moved) * ms),
            "ratio_of_medians": float(np.median(moved) / np.median(linear)) if np.median(linear) > 0 else None,
            "mean_agreement": float(np.mean(plain)), "mean_agreement_warped": float(np.mean(warped))}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--amp", type=float, default=0.15)
    ap.add_argument("--seed", type=int, default=25)
    ap.add_argument("--first_clip", type=int, default=100)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = check(a.amp, a.seed, a.first_clip, a.clips)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
