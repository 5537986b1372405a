"""The tuning estimate of DESIGN.md section 27 on rendered clips, WITHOUT the GPU: the float64 definitions alone (tests/render_oracle.py renders,
oracle/vqt_ref.py makes the features, tests/tuning_oracle.py profiles, estimates and shifts).  It answers, before the kernels exist: how far is the
estimate from the detuning a clip was rendered with, how confident is it on music and on noise (the default `min_conf` lies midway between the
smallest of the first and the largest of the second), and what does the correction do to the features?

    python tools/tuning_check.py [--first_clip 100] [--clips 6] [--long_clips 2] [--cents -49,-40,-20,-7,0,13,30,45,49] [--out FILE.json]

Every clip of scoregen.make_clip is rendered with every phase increment scaled by 2^(c / 1200) (scoregen.detune_program), on resynth's fixed
instrument and on the clip's own drawn one, at 301 frames (--clips seeds) and at 1201 frames (--long_clips seeds).  Correlations: of the detuned
clip's features with the in-tune render's over the whole clip, as they are and after a shift by -estimate / 20 bins (the float64 restatement of
a2s_shift_bins).  About 0.1 s of CPU time per 301-frame case."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import tuning_oracle as oracle                                                         # noqa: E402


def check(first_clip=100, clips=6, long_clips=2, cents=(-49, -40, -20, -7, 0, 13, 30, 45, 49), verbose=True):
    rows = []
    for frames, n in ((301, clips), (1201, long_clips)):
        for instrument in ("resynth", "own"):
            for seed in range(first_clip, first_clip + n):
                ref = None
                for c in (0,) + tuple(c for c in cents if c != 0):
                    est, x = oracle.chain(seed, c, frames, instrument, features=True)
                    if c == 0:
                        ref = x
                    S = x.shape[1] // 96                                                          # bins per semitone: 8 octaves of 12
                    row = {"frames": frames, "instrument": instrument, "seed": seed, "cents": c, "estimate": float(est[0]),
                           "error": oracle.cents_error(est[0], c), "confidence": float(est[1]), "peaks": int(est[2]),
                           "corr_uncorrected": oracle.correlation(x, ref),
                           "corr_shifted": oracle.correlation(oracle.shift_bins64(x, -float(est[0]) * S / 100.0), ref)}
                    rows.append(row)
                    if verbose:
                        print("{frames:5d} {instrument:8s} seed {seed} c {cents:4d}: estimate {estimate:8.3f} error {error:6.3f} confidence {confidence:6.3f} "
                              "peaks {peaks:6d} corr {corr_uncorrected:.4f} -> {corr_shifted:.4f}".format(**row), flush=True)
    noise = []
    for i, x in enumerate(oracle.noise_tensors()):
        est = oracle.estimate(oracle.profile(x[None], [x.shape[0]]), [0, 1], 0.0, oracle.H)[0][0]
        noise.append({"kind": "uniform" if i % 2 == 0 else "gaussian", "confidence": float(est[1]), "peaks": int(est[2])})
    worst = max(abs(r["error"]) for r in rows)
    lo, hi = min(r["confidence"] for r in rows), max(r["confidence"] for r in noise)
    summary = {"cases": len(rows), "worst_error_cents": worst, "min_confidence_rendered": lo, "max_confidence_noise": hi, "min_conf_midway": 0.5 * (lo + hi),
               "error_bound_cents": worst + 0.5 * (10.0 - worst)}
    for frames in (301, 1201):
        for instrument in ("resynth", "own"):
            sel = [r for r in rows if r["frames"] == frames and r["instrument"] == instrument]
            if sel:
                summary[f"{frames}_{instrument}"] = {"worst_error_cents": max(abs(r["error"]) for r in sel),
                                                     "min_confidence": min(r["confidence"] for r in sel)}
    by_c = {}
    for r in rows:
        by_c.setdefault(abs(r["cents"]), []).append(r)
    summary["correlation_by_abs_cents"] = {str(c): {"uncorrected_min": min(r["corr_uncorrected"] for r in v), "uncorrected_max": max(r["corr_uncorrected"] for r in v),
                                                    "shifted_min": min(r["corr_shifted"] for r in v), "shifted_max": max(r["corr_shifted"] for r in v)}
                                           for c, v in sorted(by_c.items())}
    return {"summary": summary, "noise": noise, "rows": rows}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--first_clip", type=int, default=100)
    ap.add_argument("--clips", type=int, default=6, help="seeds at 301 frames")
    ap.add_argument("--long_clips", type=int, default=2, help="seeds at 1201 frames")
    ap.add_argument("--cents", default="-49,-40,-20,-7,0,13,30,45,49")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = check(a.first_clip, a.clips, a.long_clips, tuple(int(c) for c in a.cents.split(",")))
    print(json.dumps({"summary": res["summary"], "noise": res["noise"]}, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
