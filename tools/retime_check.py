"""Resynthesis at the performed timing on rendered clips, WITHOUT the GPU: the float64 definitions (tests/render_oracle.py
renders, oracle/vqt_ref.py makes the features, tests/dtw_oracle.py aligns) and the integer definition of tests/retime_oracle.py (warp, retime).  It
answers, before a number is fixed in tests/test_gpu_retime.py: how near to the true onsets do the retimed notes stand after round 1, 2, 3, how well
does the render at that timing agree with the performance WITHOUT any warp, and does the iteration ever move onsets away from the truth?

    python tools/retime_check.py [--amp 0.15] [--seed 25] [--first_clip 100] [--clips 8] [--rounds 3] [--jobs 8] [--out FILE.json]

The clips and their warps are those of tools/dtw_alignment_check.py (every bar's events moved by g(u) = u + a sin(pi u), a = +-amp).  Prints and (with
--out) writes per round the pooled median and 90 % onset error and the mean plain agreement of the retimed render, beside linear placement, the float
performed_notes through the first warp, and the straight render's plain and warped agreement.  Minutes of CPU time."""
import argparse
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import vqt_ref                                                                       # noqa: E402
from piano_a2s_amd import resynth, scoregen, spec                                                 # noqa: E402
from tests import dtw_oracle, render_oracle, retime_oracle                                        # noqa: E402


def features(events, n_samples):
    return vqt_ref.vqt_features_librosa(render_oracle.render(resynth.program(events, n_samples), n_samples))


def paired(scn):
    """The straight events in program order and, row for row, the same notes where they are truly played."""
    notes, true = (np.concatenate([bar[k] for bar in scn["bars"]]).reshape(-1, 3) for k in ("notes", "true"))
    order = np.lexsort((notes[:, 2], notes[:, 0]))
    assert np.array_equal(notes[order], scn["straight"])
    return notes[order], true[order]


def one_clip(job):
    scn, rounds, frames = job
    hop, n_samples = scoregen.HOP, (frames - 1) * scoregen.HOP
    straight, true = paired(scn)
    x = features(scn["warped"], n_samples)
    got = retime_oracle.loop64(x, straight, scn["lines"], n_samples, hop, rounds, lambda ev: features(ev, n_samples))
    return {"linear": np.abs(straight[:, 0] - true[:, 0]).tolist(), "rounds": [np.abs(g["events"][:, 0] - true[:, 0]).tolist() for g in got],
            "agreement": [[a for a in g["agreement"] if a is not None] for g in got], "plain": [a for a, _ in got[0]["first"] if a is not None],
            "warped": [w for a, w in got[0]["first"] if a is not None]}


def check(amp, seed, first_clip, n_clips, rounds, jobs, frames=1201):
    cfg = spec.default_cfg(max_length=(200, 200))
    rng = np.random.default_rng(seed)
    scns = [dtw_oracle.warped_clip(scoregen.make_clip(cfg, s, frames=frames), cfg["max_bars"], amp, rng) for s in range(first_clip, first_clip + n_clips)]
    with ProcessPoolExecutor(max_workers=max(1, jobs)) as pool:
        per_clip = list(pool.map(one_clip, [(s, rounds, frames) for s in scns]))
    ms = 1e3 / scoregen.SR
    pool_ = lambda pick: np.concatenate([np.asarray(pick(c), dtype=np.float64) for c in per_clip])
    linear = pool_(lambda c: c["linear"])
    res = {"amp": amp, "seed": seed, "clips": [first_clip, first_clip + n_clips - 1], "notes": int(len(linear)), "bars": int(len(pool_(lambda c: c["plain"]))),
           "median_error_linear_ms": float(np.median(linear) * ms), "mean_agreement_straight": float(pool_(lambda c: c["plain"]).mean()),
           "mean_agreement_warped": float(pool_(lambda c: c["warped"]).mean()), "rounds": []}
    before = None
    for r in range(rounds):
        err = pool_(lambda c: c["rounds"][r])
        row = {"round": r + 1, "median_error_ms": float(np.median(err) * ms), "p90_error_ms": float(np.quantile(err, 0.9) * ms),
               "mean_error_ms": float(err.mean() * ms), "mean_agreement_retimed": float(pool_(lambda c: c["agreement"][r]).mean())}
        if before is not None:                                   # drift: notes that a further round moves AWAY from the truth
            row["notes_moved_away"] = int((err > before).sum())
            row["notes_moved_nearer"] = int((err < before).sum())
            row["worst_move_away_ms"] = float((err - before).max() * ms)
        before = err
        res["rounds"].append(row)
    return res


def one_dynamics_clip(job):
    """One clip of tools/dynamics_check.py --warp: the levels after `dyn_rounds` dynamics rounds, read through the first warp (no retiming, what
    section 26 reports) and on the score retimed by 1 .. rounds timing rounds (performed=None: fx = fy)."""
    from tests import dynamics_oracle
    from tools.dynamics_check import warped_performance
    clip, rng, amp, rounds, dyn_rounds, frames = job
    hop, n_samples = scoregen.HOP, (frames - 1) * scoregen.HOP
    scn = dynamics_oracle.scenario(clip, rng, 3)
    x, performed = warped_performance(clip, scn, amp, rng, n_samples, frames, "resynth")
    lines = dtw_oracle.clip_lines(clip, len(clip["ids"]["upper"]))
    levels = [dynamics_oracle.loop64(x, scn["score"], n_samples, hop, dyn_rounds, performed)[-1]]
    for g in retime_oracle.loop64(x, scn["score"], lines, n_samples, hop, rounds, lambda ev: features(ev, n_samples)):
        levels.append(dynamics_oracle.loop64(x, g["events"], n_samples, hop, dyn_rounds, None)[-1])
    return levels, scn["true_db"], scn["real"]


def check_dynamics(amp, seed, first_clip, n_clips, rounds, jobs, dyn_rounds=3, frames=1201):
    """The table of tools/dynamics_check.py --warp `amp` (same clips, same seed, same phantoms and warps) without and with retiming."""
    import copy
    from tests import dynamics_oracle
    cfg = spec.default_cfg(max_length=(200, 200))
    rng = np.random.default_rng(seed)
    work = []
    for s in range(first_clip, first_clip + n_clips):
        clip = scoregen.make_clip(cfg, s, frames=frames)
        work.append((clip, copy.deepcopy(rng), amp, rounds, dyn_rounds, frames))
        dynamics_oracle.scenario(clip, rng, 3)                                   # (the draws the clip's job makes on its copy, so that the next clip
        dtw_oracle.warped_clip(clip, len(clip["ids"]["upper"]), amp, rng)       # starts where dynamics_check.py starts it)
    with ProcessPoolExecutor(max_workers=max(1, jobs)) as pool:
        per_clip = list(pool.map(one_dynamics_clip, work))
    real = np.concatenate([r for _, _, r in per_clip])
    true = np.concatenate([t - t[r].mean() for _, t, r in per_clip])
    out = []
    for k in range(rounds + 1):
        g = np.concatenate([lv[k] - lv[k][r].mean() for lv, _, r in per_clip])
        err = g[real] - true[real]
        out.append({"timing_rounds": k, "dynamics_rounds": dyn_rounds, "notes": int(real.sum()), "phantoms": int((~real).sum()),
                    "correlation": float(np.corrcoef(g[real], true[real])[0, 1]), "rms_error_db": float(np.sqrt(np.mean(err * err))),
                    "auc_real_over_phantom": dynamics_oracle.auc(g[real], g[~real])})
    return {"amp": amp, "seed": seed, "clips": [first_clip, first_clip + n_clips - 1], "rows": out,
            "note": "timing_rounds 0: the notes read through the first warp, the score rendered straight (DESIGN.md section 26)"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dynamics", action="store_true", help="instead: the level table of tools/dynamics_check.py --warp AMP (seed 26, 12 clips) without and with retiming")
    ap.add_argument("--amp", type=float, default=0.15)
    ap.add_argument("--seed", type=int, default=25)
    ap.add_argument("--first_clip", type=int, default=100)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = check_dynamics(a.amp, a.seed, a.first_clip, a.clips, a.rounds, a.jobs) if a.dynamics else check(a.amp, a.seed, a.first_clip, a.clips, a.rounds, a.jobs)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
