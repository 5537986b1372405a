"""The note dynamics of DESIGN.md section 26 on rendered clips, WITHOUT the GPU: the float64 definitions alone (tests/render_oracle.py renders,
oracle/vqt_ref.py makes the features, tests/dynamics_oracle.py measures and updates).  It answers, before a seed is fixed in
tests/test_gpu_dynamics.py: does the loop recover the amplitudes a performance was rendered with, and does a note that is not in the audio come out
quiet?

    python tools/dynamics_check.py [--first_clip 100] [--clips 12] [--rounds 3] [--phantom_every 3] [--instrument resynth|own] [--warp 0.0]
                                   [--seed 26] [--out FILE.json]

The performance is the clip's notes at the clip's own drawn amplitudes (0.3 .. 1.0), on resynth's instrument or on the clip's own drawn one (other g,
n_harm, tau, attack; its noise floor off).  The score side holds those notes plus phantoms: a copy of every phantom_every-th note moved by +-3 .. 8
semitones (0: none).  --warp a > 0: every bar of the performance is warped by g(u) = u + a sin(pi u) as in section 25, the bars are aligned by the
float64 DTW of tests/dtw_oracle.py on the unit-amplitude pass, and the performed onsets go through that warp.  Levels are centred per clip.  Prints
and (with --out) writes, per round: correlation and rms error against 20 log10(amp), the AUC of real over phantom levels, the phantoms' median and
the real notes' 5 % quantile.  About 0.3 s of CPU time per clip and round; the warped variant takes minutes."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from piano_a2s_amd import resynth, scoregen, spec                                                 # noqa: E402
from tests import dynamics_oracle as oracle                                                       # noqa: E402


def performance_program(events, amps, n_samples, clip, instrument):
    """The render program of what is performed: on resynth's instrument, or on the clip's own with its noise floor off."""
    if instrument == "resynth":
        return resynth.program(events, n_samples, amps=amps)
    p = scoregen.pack_program(dict(clip, events=events, amps=np.asarray(amps, dtype=np.float32), n_samples=n_samples))
    p[0, 6] = 0
    return p


def warped_performance(clip, scn, amp, rng, n_samples, frames, instrument):
    """-> (the performance's features, the performed onsets of scn["score"]): the clip's bars warped, aligned by the float64 DTW."""
    from tests import dtw_oracle, resynth_oracle
    bars, hop = len(clip["ids"]["upper"]), scoregen.HOP
    w = dtw_oracle.warped_clip(clip, bars, amp, rng)
    amp_of = {(int(o), int(m)): float(a) for (o, _, m), a in zip(scn["events"], scn["amps"])}
    played = sorted((int(t[0]), int(t[2]), int(t[1]), amp_of[(int(s[0]), int(s[2]))]) for bar in w["bars"] for s, t in zip(bar["notes"], bar["true"]))
    x = oracle.features64(performance_program(np.array([(o, l, m) for o, m, l, _ in played], dtype=np.int64), [a for *_, a in played], n_samples, clip,
                                              instrument), n_samples)[None]
    y = oracle.features64(resynth.program(scn["score"], n_samples), n_samples)[None]
    seg, _ = resynth.bar_segments([{"events": scn["score"], "bar_lines": w["lines"]}], hop, frames)
    aligned = []
    for _, f0, f1 in seg:
        n = int(f1 - f0)
        sums = resynth_oracle.five_sums(x, y, [(0, f0, f1)])[0]
        if resynth_oracle.correlation(sums, n * x.shape[2]) is None:
            aligned.append(None)
            continue
        r = resynth.dtw_band(n)
        path, _ = dtw_oracle.align(dtw_oracle.cost(x, y, (0, f0, f1, r), off=(sums[0] - sums[1]) / (n * x.shape[2])), r)
        aligned.append({"warp": dtw_oracle.warp_from_path(path, n)[0], "first_frame": int(f0)})
    return x[0], resynth.performed_onsets(scn["score"], w["lines"], aligned, hop)


def check(first_clip=100, n_clips=12, rounds=3, phantom_every=3, instrument="resynth", warp=0.0, seed=26, frames=1201, verbose=True):
    cfg = spec.default_cfg(max_length=(200, 200))
    hop, n_samples = scoregen.HOP, (frames - 1) * scoregen.HOP
    rng = np.random.default_rng(seed)
    got, true, real = [[] for _ in range(rounds)], [], []
    for clip_seed in range(first_clip, first_clip + n_clips):
        clip = scoregen.make_clip(cfg, clip_seed, frames=frames)
        scn = oracle.scenario(clip, rng, phantom_every)
        if warp:
            x, performed = warped_performance(clip, scn, warp, rng, n_samples, frames, instrument)
        else:
            x, performed = oracle.features64(performance_program(scn["events"], scn["amps"], n_samples, clip, instrument), n_samples), None
        cums = oracle.loop64(x, scn["score"], n_samples, hop, rounds, performed)
        r = scn["real"]
        for k, cum in enumerate(cums):
            got[k].append(cum - cum[r].mean())                                   # centred per clip, on the real notes
        true.append(scn["true_db"] - scn["true_db"][r].mean())
        real.append(r)
        if verbose:
            print(f"clip {clip_seed}: {int(r.sum())} notes, {int((~r).sum())} phantoms, rms error per round "
                  + ", ".join(f"{oracle.level_errors(c, scn)[0]:.2f}" for c in cums) + " dB", flush=True)
    true, real = np.concatenate(true), np.concatenate(real)
    res = {"clips": [first_clip, first_clip + n_clips - 1], "frames": frames, "rounds": rounds, "phantom_every": phantom_every, "instrument": instrument,
           "warp": warp, "seed": seed, "notes": int(real.sum()), "phantoms": int((~real).sum()), "true_level_std_db": float(true[real].std()), "per_round": []}
    for k in range(rounds):
        g = np.concatenate(got[k])
        err = g[real] - true[real]
        res["per_round"].append({"round": k + 1, "correlation": float(np.corrcoef(g[real], true[real])[0, 1]), "rms_error_db": float(np.sqrt(np.mean(err * err))),
                                 "auc_real_over_phantom": oracle.auc(g[real], g[~real]),
                                 "phantom_median_db": float(np.median(g[~real])) if (~real).any() else None,
                                 "real_quantile_05_db": float(np.quantile(g[real], 0.05))})
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--first_clip", type=int, default=100)
    ap.add_argument("--clips", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--phantom_every", type=int, default=3, help="a phantom beside every n-th note (0: none)")
    ap.add_argument("--instrument", choices=("resynth", "own"), default="resynth", help="what renders the performance")
    ap.add_argument("--warp", type=float, default=0.0, help="amplitude of the bar warp of the performance (0: straight)")
    ap.add_argument("--seed", type=int, default=26)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = check(a.first_clip, a.clips, a.rounds, a.phantom_every, a.instrument, a.warp, a.seed)
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
