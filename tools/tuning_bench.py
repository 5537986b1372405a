"""The tuning estimate, measured on the MI355X: python tools/tuning_bench.py [out.json] [quick]

1. kernels: a2s_tuning_profile and a2s_tuning_estimate on 256 windows of 1201 x 480 features, ALTERNATING in one process with a2s_onset_strength (the
   yardstick: it streams the same tensor once) and a2s_shift_bins on the same tensor, and with a plain-torch restatement of the profile (3 warm-up +
   10 timed calls each between device events; median / min / max).  The profile is timed on three tensors, which tells its parts apart: rendered music
   (few peaks, most of them in a few cells: LDS atomics on one address), uniform noise (six times the peaks, spread over all cells) and silence (all
   ones: no peak, the stream alone).  The plain-torch profile is also compared with the kernel's integers.
2. the chain on rendered clips: the estimate against the detuning of the render, the correlation with the in-tune features before and after.
3. a 10-minute recording through transcribe_waveform with and without tuning="auto" (host clock around work that ends in a read-back; the shipped
   model size on seeded procedural weights: the cost, not a score), taking turns, three calls each.
Nothing here is a pass / fail number.  `quick`: every section at a small size (a rehearsal of the script, not a measurement)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import tuning_oracle as oracle                                                        # noqa: E402
from tools.beat_bench import HP, _clock, bursts                                                  # noqa: E402
from tools.transpose_augment_bench import HBM_ROOF_GBS, _alternating, _stats                     # noqa: E402


def torch_profile(x, thr=0.5, S=5):
    """a2s_tuning_profile in plain torch (all rows count): masks, a gather of the peaks, float64 arithmetic, two index_adds."""
    B = x.shape[0]
    a, c, e = x[..., :-2], x[..., 1:-1], x[..., 2:]
    b, t, j = ((c > a) & (c >= e) & (c >= thr)).nonzero(as_tuple=True)
    a, c, e = a[b, t, j].double(), c[b, t, j].double(), e[b, t, j].double()
    delta = torch.nan_to_num(0.5 * (a - e) / ((a - c) + (e - c)), nan=0.0)
    u = ((j + 1) % S).double() + delta + S / 2.0
    u = torch.where(u >= S, u - S, u)
    cell = torch.clamp(torch.floor(u * oracle.H / S), max=oracle.H - 1).long()
    w = 1 + torch.round(torch.clamp(c - thr, max=1.0) * oracle.Q).long()
    hist = torch.zeros(B * (oracle.H + 1), dtype=torch.int64, device=x.device)
    hist.index_add_(0, b * (oracle.H + 1) + cell, w)
    hist.index_add_(0, b * (oracle.H + 1) + oracle.H, torch.ones_like(w))
    return hist.view(B, oracle.H + 1)


def rendered_features(dev, seeds, cents, frames):
    """The GPU render and GPU VQT of scoregen's clips on resynth's instrument, every clip at every detuning -> ((len(seeds) * len(cents), 1, T, F), truth)."""
    from piano_a2s_amd import render, scoregen, transcribe
    progs, truth = [], []
    for s in seeds:
        p, n_samples = oracle.clip_program(s, frames, "resynth")
        for c in cents:
            progs.append(scoregen.detune_program(p, c))
            truth.append((s, c))
    return transcribe._vqt(dev, HP)(render.render(torch.from_numpy(np.stack(progs)).to(dev), n_samples)), truth


def kernel_times(dev, B, rows, F=480):
    from piano_a2s_amd import hip, tuning
    music, _ = rendered_features(dev, range(100, 100 + min(B, 16)), (13,), rows)
    tensors = {"music": music[:, 0].repeat(-(-B // music.shape[0]), 1, 1)[:B].contiguous(), "noise": torch.rand(B, rows, F, device=dev),
               "silence": torch.ones(B, rows, F, device=dev)}
    x = tensors["music"]
    y = torch.empty_like(x)
    n_rows = torch.full((B,), rows, dtype=torch.int32, device=dev)
    hist = {k: torch.empty((B, oracle.H + 1), dtype=torch.int64, device=dev) for k in tensors}
    ef, el = torch.empty((B, rows), device=dev), torch.empty((B, rows), device=dev)
    first_all, first_each = torch.tensor([0, B], dtype=torch.int32, device=dev), torch.arange(B + 1, dtype=torch.int32, device=dev)
    eff = torch.full((B,), -0.65, device=dev)
    hip.tuning_profile(x, n_rows, out=hist["music"])
    same = bool(torch.equal(torch_profile(x), hist["music"]))
    fns = [lambda: hip.onset_strength(x, n_rows, 1, 180, env_full=ef, env_low=el), lambda: hip.shift_bins(x, eff, y=y),
           lambda: hip.tuning_profile(tensors["music"], n_rows, out=hist["music"]), lambda: hip.tuning_profile(tensors["noise"], n_rows, out=hist["noise"]),
           lambda: hip.tuning_profile(tensors["silence"], n_rows, out=hist["silence"]),
           lambda: hip.tuning_estimate(hist["music"], first_all, tuning.MIN_CONF, tuning.MIN_PEAKS),
           lambda: hip.tuning_estimate(hist["music"], first_each, tuning.MIN_CONF, tuning.MIN_PEAKS), lambda: torch_profile(x)]
    names = ["onset_strength", "shift_bins", "tuning_profile_music", "tuning_profile_noise", "tuning_profile_silence", "tuning_estimate_one_group",
             "tuning_estimate_group_per_clip", "plain_torch_profile_music"]
    n = x.numel() * 4
    out = {"batch": B, "rows": rows, "freq_bins": F, "feature_bytes": n, "plain_torch_profile_equals_the_kernel": same}
    times = _alternating(fns)
    out["peaks_per_clip"] = {k: float(h[:, oracle.H].double().mean()) for k, h in hist.items()}
    out["peaks_in_the_fullest_cell"] = {k: float((h[:, :oracle.H].sum(0).max() / h[:, :oracle.H].sum().clamp(min=1)).item()) for k, h in hist.items()}
    for name, ms in zip(names, times):
        out[name] = {"ms": _stats(ms)}
        if name.startswith("tuning_profile") or name == "onset_strength":
            tbs = n / (out[name]["ms"]["median"] * 1e-3) / 1e12
            out[name].update(tb_per_s_of_the_features=tbs, share_of_8tb_roof=tbs * 1e3 / HBM_ROOF_GBS)
    for k in ("music", "noise", "silence"):
        out[f"tuning_profile_{k}"]["ratio_to_onset_strength"] = out[f"tuning_profile_{k}"]["ms"]["median"] / out["onset_strength"]["ms"]["median"]
    return out


def chain(dev, seeds, cents, frames=301):
    from piano_a2s_amd import hip, resynth, tuning
    x, truth = rendered_features(dev, seeds, cents, frames)
    y, est, _ = tuning.Tuner(dev)(x)
    est = est.cpu().numpy()
    ref = torch.cat([x[i - i % len(cents) + list(cents).index(0)][None] for i in range(len(truth))])
    seg, cells = [(i, 0, x.shape[-2]) for i in range(len(truth))], x.shape[-2] * x.shape[-1]
    before = [resynth.agreement(r, cells) for r in hip.segment_agreement(x, ref, seg).cpu().numpy()]
    after = [resynth.agreement(r, cells) for r in hip.segment_agreement(y, ref, seg).cpu().numpy()]
    rows = [{"seed": s, "cents": c, "estimate": float(e[0]), "error": oracle.cents_error(e[0], c), "confidence": float(e[1]), "peaks": int(e[2]),
             "float64_chain_estimate": float(oracle.chain(s, c, frames, "resynth")[0]), "corr_uncorrected": b, "corr_corrected": a}
            for (s, c), e, b, a in zip(truth, est, before, after)]
    by_c = {}
    for r in rows:
        by_c.setdefault(abs(r["cents"]), []).append(r)
    return {"frames": frames, "instrument": "resynth", "worst_error_cents": max(abs(r["error"]) for r in rows), "min_confidence": min(r["confidence"] for r in rows),
            "largest_difference_to_the_float64_chain_cents": max(abs(oracle.cents_error(r["estimate"], r["float64_chain_estimate"])) for r in rows),
            "correlation_by_abs_cents": {str(c): {"uncorrected": [min(r["corr_uncorrected"] for r in v), max(r["corr_uncorrected"] for r in v)],
                                                  "corrected": [min(r["corr_corrected"] for r in v), max(r["corr_corrected"] for r in v)]}
                                         for c, v in sorted(by_c.items())}, "per_clip": rows}


def recording(dev, seconds):
    import models
    from piano_a2s_amd import hip, spec, transcribe
    wave, _, _ = bursts(seconds)
    downbeats = [float(t) for t in np.arange(0.25, seconds - 2.0, 2.0)]
    model = models.ScoreTranscription()
    model.load_state_dict(spec.procedural_state(spec.default_cfg(), 11, eos_bias=3.0, lively=True))
    model = model.to(dev).eval()
    for t in (None, "auto"):                                                                     # untimed: tables, banks, first launches
        transcribe.transcribe_waveform(model, wave[:16000 * 24], 16000, downbeats=[d for d in downbeats if d < 24], hparams=HP, tuning=t)
    plain, auto, n0 = [], [], hip.tuning_launches()
    for _ in range(3):
        r0, ms = _clock(lambda: transcribe.transcribe_waveform(model, wave, 16000, downbeats=downbeats, hparams=HP))
        plain.append(ms)
        r1, ms = _clock(lambda: transcribe.transcribe_waveform(model, wave, 16000, downbeats=downbeats, hparams=HP, tuning="auto"))
        auto.append(ms)
    return {"seconds": seconds, "windows": len(r0["windows"]), "transcribe_ms": _stats(plain), "transcribe_tuning_auto_ms": _stats(auto),
            "added_ms_median": float(np.median(auto) - np.median(plain)), "tuning_launches_per_recording": (hip.tuning_launches() - n0) // 3,
            "tuning_of_the_tone_bursts": r1["tuning"]}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tuning.json")
    quick = len(sys.argv) > 2 and sys.argv[2] == "quick"
    if not torch.cuda.is_available():
        raise SystemExit("tuning_bench: needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    B, rows, seeds, seconds = (8, 201, range(100, 101), 30.0) if quick else (256, 1201, range(100, 104), 600.0)
    res = {"device": torch.cuda.get_device_name(0), "quick": quick}
    res["kernels"] = kernel_times(dev, B, rows)
    res["chain"] = chain(dev, seeds, (-40, -20, 0, 13, 30))
    res["recording"] = recording(dev, seconds)
    print(json.dumps({k: v for k, v in res.items() if k != "chain"}))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
