"""The beat tracker, measured on the MI355X: python tools/beat_bench.py [out.json] [quick]

1. kernels: a2s_onset_strength on 256 windows of 1201 x 480 features, ALTERNATING in one process with a2s_stretch_frames and a2s_specaug_plan on the same
   tensor (3 warm-up + 10 timed launches each between device events; median / min / max; bytes the algorithm needs, TB/s, share of the 8 TB/s roof);
   a2s_tempogram and a2s_beat_dp on the 256 envelopes of those windows and on the one envelope of a 10-minute recording (60001 frames);
2. tempogram parity at the default geometry (n = 1201): max |device - float64 definition| and its share of the a-priori bound;
3. a 10-minute recording (tone bursts at 120 beats per minute): beats.track_recording as a whole (host clock around work that ends in a read-back: tiling,
   VQT, the three kernels, the host stages), its parts, and beside it the decode of the same recording from a 16-bit 44.1 kHz stereo WAV file, the
   resampler and transcribe_waveform with the tracked downbeats (the shipped model size on seeded procedural weights: the cost of decoding, not a score);
4. beat and downbeat F-measure (+- 70 ms, one-to-one matching) on N rendered clips of scoregen, whose tempo, lead and time signature give the true beats
   and bar lines.  Reported, not asserted: the clips are 12 s long, little more than one tempogram window.
Nothing here is a pass / fail number.  `quick`: every section at a small size (a rehearsal of the script, not a measurement)."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import beat_oracle as oracle                                                          # noqa: E402
from tools.transpose_augment_bench import HBM_ROOF_GBS, _alternating, _stats, _timed          # noqa: E402

HP = dict(sample_rate=16000, hop_length=160, max_frame_num=1201, max_bars=5, bins_per_octave=60, n_octaves=8, gamma=20)
TOLERANCE_S = 0.070
BEATS_PER_BAR = {"4/4": (4, 1.0), "3/4": (3, 1.0), "2/4": (2, 1.0), "6/8": (2, 1.5), "2/2": (2, 2.0), "12/8": (4, 1.5), "3/8": (1, 1.5)}          # beats, quarters per beat


def kernel_times(dev, B, rows, long_frames, F=480):
    from piano_a2s_amd import beats, hip
    rng = np.random.default_rng(5)
    x = torch.rand(B, rows, F, device=dev).clamp_(min=0.33)
    y = torch.empty_like(x)
    n_rows = torch.full((B,), rows, dtype=torch.int32, device=dev)
    ef, el = torch.empty((B, rows), device=dev), torch.empty((B, rows), device=dev)
    step = torch.from_numpy(np.rint(65536.0 / rng.uniform(0.85, 1.15, size=B)).astype(np.int32)).to(dev)
    tab = torch.ones((B, 2, F), device=dev)
    words = torch.from_numpy(rng.integers(0, 2 ** 32, size=(B, 16), dtype=np.uint32).view(np.int32).copy()).to(dev)
    content, plan, stats, counters = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, 16), dtype=torch.int32, device=dev),
                                      torch.empty((B, 2), device=dev), torch.zeros(3, dtype=torch.int32, device=dev))
    n = x.numel() * 4
    fns = [lambda: hip.onset_strength(x, n_rows, 1, 180, env_full=ef, env_low=el), lambda: hip.stretch_frames(x, step, y=y),
           lambda: hip.specaug_plan(x, tab, words, 100, 60, 2, content, plan, stats, counters)]
    o, s, p = (_stats(ms) for ms in _alternating(fns))
    need = {"onset_strength": n + 2 * B * rows * 4, "stretch_frames": 2 * n, "specaug_plan": 2 * n + B * min(16, rows) * F * 4}
    out = {"batch": B, "rows": rows, "freq_bins": F, "feature_bytes": n}
    for name, ms in (("onset_strength", o), ("stretch_frames", s), ("specaug_plan", p)):
        tbs = need[name] / (ms["median"] * 1e-3) / 1e12
        out[name] = {"ms": ms, "bytes_needed": need[name], "tb_per_s": tbs, "share_of_8tb_roof": tbs * 1e3 / HBM_ROOF_GBS}
    pen = torch.from_numpy(beats.penalty_table()).to(dev)
    for name, R, frames in (("windows", B, rows), ("recording", 1, long_frames)):
        env = torch.rand(R, frames, device=dev) * 0.3
        env[:, 13::47] += 3.0
        nn = torch.full((R,), frames, dtype=torch.int32, device=dev)
        J = -(-frames // beats.HOP_B)
        tg = torch.empty((R, J, beats.LAG_MAX - beats.LAG_MIN + 1), device=dev)
        ls = env / env.std()
        period = torch.full((R, J), 47, dtype=torch.int32, device=dev)
        S, back = torch.empty_like(ls), torch.empty((R, frames), dtype=torch.int32, device=dev)
        bt, cnt = torch.empty((R, frames // 10 + 1), dtype=torch.int32, device=dev), torch.empty((R,), dtype=torch.int32, device=dev)
        t_ms = _stats(_timed(lambda: hip.tempogram(env, nn, J=J, out=tg)))
        d_ms = _stats(_timed(lambda: hip.beat_dp(ls, period, pen, nn, S=S, back=back, beats=bt, count=cnt)))
        out[f"tempogram_{name}"] = {"recordings": R, "frames": frames, "blocks": J, "ms": t_ms}
        out[f"beat_dp_{name}"] = {"recordings": R, "frames": frames, "beats_first_recording": int(cnt[0]), "ms": d_ms}
    return out


def tempogram_parity(dev):
    from piano_a2s_amd import hip
    rng = np.random.default_rng(6)
    env = rng.uniform(0, 0.3, size=(1, 1201)).astype(np.float32)
    env[0, 13::47] += 3.0
    got = hip.tempogram(torch.from_numpy(env).to(dev), torch.tensor([1201], dtype=torch.int32, device=dev), J=13).cpu().numpy().astype(np.float64)
    want, bound = oracle.tempogram(env, [1201], 800, 100, 20, 200, 13, with_bound=True)
    err = np.abs(got - want)
    return {"frames": 1201, "win": 800, "lags": [20, 200], "max_abs_diff_kernel_vs_float64": float(err.max()),
            "largest_share_of_the_a_priori_bound": float((err / np.maximum(bound, 1e-300)).max())}


def bursts(seconds, sr=16000, seed=12):
    """Tone bursts every 0.5 s from 0.25 s on, every fourth with an added bass tone -> (wave float32, burst times, bass burst times)."""
    rng = np.random.default_rng(seed)
    x = np.zeros(int(seconds * sr))
    tt = np.arange(int(0.4 * sr)) / sr
    shape = np.minimum(tt / 0.004, 1.0) * np.exp(-tt / 0.08)
    bass_note = 0.5 * shape * (np.sin(2 * np.pi * 55.0 * tt) + 0.7 * np.sin(2 * np.pi * 110.0 * tt))
    times = np.arange(0.25, seconds - 0.45, 0.5)
    for k, t in enumerate(times):
        f = 440.0 * 2.0 ** (rng.integers(0, 13) / 12.0)
        i0 = int(round(t * sr))
        x[i0:i0 + len(tt)] += 0.3 * shape * (np.sin(2 * np.pi * f * tt) + 0.5 * np.sin(4 * np.pi * f * tt)) + (bass_note if k % 4 == 2 else 0.0)
    return x.astype(np.float32), times, times[2::4]


def f_measure(found, truth, tol=TOLERANCE_S):
    """One-to-one matching of two ascending lists within +- tol -> (F, precision, recall)."""
    found, truth = sorted(found), sorted(truth)
    i = j = hits = 0
    while i < len(found) and j < len(truth):
        if abs(found[i] - truth[j]) <= tol:
            hits, i, j = hits + 1, i + 1, j + 1
        elif found[i] < truth[j]:
            i += 1
        else:
            j += 1
    p, r = (hits / len(found) if found else 0.0), (hits / len(truth) if truth else 0.0)
    return (2 * p * r / (p + r) if p + r else 0.0), p, r


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def recording(dev, seconds, decode):
    import models
    from piano_a2s_amd import audio, beats, spec, transcribe
    wave, times, bass = bursts(seconds)
    out = {"seconds": seconds, "frames": 1 + len(wave) // 160}
    with tempfile.TemporaryDirectory() as tmp:                                                   # the same music as a 44.1 kHz stereo file
        w44, _, _ = bursts(seconds, sr=44100)
        path = os.path.join(tmp, "take.wav")
        audio.write_wav(path, np.stack([w44, 0.8 * w44], axis=1), 44100, bits=16)
        t0 = time.perf_counter()
        x44, sr = audio.read_wav(path)
        out["wav_decode_ms"] = (time.perf_counter() - t0) * 1e3
    transcribe.to_16k(x44[:44100], sr, dev, HP)                                                  # untimed: table upload, first launch
    _, out["resample_ms"] = _clock(lambda: transcribe.to_16k(x44, sr, dev, HP))
    w = torch.from_numpy(wave).to(dev)
    beats.track_recording(w[:16000 * 15], HP)                                                    # untimed: VQT banks, first launches
    calls = []
    for _ in range(3):
        res, ms = _clock(lambda: beats.track_recording(w, HP))
        calls.append(ms)
    out["track_recording_ms"] = _stats(calls)
    stages = beats.hip_stages(dev)
    feats, ms_vqt = _clock(lambda: transcribe._vqt(dev, HP)(torch.zeros((len(beats.tile_plan(out["frames"], 1201)[0]), 192000), device=dev)))
    out["of_which_vqt_of_the_windows_ms"] = ms_vqt
    env = np.random.default_rng(1).random(out["frames"]).astype(np.float32)
    _, out["of_which_track_behind_the_envelopes_ms"] = _clock(lambda: beats.track(env, env, out["frames"], stages))
    inner = lambda a: [t for t in a if 2.0 <= t <= seconds - 2.0]
    out["beats"], out["downbeats"], out["beats_per_bar"] = len(res["beats_s"]), len(res["downbeats_s"]), res["beats_per_bar"]
    out["beat_f_measure"] = f_measure(inner(res["beats_s"]), inner(times))[0]
    out["downbeat_f_measure"] = f_measure(inner(res["downbeats_s"]), inner(bass))[0]
    out["periods"] = sorted(set(res["period_frames"]))
    if decode:
        cfg = spec.default_cfg()
        model = models.ScoreTranscription()
        model.load_state_dict(spec.procedural_state(cfg, 11, eos_bias=3.0, lively=True))
        model = model.to(dev).eval()
        transcribe.transcribe_waveform(model, wave[:16000 * 24], 16000, downbeats=[d for d in res["downbeats_s"] if d < 24], hparams=HP)          # untimed
        r, ms = _clock(lambda: transcribe.transcribe_waveform(model, wave, 16000, downbeats=res["downbeats_s"], hparams=HP))
        out["transcribe_with_given_downbeats_ms"], out["windows"] = ms, len(r["windows"])
        r, ms = _clock(lambda: transcribe.transcribe_waveform(model, wave, 16000, downbeats="track", hparams=HP))
        out["transcribe_with_tracked_downbeats_ms"] = ms
    return out


def rendered_clips(dev, n_clips):
    from piano_a2s_amd import beats, scoregen, spec
    from piano_a2s_amd.render import render
    cfg = spec.default_cfg()
    rows, by_sig = [], {}
    for seed in range(n_clips):
        clip = scoregen.make_clip(cfg, 5000 + seed, frames=1201)
        wave = render(torch.from_numpy(scoregen.pack_program(clip)[None]).to(dev))[0]
        res = beats.track_recording(wave, HP)
        n_beats, quarters = BEATS_PER_BAR[clip["time_sig"]]
        beat_s = quarters * clip["spq"] / 16000.0
        bars = [clip["lead"] / 16000.0 + b * n_beats * beat_s for b in range(cfg["max_bars"])]
        truth = [t + k * beat_s for t in bars for k in range(n_beats)]
        fb, fd = f_measure(res["beats_s"], truth)[0], f_measure(res["downbeats_s"], bars)[0]
        rows.append({"seed": 5000 + seed, "time_signature": clip["time_sig"], "beat_period_frames": beat_s * 100, "tracked_periods": sorted(set(res["period_frames"])),
                     "beats_per_bar": res["beats_per_bar"], "beat_f": fb, "downbeat_f": fd})
        by_sig.setdefault(clip["time_sig"], []).append((fb, fd))
    return {"clips": n_clips, "seconds_per_clip": 12.0, "tolerance_s": TOLERANCE_S, "mean_beat_f_measure": float(np.mean([r["beat_f"] for r in rows])),
            "mean_downbeat_f_measure": float(np.mean([r["downbeat_f"] for r in rows])),
            "by_time_signature": {k: {"clips": len(v), "beat_f": float(np.mean([a for a, _ in v])), "downbeat_f": float(np.mean([b for _, b in v]))}
                                  for k, v in sorted(by_sig.items())}, "per_clip": rows}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "beat_tracking.json")
    quick = len(sys.argv) > 2 and sys.argv[2] == "quick"
    if not torch.cuda.is_available():
        raise SystemExit("beat_bench: needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda:0")
    B, rows, long_frames, seconds, n_clips = (8, 201, 3001, 30.0, 2) if quick else (256, 1201, 60001, 600.0, 32)
    res = {"device": torch.cuda.get_device_name(0), "quick": quick}
    res["kernels"] = kernel_times(dev, B, rows, long_frames)
    res["tempogram_parity"] = tempogram_parity(dev)
    res["recording"] = recording(dev, seconds, decode=True)
    res["rendered_clips"] = rendered_clips(dev, n_clips)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
