"""The synthesiser of the rendered synthetic corpus, timed: python tools/render_bench.py [batch] [reps] [out.json] [step_ms]

Milliseconds per batch of `batch` 12 s clips at the generator's default density -- the render kernel alone, and program -> features (render + VQT) --
with device events around `reps` calls after a warm-up; and the host time per generated clip (score, events, program).  `step_ms`: the training
step's milliseconds from a `bench.py` run made beside this one (same batch); the result then also holds both times as shares of that step."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, reps, rounds=5):
    """Milliseconds per call: `rounds` windows of `reps` calls between two device events."""
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out


def main():
    from piano_a2s_amd import hip, scoregen, spec
    from piano_a2s_amd.render import render
    from piano_a2s_amd.vqt import VQT
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    path = sys.argv[3] if len(sys.argv) > 3 else None
    step_ms = float(sys.argv[4]) if len(sys.argv) > 4 else None
    cfg = spec.default_cfg()
    t0 = time.perf_counter()
    clips = [scoregen.make_clip(cfg, 1234 + i) for i in range(B)]
    progs = np.stack([scoregen.pack_program(c) for c in clips])
    host_ms = (time.perf_counter() - t0) / B * 1e3
    events = np.array([len(c["events"]) for c in clips])
    tokens = np.array([sum(len(b) for s in ("upper", "lower") for b in c["ids"][s]) for c in clips])
    n = int(progs[0, 0, 0])
    # partial-samples the kernel evaluates: per event (length + release, cut at the clip's end) x the partials below the Nyquist frequency
    sines = 0
    for c, p in zip(clips, progs):
        for i in range(1, 1 + len(c["events"])):
            inc = int(p[i, 2:3].view(np.uint32)[0])
            sines += min(n - int(p[i, 0]), int(p[i, 1]) + int(p[0, 3])) * min(int(p[i, 6]), (2 ** 31 - 1) // inc)
    dev = torch.device("cuda:0")
    P = torch.from_numpy(progs).to(dev)
    front = VQT(dev)
    for _ in range(3):                                                     # warm-up of both shapes
        front(render(P, n))
    torch.cuda.synchronize()
    k0 = hip.render_launches()
    kernel = _timed(lambda: render(P, n), reps)
    assert hip.render_launches() == k0 + 5 * reps
    both = _timed(lambda: front(render(P, n)), max(1, reps // 4))
    res = {"batch": B, "seconds_per_clip": n / 16000, "rows_per_clip": int(progs.shape[1]), "program_bytes_per_batch": int(progs.nbytes),
           "events_per_clip_mean": float(events.mean()), "events_per_clip_max": int(events.max()), "tokens_per_clip_mean": float(tokens.mean()),
           "partial_samples_per_batch": int(sines), "render_ms": {"median": float(np.median(kernel)), "min": min(kernel), "max": max(kernel), "windows": kernel, "calls_per_window": reps},
           "render_gsines_per_s": sines / (float(np.median(kernel)) * 1e-3) / 1e9,
           "program_to_features_ms": {"median": float(np.median(both)), "min": min(both), "max": max(both), "windows": both},
           "generator_host_ms_per_clip": host_ms, "device": torch.cuda.get_device_name(0)}
    if step_ms:
        res.update(training_step_ms=step_ms, render_share_of_step=res["render_ms"]["median"] / step_ms,
                   program_to_features_share_of_step=res["program_to_features_ms"]["median"] / step_ms)
    print(json.dumps(res))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
