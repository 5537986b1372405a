"""The resampler in front of the VQT, timed: python tools/resample_bench.py OUT.json [step_ms]

256 clips of 12 s at 44.1 kHz stereo and at 48 kHz mono, in milliseconds per batch (device events around `reps` calls after a warm-up, five windows
each): a2s_resample_rows, with the FMAs of its definition, its FLOP/s against the 157.3 TFLOP/s fp32 vector roof and the bytes it must move against
the 8 TB/s of the HBM; beside it a plain-torch restatement on the same tensors (the mono mix, then one strided conv1d per phase group -- a single one
for L = 1), with its largest difference from the kernel.  Then file to features for a 10-minute recording at 44.1 kHz stereo, stage by stage (host
clock around work that ends in a device synchronise).  `step_ms`: the training step's milliseconds from a `bench.py` run made beside this one; the
result then also holds the resampler's time as a share of that step."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FP32_ROOF = 157.3e12
HBM_ROOF = 8.0e12


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


def _ms(windows, reps):
    return {"median": float(np.median(windows)), "min": min(windows), "max": max(windows), "windows": windows, "calls_per_window": reps}


def torch_resample(x, C, table, L, M, Hh, n_out):
    """The definition through torch: x (B, N * C) -> (B, n_out).  Outputs n0 + r L (r = 0, 1, ...) share the phase p = n0 M mod L and their inputs lie
    M apart: one conv1d of stride M per n0."""
    B = x.shape[0]
    K = table.shape[1]
    mono = x.view(B, -1, C).sum(dim=2) * (1.0 / C) if C > 1 else x
    reach = K + M
    xp = torch.nn.functional.pad(mono, (reach, reach + M))[:, None, :]
    y = torch.empty((B, n_out), dtype=torch.float32, device=x.device)
    w = table.flip(1)[:, None, :]                                           # conv1d correlates: w[j] = table[p][K - 1 - j]
    for n0 in range(min(L, n_out)):
        q = n0 * M
        p, m0 = q % L, q // L
        count = (n_out - n0 + L - 1) // L
        start = reach + m0 + Hh - (K - 1)
        seg = xp[:, :, start:start + (count - 1) * M + K]
        y[:, n0::L] = torch.nn.functional.conv1d(seg, w[p:p + 1], stride=M)[:, 0, :count]
    return y


def kernel_case(dev, sr, C, B, seconds, reps, torch_reps):
    from piano_a2s_amd import audio, hip
    rs = audio.Resampler(dev, sr)
    N = int(sr * seconds)
    n_out = rs.n_out(N)
    gen = torch.Generator(device=dev).manual_seed(sr)
    x = torch.rand((B, N * C), dtype=torch.float32, device=dev, generator=gen) * 2.0 - 1.0
    n_in = torch.full((B,), N, dtype=torch.int32, device=dev)
    y = torch.empty((B, n_out), dtype=torch.float32, device=dev)
    run = lambda: hip.resample_rows(x, n_in, rs.table, rs.M, rs.Hh, channels=C, y=y, n_out_max=n_out, n_in_max=N)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    k0 = hip.resample_launches()
    t_k = _timed(run, reps)
    assert hip.resample_launches() == k0 + 5 * reps
    fmas = B * n_out * rs.K
    nbytes = 4 * (B * N * C + B * n_out) + rs.table.numel() * 4
    sec = float(np.median(t_k)) * 1e-3
    floor_s = max(2 * fmas / FP32_ROOF, nbytes / HBM_ROOF)
    res = {"sample_rate_in": sr, "channels": C, "batch": B, "seconds_per_clip": seconds, "L": rs.L, "M": rs.M, "K": rs.K, "table_bytes": rs.table.numel() * 4,
           "n_out_per_clip": n_out, "tile_samples": hip.resample_tile_samples(), "resample_rows_ms": _ms(t_k, reps), "fmas_of_the_definition_per_batch": fmas,
           "bytes_moved_per_batch": nbytes, "tflops": 2 * fmas / sec / 1e12, "share_of_fp32_roof": 2 * fmas / sec / FP32_ROOF, "gb_per_s": nbytes / sec / 1e9,
           "share_of_hbm_roof": nbytes / sec / HBM_ROOF, "bound_by": "fp32" if 2 * fmas / FP32_ROOF >= nbytes / HBM_ROOF else "hbm",
           "floor_ms_at_the_roofs": floor_s * 1e3, "share_of_the_floor": floor_s / sec}
    try:
        ref = torch_resample(x, C, rs.table, rs.L, rs.M, rs.Hh, n_out)
        res["torch_max_abs_difference_from_the_kernel"] = float((ref - y).abs().max())
        del ref
        torch.cuda.synchronize()
        t_t = _timed(lambda: torch_resample(x, C, rs.table, rs.L, rs.M, rs.Hh, n_out), torch_reps, rounds=3)
        res["torch_conv1d_ms"] = _ms(t_t, torch_reps)
        res["kernel_over_torch"] = float(np.median(t_k)) / float(np.median(t_t))
    except RuntimeError as e:                                                # (the restatement is a yardstick, not the product: say so and go on)
        res["torch_conv1d_ms"] = None
        res["torch_error"] = str(e).splitlines()[0][:200]
    return res


def file_to_features(dev, minutes=10.0, sr=44100, C=2):
    """A recording of `minutes` on disk (PCM16) -> the features of its 12 s windows: every stage by the host clock, each ended by a synchronise."""
    from piano_a2s_amd import audio
    from piano_a2s_amd.vqt import VQT
    rng = np.random.default_rng(1)
    x = (rng.uniform(-0.5, 0.5, size=(int(minutes * 60 * sr), C))).astype(np.float32)
    front = VQT(dev)
    rs = audio.Resampler(dev, sr)
    out = {"minutes": minutes, "sample_rate_in": sr, "channels": C}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "recording.wav")
        audio.write_wav(path, x, sr)
        out["file_bytes"] = os.path.getsize(path)
        for attempt in ("first", "second"):                                  # the first pass warms every shape up
            stages = {}
            t = time.perf_counter()
            data, rate = audio.read_wav(path)
            stages["read_wav_ms"] = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            d = torch.from_numpy(data).to(dev)[None]
            torch.cuda.synchronize()
            stages["to_device_ms"] = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            wave, n_out = rs(d)
            torch.cuda.synchronize()
            stages["resample_ms"] = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            plan = audio.plan_windows(wave.shape[1])
            win = audio.cut_windows(wave[0], plan, 192000)
            torch.cuda.synchronize()
            stages["cut_windows_ms"] = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            feats = front(win)
            torch.cuda.synchronize()
            stages["vqt_ms"] = (time.perf_counter() - t) * 1e3
            stages["total_ms"] = sum(stages.values())
            stages["windows"] = len(plan)
            stages["features_shape"] = list(feats.shape)
            out[attempt + "_pass"] = stages
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else None
    step_ms = float(sys.argv[2]) if len(sys.argv) > 2 else None
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "fp32_roof_tflops": FP32_ROOF / 1e12, "hbm_roof_gb_per_s": HBM_ROOF / 1e9,
           "cases": [kernel_case(dev, 44100, 2, 256, 12.0, 10, 2), kernel_case(dev, 48000, 1, 256, 12.0, 10, 2)],
           "file_to_features": file_to_features(dev)}
    if step_ms:
        res["training_step_ms"] = step_ms
        for c in res["cases"]:
            c["share_of_step"] = c["resample_rows_ms"]["median"] / step_ms
    print(json.dumps(res))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
