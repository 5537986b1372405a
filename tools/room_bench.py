"""The room acoustics of the rendered corpus, timed: python tools/room_bench.py [batch] [reps] [out.json] [step_ms]

At `batch` 12 s generator clips with the default rooms, in milliseconds per batch (device events around `reps` calls after a warm-up, five windows
each): room_ir alone, fir_rows alone (with the FMAs it executes, its FLOP/s and its share of the 157.3 TFLOP/s fp32 vector roof), the render kernel,
program -> features without and with the room, and the same convolution through torch.fft (rfft of waveforms and impulse responses, product, irfft)
on the same tensors, with its largest difference from fir_rows.  Then the feature change dry against room, on the device: mean and largest |change|
in dB (x 80).  `step_ms`: the training step's milliseconds from a `bench.py` run made beside this one (same batch); the result then also holds the
times as shares of that step."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FP32_ROOF = 157.3e12


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


def fir_fmas(n_samples, L, tile):
    """The FMAs fir_rows executes: per tile at t0 the taps below min(L, t0 + tile), in blocks of 8, for all `tile` samples of the tile."""
    total = 0
    for t0 in range(0, n_samples, tile):
        leff = np.minimum(L, t0 + tile)
        total += int(((leff + 7) // 8 * 8).sum()) * tile
    return total


def main():
    from piano_a2s_amd import hip, scoregen, spec
    from piano_a2s_amd.render import render
    from piano_a2s_amd.room import Room, room_seeds
    from piano_a2s_amd.vqt import VQT
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    path = sys.argv[3] if len(sys.argv) > 3 else None
    step_ms = float(sys.argv[4]) if len(sys.argv) > 4 else None
    cfg = spec.default_cfg()
    progs = np.stack([scoregen.pack_program(scoregen.make_clip(cfg, 1234 + i)) for i in range(B)])
    n = int(progs[0, 0, 0])
    seeds = room_seeds(progs)
    room = Room()
    table = room.params(seeds)
    L = table[:, 1].astype(np.int64)
    tile = hip.fir_tile_samples()
    fmas = fir_fmas(n, L, tile)
    Lc = np.minimum(L, n)
    needed = int((Lc * (Lc + 1) // 2 + (n - Lc) * Lc).sum())             # the definition's products: sum_n min(L, n + 1) per clip
    dev = torch.device("cuda:0")
    P = torch.from_numpy(progs).to(dev)
    front = VQT(dev)
    wave = render(P, n)
    for _ in range(2):                                                     # warm-up of every shape
        front(room.apply(render(P, n), seeds))
        front(render(P, n))
    ir, params = room.impulse_responses(seeds, dev)
    ir, params = ir.clone(), params.clone()
    dseeds = torch.from_numpy(seeds.view(np.int32)).to(dev)
    y = torch.empty_like(wave)
    n_fft = 204800                                                         # 2^13 * 25 >= n + L_max - 1
    assert n_fft >= n + room.L_max - 1

    def fft_conv():
        return torch.fft.irfft(torch.fft.rfft(wave, n=n_fft) * torch.fft.rfft(ir, n=n_fft), n=n_fft)[:, :n]

    hip.fir_rows(wave, ir, params, room.L_max, y=y)
    ref = fft_conv()
    fft_diff = float((ref - y).abs().max())
    del ref
    torch.cuda.synchronize()
    k0 = hip.room_launches()
    t_ir = _timed(lambda: hip.room_ir(dseeds, params, room.L_max, ir=ir), reps * 4)
    t_fir = _timed(lambda: hip.fir_rows(wave, ir, params, room.L_max, y=y), reps)
    assert hip.room_launches() == k0 + 5 * reps * 4 + 5 * reps
    t_fft = _timed(fft_conv, reps)
    t_render = _timed(lambda: render(P, n), reps)
    t_dry = _timed(lambda: front(render(P, n)), max(1, reps // 2))
    t_room = _timed(lambda: front(room.apply(render(P, n), seeds)), max(1, reps // 2))
    dry = front(render(P, n))
    wet = front(room.apply(render(P, n), seeds))
    change = (wet - dry).abs() * 80.0
    per_clip = change.flatten(1).mean(dim=1)
    fir_s = float(np.median(t_fir)) * 1e-3
    res = {"batch": B, "seconds_per_clip": n / 16000, "room": room.describe(), "taps_per_clip": {"mean": float(L.mean()), "min": int(L.min()), "max": int(L.max())},
           "fir_tile_samples": tile, "fir_tap_chunk": hip.fir_tap_chunk(),
           "room_ir_ms": _ms(t_ir, reps * 4), "fir_rows_ms": _ms(t_fir, reps),
           "fir_fmas_executed_per_batch": fmas, "fir_products_of_the_definition_per_batch": needed,
           "fir_tflops_executed": 2 * fmas / fir_s / 1e12, "fir_tflops_of_the_definition": 2 * needed / fir_s / 1e12,
           "fp32_roof_tflops": FP32_ROOF / 1e12, "fir_share_of_fp32_roof_executed": 2 * fmas / fir_s / FP32_ROOF,
           "fir_share_of_fp32_roof_of_the_definition": 2 * needed / fir_s / FP32_ROOF, "fir_floor_ms_at_the_roof": 2 * needed / FP32_ROOF * 1e3,
           "torch_fft_conv_ms": _ms(t_fft, reps), "torch_fft_n": n_fft, "torch_fft_max_abs_difference_from_fir_rows": fft_diff,
           "fir_over_torch_fft": float(np.median(t_fir)) / float(np.median(t_fft)),
           "render_ms": _ms(t_render, reps), "program_to_features_ms": _ms(t_dry, max(1, reps // 2)),
           "program_to_features_with_room_ms": _ms(t_room, max(1, reps // 2)),
           "feature_change_db": {"mean": float(change.mean()), "max": float(change.max()), "per_clip_mean_min": float(per_clip.min()),
                                 "per_clip_mean_max": float(per_clip.max())},
           "device": torch.cuda.get_device_name(0)}
    if step_ms:
        res.update(training_step_ms=step_ms, fir_share_of_step=res["fir_rows_ms"]["median"] / step_ms, room_ir_share_of_step=res["room_ir_ms"]["median"] / step_ms,
                   program_to_features_share_of_step=res["program_to_features_ms"]["median"] / step_ms,
                   program_to_features_with_room_share_of_step=res["program_to_features_with_room_ms"]["median"] / step_ms)
    print(json.dumps(res))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
