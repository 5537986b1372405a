#!/usr/bin/env python3
"""Cost of scoring a validation split (metrics.corpus_wer, both staves) on the host loop and on the device, same process, same inputs, and
the greedy decode rate it has to stay under (needs the MI355X).  N synthetic 5-bar clips at the benchmark's length distribution
(synthetic.make_wer_corpus) with two hypothesis sets: "near" = the targets with about 10 % of the tokens dropped / substituted, "no_eos" =
398 / 189 random ids per bar (what an untrained decoder leaves after metrics.unpad).  The two results must compare equal.  Writes
profiles/wer_device.json and prints it.

usage: python tools/wer_bench.py [--clips 512] [--host-clips N] [--decode-rate CLIPS_PER_S] [--out profiles/wer_device.json]
  --host-clips   time the host loop on the first N clips only (the device result of those clips is compared; default: all)
  --decode-rate  greedy decoding at B = 256 in clips/s as tools/infer_bench.py 256 reports it on this box (default: run it, in a child process)"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from data_processing.humdrum import LabelsMultiple  # noqa: E402
from piano_a2s_amd import hip, metrics, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--clips", type=int, default=512)
ap.add_argument("--host-clips", type=int, default=0)
ap.add_argument("--decode-rate", type=float, default=0.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wer_device.json"))
args = ap.parse_args()
N = args.clips
M = args.host_clips or N

decode = {"clips_per_s": args.decode_rate, "source": "--decode-rate"}
if not args.decode_rate:
    # a process of its own, before this one opens the GPU
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "infer_bench.py"), "256"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    if r.returncode != 0:
        sys.exit(f"tools/infer_bench.py 256 failed ({r.returncode}):\n{r.stderr[-2000:]}")
    line = json.loads(r.stdout.strip().splitlines()[-1])
    decode = {"clips_per_s": line["clips_per_s"], "source": "tools/infer_bench.py 256, same box, before this run", "line": line}
decode["ms_per_clip"] = 1e3 / decode["clips_per_s"]
print("decode", json.dumps(decode), flush=True)

inv = LabelsMultiple(extended=True).labels_map_inv
corpus = synthetic.make_wer_corpus(N, 2024)
torch.zeros(1, device="cuda")                                        # the model has run: the device path's precondition
L = hip.lib()
out = {"clips": N, "host_clips": M, "capacity_words": metrics.edit_distance_capacity(), "decode": decode, "sets": {}}
for name, pick in (("near", 1), ("no_eos", 2)):
    row = {"host_seconds": 0.0, "device_seconds": 0.0, "pack_seconds": 0.0, "transfer_kernel_seconds": 0.0, "pairs": 0, "host_pairs": 0, "staves": {}}
    for staff in ("upper", "lower"):
        target = corpus[staff][0]
        pred = {k: [metrics.unpad(r).tolist() for r in rows] for k, rows in corpus[staff][pick].items()}
        metrics.WER_DEVICE = True
        metrics.corpus_wer(pred, target, inv)                        # untimed: first launch of the process (code object load)
        launches = L.a2s_debug_get(b"edit_distance_launches")
        best = None
        for _ in range(3):
            torch.cuda.synchronize()
            dev = metrics.corpus_wer(pred, target, inv)
            st = dict(metrics.last_wer_stats)
            assert st["backend"] == "device" and st["host_pairs"] == 0, st
            best = st if best is None or st["seconds"] < best["seconds"] else best
        assert L.a2s_debug_get(b"edit_distance_launches") == launches + 3
        keys = list(pred)[:M]
        metrics.WER_DEVICE = False
        t0 = time.perf_counter()
        host = metrics.corpus_wer({k: pred[k] for k in keys}, {k: target[k] for k in keys}, inv)
        host_s = time.perf_counter() - t0
        assert metrics.last_wer_stats["backend"] == "host"
        assert host[1] == {k: dev[1][k] for k in keys}, f"{name} {staff}: device and host results differ"
        if M == N:
            assert host == dev
        ref_w, ref_o, table = metrics.pack_words([target[k] for k in pred], inv)
        hyp_w, hyp_o, _ = metrics.pack_words([pred[k] for k in pred], inv, table)
        row["staves"][staff] = {"host_seconds": host_s, "host_clips": len(keys), "device_seconds": best["seconds"], "pack_seconds": best["pack_seconds"],
                                "transfer_kernel_seconds": best["device_seconds"], "mean_wer": dev[0],
                                "mean_ref_words": float(ref_o[-1]) / N, "mean_hyp_words": float(hyp_o[-1]) / N}
        row["host_seconds"] += host_s * N / len(keys)
        row["device_seconds"] += best["seconds"]
        row["pack_seconds"] += best["pack_seconds"]
        row["transfer_kernel_seconds"] += best["device_seconds"]
        row["pairs"] += N
        print(name, staff, json.dumps(row["staves"][staff]), flush=True)
    row["host_ms_per_clip"] = row["host_seconds"] / N * 1e3
    row["device_ms_per_clip"] = row["device_seconds"] / N * 1e3
    row["speedup"] = row["host_seconds"] / row["device_seconds"]
    row["under_decode_time"] = row["device_ms_per_clip"] < decode["ms_per_clip"]
    out["sets"][name] = row
metrics.WER_DEVICE = True
out["note"] = ("per set: both staves together; host_seconds scaled from host_clips to clips when fewer were timed; device_seconds = best of 3 calls of "
               "corpus_wer including packing and transfers; the bar is device_ms_per_clip < decode.ms_per_clip")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
