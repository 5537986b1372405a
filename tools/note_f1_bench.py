#!/usr/bin/env python3
"""Cost of the note-level F1 (metrics.corpus_note_f1) with the host definition and on the device, same process, same inputs
(needs the MI355X).  Every set is scored both ways, each the best of --repeat calls, and the two results must compare equal.  The device time is
split into packing (rows -> CSR on the host), transfers + kernel (metrics.device_note_counts) and, from device events around the launch alone
with the inputs resident, the kernel.  Sets:
  valid_split   N rendered-corpus scores at the shipped max_length (synthetic.make_note_corpus), both staves, against copies with token
                substitutions, deletions and insertions at --rate: what a VALID stage scores
  small_split   the first 64 of them: where a fixed cost per call would show
  dense_398     512 bar pairs of 398 ids (the shipped max_length of the upper staff), every row nothing but notes, a line break behind every
                fourth (177 notes on 45 lines), the prediction a mutated copy: the longest row a shipped decoder can emit, about as dense as
                a row can be
  dense_1024    256 bar pairs at the kernel's capacity without a single separator, 512 notes a side: the worst case of the quadratic count
Writes profiles/note_f1_device.json and prints it.

usage: python tools/note_f1_bench.py [--clips 1024] [--rate 0.05] [--repeat 5] [--out profiles/note_f1_device.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from data_processing.humdrum import LabelsMultiple  # noqa: E402
from piano_a2s_amd import hip, metrics, synthetic  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--clips", type=int, default=1024)
ap.add_argument("--rate", type=float, default=0.05)
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "note_f1_device.json"))
args = ap.parse_args()
N, R = args.clips, args.repeat

torch.zeros(1, device="cuda")                                        # the model has run: the device path's precondition
tb = metrics.note_tables()
tabs = [torch.from_numpy(tb[k].copy()).cuda() for k in ("dur_ticks", "midi", "cls")]


def measure(target, pred):
    """One staff's dicts -> seconds of the two backends (best of R calls each) and of the launch alone."""
    metrics.NOTE_DEVICE = True
    metrics.corpus_note_f1(pred, target)                             # untimed: first launch of the process (code object load, table upload)
    launches, best = hip.note_match_launches(), None
    for _ in range(R):
        torch.cuda.synchronize()
        dev = metrics.corpus_note_f1(pred, target)
        st = dict(metrics.last_note_stats)
        assert st["backend"] == "device" and st["host_rows"] == 0, st
        best = st if best is None or st["seconds"] < best["seconds"] else best
    assert hip.note_match_launches() == launches + R
    metrics.NOTE_DEVICE = False
    host_s = []
    for _ in range(R):
        t0 = time.perf_counter()
        host = metrics.corpus_note_f1(pred, target)
        host_s.append(time.perf_counter() - t0)
    assert metrics.last_note_stats["backend"] == "host"
    metrics.NOTE_DEVICE = True
    assert host == dev, "device and host results differ"
    ref, hyp, _ = metrics._pair_rows([target[k] for k in pred], [pred[k] for k in pred])
    (ref_ids, ref_off), (hyp_ids, hyp_off) = metrics._csr_rows(ref), metrics._csr_rows(hyp)
    d = [torch.from_numpy(a).cuda() for a in (ref_ids, ref_off, hyp_ids, hyp_off)]
    res = torch.empty((len(ref), 8), dtype=torch.int32, device="cuda")
    kernel_ms = []
    for _ in range(R + 1):                                           # (the first is not counted)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip.note_match(d[0], d[1], d[2], d[3], len(ref), *tabs, res)
        e1.record()
        e1.synchronize()
        kernel_ms.append(e0.elapsed_time(e1))
    lens = np.diff(ref_off)
    return {"host_seconds": min(host_s), "host_seconds_max": max(host_s), "device_seconds": best["seconds"], "pack_seconds": best["pack_seconds"],
            "transfer_kernel_seconds": best["device_seconds"], "kernel_seconds": min(kernel_ms[1:]) / 1e3, "kernel_seconds_max": max(kernel_ms[1:]) / 1e3,
            "rows": len(ref), "mean_ids_per_row": float(lens.mean()), "max_ids_per_row": int(max(lens.max(), np.diff(hyp_off).max())),
            "notes": int(sum(v["n_ref"] for v in dev[1].values())), "f1_pitch": dev[0]["f1_pitch"], "f1_onset": dev[0]["f1_onset"], "f1_value": dev[0]["f1_value"]}


def both_staves(corpus):
    staves = {staff: measure(*corpus[staff]) for staff in ("upper", "lower")}
    row = {k: sum(s[k] for s in staves.values()) for k in ("host_seconds", "device_seconds", "pack_seconds", "transfer_kernel_seconds", "kernel_seconds", "rows")}
    row.update(speedup=row["host_seconds"] / row["device_seconds"], staves=staves)
    return row


def dense(n_pairs, n_ids, seed, per_line):
    """Rows of up to n_ids ids that are nothing but notes: DUR PITCH pairs, a line break behind every per_line-th (0: none)."""
    ids = LabelsMultiple(extended=True).labels_map
    rng = np.random.default_rng(seed)
    durs, pitches = [ids[s] for s in ("4", "8", "8.", "16", "2")], [ids[s] for s in ("c", "e", "g", "cc", "G", "d#", "b-")]
    target = {}
    for p in range(n_pairs):
        row = []
        notes = 0
        while len(row) + 2 <= n_ids:
            row += [durs[rng.integers(len(durs))], pitches[rng.integers(len(pitches))]]
            notes += 1
            if per_line and notes % per_line == 0 and len(row) + 3 <= n_ids:
                row.append(ids["\n"])
        target[f"dense{p}"] = [row]
    return target, {k: [synthetic.mutate_row(rows[0], args.rate, rng)[:n_ids]] for k, rows in target.items()}


corpus = synthetic.make_note_corpus(N, args.rate, 2024)
out = {"clips": N, "rate": args.rate, "repeat": R, "capacity_ids": metrics.note_match_capacity(), "sets": {}}
out["sets"]["valid_split"] = both_staves(corpus)
small = {staff: tuple({k: d[k] for k in list(d)[:64]} for d in corpus[staff]) for staff in ("upper", "lower")}
out["sets"]["small_split"] = dict(both_staves(small), clips=min(64, N))
for name, n_pairs, n_ids, per_line in (("dense_398", 512, 398, 4), ("dense_1024", 256, 1024, 0)):
    out["sets"][name] = measure(*dense(n_pairs, n_ids, 7, per_line))
    out["sets"][name]["kernel_us_per_pair"] = out["sets"][name]["kernel_seconds"] / n_pairs * 1e6
for name, row in out["sets"].items():
    print(name, json.dumps({k: v for k, v in row.items() if k != "staves"}), flush=True)
v = out["sets"]["valid_split"]
out["host_ms_per_clip"], out["device_ms_per_clip"] = v["host_seconds"] / N * 1e3, v["device_seconds"] / N * 1e3
out["note"] = ("host_seconds / device_seconds = best of `repeat` whole calls of corpus_note_f1 each (device: pairing and packing on the host, transfers, "
               "kernel, per-clip sums and floats); kernel_seconds = the launch alone between device events, inputs resident, best of `repeat`; the split "
               "sets are both staves together")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
