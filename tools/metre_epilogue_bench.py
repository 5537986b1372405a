#!/usr/bin/env python3
"""What the metre predicate costs in the step epilogue, like for like: a2s_grammar_argmax_rows against a2s_metre_argmax_rows
on the SAME logits and syntax states, the rows at the start of a note of a 4/4 bar (state START, nothing sounding), where every lane that holds a
duration symbol reads `fillable`.

    metre_epilogue_bench.py OUT.json [--rows 256,8] [--launches 400] [--windows 15]

Event-timed windows of `launches` back-to-back launches, the two kernels alternating window by window after one warm-up window each; every launch
of a window works on its own copy of the states (the op moves a row on), restored outside the timed region.  Median and spread
((max - min) / median) of the per-launch time per kernel, and their ratio, go to OUT.json (merged into it when it exists, under "metre_epilogue").
The time of one launch in a stream of launches is what a decode step pays; it is not the kernel's busy time."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from piano_a2s_amd import hip
from piano_a2s_amd.kern_grammar import KernMetre

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--rows", default="256,8")
ap.add_argument("--launches", type=int, default=400)
ap.add_argument("--windows", type=int, default=15)
args = ap.parse_args()

dev = torch.device("cuda:0")
metre = KernMetre()
V = metre.grammar.vocab_size
table = metre.grammar.device_table(dev)
L = hip.lib()
result = {"what": "a2s_grammar_argmax_rows vs a2s_metre_argmax_rows on the same logits, rows at the start of a note in 4/4 (y written, V = 173): "
                  "microseconds per launch in event-timed windows of back-to-back launches, the two alternating", "launches_per_window": args.launches,
          "windows": args.windows, "rows": {}}
for R in [int(r) for r in args.rows.split(",")]:
    g = torch.Generator(device="cpu").manual_seed(R)
    x = (torch.rand((R, V), generator=g) * 2 - 1).to(dev)
    y = torch.empty((R, V), device=dev)
    n = args.launches
    state0 = torch.full((n, R), metre.grammar.start, dtype=torch.int32, device=dev)
    rows0 = hip.metre_rows(metre, torch.zeros(R, dtype=torch.int32, device=dev)).repeat(n, 1, 1).contiguous()
    state, rows = state0.clone(), rows0.clone()

    # the argument lists of every launch are made here, outside the timed region: inside it the host does one library call per launch, the same for both
    choice = torch.empty(R, dtype=torch.int32, device=dev)
    head = (hip._p(x), x.stride(0), hip._p(y), y.stride(0), hip._p(table), table.shape[0])
    calls = {"grammar": [(L.a2s_grammar_argmax_rows, head + (hip._p(state[i]), hip._p(choice), R, V)) for i in range(n)],
             "metre": [(L.a2s_metre_argmax_rows, head + (hip._p(state[i]), *hip.metre_ref(metre, rows[i]), hip._p(choice), R, V)) for i in range(n)]}

    def window(kind):
        state.copy_(state0)
        rows.copy_(rows0)
        torch.cuda.synchronize()
        st = hip.stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = 0
        for fn, a in calls[kind]:
            rc |= fn(st, *a)
        e1.record()
        torch.cuda.synchronize()
        hip.check(rc, kind)
        return 1e3 * e0.elapsed_time(e1) / n

    # the same choice where the metre forbids nothing the syntax allows on top: checked once, on the first copy
    a, b = hip.grammar_argmax_rows(x, table, state0[0].clone(), y=y), hip.metre_argmax_rows(x, table, state0[0].clone(), metre, rows0[0].clone(), y=y)
    same = float((a == b).float().mean())
    times = {"grammar": [], "metre": []}
    for kind in times:
        window(kind)
    for _ in range(args.windows):
        for kind in times:
            times[kind].append(window(kind))
    rec = {}
    for kind, t in times.items():
        med = statistics.median(t)
        rec[kind] = {"us_per_launch": round(med, 3), "spread": round((max(t) - min(t)) / med, 4), "all": [round(v, 3) for v in t]}
    rec["ratio_metre_over_grammar"] = round(rec["metre"]["us_per_launch"] / rec["grammar"]["us_per_launch"], 4)
    rec["rows_with_the_same_choice"] = same
    print(json.dumps({"R": R, **{k: v for k, v in rec.items() if k != "all"}}), flush=True)
    result["rows"][str(R)] = rec

merged = {}
if os.path.exists(args.out):
    with open(args.out) as f:
        merged = json.load(f)
merged["metre_epilogue"] = result
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(merged, f, indent=1)
