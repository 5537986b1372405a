#!/usr/bin/env python3
"""Greedy-decode throughput (BASELINE.json configs[4]): batched 12 s clips -> Kern tokens on one MI355X, eval mode, procedural
weights with <eos> bias so decoding terminates at data-dependent steps.  Prints one JSON line (clips/s, tokens/s, decode steps).

    infer_bench.py [B]                  greedy as shipped
    infer_bench.py [B] --stepwise       greedy forced onto the launch-per-step loop (dec_persist 0, dec_fused 0)
    infer_bench.py [B] --constrained    greedy under the kern token grammar (Engine.kern_grammar)
    infer_bench.py [B] --metrical       ... and under the metre of each bar's predicted time signature (Engine.kern_metre)
    infer_bench.py --compare OUT.json [--batches 256,8] [--repeats 3]
                                        the variants (i) greedy, (ii) stepwise, (iii) constrained, (iv) metrical in ONE process, alternating, `repeats`
                                        timed forwards each (after one warm-up each): one JSON line per forward, the summary (median, spread) to
                                        OUT.json.  The variants decode different token sequences of different lengths: their times do not compare
                                        like for like (tools/metre_epilogue_bench.py times the two epilogues on the same logits)
    infer_bench.py --compare OUT.json --beam [--batches 256,8] [--repeats 3]
                                        the same for beam search (Engine.beam_size), all under the kern grammar: constrained
                                        greedy on the launch-per-step loop (the like-for-like baseline, run twice per round: its spread against
                                        itself is the margin of every comparison), the beam loop forced at K = 1, K = 2 and K = 4
    infer_bench.py --compare OUT.json --align [--batches 256,8] [--repeats 3]
                                        the same for the audio alignment (Engine.alignment): greedy as shipped (twice per round), greedy
                                        forced onto the launch-per-step loop, and greedy with alignment"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from piano_a2s_amd import engine, hip, spec, synthetic
from piano_a2s_amd.kern_grammar import KernGrammar, KernMetre, complete_share, legal_share

ap = argparse.ArgumentParser()
ap.add_argument("batch", nargs="?", type=int, default=64)
ap.add_argument("--constrained", action="store_true")
ap.add_argument("--metrical", action="store_true")
ap.add_argument("--stepwise", action="store_true")
ap.add_argument("--compare", metavar="OUT.json")
ap.add_argument("--beam", action="store_true")
ap.add_argument("--align", action="store_true")
ap.add_argument("--batches", default="256,8")
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()

dev = torch.device("cuda:0")
cfg = spec.default_cfg()
S = {k: v.to(dev) for k, v in spec.procedural_state(cfg, 2032, eos_bias=2.5, lively="token").items()}
GRAMMAR = KernGrammar()
METRE = KernMetre(GRAMMAR)
L = hip.lib()


def set_stepwise(on):
    for key in (b"dec_persist", b"dec_fused"):
        hip.check(L.a2s_debug_set(key, 0 if on else 1), "a2s_debug_set")


def forward(x, variant):
    """One timed forward of `variant` ("greedy", "greedy_again", "stepwise", "align", "constrained", "constrained_again", "beam1", "beam2" or "beam4") -> the
    record of the run."""
    set_stepwise(variant == "stepwise")
    eng = engine.Engine(cfg)
    eng.alignment = variant == "align"
    eng.kern_grammar = GRAMMAR if variant.startswith(("constrained", "beam", "metrical")) else None
    eng.kern_metre = METRE if variant == "metrical" else None
    eng.beam_size = int(variant[4:]) if variant.startswith("beam") else 1
    engine._BEAM_FORCE = variant == "beam1"                 # one slot through the beam loop: what the loop itself costs
    n0, g0, b0, a0, m0 = L.a2s_launch_count(), hip.grammar_launches(), hip.beam_launches(), hip.align_launches(), hip.metre_launches()
    torch.cuda.synchronize(); t0 = time.time()
    try:
        with torch.no_grad():
            ts, key, up, lo = eng.forward(S, x, inference=True)
        torch.cuda.synchronize(); dt = time.time() - t0
    finally:
        engine._BEAM_FORCE = False
    set_stepwise(False)
    B = x.shape[0]
    calls = [b["staff"][k][2] for b in eng.saved["bars"] for k in ("up", "lo")]
    steps, launched = sum(c["steps"] for c in calls), sum(c["launched"] for c in calls)
    tokens = int((up.abs().sum(-1) > 0).sum() + (lo.abs().sum(-1) > 0).sum())
    if eng.decoded is not None:
        ids = {k: eng.decoded[k][0].cpu().numpy() for k in ("up", "lo")}
    else:
        ids = {"up": up.argmax(-1).cpu().numpy(), "lo": lo.argmax(-1).cpu().numpy()}
    from piano_a2s_amd import metrics
    rows = {k: [metrics.unpad(r).tolist() for clip in v for r in clip] for k, v in ids.items()}
    ts_rows = [int(t) for clip in ts.argmax(-1).cpu().numpy() for t in clip]          # one predicted time signature per (clip, bar), in the order of `rows`
    return {"metric": "greedy decode clips/s", "variant": variant, "batch": B, "seconds": round(dt, 4), "clips_per_s": round(B / dt, 2),
            "decoded_token_rows_per_s": round(tokens / dt), "executed_steps": steps, "launched_steps": launched,
            "us_per_executed_step": round(1e6 * dt / max(steps, 1), 2),
            # every launch of the forward (ConvStack, encoder and bar level included) over the decode steps it launched
            "launches_per_launched_step": round((L.a2s_launch_count() - n0) / max(launched, 1), 2),
            "grammar_epilogues": hip.grammar_launches() - g0, "beam_epilogues": hip.beam_launches() - b0, "align_launches": hip.align_launches() - a0, "persistent_calls": sum(c.get("persist_ws") is not None for c in calls),
            "metre_epilogues": hip.metre_launches() - m0,
            "well_formed_bar_share": round(legal_share(rows, GRAMMAR), 4),
            # bars that are complete under the time signature predicted for them (a row cut at max_length is a prefix, not a complete bar)
            "complete_bars": round(complete_share(rows, {k: ts_rows for k in rows}, METRE), 4)}


if args.compare:
    variants = ("constrained", "constrained_again", "beam1", "beam2", "beam4") if args.beam else ("greedy", "stepwise", "constrained", "metrical")
    if args.align:
        variants = ("greedy", "greedy_again", "stepwise", "align")
    what = ("constrained greedy on the launch-per-step loop (twice: its spread against itself) / the beam loop at K = 1 (forced), 2 and 4, all under the "
            "kern grammar" if args.beam else "greedy as shipped (twice: its spread against itself) / forced onto the launch-per-step loop / with the audio alignment"
            if args.align else "greedy as shipped / forced onto the launch-per-step loop / under the kern grammar / under the grammar and the metre of each bar's "
            "predicted time signature (the variants decode different sequences: their times do not compare like for like)")
    summary = {"what": f"tools/infer_bench.py --compare: {what}; one process, variants alternating, median of the timed forwards", "repeats": args.repeats,
               "batches": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        x = synthetic.make_batch(B, cfg, 77, spectrogram="ridges", full_tail=0.0)[0].to(dev)
        runs = {v: [] for v in variants}
        for v in variants:
            forward(x, v)                                   # warm-up
            torch.cuda.empty_cache()                        # (a beam call holds K times the buffers of a greedy one)
        for _ in range(args.repeats):
            for v in variants:
                rec = forward(x, v)
                print(json.dumps(rec), flush=True)
                runs[v].append(rec)
        out = {}
        for v in variants:
            secs = [r["seconds"] for r in runs[v]]
            med = statistics.median(secs)
            out[v] = dict(runs[v][-1], seconds=med, seconds_all=secs, clips_per_s=round(B / med, 2),
                          us_per_executed_step=round(1e6 * med / max(runs[v][-1]["executed_steps"], 1), 2),
                          spread=round((max(secs) - min(secs)) / med, 4))
            del out[v]["decoded_token_rows_per_s"]
        summary["batches"][str(B)] = out
    os.makedirs(os.path.dirname(os.path.abspath(args.compare)), exist_ok=True)
    with open(args.compare, "w") as f:
        json.dump(summary, f, indent=1)
else:
    variant = "metrical" if args.metrical else "constrained" if args.constrained else ("stepwise" if args.stepwise else "greedy")
    x = synthetic.make_batch(args.batch, cfg, 77, spectrogram="ridges", full_tail=0.0)[0].to(dev)
    for it in range(3):
        rec = forward(x, variant)
    print(json.dumps(rec))
