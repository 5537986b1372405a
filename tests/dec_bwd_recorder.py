"""engine_bwd._note_decoder_bwd (and _note_decoder_bwd_pair) driven without a GPU, on the stand-ins of tests/abi_recorder.py: one decode call's backward
-- or a segment's two -- on CPU tensors of the real layouts, then the late entries run as Backward.finish runs them (wait for the entry's event,
record every tensor it holds on the weight-gradient stream, call the closure).  Beside the library calls the trace holds:
  ("index_select", source, index)   every gather; its result is labelled source@index, so a product shows which live index its operand came from
  ("record_stream", stream, [...])  the tensors one late entry made the weight-gradient stream record, sorted (their order carries no meaning)
  ("return", label)                 the gradient wrt the initial hidden the call handed back
and the argument block of a2s_note_decoder_bwd as {field: value}.  torch.maximum's result is labelled max(a,b), the unit scalar "one", the host arrays
of the row plan active.<key>.  tests/test_dec_bwd_plan_cpu.py asserts the wiring on these traces; run as a script (python -m tests.dec_bwd_recorder
OUT.json) it writes the traces of the whole case matrix, to compare two commits case by case: it reads _note_decoder_bwd's signature, so the same file
drives the function as it was before dec_bwd_plan.py existed."""
import ctypes as C
import inspect
import itertools
import json
import sys
from types import SimpleNamespace
from unittest import mock

import torch

from tests import abi_recorder

CLIPS, STEPS, T, E, MAX_STEPS = 3, 5, 5, 6, 8
# (bars of the segment, clips) -> the step each row's targets run out at; the live pairs are sum(min(until, STEPS)) of STEPS * rows
UNTIL = {1: {"dense": [[5, 5, 5]], "at 0.8": [[5, 5, 2]], "below 0.8": [[5, 5, 1]], "sparse": [[5, 1, 0]], "empty": [[0, 0, 0]]},
         2: {"dense": [[5, 5, 5], [5, 5, 5]], "at 0.8": [[5, 5, 5], [5, 4, 0]], "below 0.8": [[5, 5, 5], [5, 3, 0]], "sparse": [[5, 1, 0], [2, 0, 0]],
             "empty": [[0, 0, 0], [0, 0, 0]]}}
LIVE_FORMS = ("no active", "no live index", "other live_steps") + tuple(UNTIL[1])


def make_active(live, groups):
    """The row plan as Engine.forward hands it to the kernels (decode_plan.staff_rows through engine._kernel_plan), on the host."""
    from piano_a2s_amd import decode_plan, engine
    if live == "no active":
        return None
    until = torch.tensor(UNTIL[groups]["sparse" if live in ("no live index", "other live_steps") else live], dtype=torch.int32)
    active = engine._kernel_plan(decode_plan.staff_rows(until, STEPS, live_rows=live != "no live index"), lambda t: t)
    if live == "other live_steps":
        active["live_steps"] = STEPS + 1
    return active


def make_call(rec, tag, prefix, H, groups, live, gt, drop, persist_ws, step_ws):
    """What one _note_decoder_bwd call reads: sv as Engine._decode_staff saves it, the keys, the loss gradient and the output views, dK, dEnc; all named."""
    from piano_a2s_amd.spec import VOCAB_SIZE
    B, n, H2, ldx = groups * CLIPS, STEPS, 2 * H, E + 2 * H
    r = lambda *s: torch.rand(*s) + 0.5
    sv = dict(h=r(n + 1, B, H2), x=r(n + 1, B, ldx), q=r(n, B, H), o=r(n, B, 2 * H2), gates=r(n, B, 4 * H2), attw=r(n, B, T), steps=n, launched=n,
              drop=(torch.rand(n + 1, B, E) >= 0.1).to(torch.uint8) if drop else None, ids=torch.randint(0, 9, (B, MAX_STEPS), dtype=torch.int32),
              flags=[1, 0, 3, 2, 1][:n], gt_bar=torch.randint(0, 9, (B, MAX_STEPS)) if gt else None, prefix=prefix, max_steps=MAX_STEPS, drop_p=0.1,
              attn_ws=r(16), gemm_ws=r(16), active=make_active(live, groups), flags_dev=torch.tensor([1, 0, 3, 2, 1][:n], dtype=torch.int32) if gt == "flags_dev" else None,
              step_ws=r(16) if step_ws else None, persist_ws=torch.zeros(64, dtype=torch.uint8) if persist_ws else None, groups=groups)
    io = dict(keys=r(CLIPS, T, H), dprobs=r(B, MAX_STEPS, VOCAB_SIZE), probs=r(B, MAX_STEPS, VOCAB_SIZE), dK=r(CLIPS, T, H), dEnc=r(CLIPS, T, H2))
    rec.name_tree(f"{tag}.sv", {k: v for k, v in sv.items() if k != "active"})
    rec.name_tree(f"{tag}.active", sv["active"])
    for k in ("n_active", "m_active", "n_rows_active"):
        if sv["active"] and sv["active"].get(k) is not None:
            rec.name_host(f"{tag}.active.{k}", sv["active"][k])
    rec.name_tree(tag, io)
    return sv, io


def make_weights(rec, H):
    from piano_a2s_amd.spec import VOCAB_SIZE
    S = {}
    for prefix in ("decoder.upper_decoder", "decoder.lower_decoder"):
        shapes = {".attn.attn.weight": (H, 4 * H), ".attn.attn.bias": (H,), ".attn.v.weight": (1, H), ".gru.weight_ih_l0": (6 * H, E + 2 * H), ".gru.bias_ih_l0": (6 * H,),
                  ".gru.weight_hh_l0": (6 * H, 2 * H), ".gru.bias_hh_l0": (6 * H,), ".out.weight": (VOCAB_SIZE, 4 * H), ".out.bias": (VOCAB_SIZE,),
                  ".embedding.weight": (VOCAB_SIZE, E)}
        S.update({prefix + k: torch.rand(*s) + 0.5 for k, s in shapes.items()})
    G = {k: torch.zeros_like(v) for k, v in S.items()}
    rec.name_tree("S", S)
    rec.name_tree("G", G)
    return S, G


def run_case(late=True, live="sparse", groups=1, gt="flags", drop=True, persist_ws=False, step_ws=True, pair=False, H=4, fast=1):
    """One call (pair: a segment's two, by _note_decoder_bwd_pair) under the recorder.  gt: None, "flags" (host teacher-forcing bits) or "flags_dev".
    Returns the Recorder; rec.svs: the saved dicts of the calls."""
    from piano_a2s_amd import engine_bwd, hip
    torch.manual_seed(0)
    rec = abi_recorder.Recorder(blocks={"a2s_attn_dk_blocks": 7}, debug={"attn_deferred_fast": fast})
    S, G = make_weights(rec, H)
    eng = SimpleNamespace(cfg={"hidden_size": H, "note_emb_size": E})
    enc, enc_amax = torch.rand(CLIPS, T, 2 * H) + 0.5, torch.rand(1) + 0.5
    rec.name("enc", enc)
    rec.name("enc_amax", enc_amax)
    rec.name("one", getattr(engine_bwd, "_one", hip.one)("cpu"))
    old = "deferred" in inspect.signature(engine_bwd._note_decoder_bwd).parameters          # (before dec_bwd_plan.py: a stream argument, (dh0, event) back)
    late_list = [] if late else None
    calls, rec.svs = [], []
    for tag, prefix in (("up", "decoder.upper_decoder"), ("lo", "decoder.lower_decoder"))[:2 if pair else 1]:
        sv, io = make_call(rec, tag, prefix, H, groups, live, gt, drop, persist_ws, step_ws)
        rec.svs.append(sv)
        calls.append((eng, S, G, sv, io["keys"], enc, io["dprobs"], io["probs"], io["dK"], io["dEnc"], CLIPS, T) + ((None,) if old else ()) + (enc_amax, late_list))
    main, side = abi_recorder.Stream(rec, "main"), abi_recorder.Stream(rec, "side")
    staff = [abi_recorder.Stream(rec, "upper", 1), abi_recorder.Stream(rec, "lower", 2)]
    empty, select, maximum, recorded = torch.empty, torch.Tensor.index_select, torch.maximum, []

    def kept_empty(*a, **kw):          # (a fresh tensor the trace only ever sees as an address in the argument block keeps that address to itself)
        t = empty(*a, **kw)
        rec.keep.append(t)
        return t

    def index_select(src, dim, index):
        out, s, i = select(src, dim, index), rec.label(src), rec.label(index)
        assert dim == 0
        rec.events.append(("index_select", s, i))
        rec.name(f"{s}@{i}", out)
        return out

    def labelled_maximum(a, b):
        out = maximum(a, b)
        rec.name(f"max({rec.label(a)},{rec.label(b)})", out)
        return out

    extra = ((torch, "empty", kept_empty), (torch.Tensor, "index_select", index_select), (torch, "maximum", labelled_maximum),
             (torch.Tensor, "record_stream", lambda t, s: recorded.append((rec.label(t), s.name))))
    with abi_recorder.patched(rec, engine_bwd, hip, main, side, follow_current=True, extra=extra):
        res = engine_bwd._note_decoder_bwd_pair(calls, staff, dict(order=torch.arange(CLIPS, dtype=torch.int32), rank=torch.arange(CLIPS, dtype=torch.int32),
                                                                  n_active=(C.c_int * STEPS)(*[CLIPS] * STEPS))) if pair else [engine_bwd._note_decoder_bwd(*calls[0])]
        for r in res:
            rec.events.append(("return", rec.label(r[0] if isinstance(r, tuple) else r)))
        with torch.cuda.stream(side):          # Backward.finish
            for fn, ev, tensors in late_list or ():
                side.wait_event(ev)
                for t in tensors:
                    if t is not None:
                        t.record_stream(side)
                assert all(s == "side" for _, s in recorded)
                rec.events.append(("record_stream", "side", sorted(lab for lab, _ in recorded)))
                recorded.clear()
                fn()
    assert not recorded
    return rec


def matrix():
    for late, live, groups, gt, drop, persist_ws, step_ws, pair, (H, fast) in itertools.product(
            (False, True), LIVE_FORMS, (1, 2), (None, "flags", "flags_dev"), (False, True), (False, True), (False, True), (False, True), ((4, 1), (256, 1), (256, 0))):
        yield dict(late=late, live=live, groups=groups, gt=gt, drop=drop, persist_ws=persist_ws, step_ws=step_ws, pair=pair, H=H, fast=fast)


if __name__ == "__main__":
    traces = {json.dumps(case, sort_keys=True): run_case(**case).trace() for case in matrix()}
    with open(sys.argv[1], "w") as f:
        json.dump(traces, f)
    print(len(traces), "cases,", len({json.dumps(t) for t in traces.values()}), "distinct sequences,", sum(e[0] == "call" for t in traces.values() for e in t), "library calls")
