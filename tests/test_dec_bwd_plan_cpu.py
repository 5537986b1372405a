"""The host plan of the note decoders' backward (piano_a2s_amd.dec_bwd_plan) and its executor engine_bwd._note_decoder_bwd, without a GPU:
  1. the two planners against a literal restatement of the conditions engine_bwd applied inline before the plan existed, over their whole input
     matrix; the product table and the keep-alive list against what that code spelled out by hand;
  2. the executor's wiring on the calls a fake library records at the C-ABI level (tests/dec_bwd_recorder.py): rows, gathers, operand ranges,
     what runs before the event and what in the closure, what the weight-gradient stream records, the row plan of the argument block;
  3. a group whose slice of the encoder output is not contiguous is refused."""
import itertools
import os
import re
import subprocess
import sys
from types import SimpleNamespace
from unittest import mock

import pytest
import torch

from piano_a2s_amd import dec_bwd_plan
from piano_a2s_amd.dec_bwd_plan import GATHER_BELOW, PRODUCTS, plan_note_decoder_bwd, plan_staff_issue
from tests import dec_bwd_recorder as rec_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOOLS = (False, True)


def test_module_is_pure_host_code():
    code = ("import sys, piano_a2s_amd.dec_bwd_plan; "
            "bad = [m for m in ('torch', 'ctypes', 'piano_a2s_amd.hip', 'piano_a2s_amd.abi', 'piano_a2s_amd.engine', 'piano_a2s_amd.engine_bwd') if m in sys.modules]; "
            "assert not bad, bad")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


# ================================================================================================ 1. the planners
def _expected(steps, rows, live_steps, n_live, late):
    """What _note_decoder_bwd did when these decisions sat in its closure deferred_work(part) and in after_launch, written as that code ran."""
    R = steps * rows
    live = n_live if (n_live is not None and live_steps == steps) else None          # (the live index counts only for the step count it was planned for)
    Rw, gathered, returned = R, False, False
    if live is not None and live < 0.8 * R:
        Rw, gathered = live, True
        if Rw == 0:
            returned = True          # "nothing ran: every gradient of this call is zero"
    def deferred_work(part, issued):
        if part == "attn":
            issued.append("keys")
            return
        issued.append("weights")          # (the operand ranges are measured before the rows are looked at)
        if returned:
            return
        if part == "all":
            issued.append("keys")
        issued.append("scatter")
    on_stream, in_closure = [], []
    if late:
        deferred_work("attn", on_stream)
        deferred_work("weights", in_closure)
    else:
        deferred_work("all", on_stream)
    return dict(gather=gathered, rw=Rw, empty=returned, placement="late" if late else "inline", on_stream=tuple(on_stream), in_closure=tuple(in_closure))


def test_note_decoder_plan_against_the_rules_over_the_whole_matrix():
    n = 0
    for steps, rows, late in itertools.product(range(0, 7), (1, 3, 5, 6), BOOLS):
        for live_steps, n_live in itertools.product((None, steps, steps + 1, 0), (None,) + tuple(range(steps * rows + 1))):
            plan = plan_note_decoder_bwd(steps, rows, live_steps, n_live, late)
            got = {k: v for k, v in plan._asdict().items() if k not in ("products", "operands", "keep_alive")}
            assert got == _expected(steps, rows, live_steps, n_live, late), (steps, rows, live_steps, n_live, late)
            assert plan.products is PRODUCTS and plan.operands == dec_bwd_plan.OPERANDS and plan.keep_alive == dec_bwd_plan.keep_alive()
            n += 1
    assert n == 2 * 4 * sum(steps * rows + 2 for steps in range(7) for rows in (1, 3, 5, 6))
    assert GATHER_BELOW == 0.8
    # the threshold itself, at the sizes the recorder's cases use: 12 of 15 and 24 of 30 pairs are not gathered, one fewer is
    assert [plan_note_decoder_bwd(5, r, 5, k, True).gather for r, k in ((3, 12), (3, 11), (6, 24), (6, 23))] == [False, True, False, True]


def test_staff_issue_truth_table():
    for concurrent, staves, persist, has_pair, switch in itertools.product(BOOLS, repeat=5):
        concurrent_g = concurrent and staves and not persist          # (as Backward.decoder_group spelled it over its locals)
        if concurrent_g and has_pair and switch:
            want = "pair"
        elif concurrent_g:
            want = "fork"
        else:
            want = "serial"
        assert plan_staff_issue(concurrent, staves, persist, has_pair, switch) == want


def test_product_table_is_what_the_four_spellings_said():
    """_linear_bwd(o, W_out, dlog, ..., x_bound=max(one, enc)); _linear_bwd(x, W_ih, dgi, ..., x_bound=max(emb, enc)); _linear_bwd(h, W_hh, dgh, ..., x_bound=one);
    hip.gemm(dq, 1, H, h, 2H, 1, G[attn.attn.weight], 4H, H, 2H, Rw, ..., two_term=(absmax(dq), one)) + the bias sum: input, gradient, names, (K, ldc, column), bound."""
    assert [tuple(p) for p in PRODUCTS] == [
        ("out", "o", "dlog", ".out.weight", ".out.bias", "4H", "4H", 0, "max(one, enc)", "dlog_amax"),
        ("w_ih", "x", "dgi", ".gru.weight_ih_l0", ".gru.bias_ih_l0", "E+2H", "E+2H", 0, "max(emb, enc)", "measure"),
        ("w_hh", "h", "dgh", ".gru.weight_hh_l0", ".gru.bias_hh_l0", "2H", "2H", 0, "one", "measure"),
        ("attn_q", "h", "dq", ".attn.attn.weight", ".attn.attn.bias", "2H", "4H", 0, "one", "measure")]
    assert [dec_bwd_plan.dim(k, 256, 32) for k in ("2H", "4H", "E+2H")] == [512, 1024, 544]
    assert set(dec_bwd_plan.OPERANDS) == {v for p in PRODUCTS for v in (p.x, p.dy)}


def test_keep_alive_is_derived_and_not_smaller_than_the_hand_written_tuple():
    by_hand = {"dlog", "do_all", "dgi", "dgh", "dq", "dx", "x", "h", "o", "ids", "drop", "gt_bar", "flags_dev", "live_idx", "dlog_amax", "enc_amax"}
    kept = dec_bwd_plan.keep_alive()
    assert len(set(kept)) == len(kept) and set(kept) >= by_hand
    assert set(kept) >= set(dec_bwd_plan.OPERANDS) | set(dec_bwd_plan.SCATTER_READS) | {"live_idx"}
    # a product added to the table brings its operands and its measured-once range along
    more = PRODUCTS + (dec_bwd_plan.Product("extra", "q", "ds", ".w", ".b", "2H", "2H", 0, "one", "ds_amax"),)
    assert set(dec_bwd_plan.keep_alive(more)) - set(kept) == {"q", "ds", "ds_amax"}


# ================================================================================================ 2. the executor's wiring
WIRING_CASES = [dict(late=late, live=live, groups=groups, pair=pair) for late, live, groups, pair in itertools.product(BOOLS, rec_mod.LIVE_FORMS, (1, 2), BOOLS)
                if not (pair and groups == 2)] + \
               [dict(late=True, live="sparse", H=256, fast=fast, gt=gt, drop=drop) for fast, gt, drop in ((1, None, False), (0, "flags_dev", True), (1, "flags", True))] + \
               [dict(late=False, live="below 0.8", persist_ws=True, step_ws=False, gt=None)]
KEY_SIDE = ("a2s_attn_denc_accum", "a2s_attn_dk_accum")


def _strip(label):
    """A label without the shape the trace completes a fresh tensor's with."""
    return re.sub(r"\[[\d, ]*\]$", "", label) if isinstance(label, str) and label.startswith("new#") else label


def _args_strings(e):
    for v in (e[2].values() if e[0] == "call" else e[1:]):
        for x in (v.values() if isinstance(v, dict) else v if isinstance(v, (list, tuple)) else (v,)):
            if isinstance(x, str):
                yield _strip(x)


def _calls_of(ev, tag, prefix, block):
    """The library calls of one staff's backward: those that name a tensor of the call, a parameter of its decoder, a tensor of its argument block, or a
    fresh tensor an earlier one of them produced (the pair's one launch aside)."""
    owned, part, out = {_strip(v) for v in block.values() if isinstance(v, str) and v.startswith("new#")}, prefix.split(".")[1], []
    for k, e in enumerate(ev):
        if e[0] != "call" or e[1] == "a2s_note_decoder_bwd_pair":
            continue
        strs = list(_args_strings(e))
        if any(f"{tag}." in s or f".{part}." in s or s in owned for s in strs):
            owned |= {s for s in strs if s.startswith("new#")}
            out.append((k, e[1], e[2]))
    return out


@pytest.mark.parametrize("case", WIRING_CASES, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_executor_wiring(case):
    from piano_a2s_amd import hip
    kw = dict(late=True, live="sparse", groups=1, gt="flags", drop=True, persist_ws=False, step_ws=True, pair=False, H=4, fast=1)
    kw.update(case)
    rec = rec_mod.run_case(**kw)
    ev = rec.calls()
    H, E, B, n = kw["H"], rec_mod.E, kw["groups"] * rec_mod.CLIPS, rec_mod.STEPS
    for tag, prefix, sv in zip(("up", "lo"), ("decoder.upper_decoder", "decoder.lower_decoder"), rec.svs):
        act = sv["active"] or {}
        live = act.get("live_idx")
        plan = plan_note_decoder_bwd(n, B, act.get("live_steps"), live.numel() if live is not None else None, kw["late"])
        if kw["pair"]:
            block = next(e[2] for e in ev if e[0] == "call" and e[1] == "a2s_note_decoder_bwd_pair")["upper" if tag == "up" else "lower"]
        else:
            block = next(e[2] for e in ev if e[0] == "call" and e[1] == "a2s_note_decoder_bwd")["args"]
        calls = _calls_of(ev, tag, prefix, block)
        absmax_of = {a["out"]: a["x"] for _, fn, a in calls if fn == "a2s_absmax"}

        # ---- the argument block: what the reverse loop reads and writes, and the row plan hip.set_row_plan gives for the case
        want = hip.NoteDecBwdArgs()
        hip.set_row_plan(want, sv["active"])
        row_fields = ("clip_order", "clip_rank", "row_until", "row_list", "n_active", "m_active", "n_rows_active", "n_clips")
        assert {f: block[f] for f in row_fields} == {f: rec.label(C_byref_field(want, f)) for f in row_fields}
        assert (block["R"], block["T"], block["H"], block["E"], block["steps"]) == (B, rec_mod.T, H, E, n)
        assert [block[f] for f in ("h", "x", "q", "gates", "attw", "keys", "enc")] == [f"{tag}.sv.{f}" for f in ("h", "x", "q", "gates", "attw")] + [f"{tag}.keys", "enc"]
        assert (block["step_ws"] is not None) == kw["step_ws"] and (block["persist_ws"] is not None) == kw["persist_ws"]
        dlog = next(a for _, fn, a in calls if fn == "a2s_log_softmax_bwd_rows")["dx"]
        dlog_amax = next(out for out, x in absmax_of.items() if x == dlog)
        named = {"dlog": dlog, "o": f"{tag}.sv.o", "x": f"{tag}.sv.x", "h": f"{tag}.sv.h", "dgi": block["dgi_all"], "dgh": block["dgh_all"], "dq": block["dq_all"],
                 "dx": block["dx"], "do_all": block["do_all"]}
        named = {k: _strip(v) for k, v in named.items()}
        idx = f"{tag}.active.live_idx"

        # ---- the products: exactly plan.rw rows, operands gathered from the one live index or not at all, the ranges the table states
        products = [(k, a) for k, fn, a in calls if fn == "a2s_gemm_f32_affine_scaled" and isinstance(a["C"], str) and a["C"].startswith("G.") and "attn.v" not in a["C"]]
        if plan.empty:
            assert not products
        else:
            assert [a["C"] for _, a in products] == [f"G.{prefix}{p.weight}" for p in PRODUCTS]
        for (k, a), p in zip(products, PRODUCTS):
            assert (a["K"], a["N"], a["ldc"], a["beta"]) == (plan.rw, dec_bwd_plan.dim(p.cols, H, E), dec_bwd_plan.dim(p.ld, H, E), 1.0), (p.name, a)
            dy, x = a["A"].split("[")[0], a["B"].split("[")[0]
            assert (dy, x) == ((f"{named[p.dy]}@{idx}", f"{named[p.x]}@{idx}") if plan.gather else (named[p.dy], named[p.x])), (p.name, a)
            assert absmax_of[a["a_absmax"]].split("[")[0] == (named["dlog"] if p.dy_range == "dlog_amax" else dy), (p.name, a)          # max |dlog| over all rows bounds the gathered ones
            if p.x_bound == "one":
                assert a["b_absmax"] == "one"
            elif p.x_bound == "max(one, enc)":
                assert a["b_absmax"] == "max(one,enc_amax)"
            else:
                emb_range = next(out for out, xx in absmax_of.items() if xx == f"S.{prefix}.embedding.weight")
                assert a["b_absmax"] == f"max({_strip(emb_range)},enc_amax)"
            bias = ev[k + 1]
            assert bias[1] == "a2s_col_sum" and (bias[2]["x"], bias[2]["out"], bias[2]["rows"], bias[2]["C"]) == (a["A"], f"G.{prefix}{p.bias}", plan.rw, a["M"]), (p.name, bias)
        scatter = [(k, a) for k, fn, a in calls if fn == "a2s_embed_scatter_add"]
        assert len(scatter) == (0 if plan.empty else 1)
        for k, a in scatter:
            assert (a["R"], a["table_grad"], a["ldg"]) == (plan.rw, f"G.{prefix}.embedding.weight", E if plan.gather else E + 2 * H)
            assert a["g"].split("[")[0] == (f"{named['dx']}@{idx}" if plan.gather else named["dx"])
            assert a["ids32"].endswith(f"@{idx}[{plan.rw}]") == plan.gather
            assert a["keep_mask"] == (None if not kw["drop"] else f"{tag}.sv.drop@{idx}" if plan.gather else f"{tag}.sv.drop")
        gathers = [e for e in ev if e[0] == "index_select" and e[2] == idx]
        assert len(gathers) == ((len(plan.operands) + 2 + bool(kw["drop"])) if plan.gather and not plan.empty else 0)
        assert not [e for e in ev if e[0] == "index_select" and e[1].startswith(f"{tag}.") and e[2] != idx]

        # ---- the key side: once, unless an inline call is empty; the live-pair kernel at 2H = 512 unless switched off
        keys = [(k, fn, a) for k, fn, a in calls if fn in KEY_SIDE or (fn == "a2s_gemm_f32_affine_scaled" and a["C"] == f"{tag}.dEnc")]
        assert [fn for _, fn, _ in keys] == ([] if "keys" not in plan.on_stream else
                                             ["a2s_attn_denc_accum" if (2 * H == 512 and kw["fast"]) else "a2s_gemm_f32_affine_scaled", "a2s_attn_dk_accum"])

        # ---- placement: late, nothing that accumulates into a weight gradient is issued outside the closure, and the key side comes before the event
        accumulates = [k for k, fn, a in calls if any(isinstance(v, str) and v.startswith("G.") and ".attn.v." not in v for v in a.values())]
        if not kw["late"]:
            assert not [e for e in ev if e[0] in ("record", "record_stream", "wait_event")]
            if not plan.empty:
                assert max(k for k, _ in products) < min(k for k, _, _ in keys) and max(k for k, _, _ in keys) < scatter[0][0]
            continue
        k_event = next(k for k, e in enumerate(ev) if e[0] == "record" and e[2] == ("main" if not kw["pair"] else "upper" if tag == "up" else "lower") and
                       k > max([kk for kk, _, _ in keys]))
        event = ev[k_event][1]
        k_wait = next(k for k, e in enumerate(ev) if e == ("wait_event", "side", event))
        k_end = min([k for k, e in enumerate(ev) if k > k_wait and e[0] in ("wait_event", "exit")])
        assert all(k < k_event for k, _, _ in keys) and bool(accumulates) == (not plan.empty) and all(k_wait < k < k_end for k in accumulates)
        assert all(ev[k][2]["stream"] == "side" for k in range(k_wait, k_end) if ev[k][0] == "call")

        # ---- what the weight-gradient stream records: every tensor a call in the closure reads that was made before it, and no less than the tuple written by hand
        assert ev[k_wait + 1][:2] == ("record_stream", "side")
        recorded = {_strip(v) for v in ev[k_wait + 1][2]}
        before = {_strip(s) for e in ev[:k_wait] for s in _args_strings(e)}
        read = {_strip(s) for e in ev[k_wait + 2:k_end] for s in _args_strings(e)}
        outlives = lambda s: s.startswith(("S.", "G.")) or s in ("one", "side") or s.startswith("max(") or "@" in s
        assert {s for s in read & before if not outlives(s)} <= recorded
        by_hand = {named[k] for k in ("dlog", "do_all", "dgi", "dgh", "dq", "dx", "x", "h", "o")} | {f"{tag}.sv.ids", _strip(dlog_amax), "enc_amax"} | \
            ({f"{tag}.sv.drop"} if kw["drop"] else set()) | ({f"{tag}.sv.gt_bar"} if kw["gt"] else set()) | ({f"{tag}.sv.flags_dev"} if kw["gt"] == "flags_dev" else set()) | \
            ({idx} if live is not None else set())
        assert recorded >= by_hand, by_hand - recorded


def C_byref_field(block, field):
    """A field of an argument block as the recorder sees it in a call: the pointer fields as c_void_p."""
    import ctypes as C
    v = getattr(block, field)
    return C.c_void_p(v) if dict(block._fields_)[field] is C.c_void_p else v


def test_empty_inline_call_skips_the_key_side_too():
    """The quirk the plan keeps: inline, a gathered call in which nothing ran returns before the key-side gradients; late, they have been issued by then."""
    inline = [e[1] for e in rec_mod.run_case(late=False, live="empty").calls() if e[0] == "call"]
    late = [e[1] for e in rec_mod.run_case(late=True, live="empty").calls() if e[0] == "call"]
    assert "a2s_attn_dk_accum" not in inline and "a2s_attn_dk_accum" in late
    assert inline[-1] == late[-1] == "a2s_absmax" and "a2s_embed_scatter_add" not in inline + late


# ================================================================================================ 3. the refusal
def test_a_group_slice_of_the_encoder_output_that_is_not_contiguous_is_refused():
    from piano_a2s_amd import engine_bwd, hip
    H = 4
    ctx = engine_bwd.Backward.__new__(engine_bwd.Backward)
    ctx.eng = SimpleNamespace(cfg=dict(hidden_size=H, staff_emb_size=2, time_sig_emb_size=2, key_emb_size=2, max_bars=1))
    ctx.S, ctx.G, ctx.dev, ctx.T, ctx.names, ctx.offs = {}, {}, torch.device("cpu"), 5, [], []
    ctx.group_flat, ctx.group_ptrs, ctx.dEnc, ctx.dK, ctx.dEnc_staff, ctx.d_hidden = [None], [None], torch.zeros(2, 5, 2 * H), {}, [], None
    ctx.concurrent, ctx.bar_major, ctx.clip_groups = False, False, [(0, 2)]
    gs = dict(range=(0, 2), enc=torch.zeros(2, 5, 4 * H)[:, :, ::2], keys={}, outs=(None,) * 4, segments=[])
    with mock.patch.object(hip, "lib", lambda: SimpleNamespace()):
        with pytest.raises(ValueError, match="not contiguous"):
            ctx.decoder_group(0, gs, None, None, None, None)
