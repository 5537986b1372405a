"""The host plan of the ConvStack's backward (piano_a2s_amd.conv_bwd_plan) and its executor engine_bwd._convstack_bwd, without a GPU:
  1. the planner against a literal restatement of its rules over the whole switch matrix, and its two refusals;
  2. the executor's wiring -- which launch's range, partials and saved tensors reach which launch -- on the calls a fake library records at the C-ABI
     level (tests/conv_bwd_recorder.py), for the default switches, every single switch flipped, and synchronised BatchNorm;
  3. the switches are module attributes of engine_bwd, read per call."""
import itertools
import os
import subprocess
import sys

import pytest

from piano_a2s_amd.conv_bwd_plan import CHANS, ConvBwdFlags, LayerPlan, LinearPlan, plan_convstack_bwd, stats_source
from tests import conv_bwd_recorder as rec_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOOLS = (False, True)
PLACES = ("before", "beside", 4, 3, 2)


def test_module_is_pure_host_code():
    code = ("import sys, piano_a2s_amd.conv_bwd_plan; "
            "bad = [m for m in ('torch', 'piano_a2s_amd.hip', 'piano_a2s_amd.abi', 'piano_a2s_amd.engine', 'piano_a2s_amd.engine_bwd') if m in sys.modules]; "
            "assert not bad, bad")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


# ================================================================================================ 1. the planner
def _expected(fl, sync_bn, rows, F, linear_kernels, lin_ok, rows_ok):
    """The rules as engine_bwd._convstack_bwd applied them inline before the planner existed, written as that loop was: what the incoming gradient
    carries is two locals carried from one layer's turn to the next."""
    fused_ok = (not sync_bn) or fl.sync_fused
    stats = fl.dgrad_bnstats and fused_ok
    if stats and F >= 128 and F % 4 == 0 and rows > 64:
        lin_dgrad = "own" if (linear_kernels and lin_ok) else "generic"
    else:
        lin_dgrad = "gemm"
    lin = dict(stats="sync_own" if sync_bn else "own", absmax_after=sync_bn, dgrad=lin_dgrad, wgrad_at=fl.lin_wgrad_at, join_side=fl.lin_wgrad_at != "before")
    has_partial, has_range = lin_dgrad != "gemm", lin_dgrad == "own"
    layers = []
    for i in (4, 3, 2, 1):
        ci, co = ((1, 20), (20, 20), (20, 40), (40, 40))[i - 1]
        e = dict(i=i, ci=ci, co=co, dy_range=i > 1 and fused_ok, lin_wgrad=fl.lin_wgrad_at == i)
        if fl.fuse_bn_rows and fused_ok and i > 1 and has_partial and has_range and rows_ok:
            e["form"] = "rows"
        elif sync_bn or not (fl.fuse_bn_apply or (i == 1 and fl.fuse_bn_apply_l1)):
            e["form"] = "apply"
        else:
            e["form"] = "tiled"
        stats_only = e["form"] != "apply"
        if has_partial and not sync_bn:
            e["stats"] = "partial"
        elif has_partial and stats_only:
            e["stats"] = "sync_partial"
        else:
            assert not (sync_bn and stats_only)          # (no kernel does that: unreachable, as "tiled" needs not sync_bn and "rows" needs partials)
            e["stats"] = "sync_own" if sync_bn else "own"
        e["absmax_after"] = e["form"] == "apply" and sync_bn and e["dy_range"]
        if i == 1:
            e.update(dgrad="none", dgrad_range=False, out_range=False)
        elif stats:
            # the data gradient is given the layer's max |dy| unless fuse_bn_apply is set -- whatever form the layer took.  (Only "tiled" writes no
            # range; under fuse_bn_apply a "rows" or synchronised "apply" layer writes one that the data gradient is then not given.  That is what
            # the code before the planner did; the planner keeps it.)
            e.update(dgrad="bnstats", dgrad_range=e["dy_range"] and not fl.fuse_bn_apply, out_range=fl.fuse_bn_rows and i > 2)
        else:
            e.update(dgrad="plain", dgrad_range=False, out_range=False)
        has_partial, has_range = e["dgrad"] == "bnstats", e["out_range"]
        layers.append(e)
    return lin, layers


def test_planner_against_the_rules_over_the_whole_matrix():
    n = 0
    for flags in itertools.product(BOOLS, repeat=5):
        for place, sync_bn, (rows, F), linear_kernels, lin_ok, rows_ok in itertools.product(
                PLACES, BOOLS, ((69, 128), (10, 8), (64, 128), (65, 128), (69, 130), (69, 64)), BOOLS, BOOLS, BOOLS):
            fl = ConvBwdFlags(*flags, place)
            want_lin, want_layers = _expected(fl, sync_bn, rows, F, linear_kernels, lin_ok, rows_ok)
            for eligible in (rows_ok, {c: rows_ok for c in CHANS[1:]}):
                lin, layers = plan_convstack_bwd(fl, sync_bn, rows, F, linear_kernels, lin_ok, eligible)
                assert isinstance(lin, LinearPlan) and lin._asdict() == want_lin, (fl, sync_bn, rows, F)
                assert [lp.i for lp in layers] == [4, 3, 2, 1] and all(isinstance(lp, LayerPlan) for lp in layers)
                assert [lp._asdict() for lp in layers] == want_layers, (fl, sync_bn, rows, F, linear_kernels, lin_ok, rows_ok)
                assert all(type(v) in (str, bool, int) for rec in (lin,) + layers for v in rec)          # host data only
                n += 1
    assert n == 32 * 5 * 2 * 6 * 8 * 2


def test_planner_takes_eligibility_per_layer():
    some = {(20, 20): True, (20, 40): False, (40, 40): True}
    _, layers = plan_convstack_bwd(ConvBwdFlags(), False, 69, 128, True, True, some)
    assert [lp.form for lp in layers] == ["rows", "apply", "rows", "tiled"]


def test_flags_defaults_are_the_module_attributes_defaults():
    assert ConvBwdFlags() == ConvBwdFlags(fuse_bn_rows=True, dgrad_bnstats=True, sync_fused=True, fuse_bn_apply=False, fuse_bn_apply_l1=True, lin_wgrad_at="before")


def test_statistics_source_refuses_the_combination_no_kernel_serves():
    assert [stats_source(s, o, p) for s, o, p in ((False, False, True), (False, True, True), (True, True, True), (False, False, False), (False, True, False),
                                                   (True, False, False), (True, False, True))] == ["partial", "partial", "sync_partial", "own", "own", "sync_own", "sync_own"]
    with pytest.raises(ValueError):
        stats_source(sync_bn=True, stats_only=True, has_partial=False)


@pytest.mark.parametrize("bad", ["befor", "", 5, 1, 0, True, None, "4"])
def test_planner_refuses_an_unknown_placement(bad):
    with pytest.raises(ValueError):
        plan_convstack_bwd(ConvBwdFlags(lin_wgrad_at=bad), False, 69, 128, True, True, True)


# ================================================================================================ 2. the executor's wiring
B, T, F = SHAPE = (3, 23, 128)
ROWS = B * T
WIRING_CASES = {"default": {}, "sync_bn": dict(sync_bn=True), "sync_bn, not fused": dict(sync_bn=True, _SYNC_FUSED=False),
                "_FUSE_BN_ROWS off": dict(_FUSE_BN_ROWS=False), "_DGRAD_BNSTATS off": dict(_DGRAD_BNSTATS=False), "_SYNC_FUSED off": dict(_SYNC_FUSED=False),
                "_FUSE_BN_APPLY on": dict(_FUSE_BN_APPLY=True), "_FUSE_BN_APPLY on, rows off": dict(_FUSE_BN_APPLY=True, _FUSE_BN_ROWS=False),
                "_FUSE_BN_APPLY_L1 off": dict(_FUSE_BN_APPLY_L1=False), "rows not eligible": dict(rows_eligible=0), "linear dgrad not eligible": dict(linear_eligible=0, linear_wgrad_eligible=1),
                **{f"_LIN_WGRAD_AT {p!r}": dict(_LIN_WGRAD_AT=p) for p in PLACES[1:]}, "sync_bn, _LIN_WGRAD_AT 3": dict(sync_bn=True, _LIN_WGRAD_AT=3)}
WGRAD_FORMS = {"a2s_conv3x3_wgrad_bn_ranged": "rows", "a2s_conv3x3_wgrad_ranged": "apply", "a2s_conv3x3_wgrad_bn": "tiled"}
LIN_DGRADS = ("a2s_linear_dgrad_bnstats", "a2s_gemm_f32_bnstats_scaled", "a2s_gemm_f32")


def _bn_of(a, saved):
    assert [a[k] for k in ("mean", "invstd", "scale", "shift")] == [f"{saved}[{j}]" for j in range(4)], (a, saved)


def _is_fresh(label, shape):
    return isinstance(label, str) and label.startswith("new#") and label.endswith(str(list(shape)))


@pytest.mark.parametrize("case", list(WIRING_CASES))
def test_executor_wiring(case):
    kw = WIRING_CASES[case]
    sync_bn, place = kw.get("sync_bn", False), kw.get("_LIN_WGRAD_AT", "before")
    ev = rec_mod.run_case(SHAPE, **kw).calls()
    calls = [(k, e[1], e[2]) for k, e in enumerate(ev) if e[0] == "call"]

    def one(pred, what):
        hits = [(k, n, a) for k, n, a in calls if pred(n, a)]
        assert len(hits) == 1, (case, what, [h[1] for h in hits])
        return hits[0]

    # ---- every parameter gradient is written by exactly one launch
    written = [v for _, _, a in calls for v in a.values() if isinstance(v, str) and v.startswith("G.")]
    names = [f"G.convstack.conv{i}.weight" for i in range(1, 5)] + [f"G.convstack.bn{i}.{w}" for i in range(1, 5) for w in ("weight", "bias")] + \
        ["G.convstack.out.weight", "G.convstack.out_bn.weight", "G.convstack.out_bn.bias"]
    assert sorted(written) == sorted(names), case

    # ---- BatchNorm1d over the Linear's output: saved tensors, the mask, in place; its range scalar (from the launch, or a2s_absmax when synchronised)
    k_out, n_out, a_out = one(lambda n, a: a.get("dgamma") == "G.convstack.out_bn.weight", "out_bn")
    assert n_out == ("a2s_bn_bwd_apply" if sync_bn else "a2s_bn_bwd_amax") and (a_out["g"], a_out["x"], a_out["dx"], a_out["keep_mask"]) == ("d_out", "cs.z", "d_out", "cs.drop")
    _bn_of(a_out, "cs.out_bn")
    assert (a_out["rows"], a_out["C"], a_out["F"]) == (ROWS, rec_mod.CF, 1)
    if sync_bn:
        _, _, a_abs = calls[[k for k, _, _ in calls].index(k_out) + 1]
        assert (a_abs["x"], a_abs["n"]) == ("d_out", ROWS * rec_mod.CF)
        dz_range = a_abs["out"]
    else:
        dz_range = a_out["dx_absmax"]
    assert _is_fresh(dz_range, (1,))

    # ---- the Linear: weight gradient (activation re-formed from y4 with bn4's affine, bounded by abound[3]) and data gradient
    k_lw, _, a_lw = one(lambda n, a: n == "a2s_linear_wgrad", "linear wgrad")
    assert (a_lw["dz"], a_lw["y"], a_lw["G"], a_lw["scale"], a_lw["shift"], a_lw["period"], a_lw["dz_absmax"], a_lw["y_absmax"]) == \
        ("d_out", "cs.y[3]", "G.convstack.out.weight", "cs.bn[3][2]", "cs.bn[3][3]", F, dz_range, "cs.abound[3]")
    k_ld, n_ld, a_ld = one(lambda n, a: n in LIN_DGRADS, "linear dgrad")
    stats = kw.get("_DGRAD_BNSTATS", True) and (not sync_bn or kw.get("_SYNC_FUSED", True))
    assert n_ld == ("a2s_gemm_f32" if not stats else "a2s_linear_dgrad_bnstats" if kw.get("linear_eligible", 1) else "a2s_gemm_f32_bnstats_scaled"), case
    if n_ld == "a2s_gemm_f32":
        g_in, partial_in, range_in = a_ld["C"], None, None
        assert (a_ld["A"], a_ld["B"]) == ("d_out", "S.convstack.out.weight")
    else:
        g_in, partial_in, range_in = a_ld["da" if n_ld == "a2s_linear_dgrad_bnstats" else "C"], (a_ld["partial"], None), (a_ld.get("da_absmax_out"), 1)
        assert a_ld["dz" if n_ld == "a2s_linear_dgrad_bnstats" else "A"] == "d_out" and a_ld["y"] == "cs.y[3]" and a_ld["period"] == F
        _bn_of(a_ld, "cs.bn[3]")
        assert (a_ld["dz_absmax" if n_ld == "a2s_linear_dgrad_bnstats" else "a_absmax"], a_ld["w_absmax" if n_ld == "a2s_linear_dgrad_bnstats" else "b_absmax"]) == \
            (dz_range, "cs.w_out_amax")
        blocks = rec_mod.BLOCKS["a2s_linear_dgrad_blocks" if n_ld == "a2s_linear_dgrad_bnstats" else "a2s_gemm_bnstats_blocks"]
        assert _is_fresh(a_ld["partial"], (blocks, 40, 2))
        partial_in = (a_ld["partial"], blocks)
        if range_in[0] is None:
            range_in = None
        else:
            assert _is_fresh(range_in[0], (1,))

    # ---- layers 4 .. 1
    scalars, first_of_layer, stat_blocks = [dz_range], {}, rec_mod.BLOCKS["a2s_conv3x3_stat_blocks"]
    for i in (4, 3, 2, 1):
        ci, co = CHANS[i - 1]
        saved_bn, y, x_in = f"cs.bn[{i - 1}]", f"cs.y[{i - 1}]", f"cs.y[{i - 2}]" if i > 1 else "cs.x0"
        k_w, n_w, a_w = one(lambda n, a: a.get("dW") == f"G.convstack.conv{i}.weight", f"wgrad {i}")
        form = WGRAD_FORMS[n_w]
        bn_calls = [(k, n, a) for k, n, a in calls if a.get("dgamma") == f"G.convstack.bn{i}.weight"]
        assert len(bn_calls) == 1 and bn_calls[0][0] < k_w
        k_bn, n_bn, a_bn = bn_calls[0]
        assert a_bn["dbeta"] == f"G.convstack.bn{i}.bias"
        first_of_layer[i] = k_bn
        # what the BatchNorm backward read: the incoming gradient, this layer's saved output and statistics -- or the producer's partials alone
        if n_bn == "a2s_bn_bwd_c12_from_sums":
            k_s, n_s, a_s = calls[[k for k, _, _ in calls].index(k_bn) - 1]
            assert n_s == "a2s_bn_bwd_sums_from_partial" and (a_s["partial"], a_s["nblocks"]) == partial_in and a_s["C"] == a_bn["C"] == co
            assert a_s["sums"] == a_bn["sums_local"] and form == "rows"
            first_of_layer[i] = k_s
        else:
            assert (a_bn["g"], a_bn["x"], a_bn["rows"], a_bn["C"], a_bn["F"]) == (g_in, y, ROWS, co, F)
            _bn_of(a_bn, saved_bn)
            if n_bn == "a2s_bn_bwd_from_partial_amax":
                assert (a_bn["partial"], a_bn["nblocks"]) == partial_in and not sync_bn
            else:
                assert a_bn["keep_mask"] is None
            if n_bn == "a2s_bn_bwd_apply":
                k_s, n_s, a_s = calls[[k for k, _, _ in calls].index(k_bn) - 1]
                assert n_s == "a2s_bn_bwd_stats" and a_s["sums"] == a_bn["sums_local"] and (a_s["g"], a_s["x"]) == (g_in, y) and sync_bn
                first_of_layer[i] = k_s
            else:
                assert not sync_bn and (partial_in is None) == (n_bn == "a2s_bn_bwd_amax")
            assert a_bn["dx"] == (g_in if form == "apply" else None)
        assert a_bn["count_global"] == float(B * T * F) if "count_global" in a_bn else True
        # the weight gradient, and who wrote the layer's range scalar
        if form == "apply":
            produced = a_bn.get("dx_absmax")
            if sync_bn and i > 1 and kw.get("_SYNC_FUSED", True):
                _, n_abs, a_abs = calls[[k for k, _, _ in calls].index(k_bn) + 1]
                assert n_abs == "a2s_absmax" and (a_abs["x"], a_abs["n"]) == (g_in, ROWS * co * F)
                produced = a_abs["out"]
            assert (a_w["dy"], a_w["x"], a_w["dy_absmax"]) == (g_in, x_in, produced)
            assert (a_w["in_scale"], a_w["in_shift"], a_w["act_absmax"]) == ((f"cs.bn[{i - 2}][2]", f"cs.bn[{i - 2}][3]", f"cs.abound[{i - 2}]") if i > 1 else (None, None, None))
            dy = g_in
        else:
            assert (a_w["g"], a_w["y"], a_w["c12"], a_w["x"]) == (g_in, y, a_bn["c12"], x_in) and a_bn.get("dx_absmax") is None
            _bn_of(a_w, saved_bn)
            assert (a_w["in_scale"], a_w["in_shift"]) == ((f"cs.bn[{i - 2}][2]", f"cs.bn[{i - 2}][3]") if i > 1 else (None, None))
            if form == "rows":
                assert i > 1 and (a_w["g_absmax"], a_w["g_absmax_n"]) == range_in and partial_in is not None
                assert (a_w["y_absmax"], a_w["act_absmax"], a_w["dy_out"]) == (f"cs.yabs[{i - 1}]", f"cs.abound[{i - 2}]", g_in)
                produced, dy = a_w["dy_absmax_out"], g_in
            else:
                produced, dy = None, a_w["dy_out"]
                assert (dy is None) if i == 1 else (_is_fresh(dy, (B, T, co, F)) and dy != g_in)
        assert (a_w["B"], a_w["T"], a_w["F"], a_w["Cin"], a_w["Cout"]) == (B, T, F, ci, co)
        if produced is not None:
            assert _is_fresh(produced, (1,)) and produced not in scalars, (case, i)
            scalars.append(produced)
        if i == 1:
            assert not any(a.get("w") == "S.convstack.conv1.weight" for _, _, a in calls)
            break
        # the data gradient: this layer's dy and range in, the gradient of the layer below with its partials and per-channel range out
        k_d, n_d, a_d = one(lambda n, a: a.get("w") == f"S.convstack.conv{i}.weight", f"dgrad {i}")
        assert k_d > k_w and n_d == ("a2s_conv3x3_dgrad_bnstats_ranged" if stats else "a2s_conv3x3")
        assert (a_d["B"], a_d["T"], a_d["F"], a_d["Cin"], a_d["Cout"]) == (B, T, F, co, ci)          # (flipped: the kernel's Cin is the layer's output)
        if stats:
            # (under _FUSE_BN_APPLY the data gradient is not given the range even where the layer wrote one: see _expected)
            assert a_d["dy_absmax"] == (None if form == "tiled" or kw.get("_FUSE_BN_APPLY", False) else produced), (case, i)
            assert (a_d["dy"], a_d["yl"]) == (dy, f"cs.y[{i - 2}]")
            assert [a_d[k] for k in ("yl_mean", "yl_invstd", "yl_scale", "yl_shift")] == [f"cs.bn[{i - 2}][{j}]" for j in range(4)]
            assert _is_fresh(a_d["stat_partial"], (stat_blocks, ci, 2))
            partial_in, stat_blocks = (a_d["stat_partial"], stat_blocks), stat_blocks + 1
            range_in = (a_d["g_absmax_out"], ci) if a_d["g_absmax_out"] is not None else None
            assert (range_in is not None) == (kw.get("_FUSE_BN_ROWS", True) and i > 2) and (range_in is None or _is_fresh(range_in[0], (ci,)))
            g_in = a_d["g"]
        else:
            assert (a_d["x"], a_d["in_scale"], a_d["in_shift"], a_d["stat_partial"], a_d["flip"]) == (dy, None, None, None, 1)
            partial_in, range_in, g_in = None, None, a_d["y"]
        assert _is_fresh(g_in, (B, T, ci, F))

    # ---- synchronised BatchNorm: one all-reduce per BatchNorm layer, of the copy the second half then reads as the global sums
    reduces = [k for k, e in enumerate(ev) if e[0] == "all_reduce"]
    assert len(reduces) == (5 if sync_bn else 0)
    for k in reduces:
        assert ev[k - 1][1] in ("a2s_bn_bwd_stats", "a2s_bn_bwd_sums_from_partial") and ev[k + 1][1] in ("a2s_bn_bwd_apply", "a2s_bn_bwd_c12_from_sums")
        assert ev[k][1] == ev[k + 1][2]["sums_global"] != ev[k + 1][2]["sums_local"]

    # ---- where the Linear's weight gradient is issued
    stream_events = [(k, e) for k, e in enumerate(ev) if e[0] != "call" and e[0] != "all_reduce"]
    if place == "before":
        assert not stream_events and k_out < k_lw < k_ld
    else:
        assert [e[0] for _, e in stream_events] == ["record", "wait_event", "enter", "exit", "wait_stream"]
        (k0, rec_ev), (k1, wait), (k2, enter), (k3, leave), (k4, join) = stream_events
        assert wait == ("wait_event", "side", rec_ev[1]) and enter == ("enter", "side") and leave == ("exit", "side")
        assert (k0, k1, k2, k3) == (k_lw - 3, k_lw - 2, k_lw - 1, k_lw + 1)          # the weight gradient alone, inside the side-stream context
        assert join == ("wait_stream", "main", "side") and k4 == len(ev) - 1          # the main stream waits for that stream last
        if place == "beside":
            assert k_out < k_lw < k_ld
        else:
            prev_dgrad = max(k for k, n, a in calls if k < first_of_layer[place] and k != k_lw)
            assert k_ld < k_lw and prev_dgrad < k0 and k3 < first_of_layer[place]          # at the top of that layer's turn


def test_a_materialised_a4_is_refused():
    import torch
    with pytest.raises(ValueError):
        rec_mod.run_case(SHAPE, cs_extra={"a4": torch.zeros(ROWS, 40 * F)})


# ================================================================================================ 3. the switches are read per call
def test_switch_attributes_are_read_per_call():
    from piano_a2s_amd import engine_bwd
    fused = lambda: sum(e[1] == "a2s_conv3x3_wgrad_bn_ranged" for e in rec_mod.run_case(SHAPE).trace())
    prev = engine_bwd._FUSE_BN_ROWS
    try:
        engine_bwd._FUSE_BN_ROWS = True
        assert fused() == 3
        engine_bwd._FUSE_BN_ROWS = False
        assert fused() == 0
    finally:
        engine_bwd._FUSE_BN_ROWS = prev
    assert engine_bwd._FUSE_BN_ROWS == (os.environ.get("A2S_FUSE_BN_ROWS", "1") != "0")
    assert (engine_bwd._DGRAD_BNSTATS, engine_bwd._SYNC_FUSED, engine_bwd._FUSE_BN_APPLY, engine_bwd._FUSE_BN_APPLY_L1, engine_bwd._LIN_WGRAD_AT) == \
        ConvBwdFlags()[1:]
