"""ONE NoteDecoder.decode_notes call (a2s_note_decoder_fwd / a2s_note_decoder_bwd) against the float64 oracle of tests/note_decoder_oracle.py, on every
path the call can take -- the persistent launch, the few-row kernels (with their hand-over to the mid-size kernels above 160 rows and their `rowmap`
tails), the bulk loop on the mid-size kernels and the library-style loop with its `m_active` prefix products -- each forced by the library's switches and
proved by its own counters.  Compared per tensor, at the live (step, row) pairs: every per-step tensor the backward reads, the log-probabilities, the
ids; then dh0, dK, dEnc and the ten parameter gradients of the reverse call.  A failure names the tensor, the row and the step.

Bars: per tensor, max(project bar, 3 x the deviation of the oracle's own float32 evaluation from its float64 one), the rule of
test_gpu_attn_range.py::_model_reference; project bar 2e-5 forward, 5e-5 gradients (test_gpu_dec_persist.py).  Every figure goes, with the float32
deviation and the bar used, to the file test_gpu_ops.py::_report writes.

The inputs' preconditions (argmax margins, row plans) are checked on the CPU by tests/test_note_decoder_oracle_cpu.py, over CASES / GREEDY below."""
import functools
import os
from collections import namedtuple

import pytest
import torch

from tests import note_decoder_oracle as oracle

pytestmark = pytest.mark.gpu

PREFIX = "decoder.upper_decoder"
H, E, V = 256, 16, 173
FWD_BAR, GRAD_BAR = 2e-5, 5e-5
MIN_MARGIN = 1e-3

# planned: False = plain rows (active=None: every row its own clip, all rows run every step); True = a row plan of decode_plan.staff_rows over
# rows that finish at different steps; "full" = the same plan fields, every row running every step
Case = namedtuple("Case", "name path clips bars T n planned seed")
CASES = [
    # persistent launch: 32 workgroups of 38 frames per clip -- T 37 / 38 / 39 = one workgroup not full, exactly full, 38 + 1; T 1201 = all 32, the last with 23
    Case("persist_1x1_T37", "persistent", 1, 1, 37, 6, False, 6),
    Case("persist_3x2_T38", "persistent", 3, 2, 38, 7, True, 8),
    Case("persist_5x3_T39", "persistent", 5, 3, 39, 7, True, 11),
    Case("persist_8x5_T1201", "persistent", 8, 5, 1201, 6, True, 4),
    Case("persist_8x5_T1201_full", "persistent", 8, 5, 1201, 6, "full", 3),
    # few-row kernels: 16-row tiles
    Case("few_1", "few-row", 1, 1, 61, 6, False, 2),
    Case("few_15", "few-row", 15, 1, 61, 6, False, 0),
    Case("few_16", "few-row", 16, 1, 61, 6, False, 1),
    Case("few_17", "few-row", 17, 1, 61, 6, False, 1),
    Case("few_8x5", "few-row", 8, 5, 61, 8, True, 2),
    # (five fused bars never leave their combine to the GRU step -- a2s_seq.hip: groups <= 4 -- so the 40 rows that do are 10 clips x 4 bars)
    Case("few_10x4", "few-row", 10, 4, 61, 8, True, 7),
    Case("few_33x5", "few-row", 33, 5, 61, 8, True, 16),
    # bulk loop on the mid-size kernels: 64-row workgroups
    Case("bulk_15", "bulk", 15, 1, 61, 6, False, 0),
    Case("bulk_63", "bulk", 63, 1, 61, 6, False, 1),
    Case("bulk_64", "bulk", 64, 1, 61, 6, False, 1),
    Case("bulk_65", "bulk", 65, 1, 61, 6, False, 0),
    Case("bulk_40x5", "bulk", 40, 5, 61, 8, True, 18),
    # library-style loop: tiled GEMMs, batched over the bars on the m_active prefix
    Case("lib_17", "library", 17, 1, 61, 6, False, 1),
    Case("lib_40x5", "library", 40, 5, 61, 8, True, 18),
]
Greedy = namedtuple("Greedy", "name rows T seed")
GREEDY = [Greedy("greedy_3", 3, 61, 3), Greedy("greedy_17", 17, 61, 0)]
# few-row cases run under both values of "attn_defer_combine"
VARIANTS = [(c, v) for c in CASES for v in ((0, 1) if c.path == "few-row" else (None,))]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def cfg():
    from piano_a2s_amd import spec
    return spec.default_cfg(freq_bins=48, max_length=(24, 14))          # the model's widths (hidden 256, E 16, V 173), short bars


WEIGHTS_SEED = 41


@functools.lru_cache(maxsize=None)
def _weights():
    from piano_a2s_amd import spec
    return oracle.prefix_tensors(spec.procedural_state(cfg(), WEIGHTS_SEED, eos_bias=2.0, lively="token"), PREFIX)


def plan_until(clips, bars, n, g):
    """(bars, clips) int32: the steps every row runs, as Engine.forward's plan would hold them for clips sorted longest first (plan_clip_groups): the
    first clips // 4 clips each have ONE row that runs all n steps, every other row ends at least two steps earlier.  Only ONE row ends after one step, so
    that step 1 still runs all rows but one: a `rowmap` launch over nearly every row (165 rows: 164, on the mid-size kernels).  That row is the first bar
    of the last clip, not the last row of the call: the rows of step 1 are then no permutation of 0 .. rows - 2, and a kernel that ignores its `rowmap` misses one."""
    ri = lambda lo, hi, shape=(): torch.randint(lo, hi + 1, shape, generator=g)
    n_long = max(1, clips // 4)
    clip_until = torch.cat([torch.full((n_long,), n), ri(2, n - 2, (clips - n_long,))])
    until = torch.empty(bars, clips, dtype=torch.long)
    for c in range(clips):
        until[:, c] = ri(2, int(clip_until[c]) if c >= n_long else n - 2, (bars,))
        until[int(ri(0, bars - 1)), c] = clip_until[c]
    until[0, clips - 1] = 1
    return until.to(torch.int32)


@functools.lru_cache(maxsize=None)
def inputs(clips, bars, T, n, planned, seed):
    """Everything one training call reads, on the CPU: weights, enc = tanh(randn), h0 = tanh(randn), targets, per-step teacher-forcing masks (one step all
    forced, one none), the row plan's `until` (flat, row = bar * clips + clip; None for plain rows) and dprobs (random at the live pairs, zero elsewhere)."""
    from piano_a2s_amd.spec import EOS, PAD
    U = cfg()["max_length"][0]
    g = torch.Generator().manual_seed(1000 * seed + 7 * clips + bars)
    R = clips * bars
    enc = torch.tanh(torch.randn(clips, T, 2 * H, generator=g))
    h0 = torch.tanh(torch.randn(R, 2 * H, generator=g))
    gt = torch.randint(0, 145, (R, U), generator=g)
    until = None
    if planned:
        until = (plan_until(clips, bars, n, g) if planned is True else torch.full((bars, clips), n, dtype=torch.int32)).reshape(-1)
        t_ = torch.arange(U).unsqueeze(0)
        ends = torch.rand(R, generator=g) < 0.5                        # half of the rows end in <eos>, the others in a plain token
        gt = torch.where((t_ == until.unsqueeze(1) - 1) & ends.unsqueeze(1), torch.full_like(gt, EOS), gt)
        if planned is True:
            gt = torch.where(t_ >= until.unsqueeze(1), torch.full_like(gt, PAD), gt)
    else:
        gt = torch.where(torch.rand(R, U, generator=g) < 0.05, torch.full_like(gt, EOS), gt)
    flags = torch.randint(0, 1 << bars, (n,), generator=g).tolist()
    a, b = torch.randperm(n - 1, generator=g)[:2].tolist()             # (not the last step: what it hands on is consumed by nobody)
    flags[a], flags[b] = (1 << bars) - 1, 0
    dprobs = torch.randn(R, n, V, generator=g) * oracle.live_pairs(until, R, n).unsqueeze(2)
    return dict(W=_weights(), enc=enc, h0=h0, gt=gt, flags=flags, until=until, dprobs=dprobs, U=U, R=R)


def case_inputs(c):
    return inputs(c.clips, c.bars, c.T, c.n, c.planned, c.seed)


@functools.lru_cache(maxsize=None)
def _reference(clips, bars, T, n, planned, seed):
    i = inputs(clips, bars, T, n, planned, seed)
    return oracle.reference(i["W"], i["enc"], i["h0"], i["gt"], i["flags"], bars, clips, n, i["U"], until=i["until"], dprobs=i["dprobs"])


@functools.lru_cache(maxsize=None)
def greedy_inputs(rows, T, seed):
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + 500)
    return dict(W=_weights(), enc=torch.tanh(torch.randn(rows, T, 2 * H, generator=g)), h0=torch.tanh(torch.randn(rows, 2 * H, generator=g)),
                U=cfg()["max_length"][0], R=rows)


@functools.lru_cache(maxsize=None)
def _greedy_reference(rows, T, seed):
    i = greedy_inputs(rows, T, seed)
    return oracle.reference(i["W"], i["enc"], i["h0"], None, None, 1, rows, i["U"], i["U"])


# ------------------------------------------------------------------------------------------- driving one call
_SWITCHES = ("dec_persist", "dec_fused", "dec_mid", "dec_fused_max_rows", "attn_defer_combine")
_ENV = ("A2S_DEC_PERSIST", "A2S_DEC_FUSED")


class _path:
    """The library's switches (and the two environment variables that shadow them) set for one path, everything put back on the way out."""
    def __init__(self, path, defer=None):
        self.kv = {"persistent": dict(dec_persist=1), "few-row": dict(dec_persist=0, dec_fused=1, dec_mid=1, dec_fused_max_rows=192),
                   "bulk": dict(dec_persist=0, dec_fused=0, dec_mid=1), "library": dict(dec_persist=0, dec_fused=0, dec_mid=0)}[path]
        if defer is not None:
            self.kv["attn_defer_combine"] = defer

    def __enter__(self):
        from piano_a2s_amd import hip
        self.L = hip.lib()
        self.prev = {k: self.L.a2s_debug_get(k.encode()) for k in _SWITCHES}
        self.env = {k: os.environ.get(k) for k in _ENV}
        for k, v in self.kv.items():
            hip.check(self.L.a2s_debug_set(k.encode(), v), "debug_set")
        os.environ["A2S_DEC_PERSIST"] = str(self.kv["dec_persist"])
        if "dec_fused" in self.kv:
            os.environ["A2S_DEC_FUSED"] = str(self.kv["dec_fused"])
        return self

    def __exit__(self, *a):
        for k, v in self.prev.items():
            self.L.a2s_debug_set(k.encode(), v)
        for k, v in self.env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _counters(L):
    return {k: L.a2s_debug_get(k.encode()) for k in ("dec_persist_launches", "dec_mid_launches", "dec_cmb_launches")}


def _setup(dev, i, clips, T):
    from piano_a2s_amd import engine
    S = {PREFIX + k: v.to(dev) for k, v in i["W"].items()}
    eng = engine.Engine(cfg())
    enc = i["enc"].to(dev)
    keys = eng._keys(S, PREFIX + ".attn", enc.view(clips * T, 2 * H), H).view(clips, T, H)
    return S, eng, enc, keys


def _forward(dev, c, i, persist):
    """The forward call as Engine.forward issues it.  Returns what the backward needs and the call's tensors."""
    from piano_a2s_amd import decode_plan, engine, hip
    S, eng, enc, keys = _setup(dev, i, c.clips, c.T)
    R, U = i["R"], i["U"]
    active = None
    if c.planned:
        active = engine._kernel_plan(decode_plan.staff_rows(i["until"].view(c.bars, c.clips), c.n, engine._TAIL_PREFIX, engine._TAIL_ROWS, engine._LIVE_ROWS),
                                     lambda t: t.to(dev))
    probs = torch.zeros(R, U, V, device=dev)
    flags_dev = torch.tensor(i["flags"], dtype=torch.int32, device=dev)
    ids, lengths, sv = eng._decode_staff(S, PREFIX, keys, enc, i["h0"].to(dev), U, probs, i["gt"].to(dev), c.n, i["flags"], True, 0.0, R, c.T,
                                         hip.attn_workspace(c.clips, c.T, H, dev, groups=c.bars), hip.gemm_workspace(R, dev), active, None, flags_dev, persist)
    sv["groups"] = c.bars          # (as Engine.forward does)
    torch.cuda.synchronize()
    return S, eng, enc, keys, probs, ids, lengths, sv


def _backward(dev, c, i, S, eng, enc, keys, probs, sv):
    from piano_a2s_amd import engine_bwd, hip
    G = {k: torch.zeros_like(v) for k, v in S.items()}
    dK, dEnc = torch.zeros(c.clips, c.T, H, device=dev), torch.zeros(c.clips, c.T, 2 * H, device=dev)
    dprobs = torch.zeros_like(probs)
    dprobs[:, :c.n] = i["dprobs"].to(dev)
    dh0 = engine_bwd._note_decoder_bwd(eng, S, G, sv, keys, enc, dprobs, probs, dK, dEnc, c.clips, c.T, hip.absmax(enc))
    torch.cuda.synchronize()
    return dict(dh0=dh0.clone().cpu(), dK=dK.cpu(), dEnc=dEnc.cpu(), params={k: G[PREFIX + k].cpu() for k in oracle.SUFFIXES})


def _report(label, name, err, dev32, bar):
    """One line per case and tensor -- "<case> <tensor> (float32 oracle <deviation>, bar <bar>): <error>" -- in the file the per-kernel tests of
    test_gpu_ops.py report to (one place names it)."""
    from tests import test_gpu_ops
    test_gpu_ops._report(f"note_decoder_call {label} {name} (float32 oracle {dev32:.3e}, bar {bar:.3e})", err)


def _compare(label, views, dev32, project_bar, live, bad, what):
    for name, ref, got in views:
        lv = live if what == "forward" else None
        err = oracle.rel_err(got, ref, lv)
        bar = max(project_bar, 3 * dev32[name])
        _report(label, name, err, dev32[name], bar)
        print(f"{label} {name}: {err:.3e}  float32 oracle {dev32[name]:.3e}  bar {bar:.3e}")
        if not err <= bar:
            at, size = oracle.worst(got, ref, lv)
            where = f"row {at[0]}, step {at[1]}, column {at[2]}" if what == "forward" else f"index {at}"
            bad.append(f"{name}: {err:.3e} > {bar:.3e} (largest |got - ref| {size:.3e} at {where})")


def _saved(sv, probs, n):
    got = {k: sv[k].detach().cpu() for k in ("h", "x", "q", "o", "gates", "attw")}
    got["probs"], got["steps"] = probs[:, :n].detach().cpu(), n
    return got


def _assert_finite(got, n, persist):
    """Everything behind `until` included: the backward reads those rows as operands, and a2s_log_softmax_bwd_rows turns a NaN among the
    log-probabilities into a NaN gradient even under a zero dprobs."""
    hint = " (a wait timed out?)" if persist else ""
    for name, t in (("h", got["h"][:n + 1]), ("x", got["x"][:n]), ("x (next token)", got["x"][n][:, :E]), ("q", got["q"][:n]), ("o", got["o"][:n]),
                    ("gates", got["gates"][:n]), ("probs", got["probs"])):
        assert torch.isfinite(t).all(), f"{name}: non-finite{hint}"


@pytest.mark.parametrize("c,defer", VARIANTS, ids=[c.name + ("" if v is None else f"-defer{v}") for c, v in VARIANTS])
def test_training_call_against_the_oracle(dev, c, defer):
    from piano_a2s_amd import hip
    i = case_inputs(c)
    f64, g64, dev32 = _reference(c.clips, c.bars, c.T, c.n, c.planned, c.seed)
    n, R, persist = c.n, i["R"], c.path == "persistent"
    label = c.name + ("" if defer is None else f"-defer{defer}")
    L = hip.lib()
    with _path(c.path, defer):
        c0 = _counters(L)
        S, eng, enc, keys, probs, ids, lengths, sv = _forward(dev, c, i, persist)
        c1 = _counters(L)
        grads = _backward(dev, c, i, S, eng, enc, keys, probs, sv)
        c2 = _counters(L)
    d1, d2 = {k: c1[k] - c0[k] for k in c0}, {k: c2[k] - c1[k] for k in c0}
    # ---- the path taken
    if persist:
        assert sv["persist_ws"] is not None and d1["dec_persist_launches"] == 1 and d2["dec_persist_launches"] == 1, (d1, d2)
    else:
        assert sv["persist_ws"] is None and d1["dec_persist_launches"] == 0 and d2["dec_persist_launches"] == 0, (d1, d2)
    mid = d1["dec_mid_launches"] + d2["dec_mid_launches"]
    if c.path == "few-row":
        # (a call that silently fell through to the bulk loop would count one mid-size launch per forward and per reverse step)
        assert (mid == 0) if R <= 160 else (0 < mid < 2 * n), f"{mid} mid-size launches over {R} rows"
        defers = c.planned and c.bars <= 4 and defer == 1
        assert (d1["dec_cmb_launches"] > 0) == defers, f"dec_gru_step_cmb launches: {d1['dec_cmb_launches']} (attn_defer_combine = {defer}, {c.bars} bars)"
    elif c.path == "bulk":
        assert d1["dec_mid_launches"] >= n and d2["dec_mid_launches"] >= n, (d1, d2)
    elif c.path == "library":
        assert mid == 0, (d1, d2)
    # ---- forward
    got = _saved(sv, probs, n)
    _assert_finite(got, n, persist)
    live = oracle.live_pairs(i["until"], R, n)
    bad = []
    wrong = (ids[:, :n].cpu().long() != f64["ids"]) & live
    if bool(wrong.any()):
        r, t = [int(v) for v in wrong.nonzero()[wrong.nonzero()[:, 1].argmin()]]
        bad.append(f"ids: {int(wrong.sum())} of {int(live.sum())} live pairs differ, the earliest at row {r}, step {t}: {int(ids[r, t])}, the oracle {int(f64['ids'][r, t])} "
                   f"(its margin {float(f64['margin'][r, t]):.2e})")
    if not torch.equal(lengths.cpu(), f64["lengths"]):
        bad.append(f"lengths: {lengths.cpu().tolist()}, the oracle {f64['lengths'].tolist()}")
    _compare(label, oracle.forward_views(f64, got, E), dev32, FWD_BAR, live, bad, "forward")
    assert not bad, f"{label} forward: " + "; ".join(bad)
    # ---- backward
    for name, _, t in oracle.grad_views(g64, grads):
        assert torch.isfinite(t).all(), f"{name}: non-finite gradient" + (" (a wait timed out?)" if persist else "")
    H2 = 2 * H
    aw = ".attn.attn.weight"
    assert float(g64["params"][aw][:, H2:].abs().max()) == 0.0          # (the key half is Backward.finish's, from dK: not the call's)
    grads["params"][aw] = torch.cat([grads["params"][aw][:, :H2], torch.zeros(H, H2)], dim=1)
    _compare(label, oracle.grad_views(g64, grads), dev32, GRAD_BAR, None, bad, "backward")
    assert not bad, f"{label} backward: " + "; ".join(bad)


GREEDY_VARIANTS = [(g, v) for g in GREEDY for v in ("eager", "graph", "persistent") if not (v == "persistent" and g.rows != 3)]


@pytest.mark.parametrize("g,variant", GREEDY_VARIANTS, ids=[f"{g.name}-{v}" for g, v in GREEDY_VARIANTS])
def test_greedy_call_against_the_oracle(dev, g, variant):
    """gt=None, training=False: ids, lengths and the executed-step count equal the oracle's exactly, the log-probabilities hold the forward bar over the
    steps the oracle executed.  graph: the replayed hipGraph, captured on a created stream as in test_greedy_graph_replay_matches_eager."""
    from piano_a2s_amd import engine, hip
    i = greedy_inputs(g.rows, g.T, g.seed)
    f64, _, dev32 = _greedy_reference(g.rows, g.T, g.seed)
    R, U, n = i["R"], i["U"], f64["steps"]
    L = hip.lib()
    persist = variant == "persistent"
    with _path("persistent" if persist else "few-row"):
        c0 = _counters(L)
        S, eng, enc, keys = _setup(dev, i, R, g.T)
        eng.greedy_graph = variant == "graph"
        probs = torch.zeros(R, U, V, device=dev)
        args = (S, PREFIX, keys, enc, i["h0"].to(dev), U, probs, None, U, None, False, 0.0, R, g.T, hip.attn_workspace(R, g.T, H, dev), hip.gemm_workspace(R, dev),
                None, None, None, persist)
        if variant == "graph":
            st = engine.side_streams(dev)[0]
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                ids, lengths, sv = eng._decode_staff(*args)
            torch.cuda.current_stream().wait_stream(st)
        else:
            ids, lengths, sv = eng._decode_staff(*args)
        torch.cuda.synchronize()
        c1 = _counters(L)
    assert c1["dec_persist_launches"] - c0["dec_persist_launches"] == (1 if persist else 0) and (sv["persist_ws"] is not None) == persist
    assert c1["dec_mid_launches"] == c0["dec_mid_launches"]
    got = probs[:, :n].cpu()
    assert torch.isfinite(got).all(), "probs: non-finite" + (" (a wait timed out?)" if persist else "")
    assert sv["steps"] == n, f"steps_exec {sv['steps']}, the oracle executed {n}"
    assert torch.equal(ids[:, :n].cpu().long(), f64["ids"]), "ids"
    assert torch.equal(lengths.cpu(), f64["lengths"]), "lengths"
    bad = []
    _compare(f"{g.name}-{variant}", [("probs", f64["probs"], got)], dev32, FWD_BAR, oracle.live_pairs(None, R, n), bad, "forward")
    assert not bad, "; ".join(bad)
