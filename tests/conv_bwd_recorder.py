"""engine_bwd._convstack_bwd driven without a GPU: a fake liba2s_hip at the C-ABI level that records every call, recording stand-ins for the streams,
events and the all-reduce, CPU tensors everywhere.  The real hip.py wrappers run.  Every pointer argument is labelled by identity: a tensor of cs, S
or G by its key (cs.abound[2], G.convstack.conv3.weight), d_out by its name, a tensor first seen during the call as new#k in order of first
appearance, with its shape.  Every call is held to the parameter count of its prototype in include/a2s.h, whose parameter names Recorder.calls() attaches.
Pure queries (*_eligible, *_blocks, *_bytes, *_floats, a2s_debug_get, a2s_gemm_pick_splitk) answer fixed values -- the k-th call of a *_blocks function
its own number, so that a block count handed to the wrong consumer shows -- and stay out of the trace.  tests/test_conv_bwd_plan_cpu.py asserts the wiring
on these traces; run as a script (python -m tests.conv_bwd_recorder OUT.json) it writes the traces of the whole switch matrix, to compare two commits
case by case."""
import contextlib
import ctypes as C
import itertools
import json
import os
import re
import sys
from types import SimpleNamespace
from unittest import mock

import torch

CHANS = [(1, 20), (20, 20), (20, 40), (40, 40)]
FLAGS = ("_FUSE_BN_ROWS", "_DGRAD_BNSTATS", "_SYNC_FUSED", "_FUSE_BN_APPLY", "_FUSE_BN_APPLY_L1")
CF = 8
QUERY_ANSWERS = {"_bytes": 64, "_floats": 16}
BLOCKS = {"a2s_conv3x3_stat_blocks": 11, "a2s_linear_dgrad_blocks": 21, "a2s_gemm_bnstats_blocks": 31}          # answer of the first call; +1 per further call


def _header_params():
    """{function: [parameter names]} of include/a2s.h."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "a2s.h")) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    return {m.group(1): [re.split(r"[\s*]+", p.strip())[-1] for p in m.group(2).split(",")] for m in re.finditer(r"\b(a2s_\w+)\s*\(([^()]*)\)", text)}


PARAMS = _header_params()


def make_inputs(B, T, F):
    """cs as Engine.convstack(training=True) saves it, S, G and d_out: CPU tensors of the real shapes with distinct storage."""
    rows, r = B * T, lambda *s: torch.rand(*s) + 0.5
    cs = {"x0": r(B, 1, T, F), "y": [r(B, T, co, F) for _, co in CHANS], "bn": [tuple(r(co) for _ in range(4)) for _, co in CHANS],
          "yabs": [r(co) for _, co in CHANS], "abound": [r(1) for _ in CHANS], "w_out_amax": r(1), "a4": None, "z": r(rows, CF),
          "out_bn": tuple(r(CF) for _ in range(4)), "drop": r(rows, CF)}
    S = {f"convstack.conv{i}.weight": r(co, ci, 3, 3) for i, (ci, co) in enumerate(CHANS, start=1)}
    S["convstack.out.weight"] = r(CF, 40 * F)
    G = {k: torch.zeros_like(v) for k, v in S.items()}
    for name, n in [(f"convstack.bn{i}", co) for i, (_, co) in enumerate(CHANS, start=1)] + [("convstack.out_bn", CF)]:
        for leaf in ("weight", "bias"):
            G[f"{name}.{leaf}"] = torch.zeros(n)
    return cs, S, G, r(B, T, CF)


class Recorder:
    def __init__(self, rows_eligible=1, linear_eligible=1, linear_wgrad_eligible=None):
        self.eligible = {"a2s_conv3x3_wgrad_bn_ranged_eligible": rows_eligible, "a2s_linear_dgrad_eligible": linear_eligible,
                         "a2s_linear_wgrad_eligible": linear_eligible if linear_wgrad_eligible is None else linear_wgrad_eligible}
        self.events, self.by_ptr, self.shapes, self.keep, self.fresh, self.block_calls = [], {}, {}, [], 0, {}

    # ---- labels
    def name(self, label, t):
        self.by_ptr[t.data_ptr()], self.shapes[label] = label, tuple(t.shape)
        self.keep.append(t)

    def name_inputs(self, cs, S, G, d_out):
        for k, v in cs.items():
            if isinstance(v, torch.Tensor):
                self.name(f"cs.{k}", v)
            elif isinstance(v, list):
                for i, e in enumerate(v):
                    if isinstance(e, tuple):
                        for j, t in enumerate(e):
                            self.name(f"cs.{k}[{i}][{j}]", t)
                    else:
                        self.name(f"cs.{k}[{i}]", e)
            elif isinstance(v, tuple):
                for j, t in enumerate(v):
                    self.name(f"cs.{k}[{j}]", t)
        for k, v in S.items():
            self.name(f"S.{k}", v)
        for k, v in G.items():
            self.name(f"G.{k}", v)
        self.name("d_out", d_out)

    def label(self, v):
        if isinstance(v, (C.c_void_p, C.c_size_t, C.c_int, C.c_float)):
            v = v.value
            if v is None:
                return None
            if v > 1 << 20:                     # an address (hip.gemm offsets its operands itself)
                return self._ptr_label(v, None)
            return v
        if isinstance(v, torch.Tensor):
            return self._ptr_label(v.data_ptr(), v)
        if isinstance(v, float):
            return round(v, 9)
        return v

    def _ptr_label(self, ptr, t):
        lab = self.by_ptr.get(ptr)
        if lab is None:
            lab = self.by_ptr[ptr] = f"new#{self.fresh}"
            self.fresh += 1
        if t is not None:
            self.keep.append(t)                 # (its address is not handed to a later allocation)
            self.shapes.setdefault(lab, tuple(t.shape))
        return lab

    # ---- the fake library
    def __getattr__(self, fn):
        if not fn.startswith("a2s_"):
            raise AttributeError(fn)
        if fn in self.eligible:
            return lambda *a: self.eligible[fn]
        if fn in BLOCKS:
            def blocks(*a):
                self.block_calls[fn] = self.block_calls.get(fn, -1) + 1
                return BLOCKS[fn] + self.block_calls[fn]
            return blocks
        for sfx, val in QUERY_ANSWERS.items():
            if fn.endswith(sfx):
                return lambda *a: val
        if fn == "a2s_debug_get":
            return lambda *a: 1
        if fn == "a2s_gemm_pick_splitk":
            return lambda *a: 2

        def call(*args):
            assert len(args) == len(PARAMS[fn]), (fn, len(args), PARAMS[fn])
            self.events.append(("call", fn) + tuple(self.label(a) for a in args))
            return 0
        return call

    def trace(self):
        """The events with every new#k completed by the shape it was seen with (a tensor only ever passed as an address has none)."""
        done = lambda v: f"{v}{list(self.shapes[v])}" if isinstance(v, str) and v.startswith("new#") and v in self.shapes else v
        return [tuple(done(v) for v in e) for e in self.events]

    def calls(self):
        """The trace with every library call as ("call", name, {parameter name of include/a2s.h: argument}); the other events as they are."""
        return [("call", e[1], dict(zip(PARAMS[e[1]], e[2:]))) if e[0] == "call" else e for e in self.trace()]


class _Stream:
    def __init__(self, rec, name):
        self.rec, self.name, self.cuda_stream = rec, name, 0

    def wait_event(self, ev):
        self.rec.events.append(("wait_event", self.name, ev.name))

    def wait_stream(self, other):
        self.rec.events.append(("wait_stream", self.name, other.name))


@contextlib.contextmanager
def patched(rec, engine_bwd, hip):
    main, side, n_events = _Stream(rec, "main"), _Stream(rec, "side"), itertools.count()

    class Event:
        def __init__(self):
            self.name = f"event#{next(n_events)}"

        def record(self):
            rec.events.append(("record", self.name))

    @contextlib.contextmanager
    def on_stream(s):
        rec.events.append(("enter", s.name))
        yield
        rec.events.append(("exit", s.name))

    def all_reduce(t):
        rec.events.append(("all_reduce", rec.label(t)))

    with contextlib.ExitStack() as st:
        for target, attr, new in ((hip, "lib", lambda: rec), (hip, "_p", lambda t: t), (hip, "stream", lambda: "stream"),
                                  (torch.cuda, "Event", Event), (torch.cuda, "stream", on_stream), (torch.cuda, "current_stream", lambda *a: main),
                                  (engine_bwd, "_weight_grad_stream", lambda dev: side), (torch.distributed, "all_reduce", all_reduce)):
            st.enter_context(mock.patch.object(target, attr, new))
        yield


def run_case(shape=(3, 23, 128), sync_bn=False, rows_eligible=1, linear_eligible=1, linear_wgrad_eligible=None, cs_extra=None, **attrs):
    """One _convstack_bwd call under the recorder; attrs: engine_bwd module attributes (_FUSE_BN_ROWS=False, _LIN_WGRAD_AT=3, ...).  Returns the Recorder."""
    import torch.distributed  # noqa: F401
    from piano_a2s_amd import engine_bwd, hip
    B, T, F = shape
    torch.manual_seed(0)
    cs, S, G, d_out = make_inputs(B, T, F)
    cs.update(cs_extra or {})
    rec = Recorder(rows_eligible, linear_eligible, linear_wgrad_eligible)
    rec.name_inputs(cs, S, G, d_out)
    eng = SimpleNamespace(cfg={"conv_feature_size": CF}, sync_bn=sync_bn,
                          bn_counts={**{f"convstack.bn{i}": float(B * T * F) for i in range(1, 5)}, "convstack.out_bn": float(B * T)})
    with contextlib.ExitStack() as st:
        for k, v in attrs.items():
            st.enter_context(mock.patch.object(engine_bwd, k, v))
        st.enter_context(patched(rec, engine_bwd, hip))
        engine_bwd._convstack_bwd(eng, S, G, cs, d_out, B, T, F)
    return rec


def matrix():
    for flags in itertools.product((True, False), repeat=len(FLAGS)):
        for sync_bn, shape, rows_ok, lin_ok, lin_at in itertools.product((False, True), ((3, 23, 128), (2, 5, 8)), (1, 0), (1, 0), ("before", "beside", 4, 3, 2)):
            yield dict(zip(FLAGS, flags), sync_bn=sync_bn, shape=shape, rows_eligible=rows_ok, linear_eligible=lin_ok, _LIN_WGRAD_AT=lin_at)


if __name__ == "__main__":
    traces = {json.dumps(case, sort_keys=True): run_case(**case).trace() for case in matrix()}
    with open(sys.argv[1], "w") as f:
        json.dump(traces, f)
    print(len(traces), "cases,", len({json.dumps(t) for t in traces.values()}), "distinct sequences")
