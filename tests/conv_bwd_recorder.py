"""engine_bwd._convstack_bwd driven without a GPU: a fake liba2s_hip at the C-ABI level that records every call, recording stand-ins for the streams,
events and the all-reduce, CPU tensors everywhere (the generic half: tests/abi_recorder.py).  The real hip.py wrappers run.  Every pointer argument is labelled by identity: a tensor of cs, S
or G by its key (cs.abound[2], G.convstack.conv3.weight), d_out by its name, a tensor first seen during the call as new#k in order of first
appearance, with its shape.  Every call is held to the parameter count of its prototype in include/a2s.h, whose parameter names Recorder.calls() attaches.
Pure queries (*_eligible, *_blocks, *_bytes, *_floats, a2s_debug_get, a2s_gemm_pick_splitk) answer fixed values -- the k-th call of a *_blocks function
its own number, so that a block count handed to the wrong consumer shows -- and stay out of the trace.  tests/test_conv_bwd_plan_cpu.py asserts the wiring
on these traces; run as a script (python -m tests.conv_bwd_recorder OUT.json) it writes the traces of the whole switch matrix, to compare two commits
case by case."""
import contextlib
import itertools
import json
import sys
from types import SimpleNamespace
from unittest import mock

import torch

from tests import abi_recorder

CHANS = [(1, 20), (20, 20), (20, 40), (40, 40)]
FLAGS = ("_FUSE_BN_ROWS", "_DGRAD_BNSTATS", "_SYNC_FUSED", "_FUSE_BN_APPLY", "_FUSE_BN_APPLY_L1")
CF = 8
BLOCKS = {"a2s_conv3x3_stat_blocks": 11, "a2s_linear_dgrad_blocks": 21, "a2s_gemm_bnstats_blocks": 31}          # answer of the first call; +1 per further call


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


class Recorder(abi_recorder.Recorder):
    def __init__(self, rows_eligible=1, linear_eligible=1, linear_wgrad_eligible=None):
        super().__init__({"a2s_conv3x3_wgrad_bn_ranged_eligible": rows_eligible, "a2s_linear_dgrad_eligible": linear_eligible,
                          "a2s_linear_wgrad_eligible": linear_eligible if linear_wgrad_eligible is None else linear_wgrad_eligible}, BLOCKS)

    def name_inputs(self, cs, S, G, d_out):
        for prefix, v in (("cs", cs), ("S", S), ("G", G), ("d_out", d_out)):
            self.name_tree(prefix, v)


@contextlib.contextmanager
def patched(rec, engine_bwd, hip):
    def all_reduce(t):
        rec.events.append(("all_reduce", rec.label(t)))

    with abi_recorder.patched(rec, engine_bwd, hip, abi_recorder.Stream(rec, "main"), abi_recorder.Stream(rec, "side"),
                              extra=((torch.distributed, "all_reduce", all_reduce),)):
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
