"""What the recorders of the backward pass's host code share (tests/conv_bwd_recorder.py, tests/dec_bwd_recorder.py): a fake liba2s_hip at the C-ABI
level that records every call, and recording stand-ins for the streams, events and torch.cuda.stream.  The real hip.py wrappers run, on CPU tensors.
Every pointer argument is labelled by identity: a tensor named beforehand by its name, a tensor first seen during the run as new#k in order of first
appearance, with its shape.  An argument block passed by reference is recorded as {field: value}, each pointer field labelled like any other pointer.
Every call is held to the parameter count of its prototype in include/a2s.h, whose parameter names Recorder.calls() attaches.  Pure queries (*_eligible,
*_blocks, *_bytes, *_floats, a2s_debug_get, a2s_gemm_pick_splitk) answer fixed values -- the k-th call of a *_blocks function its own number, so that a
block count handed to the wrong consumer shows -- and stay out of the trace."""
import contextlib
import ctypes as C
import itertools
import os
import re
from unittest import mock

import torch

QUERY_ANSWERS = {"_bytes": 64, "_floats": 16}


def _header_params():
    """{function: [parameter names]} of include/a2s.h."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "a2s.h")) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    return {m.group(1): [re.split(r"[\s*]+", p.strip())[-1] for p in m.group(2).split(",")] for m in re.finditer(r"\b(a2s_\w+)\s*\(([^()]*)\)", text)}


PARAMS = _header_params()


class Recorder:
    """answers: {query function: its answer}; blocks: {*_blocks function: the answer of its first call; +1 per further call}; debug: {switch: value} for
    a2s_debug_get (a switch not listed reads 1)."""

    def __init__(self, answers=None, blocks=None, debug=None):
        self.answers, self.blocks, self.debug = answers or {}, blocks or {}, debug or {}
        self.events, self.by_ptr, self.shapes, self.keep, self.fresh, self.block_calls = [], {}, {}, [], 0, {}

    # ---- labels
    @staticmethod
    def _key(t):
        return t.data_ptr() or ("empty", id(t))          # (a tensor without elements has no address: it is its own identity)

    def name(self, label, t):
        self.by_ptr[self._key(t)], self.shapes[label] = label, tuple(t.shape)
        self.keep.append(t)

    def name_tree(self, prefix, v):
        """Names every tensor of a nest of dicts, lists and tuples: prefix.key for a dict's, prefix[i] for a sequence's."""
        if isinstance(v, torch.Tensor):
            self.name(prefix, v)
        elif isinstance(v, dict):
            for k, e in v.items():
                self.name_tree(f"{prefix}.{k}", e)
        elif isinstance(v, (list, tuple)):
            for i, e in enumerate(v):
                self.name_tree(f"{prefix}[{i}]", e)

    def name_host(self, label, array):
        """A host array (ctypes) the library is handed by address."""
        self.by_ptr[C.addressof(array)] = label
        self.keep.append(array)

    def label(self, v):
        if type(v).__name__ == "CArgObject":          # C.byref(argument block)
            return {f: (self._ptr_label(x, None) if x else None) if ct is C.c_void_p else x for (f, ct), x in ((fc, getattr(v._obj, fc[0])) for fc in v._obj._fields_)}
        if isinstance(v, C.Array):
            return self._ptr_label(C.addressof(v), None)
        if isinstance(v, (C.c_void_p, C.c_size_t, C.c_int, C.c_float)):
            v = v.value
            if v is None:
                return None
            if v > 1 << 20:                     # an address (hip.gemm offsets its operands itself)
                return self._ptr_label(v, None)
            return v
        if isinstance(v, torch.Tensor):
            return self._ptr_label(self._key(v), v)
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
        if fn in self.answers:
            return lambda *a: self.answers[fn]
        if fn in self.blocks:
            def blocks(*a):
                self.block_calls[fn] = self.block_calls.get(fn, -1) + 1
                return self.blocks[fn] + self.block_calls[fn]
            return blocks
        for sfx, val in QUERY_ANSWERS.items():
            if fn.endswith(sfx):
                return lambda *a: val
        if fn == "a2s_debug_get":
            return lambda key: self.debug.get(key.decode(), 1)
        if fn == "a2s_gemm_pick_splitk":
            return lambda *a: 2

        def call(*args):
            assert len(args) == len(PARAMS[fn]), (fn, len(args), PARAMS[fn])
            self.events.append(("call", fn) + tuple(self.label(a) for a in args))
            return 0
        return call

    def trace(self):
        """The events with every new#k completed by the shape it was seen with (a tensor only ever passed as an address has none)."""
        def done(v):
            if isinstance(v, dict):
                return {k: done(x) for k, x in v.items()}
            if isinstance(v, (list, tuple)):
                return type(v)(done(x) for x in v)
            return f"{v}{list(self.shapes[v])}" if isinstance(v, str) and v.startswith("new#") and v in self.shapes else v
        return [done(e) for e in self.events]

    def calls(self):
        """The trace with every library call as ("call", name, {parameter name of include/a2s.h: argument}); the other events as they are."""
        return [("call", e[1], dict(zip(PARAMS[e[1]], e[2:]))) if e[0] == "call" else e for e in self.trace()]


class Stream:
    def __init__(self, rec, name, handle=0):
        self.rec, self.name, self.cuda_stream = rec, name, handle

    def wait_event(self, ev):
        self.rec.events.append(("wait_event", self.name, ev.name))

    def wait_stream(self, other):
        self.rec.events.append(("wait_stream", self.name, other.name))


@contextlib.contextmanager
def patched(rec, engine_bwd, hip, main, side, follow_current=False, extra=()):
    """hip and torch.cuda on the recorder.  main: the current stream; side: engine_bwd's weight-gradient stream.  follow_current: hip.stream(),
    torch.cuda.current_stream() and Event.record() follow the torch.cuda.stream contexts (else they read "stream" / main / no stream: code that
    never asks inside a context).  extra: further (object, attribute, replacement) patches."""
    n_events, current = itertools.count(), [main]

    class Event:
        def __init__(self):
            self.name = f"event#{next(n_events)}"

        def record(self):
            rec.events.append(("record", self.name) + ((current[-1].name,) if follow_current else ()))

    @contextlib.contextmanager
    def on_stream(s):
        rec.events.append(("enter", s.name))
        current.append(s)
        try:
            yield
        finally:
            current.pop()
        rec.events.append(("exit", s.name))

    with contextlib.ExitStack() as st:
        for target, attr, new in ((hip, "lib", lambda: rec), (hip, "_p", lambda t: t), (hip, "stream", (lambda: current[-1].name) if follow_current else (lambda: "stream")),
                                  (torch.cuda, "Event", Event), (torch.cuda, "stream", on_stream),
                                  (torch.cuda, "current_stream", (lambda *a: current[-1]) if follow_current else (lambda *a: main)),
                                  (engine_bwd, "_weight_grad_stream", lambda dev: side)) + tuple(extra):
            st.enter_context(mock.patch.object(target, attr, new))
        yield
