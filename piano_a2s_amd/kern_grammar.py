"""The token grammar of a **kern bar as a finite automaton (host side): the table the constrained greedy decoder walks on the device
(csrc/a2s_grammar.hip) and the checks the tests and the recipe make on decoded ids.

The language is what `LabelsMultiple.encode` can produce for one bar -- its note pattern `(\\[?)(dur)(pitch)(;?)([\\]_]?)` token by token:

    bar   := ( line (NL line)* )? EOS
    line  := field (TAB field)*
    field := NULL | note (SP note)*
    note  := OPEN? DUR PITCH FERM? CLOSE?

Token classes are derived from the symbols of the vocabulary by pattern, never from literal ids.  After <eos> a row emits <pad> only.

`KernMetre` adds the bar's metre to that automaton: every spine's notes abut, a line starts where the earliest spine
ends, and the bar ends exactly at the length of its time signature."""
import json
import os
import re

import numpy as np

from data_processing.humdrum import LabelsMultiple

CLASSES = ("DUR", "PITCH", "NULL", "OPEN", "CLOSE", "FERM", "TAB", "NL", "SP", "EOS", "PAD", "SOS")
STATES = ("START", "FIELD", "CHORD", "OPENED", "DUR", "PITCH", "FERM", "CLOSED", "NULL", "DONE")

_DUR_RE = re.compile(r"\d+\.?")
_PITCH_RE = re.compile(r"r|[a-g]{1,4}[-#]?|[A-G]{1,4}[-#]?")
_FIXED = {".": "NULL", "[": "OPEN", "_": "CLOSE", "]": "CLOSE", ";": "FERM", "\t": "TAB", "\n": "NL", "<b>": "SP",
          "<eos>": "EOS", "<pad>": "PAD", "<sos>": "SOS"}

# state -> {legal class: next state}
_AFTER_NOTE = {"SP": "CHORD", "TAB": "FIELD", "NL": "FIELD", "EOS": "DONE"}
_RULES = {
    "START": {"OPEN": "OPENED", "DUR": "DUR", "NULL": "NULL", "EOS": "DONE"},
    "FIELD": {"OPEN": "OPENED", "DUR": "DUR", "NULL": "NULL"},
    "CHORD": {"OPEN": "OPENED", "DUR": "DUR"},
    "OPENED": {"DUR": "DUR"},
    "DUR": {"PITCH": "PITCH"},
    "PITCH": dict(_AFTER_NOTE, FERM="FERM", CLOSE="CLOSED"),
    "FERM": dict(_AFTER_NOTE, CLOSE="CLOSED"),
    "CLOSED": dict(_AFTER_NOTE),
    "NULL": {"TAB": "FIELD", "NL": "FIELD", "EOS": "DONE"},
    "DONE": {"PAD": "DONE"},
}


def token_class(symbol):
    """Class name of one vocabulary symbol; raises for a symbol the grammar does not know."""
    if symbol in _FIXED:
        return _FIXED[symbol]
    if _DUR_RE.fullmatch(symbol):
        return "DUR"
    if _PITCH_RE.fullmatch(symbol):
        return "PITCH"
    raise ValueError(f"kern grammar: symbol {symbol!r} belongs to no token class")


class KernGrammar:
    """n_states, start, done; table (n_states, V) int8: next state, or -1 where the token is illegal; classes: class name per id."""

    def __init__(self, labels=None):
        labels = list(labels) if labels is not None else LabelsMultiple(extended=True).labels
        self.classes = [token_class(s) for s in labels]
        self.n_states = len(STATES)
        self.start, self.done = STATES.index("START"), STATES.index("DONE")
        self.state_names = STATES
        self.table = np.full((self.n_states, len(labels)), -1, dtype=np.int8)
        for s, name in enumerate(STATES):
            for v, cls in enumerate(self.classes):
                nxt = _RULES[name].get(cls)
                if nxt is not None:
                    self.table[s, v] = STATES.index(nxt)
        self.eos, self.pad = self.classes.index("EOS"), self.classes.index("PAD")
        self._dev = {}

    @classmethod
    def permissive(cls, V):
        """One state, every token legal (the constrained decoder then is the unconstrained one): for testing."""
        g = cls.__new__(cls)
        g.classes = ["ANY"] * V
        g.n_states, g.start, g.done = 1, 0, -1
        g.state_names = ("ANY",)
        g.table = np.zeros((1, V), dtype=np.int8)
        g.eos, g.pad = None, None
        g._dev = {}
        return g

    @property
    def vocab_size(self):
        return self.table.shape[1]

    def step(self, state, token):
        """Next state, or -1 when `token` is illegal in `state` (or no id of the vocabulary)."""
        token = int(token)
        if state < 0 or not 0 <= token < self.table.shape[1]:
            return -1
        return int(self.table[state, token])

    def first_violation(self, ids):
        """Index of the first token that is illegal where it stands, or None: `ids` is then a legal prefix (it may include the <eos>
        and the <pad> behind it)."""
        state = self.start
        for i, tok in enumerate(ids):
            state = self.step(state, tok)
            if state < 0:
                return i
        return None

    def accepts(self, ids):
        """A legal prefix; if it contains <eos>, nothing but <pad> follows."""
        return self.first_violation(ids) is None

    def device_table(self, device):
        """The table as an int8 tensor on `device` (made once per device)."""
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.table).contiguous().to(device)
        return self._dev[key]


def legal_share(pred_dict, grammar=None):
    """Share of the bar rows of a {clip: [bar ids, ...]} dict that the grammar accepts (1.0 for an empty dict).  Rows as the recipe records
    them -- cut before the <eos> -- are prefixes and judged as such."""
    grammar = grammar or KernGrammar()
    rows = [row for bars in pred_dict.values() for row in bars]
    if not rows:
        return 1.0
    return sum(1 for row in rows if grammar.accepts(row)) / len(rows)


# ---------------------------------------------------------------------------------------------------------------- the metre
METRE_W = 147840                      # ticks of a whole note (metrics.NOTE_W)
METRE_FIELDS = 8                      # spines of a bar that are timed (metrics.NOTE_FIELDS): the first line may have no more
METRE_INTS = 16                       # one row's metre state on the device, `a2s_metre_ref.row_metre` of include/a2s.h:
M_L, M_T, M_FIRST, M_NFIELDS, M_FIELD, M_CHORD, M_FDUR, M_END = 0, 1, 2, 3, 4, 5, 6, 8        # ([7] reserved, zero; [8 .. 15] = end[0 .. 7])
METRE_CLS = {"DUR": 1, "NULL": 2, "OPEN": 3, "TAB": 4, "NL": 5, "SP": 6, "EOS": 7}            # A2S_METRE_CLS_* of include/a2s.h; every other class: 0
METRE_RULES = ("syntax", "spine_sounding", "spine_silent", "overfull", "unfillable", "chord_duration", "last_field", "line_incomplete", "bar_full",
               "bar_short")


def bar_ticks():
    """Bar length in ticks per time-signature id of data_processing/metadata/time_signature_list.json: W * num / den."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data_processing", "metadata", "time_signature_list.json")
    with open(path) as f:
        sigs = json.load(f)
    out = []
    for sig in sigs:
        num, den = (int(x) for x in sig.split("/"))
        assert METRE_W * num % den == 0
        out.append(METRE_W * num // den)
    return np.array(out, dtype=np.int32)


def fillable_table(durations, n):
    """fillable[r], r = 0 .. n: r is a sum of (any number of) the given durations.  One pass per duration: an OR along every residue class."""
    fill = np.zeros(n + 1, dtype=bool)
    fill[0] = True
    for d in sorted(set(int(d) for d in durations if d > 0)):
        rows = -(-(n + 1) // d)
        pad = np.zeros(rows * d, dtype=bool)
        pad[:n + 1] = fill
        fill = np.logical_or.accumulate(pad.reshape(rows, d), axis=0).reshape(-1)[:n + 1]
    return fill


class MetreState:
    """Syntax state `s` + the metre of one row: bar length L (<= 0: unmetred), line time t, first_line, n_fields, field, in_chord, field_dur, end[8]."""
    __slots__ = ("s", "L", "t", "first_line", "n_fields", "field", "in_chord", "field_dur", "end")

    def __init__(self, s, L):
        self.s, self.L, self.t, self.first_line, self.n_fields, self.field, self.in_chord, self.field_dur = s, int(L), 0, 1, 0, 0, 0, 0
        self.end = [0] * METRE_FIELDS

    def copy(self):
        c = MetreState(self.s, self.L)
        c.t, c.first_line, c.n_fields, c.field, c.in_chord, c.field_dur, c.end = (self.t, self.first_line, self.n_fields, self.field, self.in_chord,
                                                                                  self.field_dur, list(self.end))
        return c

    def ints(self):
        """The METRE_INTS ints of the device layout."""
        return [self.L, self.t, self.first_line, self.n_fields, self.field, self.in_chord, self.field_dur, 0] + list(self.end)

    @classmethod
    def from_ints(cls, s, v):
        st = cls(s, v[M_L])
        st.t, st.first_line, st.n_fields, st.field, st.in_chord, st.field_dur = (int(x) for x in v[M_T:M_FDUR + 1])
        st.end = [int(x) for x in v[M_END:M_END + METRE_FIELDS]]
        return st


class KernMetre:
    """The kern grammar with the metre of the bar: `grammar` (a KernGrammar over the extended vocabulary), `bar_ticks` (L per time-signature id),
    `dur_ticks` (V,) int32, `cls` (V,) uint8 of METRE_CLS, `fillable` (max L + 1,) bool.  A token is legal when the syntax table allows it and
    `violation` finds no metre rule against it; a row with L <= 0 obeys the syntax alone."""

    def __init__(self, grammar=None):
        self.grammar = grammar or KernGrammar()
        labels = LabelsMultiple(extended=True).labels
        if self.grammar.vocab_size != len(labels):
            raise ValueError("KernMetre needs the grammar of the extended vocabulary: the duration of every symbol is read from it")
        self.bar_ticks = bar_ticks()
        dur = np.zeros(len(labels), dtype=np.int32)
        for i, sym in enumerate(labels):
            if self.grammar.classes[i] == "DUR":                        # reciprocal r: W / r ticks; dotted: 3 W / (2 r)   (as metrics.note_tables)
                dotted = sym.endswith(".")
                num, den = METRE_W * (3 if dotted else 1), int(sym.rstrip(".")) * (2 if dotted else 1)
                assert num % den == 0
                dur[i] = num // den
        self.dur_ticks = dur
        self.cls = np.array([METRE_CLS.get(c, 0) for c in self.grammar.classes], dtype=np.uint8)
        self.fillable = fillable_table(dur, int(self.bar_ticks.max()))
        self._dev = {}

    def length(self, ts_id):
        """L of a time-signature id; 0 (unmetred) for an id outside the list."""
        ts_id = int(ts_id)
        return int(self.bar_ticks[ts_id]) if 0 <= ts_id < len(self.bar_ticks) else 0

    def start(self, ts_id=None, L=None):
        return MetreState(self.grammar.start, self.length(ts_id) if L is None else L)

    @staticmethod
    def _line_min(st):
        n = st.field + 1 if st.first_line else st.n_fields
        return min(st.end[:min(max(n, 1), METRE_FIELDS)])

    def violation(self, st, token):
        """None when `token` is legal in `st`, else the name of the rule against it (METRE_RULES)."""
        if self.grammar.step(st.s, token) < 0:
            return "syntax"
        if st.L <= 0:
            return None
        c = int(self.cls[token])
        field = min(max(st.field, 0), METRE_FIELDS - 1)
        need_note = st.end[field] == st.t
        if c == METRE_CLS["NULL"]:
            return "spine_silent" if need_note else None
        if c == METRE_CLS["OPEN"]:
            return None if (st.in_chord or need_note) else "spine_sounding"
        if c == METRE_CLS["DUR"]:
            d = int(self.dur_ticks[token])
            if st.in_chord:
                return None if d == st.field_dur else "chord_duration"
            if not need_note:
                return "spine_sounding"
            r = st.L - st.t - d
            if r < 0:
                return "overfull"
            return None if (r < len(self.fillable) and self.fillable[r]) else "unfillable"
        if c == METRE_CLS["TAB"]:
            return None if (field < METRE_FIELDS - 1 if st.first_line else field < st.n_fields - 1) else "last_field"
        if c in (METRE_CLS["NL"], METRE_CLS["EOS"]):
            if c == METRE_CLS["EOS"] and st.first_line and field == 0 and st.end[0] == 0:
                return None                                             # the empty bar
            if not (st.first_line or field == st.n_fields - 1):
                return "line_incomplete"
            m = self._line_min(st)
            if c == METRE_CLS["NL"]:
                return None if m < st.L else "bar_full"
            return None if m == st.L else "bar_short"
        return None

    def step(self, st, token):
        """The state after `token`, or None when it is illegal in `st`."""
        if self.violation(st, token) is not None:
            return None
        nx = st.copy()
        nx.s = self.grammar.step(st.s, token)
        if st.L <= 0:
            return nx
        c = int(self.cls[token])
        field = min(max(st.field, 0), METRE_FIELDS - 1)
        if c == METRE_CLS["DUR"] and not st.in_chord:
            nx.end[field], nx.field_dur = st.t + int(self.dur_ticks[token]), int(self.dur_ticks[token])
        elif c == METRE_CLS["SP"]:
            nx.in_chord = 1
        elif c == METRE_CLS["TAB"]:
            nx.field, nx.in_chord = min(field + 1, METRE_FIELDS - 1), 0
        elif c == METRE_CLS["NL"]:
            nx.t = self._line_min(st)
            if st.first_line:
                nx.n_fields, nx.first_line = field + 1, 0
            nx.field, nx.in_chord = 0, 0
        return nx

    def legal_tokens(self, st):
        if not 0 <= st.s < self.grammar.n_states:
            return []
        allowed = np.nonzero(self.grammar.table[st.s] >= 0)[0].tolist()
        if st.L <= 0:
            return allowed
        return [v for v in allowed if self.cls[v] == 0 or self.violation(st, v) is None]       # (class 0: the metre has no rule)

    def walk(self, ids, ts_id=None, L=None):
        """-> (state behind the last legal token, index of the first illegal token or None, its rule or None)."""
        st = self.start(ts_id, L)
        for i, tok in enumerate(ids):
            tok = int(tok)
            rule = self.violation(st, tok) if 0 <= tok < self.grammar.vocab_size else "syntax"
            if rule is not None:
                return st, i, rule
            st = self.step(st, tok)
        return st, None, None

    def first_violation(self, ids, ts_id=None, L=None):
        """(index, rule) of the first token that is illegal where it stands, or None: `ids` is then a legal prefix under the time signature."""
        _, i, rule = self.walk(ids, ts_id, L)
        return None if i is None else (i, rule)

    def accepts(self, ids, ts_id=None, L=None):
        return self.walk(ids, ts_id, L)[1] is None

    def complete(self, ids, ts_id=None, L=None):
        """Accepted, ends in <eos> (nothing but <pad> behind it), and every spine ends at L.  (The empty bar `<eos>` is accepted but not complete
        when the row is metred; an unmetred row is complete when it is accepted and ends.)"""
        st, i, _ = self.walk(ids, ts_id, L)
        if i is not None or st.s != self.grammar.done:
            return False
        if st.L <= 0:
            return True
        n = min(max(st.n_fields if not st.first_line else st.field + 1, 1), METRE_FIELDS)
        return all(e == st.L for e in st.end[:n])

    def device_tables(self, device):
        """{"dur_ticks" int32 (V,), "cls" uint8 (V,), "fillable" uint8 (max L + 1,), "bar_ticks" int32} on `device` (made once per device)."""
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = {"dur_ticks": torch.from_numpy(self.dur_ticks).to(device), "cls": torch.from_numpy(self.cls).to(device),
                              "fillable": torch.from_numpy(self.fillable.astype(np.uint8)).to(device),
                              "bar_ticks": torch.from_numpy(self.bar_ticks).to(device)}
        return self._dev[key]


def complete_share(pred_dict, ts_dict, metre=None):
    """Share of the bar rows of {clip: [bar ids, ...]} that are complete bars under {clip: [time-signature id per bar]} (1.0 for an empty dict).  Rows
    as the recipe records them are cut before the <eos>: a row without one is judged with it appended."""
    metre = metre or KernMetre()
    eos = metre.grammar.eos
    rows = [(list(row), ts) for clip, bars in pred_dict.items() for row, ts in zip(bars, ts_dict[clip])]
    if not rows:
        return 1.0
    return sum(1 for row, ts in rows if metre.complete(row if eos in row else row + [eos], ts)) / len(rows)
