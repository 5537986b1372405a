"""The token grammar of a **kern bar as a finite automaton (host side): the table the constrained greedy decoder walks on the device
(csrc/a2s_grammar.hip) and the checks the tests and the recipe make on decoded ids.

The language is what `LabelsMultiple.encode` can produce for one bar -- its note pattern `(\\[?)(dur)(pitch)(;?)([\\]_]?)` token by token:

    bar   := ( line (NL line)* )? EOS
    line  := field (TAB field)*
    field := NULL | note (SP note)*
    note  := OPEN? DUR PITCH FERM? CLOSE?

Token classes are derived from the symbols of the vocabulary by pattern, never from literal ids.  After <eos> a row emits <pad> only."""
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
