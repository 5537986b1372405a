"""The kern token grammar on the host (piano_a2s_amd/kern_grammar.py) and the constrained CPU oracle (tests/constrained_oracle.py).

Table: shape, classes, no dead end.  Language: the tokenizer's known-answer strings are accepted, a list of ill-formed sequences is rejected
at the right index, random legal walks round-trip through the tokenizer.  Oracle: with the permissive table the helper IS
oracle.model_ref.forward(inference=True) (torch.equal on all four outputs -- that validates the helper); with the real grammar every decoded
row is accepted, while the unconstrained greedy output of the same case is not (asserted: otherwise the test shows nothing)."""
import json
import os
import random
from collections import Counter

import numpy as np
import pytest
import torch

from data_processing.humdrum import LabelsMultiple
from oracle import model_ref
from piano_a2s_amd import metrics, spec, synthetic
from piano_a2s_amd.kern_grammar import KernGrammar, legal_share
from tests import constrained_oracle

SMALL_BATCH = dict(frames=41, upper_range=(3, 10), lower_range=(2, 7), full_tail=0.1)
LAB = LabelsMultiple(extended=True)
ID = LAB.labels_map
SOS, EOS, PAD = ID["<sos>"], ID["<eos>"], ID["<pad>"]


@pytest.fixture(scope="module")
def gram():
    return KernGrammar()


def test_table_shape_classes_and_no_dead_end(gram):
    assert gram.table.shape == (10, 173) and gram.table.dtype == np.int8
    assert (gram.n_states, gram.table[gram.start].tolist(), gram.done) == (10, gram.table[0].tolist(), 9)
    count = Counter(gram.classes)
    assert count == {"DUR": 25, "PITCH": 137, "NULL": 1, "OPEN": 1, "CLOSE": 2, "FERM": 1, "TAB": 1, "NL": 1, "SP": 1, "EOS": 1, "PAD": 1, "SOS": 1}
    assert gram.classes[ID["r"]] == "PITCH" and gram.classes[ID["128"]] == "DUR" and gram.classes[ID["CC-"]] == "PITCH" and gram.classes[ID["8."]] == "DUR"
    legal = gram.table >= 0
    assert legal.any(axis=1).all(), "a state without a legal token is a dead end"
    assert not legal[:, SOS].any()
    assert legal[:, PAD].tolist() == [s == gram.done for s in range(10)]
    assert legal[gram.done].sum() == 1 and gram.table[gram.done, PAD] == gram.done
    assert ((gram.table >= -1) & (gram.table < 10)).all()
    # legal class sets of the issue's table, state by state
    want = {"START": {"OPEN", "DUR", "NULL", "EOS"}, "FIELD": {"OPEN", "DUR", "NULL"}, "CHORD": {"OPEN", "DUR"}, "OPENED": {"DUR"}, "DUR": {"PITCH"},
            "PITCH": {"FERM", "CLOSE", "SP", "TAB", "NL", "EOS"}, "FERM": {"CLOSE", "SP", "TAB", "NL", "EOS"}, "CLOSED": {"SP", "TAB", "NL", "EOS"},
            "NULL": {"TAB", "NL", "EOS"}, "DONE": {"PAD"}}
    for s, name in enumerate(gram.state_names):
        assert {gram.classes[v] for v in np.nonzero(legal[s])[0]} == want[name], name


def test_permissive_table():
    g = KernGrammar.permissive(173)
    assert g.table.shape == (1, 173) and g.table.dtype == np.int8 and (g.table == 0).all() and g.n_states == 1 and g.start == 0
    assert g.accepts([SOS, PAD, EOS, 5, 5])


def test_known_answer_strings_are_accepted(gram, golden_dir):
    kats = json.load(open(os.path.join(golden_dir, "tokenizer_kat.json")))["kats"]
    with_ids = [c for c in kats if "ids" in c]
    assert len(with_ids) >= 6
    for case in with_ids:
        assert gram.accepts(case["ids"]), case["text"]
        assert gram.accepts(case["ids"] + [EOS]), case["text"]
        assert gram.accepts(case["ids"] + [EOS, PAD, PAD]), case["text"]
        assert gram.first_violation(case["ids"] + [EOS, EOS]) == len(case["ids"]) + 1


def test_ill_formed_sequences_are_rejected_at_the_right_index(gram):
    dur, dur2, pitch, null, sp, opn = ID["4"], ID["8."], ID["c"], ID["."], ID["<b>"], ID["["]
    for ids, at in (([dur, dur2], 1),                       # DUR DUR
                    ([pitch], 0),                           # PITCH first
                    ([opn, pitch], 1),                      # OPEN PITCH
                    ([dur, pitch, sp, null], 3),            # SP then NULL
                    ([null, sp], 1),                        # NULL then SP
                    ([dur, EOS], 1),                        # EOS after DUR
                    ([dur, pitch, EOS, dur], 3),            # a token other than PAD after EOS
                    ([dur, pitch, EOS, EOS], 3),
                    ([SOS], 0), ([dur, SOS], 1), ([dur, pitch, SOS], 2), ([dur, pitch, EOS, SOS], 3),      # SOS anywhere
                    ([PAD], 0), ([dur, pitch, PAD], 2),     # PAD before EOS
                    ([dur, pitch, ID["]"], ID[";"]], 3),    # fermata behind the tie mark
                    ([dur, pitch, 173], 2), ([-1], 0)):     # no id of the vocabulary
        assert gram.first_violation(ids) == at, ids
        assert not gram.accepts(ids)
    assert gram.accepts([]) and gram.accepts([EOS]) and gram.accepts([opn, dur, pitch, ID[";"], ID["_"], ID["\t"], null, ID["\n"], dur2, ID["r"], EOS, PAD])
    assert gram.step(gram.start, dur) == gram.state_names.index("DUR") and gram.step(gram.start, pitch) == -1 and gram.step(-1, dur) == -1


def test_random_legal_walks_round_trip_through_the_tokenizer(gram):
    rng = random.Random(20)
    legal_ids = [np.nonzero(gram.table[s] >= 0)[0] for s in range(gram.n_states)]
    by_class = [{} for _ in range(gram.n_states)]
    for s in range(gram.n_states):
        for v in legal_ids[s]:
            by_class[s].setdefault(gram.classes[v], []).append(int(v))
    seen_states = set()
    for _ in range(3000):
        state, ids = gram.start, []
        while True:
            seen_states.add(state)
            classes = sorted(by_class[state])
            if "EOS" in classes and (len(ids) >= 40 or (ids and rng.random() < 0.15)):
                break
            classes = [c for c in classes if c != "EOS"]
            tok = rng.choice(by_class[state][rng.choice(classes)])       # class first: every structural mark is as likely as a pitch
            ids.append(tok)
            state = gram.step(state, tok)
            assert state >= 0
        assert gram.accepts(ids + [EOS])
        assert LAB.encode("".join(LAB.decode(ids))) == ids, ids
    assert seen_states == set(range(gram.n_states)) - {gram.done}


def test_legal_share(gram):
    good, bad = [ID["4"], ID["c"]], [ID["4"], ID["4"]]
    assert legal_share({}) == 1.0
    assert legal_share({"a": [good, bad], "b": [good, []]}, gram) == 0.75


# ------------------------------------------------------------------------------------------- the constrained oracle
@pytest.fixture(scope="module")
def g1(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "g1_small.json")))
    cfg = spec.default_cfg(**meta["cfg"])
    batch = synthetic.make_batch(3, cfg, meta["batch_seed"], **SMALL_BATCH)
    return meta, cfg, batch


def _state(cfg, case):
    P, B = spec.split_state(spec.procedural_state(cfg, case["weights_seed"], eos_bias=case["eos_bias"], lively=True))
    return {k: v.clone() for k, v in P.items()}, {k: v.clone() for k, v in B.items()}


def _rows(ids):
    return [r for k in ("up", "lo") for r in ids[k].reshape(-1, ids[k].shape[-1]).tolist()]


@pytest.mark.parametrize("seed", [11, 18])
def test_constrained_oracle(g1, gram, seed):
    """CPU-measured: rows with <eos> unconstrained / constrained 15 / 30 (s11), 15 / 15 (s18) of 30; unconstrained rows that are no legal
    prefix once cut before their <eos> (what the recipe records): printed below."""
    meta, cfg, batch = g1
    P, B = _state(cfg, meta["cases"][f"greedy_s{seed}"])
    with torch.no_grad():
        ref = model_ref.forward(P, B, cfg, batch[0], inference=True, training=False)
    # (1) permissive table: the helper is the reference's greedy decoder
    outs, decoded, _ = constrained_oracle.forward(P, B, cfg, batch[0], constrained_oracle.GrammarChoice(KernGrammar.permissive(173)))
    for name, a, b in zip(("ts", "key", "up", "lo"), outs, ref):
        assert torch.equal(a, b), name
    free = {}
    for k, o in (("up", ref[2]), ("lo", ref[3])):
        ran = o.abs().sum(-1) > 0
        assert torch.equal(decoded[k][0][ran], o.argmax(-1)[ran]), k
        free[k] = o.argmax(-1).numpy()
    # precondition: the unconstrained output is NOT well-formed (as the recipe records it: cut before the first <eos>)
    free_rows = [metrics.unpad(r).tolist() for r in _rows(free)]
    illegal_free = sum(1 for r in free_rows if not gram.accepts(r))
    # (2) the real grammar
    outs_c, decoded_c, gaps = constrained_oracle.forward(P, B, cfg, batch[0], constrained_oracle.GrammarChoice(gram))
    rows_c = _rows({k: decoded_c[k][0].numpy() for k in ("up", "lo")})
    eos_free = sum(1 for r in _rows(free) if EOS in r)
    eos_c = sum(1 for r in rows_c if EOS in r)
    print(f"greedy_s{seed}: rows {len(rows_c)}, with <eos> unconstrained {eos_free} constrained {eos_c}, illegal unconstrained {illegal_free}, "
          f"smallest legal top-2 gap {min(float(g.min()) for g in gaps.values()):.3e}")
    assert len(rows_c) == 30
    assert illegal_free >= 1, "precondition: the unconstrained greedy output of this case has no ill-formed row, the test would show nothing"
    for r in rows_c:
        assert gram.accepts(r), (gram.first_violation(r), r)
    for k in ("up", "lo"):
        ids, lengths = decoded_c[k]
        for row, n in zip(ids.reshape(-1, ids.shape[-1]).tolist(), lengths.reshape(-1).tolist()):
            assert n == (row.index(EOS) + 1 if EOS in row else len(row))
            assert all(t == PAD for t in row[n:])
    # the log-probabilities stay the model's: every executed row is a normalised distribution, also where the emitted token is not its argmax
    for o in outs_c[2:]:
        ran = o.abs().sum(-1) > 0
        assert torch.allclose(o[ran].exp().sum(-1), torch.ones(int(ran.sum())), atol=1e-5)


# ------------------------------------------------------------------------------------------- the recipe's option
def test_recipe_refuses_the_option_for_a_module_without_it():
    """--constrained_decoding=true with a transcription module that has no `constrained_decoding` attribute (the CPU oracle module of the
    recipe tests): a clear ValueError; without the option nothing is touched."""
    import types
    from piano_a2s_amd import recipe

    def brain(module, **hp):
        b = object.__new__(recipe.ASR)
        b.hparams, b.modules = types.SimpleNamespace(**hp), types.SimpleNamespace(transcription=module)
        return b

    plain = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="constrained_decoding"):
        brain(plain, constrained_decoding=True)._set_constrained_decoding()
    with pytest.raises(ValueError, match="constrained_decoding"):
        brain(plain, constrained_decoding="true")._set_constrained_decoding()
    for off in ({}, {"constrained_decoding": False}, {"constrained_decoding": "false"}):
        b = brain(plain, **off)
        b._set_constrained_decoding()
        assert not b._constrained() and not hasattr(plain, "constrained_decoding")
    capable = torch.nn.Linear(2, 2)
    capable.constrained_decoding = False
    brain(capable, constrained_decoding=True)._set_constrained_decoding()
    assert capable.constrained_decoding is True


def test_model_default_is_unconstrained():
    import models
    assert models.ScoreTranscription.constrained_decoding is False and models.ScoreTranscription.last_decoded is None
