"""The metre of a kern bar on the host (piano_a2s_amd/kern_grammar.py: KernMetre) and the metrical CPU oracle
(tests/metre_oracle.py).

Tables: the seven bar lengths, `fillable` against brute force.  Language: hand-written bars accepted, or rejected at the right index by the right
rule; every scoregen bar is complete under its clip's time signature; on random legal walks a legal token always exists and the walk that takes
the longest legal duration and closes lines as soon as it may ends complete; with L = 0 the metre is the syntax grammar.  Oracle: with every
L = 0 it is constrained_oracle.forward under GrammarChoice (torch.equal)."""
import json
import os
import random

import numpy as np
import pytest
import torch

from data_processing.humdrum import LabelsMultiple
from piano_a2s_amd import scoregen, spec, synthetic
from piano_a2s_amd.kern_grammar import METRE_CLS, METRE_INTS, METRE_RULES, METRE_W, KernGrammar, KernMetre, MetreState, complete_share, fillable_table
from tests import constrained_oracle, metre_oracle

SMALL_BATCH = dict(frames=41, upper_range=(3, 10), lower_range=(2, 7), full_tail=0.1)
LAB = LabelsMultiple(extended=True)
ID = LAB.labels_map
EOS, PAD = ID["<eos>"], ID["<pad>"]
TWO_SPINES = "4c\t8e 8g\n.\t8a\n4r\t4r\n2d\t2d"          # a 4/4 bar whose spines move at different paces on its first two lines


@pytest.fixture(scope="module")
def metre():
    return KernMetre()


def test_bar_lengths(metre):
    sigs = scoregen.time_signatures()
    assert sigs == ["4/4", "3/4", "2/4", "6/8", "2/2", "12/8", "3/8"]
    assert metre.bar_ticks.tolist() == [147840, 110880, 73920, 110880, 147840, 221760, 55440]
    assert [metre.length(i) for i in range(7)] == metre.bar_ticks.tolist() and metre.length(7) == 0 and metre.length(-1) == 0
    assert METRE_W == 147840 and len(metre.fillable) == 221760 + 1 and metre.start(0).ints() == [147840, 0, 1, 0, 0, 0, 0, 0] + [0] * 8
    assert len(metre.start(0).ints()) == METRE_INTS
    from piano_a2s_amd import metrics
    assert np.array_equal(metre.dur_ticks, metrics.note_tables()["dur_ticks"]) and int((metre.dur_ticks > 0).sum()) == 25


def test_fillable_against_brute_force(metre):
    durs = sorted(set(int(d) for d in metre.dur_ticks if d > 0))
    assert int(np.gcd.reduce(durs + metre.bar_ticks.tolist())) == 1
    n = 12000                                        # above the eleven shortest symbols: sums of up to 14 terms occur
    brute = [False] * (n + 1)
    brute[0] = True
    for r in range(1, n + 1):                        # the definition, one remainder at a time
        brute[r] = any(d <= r and brute[r - d] for d in durs)
    assert metre.fillable[:n + 1].tolist() == brute
    assert 0 < sum(brute) < n
    share = 1.0 - float(metre.fillable.mean())
    print(f"remainders in 0 .. {len(metre.fillable) - 1} that no sum of duration symbols fills: {share:.4f}")
    assert 0.05 < share < 0.10                       # "about 7 %"
    assert all(metre.fillable[L] for L in metre.bar_ticks) and all(metre.fillable[d] for d in durs)
    assert fillable_table([3, 5], 12).tolist() == [True, False, False, True, False, True, True, False, True, True, True, True, True]


def _ids(words):
    """Token ids of a bar written word by word: TAB, NL, SP (the chord separator) and EOS by name, every other word a symbol of the vocabulary."""
    names = {"TAB": "\t", "NL": "\n", "SP": "<b>", "EOS": "<eos>"}
    return [ID[names.get(w, w)] for w in words.split()]


def test_hand_written_bars(metre):
    ok = LAB.encode(TWO_SPINES)
    assert ok == _ids("4 c TAB 8 e SP 8 g NL . TAB 8 a NL 4 r TAB 4 r NL 2 d TAB 2 d")
    assert metre.accepts(ok, 0) and metre.first_violation(ok, 0) is None and not metre.complete(ok, 0)
    assert metre.complete(ok + [EOS], 0) and metre.complete(ok + [EOS, PAD, PAD], 0) and metre.complete(ok + [EOS], 4)          # 4/4 and 2/2
    assert metre.first_violation(ok + [EOS], 1) == (len(ok) - 5, "overfull")                                                   # 3/4: the half notes do not fit
    for words, at, rule in (
            ("4 c TAB 8 e SP 8 g NL 4 r", 9, "spine_sounding"),                    # spine 0 still sounds on line 2: rejected at the `4`
            ("4 c TAB . NL", 3, "spine_silent"),                                   # a `.` where nothing sounds
            ("2 c NL 2 d NL 8 e", 5, "bar_full"),                                  # a line break in a full bar
            ("2 c NL 2. d", 3, "overfull"),                                        # an over-full bar
            ("1 c NL", 2, "bar_full"),
            ("4 c NL 4 d EOS", 5, "bar_short"),                                    # <eos> in a half-full bar
            ("4 c SP 8 e", 3, "chord_duration"),                                   # a chord member of another duration
            ("4 c SP [ 8 e", 4, "chord_duration"),
            ("4 c SP 4 e SP 4. g", 6, "chord_duration"),
            ("4 c TAB 4 d NL 4 e", None, None),                                    # (a legal prefix)
            ("4 c TAB 4 d NL 4 e NL", 8, "line_incomplete"),                       # the second line is one field short
            ("4 c TAB 4 d NL 4 e TAB 4 f TAB", 11, "last_field"),                  # ... or one field too long
            ("4 c TAB " * 7 + "4 c TAB", 23, "last_field"),                        # more than eight spines
            ("4 c TAB 8 d NL [ 4 e", 6, "spine_sounding"),                         # a tie opens a note all the same
            ("4 c TAB 8 d NL . TAB .", 8, "spine_silent")):
        ids = _ids(words)
        want = None if rule is None else (at, rule)
        assert metre.first_violation(ids, 0) == want, (words, metre.first_violation(ids, 0), want)
        assert metre.accepts(ids, 0) == (rule is None)
    # a duration that leaves a remainder no sum of duration symbols fills
    # (from the start of a bar every duration leaves one; behind a first note on a line of its own some do not)
    durs = [int(v) for v in np.nonzero(metre.dur_ticks)[0]]
    found = [(ts, a, b) for ts in range(7) for a in durs for b in durs
             if 0 <= metre.length(ts) - metre.dur_ticks[a] - metre.dur_ticks[b] and metre.fillable[metre.length(ts) - metre.dur_ticks[a]]
             and not metre.fillable[metre.length(ts) - metre.dur_ticks[a] - metre.dur_ticks[b]]]
    print(f"{len(found)} (time signature, first, second duration) triples leave an unfillable remainder, e.g. {[LAB.labels[v] for v in found[0][1:]]}")
    assert found
    for ts, a, b in found[:50]:
        assert metre.first_violation([a, ID["c"], ID["\n"], b], ts) == (3, "unfillable")
    assert all(metre.violation(metre.start(ts), v) is None for ts in range(7) for v in durs if metre.dur_ticks[v] <= metre.length(ts))
    assert metre.accepts([EOS], 0) and metre.accepts([EOS, PAD], 0) and not metre.complete([EOS], 0) and metre.complete([EOS], 7)
    assert metre.first_violation([173], 0) == (0, "syntax") and metre.first_violation([ID["c"]], 0) == (0, "syntax")


def test_scoregen_bars_are_complete(metre):
    cfg = spec.default_cfg()
    n, seen, pred, ts = 0, set(), {}, {}
    for seed in range(300):
        clip = scoregen.make_clip(cfg, seed)
        seen.add(clip["ts"])
        for staff in ("upper", "lower"):
            for ids in clip["ids"][staff]:
                n += 1
                assert metre.complete(list(ids) + [EOS], clip["ts"]), (seed, staff, metre.first_violation(list(ids) + [EOS], clip["ts"]))
            pred[(seed, staff)], ts[(seed, staff)] = [list(ids) for ids in clip["ids"][staff]], [clip["ts"]] * len(clip["ids"][staff])
    assert n == 3000 and seen == set(range(7))
    assert complete_share(pred, ts, metre) == 1.0 and complete_share({}, {}, metre) == 1.0
    wrong = {k: [(t + 1) % 7 if metre.length((t + 1) % 7) != metre.length(t) else (t + 2) % 7 for t in v] for k, v in ts.items()}
    assert complete_share(pred, wrong, metre) == 0.0
    assert complete_share({"a": [LAB.encode(TWO_SPINES), LAB.encode("4c")]}, {"a": [0, 0]}, metre) == 0.5


def test_random_walks_never_dead_end_and_greedy_walks_end_complete(metre):
    rng = random.Random(23)
    cls, dur = metre.cls, metre.dur_ticks
    seen_rules, n_complete = set(), 0
    for i in range(3000):
        ts = i % 7
        # (a) a random legal walk: a legal token exists in every state it reaches
        st, n = metre.start(ts), 0
        while st.s != metre.grammar.done and n < 60:
            legal = metre.legal_tokens(st)
            assert legal, (ts, st.s, st.ints())
            by_class = {}
            for v in legal:
                by_class.setdefault(int(cls[v]) if cls[v] else metre.grammar.classes[v], []).append(v)
            assert all(metre.fillable[st.L - e] for e in st.end[:max(st.n_fields, st.field + 1)]), "L - end[j] stays fillable for every spine"
            if n % 7 == 0:                               # (now and then: every rejected token names a rule)
                seen_rules.update(r for r in (metre.violation(st, v) for v in range(173)) if r)
            st = metre.step(st, rng.choice(by_class[rng.choice(sorted(by_class, key=str))]))
            n += 1
        # (b) the walk that takes the longest legal duration and closes lines as soon as it may (spines: 1 .. 3) ends complete
        st, ids, spines = metre.start(ts), [], 1 + i % 3
        while st.s != metre.grammar.done:
            legal = metre.legal_tokens(st)
            assert legal
            kinds = {int(cls[v]) for v in legal}
            if METRE_CLS["EOS"] in kinds and ids:
                tok = EOS
            elif METRE_CLS["NL"] in kinds and (not st.first_line or st.field == spines - 1):
                tok = ID["\n"]
            elif METRE_CLS["TAB"] in kinds and (not st.first_line or st.field < spines - 1):
                tok = ID["\t"]
            elif METRE_CLS["NULL"] in kinds:
                tok = ID["."]
            elif METRE_CLS["DUR"] in kinds:
                tok = max((v for v in legal if cls[v] == METRE_CLS["DUR"]), key=lambda v: (dur[v], -v))
            else:
                tok = next(v for v in legal if metre.grammar.classes[v] == "PITCH")
            ids.append(int(tok))
            st = metre.step(st, tok)
            assert len(ids) < 200
        assert metre.complete(ids, ts), (ts, spines, ids)
        n_complete += 1
    assert n_complete == 3000 and set(seen_rules) <= set(METRE_RULES) and {"syntax", "spine_silent", "spine_sounding", "overfull", "unfillable", "bar_short"} <= seen_rules


def test_unmetred_rows_obey_the_syntax_alone(metre):
    gram, rng = metre.grammar, random.Random(31)
    for i in range(500):
        ids = []
        state = gram.start
        for _ in range(rng.randrange(1, 30)):
            legal = np.nonzero(gram.table[state] >= 0)[0] if state >= 0 else []
            tok = int(rng.choice(legal)) if len(legal) and rng.random() < 0.93 else rng.randrange(-1, 175)       # now and then any id
            ids.append(tok)
            state = gram.step(state, tok) if state >= 0 else -1
        for kw in (dict(L=0), dict(ts_id=7), dict(ts_id=-1), dict(L=-5)):
            assert metre.accepts(ids, **kw) == gram.accepts(ids)
            fv = metre.first_violation(ids, **kw)
            assert (fv[0] if fv else None) == gram.first_violation(ids) and (fv is None or fv[1] == "syntax")
    st = metre.start(L=0)
    nx = metre.step(st, ID["4"])
    assert nx.ints() == st.ints() and nx.s == gram.step(gram.start, ID["4"]), "an unmetred row's metre ints are never touched"
    assert MetreState.from_ints(3, metre.start(2).ints()).ints() == metre.start(2).ints()


# ------------------------------------------------------------------------------------------- the metrical oracle
@pytest.fixture(scope="module")
def g1(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "g1_small.json")))
    cfg = spec.default_cfg(**meta["cfg"])
    batch = synthetic.make_batch(3, cfg, meta["batch_seed"], **SMALL_BATCH)
    return meta, cfg, batch


def _state(cfg, case):
    P, B = spec.split_state(spec.procedural_state(cfg, case["weights_seed"], eos_bias=case["eos_bias"], lively=True))
    return {k: v.clone() for k, v in P.items()}, {k: v.clone() for k, v in B.items()}


@pytest.mark.parametrize("seed", [11, 18])
def test_metre_oracle(g1, metre, seed):
    meta, cfg, batch = g1
    P, B = _state(cfg, meta["cases"][f"greedy_s{seed}"])
    # (1) every L = 0: the helper is the constrained oracle
    ref, ref_dec, ref_gaps = constrained_oracle.forward(P, B, cfg, batch[0], constrained_oracle.GrammarChoice(metre.grammar))
    outs, dec, gaps = metre_oracle.forward(P, B, cfg, batch[0], metre_oracle.MetreChoice(metre, lengths=lambda ts: 0))
    for name, a, b in zip(("ts", "key", "up", "lo"), outs, ref):
        assert torch.equal(a, b), name
    for k in ("up", "lo"):
        assert torch.equal(dec[k][0], ref_dec[k][0]) and torch.equal(dec[k][1], ref_dec[k][1]) and torch.equal(gaps[k], ref_gaps[k])
    # (2) the metre: no dead end (asserted inside MetreChoice.pick), every row accepted under the bar's own time signature, the heads unchanged
    outs_m, dec_m, gaps_m = metre_oracle.forward(P, B, cfg, batch[0], metre_oracle.MetreChoice(metre))
    ts_ids = outs_m[0].argmax(-1)
    n_rows = n_differ = 0
    for k in ("up", "lo"):
        ids, lengths = dec_m[k]
        for b in range(ids.shape[0]):
            for bar in range(ids.shape[1]):
                row = ids[b, bar].tolist()
                assert metre.accepts(row, int(ts_ids[b, bar])), (k, b, bar, metre.first_violation(row, int(ts_ids[b, bar])))
                assert int(lengths[b, bar]) == (row.index(EOS) + 1 if EOS in row else len(row))
                if EOS in row and row.index(EOS) > 0:
                    assert metre.complete(row, int(ts_ids[b, bar]))
                n_rows += 1
                n_differ += row != ref_dec[k][0][b, bar].tolist()
    assert torch.equal(outs_m[0][:, 0], ref[0][:, 0]) and torch.equal(outs_m[1][:, 0], ref[1][:, 0]), "bar 0's heads do not depend on any note decoder"
    print(f"greedy_s{seed}: {n_differ} of {n_rows} rows differ from the syntax-only decoding; smallest legal top-2 gap "
          f"{min(float(gaps_m[k].min()) for k in ('up', 'lo')):.3e}, time-signature top-2 gap {float(gaps_m['ts'].min()):.3e}")
    assert n_rows == 30 and n_differ >= 1, "the metre changes nothing in this case: the test would show nothing"
