"""The beam-search CPU oracle (tests/beam_oracle.py) checked on the CPU: one slot under the kern grammar IS the constrained greedy oracle, and a
hand-made example pins the selection rule (ties, a finished hypothesis pushed out of the beam, a dead slot, the length penalty)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import beam_oracle, constrained_oracle

SMALL_BATCH = dict(frames=41, upper_range=(3, 10), lower_range=(2, 7), full_tail=0.1)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAD_, EOS_ = 0, 1               # the hand-made example's own five-token vocabulary: <pad>, <eos>, a, b, c


@pytest.mark.parametrize("seed", [11, 18])
def test_one_slot_under_the_grammar_is_the_constrained_oracle(seed):
    from piano_a2s_amd import spec, synthetic
    from piano_a2s_amd.kern_grammar import KernGrammar
    meta = json.load(open(os.path.join(GOLDEN, "g1_small.json")))
    cfg = spec.default_cfg(**meta["cfg"])
    batch = synthetic.make_batch(3, cfg, meta["batch_seed"], **SMALL_BATCH)
    case = meta["cases"][f"greedy_s{seed}"]
    P, B = spec.split_state(spec.procedural_state(cfg, case["weights_seed"], eos_bias=case["eos_bias"], lively=True))
    gram = KernGrammar()
    ref_outs, ref_dec, gaps = constrained_oracle.forward(P, B, cfg, batch[0], constrained_oracle.GrammarChoice(gram))
    outs, dec, scores, margins = beam_oracle.forward(P, B, cfg, batch[0], 1, gram)
    for k in ("up", "lo"):
        assert torch.equal(dec[k][0], ref_dec[k][0]) and torch.equal(dec[k][1], ref_dec[k][1]), k
    for a, b in zip(outs, ref_outs):
        assert torch.equal(a, b)
    # one slot: the step margin is the greedy oracle's smallest legal top-2 gap, and there is no runner-up
    assert margins[0] == pytest.approx(min(float(g.min()) for g in gaps.values()), abs=1e-6) and margins[1] == float("inf")
    # the score of a bar is the sum of its emitted tokens' log-probabilities
    for k, o in (("up", outs[2]), ("lo", outs[3])):
        ids, lengths = dec[k]
        for b in range(ids.shape[0]):
            for bar in range(ids.shape[1]):
                want = sum(float(o[b, bar, t, ids[b, bar, t]]) for t in range(int(lengths[b, bar])))     # (no <eos>: the call ran to max_steps)
                assert float(scores[k][b, bar]) == pytest.approx(want, abs=1e-4)


def _lp(**p):
    """log of a five-token distribution given by name; what is not named shares the rest."""
    names = ["pad", "eos", "a", "b", "c"]
    rest = (1.0 - sum(p.values())) / (5 - len(p))
    return np.log(np.array([p.get(n, rest) for n in names], dtype=np.float32)).astype(np.float32)


def _start(K):
    scores = np.full(K, -np.inf, dtype=np.float32)
    scores[0] = 0
    fin = np.ones(K, dtype=bool)
    fin[0] = False
    return scores, fin, np.zeros(K, dtype=np.int64)


def test_hand_made_two_clips():
    K = 2
    dead_row = _lp(a=0.2)
    # ---- clip 0: an exact three-way tie at the first step, then the finished hypothesis stays in the beam
    scores, fin, st = _start(K)
    tie = _lp(eos=0.3, a=0.3, b=0.3)
    tok, par, sc, st, fin, gap = beam_oracle.select(scores, fin, st, np.stack([tie, dead_row]), None, K, pad=PAD_, eos=EOS_)
    assert tok == [1, 2] and par == [0, 0] and gap == 0.0, "ties go to the lowest flat index: <eos> (1), then a (2); b (3) is dropped at the same score"
    assert fin == [True, False] and sc[0] == sc[1] == tie[1]
    tok2, par2, sc2, st2, fin2, gap2 = beam_oracle.select(np.array(sc), np.array(fin), np.array(st), np.stack([_lp(a=0.9), _lp(a=0.9, b=0.09)]), None, K, pad=PAD_, eos=EOS_)
    assert tok2 == [PAD_, 2] and par2 == [0, 1] and fin2 == [True, False], "a finished slot offers <pad> at its own score, whatever its row computes"
    assert sc2[0] == sc[0] and sc2[1] == np.float32(sc[1]) + _lp(a=0.9, b=0.09)[2]
    # ---- clip 1: a hypothesis finishes in slot 1 and is pushed out one step later by two continuations of slot 0
    scores, fin, st = _start(K)
    tok, par, sc, st, fin, _ = beam_oracle.select(scores, fin, st, np.stack([_lp(a=0.5, b=0.3), dead_row]), None, K, pad=PAD_, eos=EOS_)
    assert tok == [2, 3] and par == [0, 0] and fin == [False, False]
    tok, par, sc, st, fin, _ = beam_oracle.select(np.array(sc), np.array(fin), np.array(st), np.stack([_lp(a=0.9, b=0.05), _lp(eos=0.5)]), None, K, pad=PAD_, eos=EOS_)
    assert tok == [2, EOS_] and par == [0, 1] and fin == [False, True]
    done_before = sum(fin)
    tok, par, sc, st, fin, _ = beam_oracle.select(np.array(sc), np.array(fin), np.array(st), np.stack([_lp(a=0.5, b=0.45), dead_row]), None, K, pad=PAD_, eos=EOS_)
    assert tok == [2, 3] and par == [0, 0] and fin == [False, False], "both continuations of slot 0 beat the finished hypothesis"
    assert sum(fin) - done_before == -1, "the clip's finished count goes DOWN: the kernel adds the change, it never increments per hit"
    # ---- a dead slot: a table whose start state allows only `a` leaves the second slot without a live candidate
    table = np.full((2, 5), -1, dtype=np.int8)
    table[0, 2] = 1
    table[1, :] = 1
    scores, fin, st = _start(K)
    tok, par, sc, st, fin, gap = beam_oracle.select(scores, fin, st, np.stack([_lp(a=0.2), dead_row]), table, K, pad=PAD_, eos=EOS_)
    assert tok[0] == 2 and st[0] == 1 and not fin[0]
    assert sc[1] == -np.inf and fin[1] and (par[1], tok[1]) == (0, 0) and st[1] == 0, "dead: -inf, finished, the lowest flat index, the state not moved"
    assert gap == float("inf")
    tok, par, sc, st, fin, _ = beam_oracle.select(np.array(sc), np.array(fin), np.array(st), np.stack([_lp(a=0.5, b=0.3), dead_row]), table, K, pad=PAD_, eos=EOS_)
    assert tok == [2, 3] and par == [0, 0] and fin == [False, False], "a dead slot can never win, and is replaced as soon as there are K live candidates"
    # ---- the length penalty changes the pick
    assert beam_oracle.pick([-2.0, -2.5], [2, 5], 0.0) == (0, 0.5)
    slot, gap = beam_oracle.pick([-2.0, -2.5], [2, 5], 1.0)
    assert slot == 1 and gap == pytest.approx(0.5)
    assert beam_oracle.pick([-2.0, -2.0], [3, 3], 0.7)[0] == 0, "ties go to the lowest slot"
    assert beam_oracle.pick([-1.0, -math.inf], [3, 3], 0.0) == (0, float("inf"))
    # ---- walking back: the lineage of slot 1 after three steps, and the slot it occupied during each of them
    tokens = [np.array([2, 3]), np.array([2, EOS_]), np.array([PAD_, 4])]
    parents = [np.array([0, 0]), np.array([1, 0]), np.array([1, 0])]
    assert beam_oracle.backtrack(tokens, parents, 1, 3, eos=EOS_) == ([3, 2, 4], [0, 1, 0], -1)
    assert beam_oracle.backtrack(tokens, parents, 0, 3, eos=EOS_) == ([2, EOS_, PAD_], [0, 0, 1], 1)
