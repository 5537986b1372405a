"""Beam-search decoding on the MI355X (csrc/a2s_beam.hip, Engine.beam_size, --beam_size):

1. the op (beam_step_finalize + beam_backtrack through a2s_beam_step / a2s_beam_backtrack) against numpy;
2. one slot forced through the beam loop under the kern grammar IS the constrained greedy decoder, bit for bit (small and full width);
3. the small model against the beam CPU oracle (tests/beam_oracle.py): ids and lengths exact, log-probs and scores within 1e-4;
4. full width without an oracle: the selection replayed on the host bit for bit, every row accepted by the grammar, the run replayed through
   the teacher-forced path, the scores against the returned log-probs;
5. the recipe with --beam_size."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # as tests/test_gpu_forward.py: relative to max(1, |ref|max)
SMALL_BATCH = dict(frames=41, upper_range=(3, 10), lower_range=(2, 7), full_tail=0.1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 173
NEG = -np.inf


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gram():
    from piano_a2s_amd.kern_grammar import KernGrammar
    return KernGrammar()


# ------------------------------------------------------------------------------------------- 1. the op
def _log_softmax64(x):
    x = x.astype(np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def _select_np(score, fin, state, lp, table, K, pad, eos):
    """One clip: the specification in numpy.  score (K,) f32, fin (K,) bool, state (K,), lp (K, V) f32 -> new (tok, par, score, state, fin) arrays and
    the smallest non-zero difference between neighbours among the K + 1 best candidates (what a rounding error would have to bridge)."""
    vals = np.full((K, V), NEG, dtype=np.float32)
    valid = np.zeros((K, V), dtype=bool)
    for k in range(K):
        if fin[k]:
            valid[k, pad], vals[k, pad] = True, score[k]
        else:
            valid[k] = True
            legal = np.ones(V, dtype=bool) if table is None else table[state[k]] >= 0
            vals[k, legal] = (np.float32(score[k]) + lp[k, legal]).astype(np.float32)
    flat = np.nonzero(valid.reshape(-1))[0]
    v = vals.reshape(-1)[flat]
    order = np.lexsort((flat, -v.astype(np.float64)))
    top = v[order[:K + 1]].astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = -np.diff(top)
    d = d[np.isfinite(d) & (d > 0)]
    sep = float(d.min()) if d.size else float("inf")
    tok, par, sc, st, fn = (np.zeros(K, dtype=np.int64) for _ in range(5))
    sc = np.zeros(K, dtype=np.float32)
    for j in range(K):
        f = int(flat[order[j]])
        par[j], tok[j], sc[j] = f // V, f % V, v[order[j]]
        s = int(state[par[j]])
        if table is not None and not fin[par[j]] and table[s, tok[j]] >= 0:
            s = int(table[s, tok[j]])
        st[j] = s
        fn[j] = int(bool(fin[par[j]]) or tok[j] == eos or not sc[j] > NEG)
    return tok, par, sc, st, fn, sep


def _op_case(gram, K, with_table, rng):
    """Two launches over B = 3 clips.  Launch 0 (the start of a call): clip 0 with an exact three-way tie of legal tokens on top (first, middle and
    last legal id: different lanes, different registers) -- its new slots all share parent 0.  Launch 1 (a state set by hand): clip 0's parents
    are a cyclic permutation; clip 1 drops a finished slot (two continuations of every live slot beat it); clip 2 emits <eos> in one slot and
    carries a dead one (K >= 3)."""
    B = 3
    table = gram.table if with_table else None
    eos, pad = gram.eos, gram.pad
    s_eos = int(np.nonzero(gram.table[:, eos] >= 0)[0][0])          # a state in which <eos> is legal
    start = gram.start if with_table else 0

    def separated():
        # 173 values 0.01 apart in [-2, -0.28]: their exp sum is ~62, so a token planted at 5.0 holds 70 % of the mass and every
        # log-probability stays above -7.4
        return (rng.permutation(V).astype(np.float32) * np.float32(0.01) - np.float32(2.0)).reshape(V)

    def legal_ids(s):
        ids = np.nonzero(gram.table[s] >= 0)[0] if with_table else np.arange(V)
        return np.array([i for i in ids if i not in (eos, pad)])

    steps = []
    # ---- launch 0
    x = np.stack([separated() for _ in range(K * B)])
    lg = legal_ids(start)
    x[0 * B + 0, [lg[0], lg[len(lg) // 2], lg[-1]]] = 3.0
    steps.append(dict(logits=x, state=None))
    # ---- launch 1
    x = np.stack([separated() for _ in range(K * B)])
    score = np.zeros((K, B), dtype=np.float32)
    fin = np.zeros((K, B), dtype=bool)
    state = np.full((K, B), start, dtype=np.int64)
    if with_table:
        state[:, 0] = [(3 + k) % gram.n_states if (3 + k) % gram.n_states != gram.done else 0 for k in range(K)]
    # clip 0: slot k holds score -(1 + ((k - 1) mod K)): slot 1 is best, then 2, ..., slot 0 last; every slot has ONE dominant legal token
    for k in range(K):
        score[k, 0] = -(1.0 + ((k - 1) % K))
        x[k * B + 0, legal_ids(state[k, 0])[k % len(legal_ids(state[k, 0]))]] = 5.0
    # clip 1: the last slot is finished far behind; the live ones have two strong legal tokens each
    for k in range(K):
        score[k, 1] = -1.0 - 0.15 * k
        ids = legal_ids(state[k, 1])
        x[k * B + 1, ids[1]] = 5.0
        x[k * B + 1, ids[-2]] = 4.5
    fin[K - 1, 1], score[K - 1, 1] = True, -30.0
    if with_table:
        state[K - 1, 1] = gram.done
    # clip 2: slot 0's dominant token is <eos>; slot K - 1 is dead (K >= 3), slot 1 finished with a good score
    score[:, 2] = [-0.5 - 0.125 * k for k in range(K)]
    if with_table:
        state[0, 2] = s_eos
    x[0 * B + 2, eos] = 5.0
    if K >= 3:
        fin[K - 1, 2], score[K - 1, 2] = True, NEG
        fin[1, 2] = True
        if with_table:
            state[1, 2] = gram.done
    steps.append(dict(logits=x, state=(score, fin, state)))
    return B, table, start, eos, pad, steps


@pytest.mark.parametrize("with_table", [True, False])
@pytest.mark.parametrize("K", [2, 4])
def test_beam_step_and_backtrack_against_numpy(dev, gram, K, with_table):
    """Tokens, parents, states, finished flags, the re-parented h and q rows and the done counters exact; scores and log-probs within 1e-6
    (absolute): the logits lie in [-2, 5] and every log-probability is below 8 in magnitude, where half an ulp of fp32 is 2.4e-7 -- the bound
    of the grammar op test, with the same room for the rounding of the sum, the logarithm and the subtraction.  A score is a hand-set value
    (or 0) plus one such term."""
    from piano_a2s_amd import hip
    rng = np.random.default_rng(100 * K + int(with_table))
    B, table, start, eos, pad, steps = _op_case(gram, K, with_table, rng)
    R, E, HC, QC, max_steps, ldl = K * B, 5, 70, 33, 4, 181
    g, bt = hip.beam_buffers(B, K, max_steps, V, dev, pad, table=gram.device_table(dev) if with_table else None, start=start, alpha=0.0)
    emb = torch.from_numpy(rng.standard_normal((V, E)).astype(np.float32)).to(dev)
    n_done = torch.tensor([(K - 1) * B], dtype=torch.int32, device=dev)
    steps_exec = torch.zeros(1, dtype=torch.int32, device=dev)
    # the reference state
    score = np.full((K, B), NEG, dtype=np.float32)
    score[0] = 0
    fin = np.ones((K, B), dtype=bool)
    fin[0] = False
    state = np.full((K, B), start, dtype=np.int64)
    hist = []
    worst_lp = worst_sc = 0.0
    seen = set()
    for t, stp in enumerate(steps):
        if stp["state"] is not None:                                   # a state set by hand, on both sides
            score, fin, state = (a.copy() for a in stp["state"])
            bt["score"].copy_(torch.from_numpy(score.reshape(-1)))
            bt["finished"].copy_(torch.from_numpy(fin.reshape(-1).astype(np.int32)))
            bt["row_state"].copy_(torch.from_numpy(state.reshape(-1).astype(np.int32)))
            n_done.fill_(int(fin.sum()))
            bt["done_count"][t] = int(fin.sum())
        x = stp["logits"]
        xd = torch.full((R, ldl), float("nan"), device=dev)
        xd[:, :V] = torch.from_numpy(x).to(dev)
        h0 = rng.standard_normal((R, HC)).astype(np.float32)
        q0 = rng.standard_normal((R, QC)).astype(np.float32)
        h, q = torch.from_numpy(h0).to(dev), torch.from_numpy(q0).to(dev)
        xnext = torch.full((R, E + 3), -7.0, device=dev)
        hip.beam_step(g, xd, emb, xnext, h, q if t == 1 else None, n_done, steps_exec, B, t, max_steps, eos, V=V)
        torch.cuda.synchronize()
        lp64 = _log_softmax64(x)
        lp = lp64.astype(np.float32).reshape(K, B, V)
        new = [np.zeros((K, B), dtype=np.int64) for _ in range(5)]
        new[2] = np.zeros((K, B), dtype=np.float32)
        for b in range(B):
            out = _select_np(score[:, b], fin[:, b], state[:, b], lp[:, b], table, K, pad, eos)
            assert out[5] >= 1e-4, f"launch {t} clip {b}: candidates {out[5]:.2e} apart -- the planted cases must be exact ties or well separated"
            for dst, src in zip(new, out[:5]):
                dst[:, b] = src
        tok, par, sc, st, fn = new
        got = {k: bt[k].cpu().numpy() for k in ("token_hist", "parent_hist", "score_hist", "score", "finished", "row_state", "probs_scratch", "done_count")}
        assert np.array_equal(got["token_hist"][t], tok.reshape(-1)), (t, got["token_hist"][t], tok.reshape(-1))
        assert np.array_equal(got["parent_hist"][t], par.reshape(-1)), (t, got["parent_hist"][t], par.reshape(-1))
        assert np.array_equal(got["finished"], fn.reshape(-1)) and np.array_equal(got["row_state"], st.reshape(-1))
        assert np.array_equal(np.isinf(got["score"]), np.isinf(sc.reshape(-1))) and np.array_equal(got["score"], got["score_hist"][t])
        live = np.isfinite(sc.reshape(-1))
        worst_sc = max(worst_sc, float(np.abs(got["score"][live] - sc.reshape(-1)[live].astype(np.float64)).max()))
        worst_lp = max(worst_lp, float(np.abs(got["probs_scratch"][:, t] - lp64).max()))
        assert (got["probs_scratch"][:, t + 1:] == 0).all(), "steps that have not run stay zero"
        # the recurrent state rows, permuted in place; the query only where one is given
        src_rows = (par * B + np.arange(B)[None, :]).reshape(-1)
        assert np.array_equal(h.cpu().numpy(), h0[src_rows]), f"launch {t}: h rows are not their parents'"
        assert np.array_equal(q.cpu().numpy(), q0[src_rows] if t == 1 else q0), f"launch {t}: q rows"
        xn = xnext.cpu().numpy()
        assert np.array_equal(xn[:, :E], emb.cpu().numpy()[tok.reshape(-1)]) and (xn[:, E:] == -7.0).all()
        # the counters: n_done moves by the CHANGE of every clip's finished count
        assert int(n_done.item()) == int(fn.sum()) and int(got["done_count"][t + 1]) == int(fn.sum()) and int(steps_exec.item()) == t + 1
        for b in range(B):
            p = par[:, b].tolist()
            if len(set(p)) == 1:
                seen.add("shared parent")
            if sorted(p) == list(range(K)) and all(p[j] != j for j in range(K)):
                seen.add("cyclic")
            if fn[:, b].sum() < fin[:, b].sum():
                seen.add("finished dropped")
            if (tok[:, b] == eos).any():
                seen.add("eos")
            if np.isinf(sc[:, b]).any():
                seen.add("dead")
        if t == 0:
            assert tok[:2, 0].tolist() == sorted(tok[:2, 0].tolist()) and sc[0, 0] == sc[1, 0], "the planted tie is resolved by the lowest index"
        hist.append((tok, par))
        score, fin, state = sc, fn.astype(bool), st
    want_seen = {"shared parent", "cyclic", "finished dropped", "eos"}       # (dead slots are in every clip of launch 0 and, K >= 3, in clip 2 of launch 1)
    assert want_seen <= seen, want_seen - seen
    print(f"beam_step K={K} table={with_table}: log-prob max abs error {worst_lp:.3e}, score {worst_sc:.3e}")
    assert worst_lp <= 1e-6 and worst_sc <= 1e-6
    # ---- the pick and the walk back over the two steps, with and without a length penalty
    from tests import beam_oracle
    T = len(steps)
    for alpha in (0.0, 1.5):
        g.alpha = alpha
        probs = torch.full((B, max_steps + 1, V), -3.0, device=dev)[:, :max_steps]            # a strided view, as the engine's
        hip.beam_backtrack(g, probs, steps_exec, B, V, max_steps, eos)
        torch.cuda.synchronize()
        ids, lengths, best = bt["ids_out"].cpu().numpy(), bt["lengths_out"].cpu().numpy(), bt["score_out"].cpu().numpy()
        scratch = bt["probs_scratch"].cpu().numpy()
        for b in range(B):
            walks = [beam_oracle.backtrack([tk[:, b] for tk, _ in hist], [pr[:, b] for _, pr in hist], k, T, eos=eos) for k in range(K)]
            slot, gap = beam_oracle.pick(score[:, b], [w[2] + 1 if w[2] >= 0 else T for w in walks], alpha)
            assert gap >= 1e-4, "fixture: the pick is not a near-tie"
            w_ids, w_rows, e = walks[slot]
            assert ids[b, :T].tolist() == w_ids and (ids[b, T:] == pad).all()
            assert lengths[b] == (e + 1 if e >= 0 else max_steps) and best[b] == bt["score"].cpu().numpy()[slot * B + b]
            for t in range(T):
                assert np.array_equal(probs[b, t].cpu().numpy(), scratch[w_rows[t] * B + b, t])
            assert (probs[b, T:].cpu().numpy() == -3.0).all(), "steps that never ran are not the kernel's"


def test_beam_entry_points_refuse_bad_arguments(dev, gram):
    from piano_a2s_amd import hip
    L = hip.lib()
    B, K, max_steps = 2, 2, 3
    g, bt = hip.beam_buffers(B, K, max_steps, V, dev, gram.pad)
    x, emb = torch.zeros(K * B, V, device=dev), torch.zeros(V, 4, device=dev)
    xnext, h = torch.zeros(K * B, 4, device=dev), torch.zeros(K * B, 8, device=dev)
    n_done, steps_exec = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    before = hip.beam_launches()
    for bad in (0, 5):
        g.K = bad
        with pytest.raises(hip.A2SError):
            hip.beam_step(g, x, emb, xnext, h, None, n_done, steps_exec, B, 0, max_steps, gram.eos)
    g.K = K
    with pytest.raises(hip.A2SError):
        hip.beam_step(g, x, emb, xnext, h, None, n_done, steps_exec, B, max_steps, max_steps, gram.eos)      # a step behind the budget
    with pytest.raises(hip.A2SError):
        hip.beam_step(g, torch.zeros(K * B, 300, device=dev), emb, xnext, h, None, n_done, steps_exec, B, 0, max_steps, gram.eos)      # V > 256
    g.n_states = 3                                                          # states without a table
    with pytest.raises(hip.A2SError):
        hip.beam_step(g, x, emb, xnext, h, None, n_done, steps_exec, B, 0, max_steps, gram.eos)
    g.n_states = 0
    a = hip.NoteDecArgs()
    a.R, a.V, a.n_clips = K * B, V, B
    a.gt = x.data_ptr()                                                     # ground truth given: an argument error, nothing is launched
    assert L.a2s_note_decoder_fwd_beam(hip.stream(), C.byref(a), C.byref(g), None) == -1 and b"greedy" in L.a2s_last_error()
    a.gt = None
    a.R = K * B + 1                                                         # R != K * n_clips
    assert L.a2s_note_decoder_fwd_beam(hip.stream(), C.byref(a), C.byref(g), None) == -1 and b"K * n_clips" in L.a2s_last_error()
    a.R = K * B
    g.K = 5
    assert L.a2s_note_decoder_fwd_beam(hip.stream(), C.byref(a), C.byref(g), None) == -1
    g.K = K
    a.row_until = x.data_ptr()                                              # row bookkeeping
    assert L.a2s_note_decoder_fwd_beam(hip.stream(), C.byref(a), C.byref(g), None) == -1 and b"inference only" in L.a2s_last_error()
    assert L.a2s_note_decoder_fwd_beam(hip.stream(), None, C.byref(g), None) == -1
    assert hip.beam_launches() == before
    from piano_a2s_amd import engine, spec
    eng = engine.Engine(spec.default_cfg(freq_bins=24, conv_feature_size=32, hidden_size=32, max_length=(12, 8)))
    for bad in (0, 5, 2.0, True):
        eng.beam_size = bad
        with pytest.raises(ValueError):
            eng._beam_slots()


# ------------------------------------------------------------------------------------------- the models
@pytest.fixture(scope="module")
def g1(golden_dir):
    from piano_a2s_amd import spec, synthetic
    meta = json.load(open(os.path.join(golden_dir, "g1_small.json")))
    cfg = spec.default_cfg(**meta["cfg"])
    batch = synthetic.make_batch(3, cfg, meta["batch_seed"], **SMALL_BATCH)
    return meta, cfg, batch


def _small_state(cfg, case):
    from piano_a2s_amd import spec
    return spec.procedural_state(cfg, case["weights_seed"], eos_bias=case["eos_bias"], lively=True)


@pytest.fixture(scope="module")
def g2(golden_dir, dev):
    """The set-up of test_full_size_greedy_ids_exact: 16.36 M parameters, 2 clips, 1201 frames."""
    from piano_a2s_amd import spec, synthetic
    meta = json.load(open(os.path.join(golden_dir, "g2_full.json")))
    cfg = spec.default_cfg()
    st = spec.procedural_state(cfg, meta["weights_seed"], eos_bias=meta["eos_bias"], lively=meta["lively"])
    kw = dict(meta["batch_kwargs"])
    kw["upper_range"], kw["lower_range"] = tuple(kw["upper_range"]), tuple(kw["lower_range"])
    batch = synthetic.make_batch(2, cfg, meta["batch_seed"], **kw)
    return meta, cfg, {k: v.to(dev) for k, v in st.items()}, batch[0].to(dev)


def _run(cfg, S, spectrogram, grammar, K=1, alpha=0.0, force=False):
    from piano_a2s_amd import engine
    eng = engine.Engine(cfg)
    eng.kern_grammar, eng.beam_size, eng.beam_length_penalty = grammar, K, alpha
    old = engine._BEAM_FORCE
    engine._BEAM_FORCE = force
    try:
        outs = eng.forward(S, spectrogram, inference=True)
        torch.cuda.synchronize()
    finally:
        engine._BEAM_FORCE = old
    return eng, outs


def _calls(eng):
    return [seg["staff"][k][2] for g in eng.saved["groups"] for seg in g["segments"] for k in ("up", "lo")]


# ------------------------------------------------------------------------------------------- 2. K = 1 forced
def _assert_one_slot_is_constrained_greedy(cfg, S, spectrogram, gram, full):
    from piano_a2s_amd import hip
    L = hip.lib()
    eng0, ref = _run(cfg, S, spectrogram, gram)
    assert eng0.beam_scores is None and all("beam" not in sv for sv in _calls(eng0))
    b0, g0, m0 = hip.beam_launches(), hip.grammar_launches(), L.a2s_debug_get(b"dec_mid_launches")
    eng, outs = _run(cfg, S, spectrogram, gram, K=1, force=True)
    steps = sum(sv["launched"] for sv in _calls(eng))
    assert steps > 0 and hip.beam_launches() - b0 == steps and hip.grammar_launches() == g0, "the beam epilogue, and only it, ran every launched step"
    if full:
        assert L.a2s_debug_get(b"dec_mid_launches") - m0 >= steps, "the mid-size kernels did not run"
    for n, a, b in zip(("ts", "key", "up", "lo"), outs, ref):
        assert torch.equal(a, b), n
    for k in ("up", "lo"):
        assert torch.equal(eng.decoded[k][0], eng0.decoded[k][0]) and torch.equal(eng.decoded[k][1], eng0.decoded[k][1]), k
        assert eng.beam_scores[k].shape == eng.decoded[k][1].shape
    assert [sv["steps"] for sv in _calls(eng)] == [sv["steps"] for sv in _calls(eng0)]


@pytest.mark.parametrize("seed", [11, 18])
def test_one_slot_is_the_constrained_greedy_decoder_small(g1, dev, gram, seed):
    meta, cfg, batch = g1
    S = {k: v.to(dev) for k, v in _small_state(cfg, meta["cases"][f"greedy_s{seed}"]).items()}
    _assert_one_slot_is_constrained_greedy(cfg, S, batch[0].to(dev), gram, full=False)


def test_one_slot_is_the_constrained_greedy_decoder_full(g2, gram):
    meta, cfg, S, spectrogram = g2
    _assert_one_slot_is_constrained_greedy(cfg, S, spectrogram, gram, full=True)


# ------------------------------------------------------------------------------------------- 3. the small model against the beam oracle
# (seed, grammar, K): the seven cases whose oracle margins are at least 1e-3 (seed 11 without a grammar at K = 4 has a step margin of 6.8e-4)
ORACLE_CASES = [(11, True, 2), (11, True, 4), (18, True, 2), (18, True, 4), (11, False, 2), (18, False, 2), (18, False, 4)]


@pytest.mark.parametrize("seed,with_grammar,K", ORACLE_CASES)
def test_small_model_against_beam_oracle(g1, dev, gram, seed, with_grammar, K):
    """CPU-measured margins of the oracle (step margin / final gap): s11 kern K2 1.66e-3 / 3.9e-1, K4 1.40e-2 / 1.0; s18 kern K2 3.56e-3 / 3.0e-2,
    K4 2.30e-3 / 5.0e-2; s11 none K2 2.80e-3 / 1.2e-1; s18 none K2 1.10e-2 / 3.7e-2, K4 2.83e-3 / 3.0e-3."""
    from piano_a2s_amd import spec
    from tests import beam_oracle
    meta, cfg, batch = g1
    state = _small_state(cfg, meta["cases"][f"greedy_s{seed}"])
    P, Bf = spec.split_state(state)
    grammar = gram if with_grammar else None
    ref_outs, ref_dec, ref_scores, margins = beam_oracle.forward(P, Bf, cfg, batch[0], K, grammar)
    print(f"beam s{seed} grammar={with_grammar} K={K}: oracle step margin {margins[0]:.3e}, final gap {margins[1]:.3e}")
    assert margins[0] >= 1e-3 and margins[1] >= 1e-3, "fixture precondition: no near-tie at the edge of the beam nor between the two best hypotheses"
    S = {k: v.to(dev) for k, v in state.items()}
    eng, outs = _run(cfg, S, batch[0].to(dev), grammar, K=K)
    assert eng.decoded is not None and eng.beam_scores is not None
    for k in ("up", "lo"):
        ids, lengths = (t.cpu() for t in eng.decoded[k])
        want = ref_dec[k][0]
        assert ids.dtype == torch.int32 and lengths.dtype == torch.int64 and ids.shape == want.shape
        if not torch.equal(ids.long(), want):
            bad = tuple(int(i) for i in (ids.long() != want).nonzero()[0])
            raise AssertionError(f"{k} ids differ first at (clip,bar,step)={bad}: got {int(ids[bad])} ref {int(want[bad])}; {int((ids.long() != want).sum())} of "
                                 f"{want.numel()} differ")
        assert torch.equal(lengths, ref_dec[k][1]), k
        err = float((eng.beam_scores[k].cpu() - ref_scores[k]).abs().max())
        print(f"beam s{seed} grammar={with_grammar} K={K}.{k} scores: {err:.3e}")
        assert eng.beam_scores[k].dtype == torch.float32 and err <= 1e-4, f"{k} scores: {err:.3e}"
        if with_grammar:
            assert all(gram.accepts(row) for row in ids.reshape(-1, ids.shape[-1]).tolist())
    for n, o, r in zip(("ts", "key", "up", "lo"), outs, ref_outs):
        err = float((o.cpu() - r).abs().max()) / max(1.0, float(r.abs().max()))
        print(f"beam s{seed} grammar={with_grammar} K={K}.{n}: {err:.3e}")
        assert err <= TOL, f"{n}: {err:.3e} > {TOL}"
    for o, r in zip(outs[2:], ref_outs[2:]):
        assert torch.equal((o.abs().sum(-1) == 0).cpu(), r.abs().sum(-1) == 0), "rows never decoded stay exactly zero"


# ------------------------------------------------------------------------------------------- 4. full width without an oracle
_FULL = {}


def _full_beam(g2, gram, K):
    """One full-width beam run per K under the kern grammar: computed once, shared, never modified."""
    if K not in _FULL:
        from piano_a2s_amd import hip
        meta, cfg, S, spectrogram = g2
        m0 = hip.lib().a2s_debug_get(b"dec_mid_launches")
        _FULL[K] = _run(cfg, S, spectrogram, gram, K=K)
        assert hip.lib().a2s_debug_get(b"dec_mid_launches") > m0, "the mid-size kernels did not run"
    return _FULL[K]


@pytest.mark.parametrize("K", [3, 4])
def test_full_width_selection_replayed_on_the_host(g2, gram, K):
    """(a) every step's beam recomputed from the run's own log-probabilities, the previous step's scores, flags and states: token, parent and
    score bit for bit (a candidate score is ONE fp32 add of two values read back).  (b) every row is accepted by the grammar.  (d) a score is
    the sum of the returned log-probabilities at its tokens."""
    eng, outs = _full_beam(g2, gram, K)
    n_eos = 0
    for sv in _calls(eng):
        bt = {k: v.cpu().numpy() for k, v in sv["beam"].items() if k != "table"}
        R = bt["score"].shape[0]
        B = R // K
        T = sv["steps"]
        assert T >= 1 and sv["beam_size"] == K
        score = np.full((K, B), NEG, dtype=np.float32)
        score[0] = 0
        fin = np.ones((K, B), dtype=bool)
        fin[0] = False
        state = np.full((K, B), gram.start, dtype=np.int64)
        assert bt["done_count"][0] == (K - 1) * B
        for t in range(T):
            lp = bt["probs_scratch"][:, t].reshape(K, B, V)
            new = [np.zeros((K, B), dtype=np.int64) for _ in range(5)]
            new[2] = np.zeros((K, B), dtype=np.float32)
            for b in range(B):
                out = _select_np(score[:, b], fin[:, b], state[:, b], lp[:, b], gram.table, K, gram.pad, gram.eos)
                for dst, src in zip(new, out[:5]):
                    dst[:, b] = src
            tok, par, sc, st, fn = new
            assert np.array_equal(bt["token_hist"][t], tok.reshape(-1)) and np.array_equal(bt["parent_hist"][t], par.reshape(-1)), (sv["prefix"], t)
            assert np.array_equal(bt["score_hist"][t].view(np.int32), sc.reshape(-1).view(np.int32)), (sv["prefix"], t, "scores bit for bit")
            assert bt["done_count"][t + 1] == fn.sum()
            score, fin, state = sc, fn.astype(bool), st
        assert np.array_equal(bt["score"].view(np.int32), score.reshape(-1).view(np.int32)) and np.array_equal(bt["finished"], fin.reshape(-1))
        assert np.array_equal(bt["row_state"], state.reshape(-1)) and int(sv["n_done"].item()) == int(fin.sum())
        assert (bt["probs_scratch"][:, T:] == 0).all()
    for k, o in (("up", outs[2]), ("lo", outs[3])):
        ids, lengths = (t.cpu().numpy() for t in eng.decoded[k])
        logp, scores = o.cpu().numpy(), eng.beam_scores[k].cpu().numpy()
        for b in range(ids.shape[0]):
            for bar in range(ids.shape[1]):
                row = ids[b, bar].tolist()
                assert gram.accepts(row), (k, b, bar, gram.first_violation(row))                          # (b)
                n_exec = int((np.abs(logp[b, bar]).sum(-1) > 0).sum())
                assert all(tok == gram.pad for tok in row[n_exec:])
                if gram.eos in row:
                    n_eos += 1
                    assert lengths[b, bar] == row.index(gram.eos) + 1
                else:
                    assert lengths[b, bar] == len(row) == n_exec
                want = sum(float(logp[b, bar, t, row[t]]) for t in range(int(lengths[b, bar])))         # (d)
                assert abs(float(scores[b, bar]) - want) <= 1e-4, (k, b, bar, float(scores[b, bar]), want)
    assert n_eos > 0


@pytest.mark.parametrize("K", [3, 4])
def test_full_width_replay_through_the_teacher_forced_path(g2, gram, K):
    """(c) the beam run's own ids as ground truth of the eval-mode teacher-forced path reproduce its log-probabilities below every length: attention
    over shared rows, GRU, output and the re-parenting of h and q on the mid-size kernels against an already-tested path."""
    from piano_a2s_amd import engine
    eng, outs = _full_beam(g2, gram, K)
    meta, cfg, S, spectrogram = g2
    gt = [outs[0].argmax(-1), outs[1].argmax(-1), eng.decoded["up"][0].long(), eng.decoded["up"][1].clone(), eng.decoded["lo"][0].long(),
          eng.decoded["lo"][1].clone()]
    eng_tf = engine.Engine(cfg)
    replay = eng_tf.forward(S, spectrogram, inference=False, ground_truth=gt, teacher_forcing_ratio=1.0, training=False)
    torch.cuda.synchronize()
    for n, a, b in zip(("ts", "key"), outs[:2], replay[:2]):
        err = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
        print(f"replay K={K} {n}: {err:.3e}")
        assert err <= TOL, f"{n}: {err:.3e} > {TOL}"
    for n, a, b, lengths in (("up", outs[2], replay[2], eng.decoded["up"][1]), ("lo", outs[3], replay[3], eng.decoded["lo"][1])):
        below = torch.arange(a.shape[2], device=a.device)[None, None, :] < lengths[:, :, None]
        assert bool(below.any())
        err = float((a - b)[below].abs().max()) / max(1.0, float(b[below].abs().max()))
        print(f"replay K={K} {n}: {err:.3e} over {int(below.sum())} positions")
        assert err <= TOL, f"{n}: {err:.3e} > {TOL}"


# ------------------------------------------------------------------------------------------- 5. the recipe
def _pretrain(tmp_path, name, extra):
    import pretrain
    ws = os.path.join(str(tmp_path), name)
    os.makedirs(ws)
    args = [os.path.join(ROOT, "hparams", "pretrain.yaml"), "--device=cuda:0", f"--workspace={ws}", "--soundfont_folder=/none",
            "--synthetic_clips=8", "--hidden_size=32", "--conv_feature_size=32", "--bins_per_octave=24", "--n_octaves=1", "--max_length=(12, 8)",
            "--synthetic_frames=41", "--synthetic_lengths=[[3, 10], [2, 7]]", "--batch_size=4", "--number_of_epochs=1", "--seed=1234"] + extra
    brain = pretrain.main(args)
    res = os.path.join(ws, "1234", "pretrain.epr", "results", "test")
    bars = [bar for f in sorted(os.listdir(res)) for rec in json.load(open(os.path.join(res, f)))["pred"] for bar in rec[2:4]]
    return brain, bars


def test_recipe_with_beam_size(tmp_path, dev, gram):
    from piano_a2s_amd import hip
    b0 = hip.beam_launches()
    brain, bars = _pretrain(tmp_path, "beam", ["--beam_size=2", "--constrained_decoding=true"])
    model = brain.modules.transcription
    assert hip.beam_launches() > b0 and model.beam_size == 2 and model.last_decoded is not None and model.last_beam_scores is not None
    assert bars and all(gram.accepts(bar) for bar in bars), [gram.first_violation(bar) for bar in bars]
    # --beam_size=1 is the run without the flag.  Two training runs do not end in the same weights bit for bit (the training step is deterministic only
    # up to the order of a few float atomics, tests/test_gpu_recipe.py, and the synthetic one-epoch model sits on near-ties), so the flag is taken
    # away from the SAME trained recipe and its TEST stage run again: the recorded predictions must not move
    b1 = hip.beam_launches()
    brain, bars_one = _pretrain(tmp_path, "one", ["--beam_size=1"])
    model = brain.modules.transcription
    assert hip.beam_launches() == b1 and model.beam_size == 1 and model.last_beam_scores is None and model.last_decoded is None
    with_flag = (dict(brain.upper_pred), dict(brain.lower_pred), dict(brain.key_pred), dict(brain.time_sig_pred))
    assert with_flag[0] and brain.hparams.beam_size == 1
    delattr(brain.hparams, "beam_size")
    from datasets.syn import SyntheticClips
    test_set = SyntheticClips(model.cfg, 1, seed=1234 + 20_000, frames=41, upper_range=(3, 10), lower_range=(2, 7))
    brain.evaluate(test_set, test_loader_kwargs=brain.hparams.test_dataloader_opts, min_key="WER")
    assert (brain.upper_pred, brain.lower_pred, brain.key_pred, brain.time_sig_pred) == with_flag and hip.beam_launches() == b1
