"""Metre-aware constrained decoding on the MI355X (csrc/a2s_grammar.hip: metre_argmax_rows / metre_step_finalize, Engine.kern_metre,
--metrical_decoding):

1. the op a2s_metre_argmax_rows against numpy and the host definition KernMetre.step, on states that reach every rule;
2. scripted bars through the op, the state kept on the device: the emitted sequence is the bar, <eos> exactly at its end;
3. with every L = 0 the metre entry point IS a2s_note_decoder_fwd_grammar (torch.equal);
4. the small model against the metrical CPU oracle (tests/metre_oracle.py): ids and lengths exact, log-probs within TOL; graph replay equals eager;
5. full width: every row accepted under the run's own time signatures, every emitted token the best legal one by the run's own log-probs;
6. argument errors;
7. the recipe with and without --metrical_decoding=true."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # as tests/test_gpu_kern_grammar.py: relative to max(1, |ref|max)
SMALL_BATCH = dict(frames=41, upper_range=(3, 10), lower_range=(2, 7), full_tail=0.1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 173
TWO_SPINES = "4c\t8e 8g\n.\t8a\n4r\t4r\n2d\t2d"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def metre():
    from piano_a2s_amd.kern_grammar import KernMetre
    return KernMetre()


@pytest.fixture(scope="module")
def lab():
    from data_processing.humdrum import LabelsMultiple
    return LabelsMultiple(extended=True)


def _ids(lab, words):
    names = {"TAB": "\t", "NL": "\n", "SP": "<b>", "EOS": "<eos>"}
    return [lab.labels_map[names.get(w, w)] for w in words.split()]


# ------------------------------------------------------------------------------------------- 1. the op
def _op_states(metre, lab):
    """[(label, MetreState)]: three batches of seven.  Reached by walking the host definition along a prefix, or built by hand (the last ones:
    values no walk produces, which the kernel must clamp as the host does)."""
    from piano_a2s_amd.kern_grammar import MetreState
    durs = [int(v) for v in np.nonzero(metre.dur_ticks)[0]]
    ts_u, a_u = next((ts, a) for ts in range(7) for a in durs for b in durs
                     if 0 <= metre.length(ts) - metre.dur_ticks[a] - metre.dur_ticks[b] and metre.fillable[metre.length(ts) - metre.dur_ticks[a]]
                     and not metre.fillable[metre.length(ts) - metre.dur_ticks[a] - metre.dur_ticks[b]])
    walks = [("start: <eos> legal, `.` not", "", 0),
             ("need_null: spine 0 still sounds", "4 c TAB 8 d NL", 0),
             ("need_note: spine 1 must go on", "4 c TAB 8 d NL . TAB", 0),
             ("over-full: half the bar is gone", "2 c NL", 0),
             ("over-full in 3/8", "8 c NL", 6),
             ("chord member", "4 c SP", 0),
             ("chord member behind a tie", "4. c SP [", 1),
             ("TAB at the last field, m < L", "4 c TAB 4 d NL 4 e TAB 4 f", 0),
             ("line incomplete: only TAB or a chord", "4 c TAB 4 d NL 4 e", 0),
             ("NL, not <eos>: m < L", "4 c", 0),
             ("<eos>, not NL: m == L", "1 c", 0),
             ("<eos> with two spines at L", "1 c TAB 2 d NL . TAB 2 e", 4),
             ("eight spines: no TAB", "4 c TAB " * 7 + "4 c", 0),
             ("DONE", "1 c EOS", 0),
             ("DONE, empty bar", "EOS", 2),
             ("after `.`", "4 c TAB 8 d NL .", 0),
             ("12/8, second line", "2. c NL", 5)]
    out = []
    for label, words, ts in walks:
        st, bad, _ = metre.walk(_ids(lab, words), ts)
        assert bad is None, label
        out.append((label, st))
    st, bad, _ = metre.walk([a_u, lab.labels_map["c"], lab.labels_map["\n"]], ts_u)
    assert bad is None
    out.append(("a duration that leaves an unfillable remainder", st))
    out.append(("unmetred, START", metre.start(L=0)))
    un = metre.start(L=-7)
    un.s, un.t, un.field, un.end = metre.grammar.state_names.index("PITCH"), 5, 3, [9] * 8       # (ints of an unmetred row are never read)
    out.append(("unmetred, PITCH", un))
    hand = MetreState(metre.grammar.state_names.index("FIELD"), metre.length(0))                 # field beyond 7, spine count beyond 8
    hand.t, hand.first_line, hand.n_fields, hand.field, hand.end = 36960, 0, 20, 11, [36960] * 7 + [36960]
    out.append(("clamped field", hand))
    assert len(out) == 21
    return out


def _op_batch(metre, states, rng, tie_rows):
    """logits in [-1, 1]; on top, at 1.5, a token the row may not emit (one the syntax allows and the metre forbids where there is one, else <sos>);
    rows in tie_rows: an exact tie of up to three legal tokens at 1.25 (the first, the middle and the last legal id)."""
    sos = metre.grammar.classes.index("SOS")
    x = rng.uniform(-1.0, 1.0, (len(states), V)).astype(np.float32)
    blocked = []
    for r, (_, st) in enumerate(states):
        legal = metre.legal_tokens(st)
        assert legal
        syntax_only = [v for v in np.nonzero(metre.grammar.table[st.s] >= 0)[0].tolist() if v not in legal]
        top = syntax_only[len(syntax_only) // 2] if syntax_only else sos
        blocked.append(bool(syntax_only))
        x[r, top] = 1.5
        if r in tie_rows:
            x[r, [legal[0], legal[len(legal) // 2], legal[-1]]] = 1.25
    return x, blocked


@pytest.mark.parametrize("with_y", [True, False])
def test_metre_argmax_rows_against_numpy(dev, metre, lab, with_y):
    """Emitted id, next syntax state and all 16 metre ints equal the host's; y = log_softmax within 1e-6 (absolute; logits in [-1, 1.5], as in
    tests/test_gpu_kern_grammar.py: every log-probability is below 8 in magnitude, half an ulp there is 2.4e-7)."""
    from piano_a2s_amd import hip
    table = metre.grammar.device_table(dev)
    states = _op_states(metre, lab)
    rng = np.random.default_rng(7)
    ldx, ldy = 192, 181
    worst, n_blocked, seen = 0.0, 0, set()
    for i, ties in enumerate(({1, 4, 6}, {0, 2, 3, 5}, {0, 2, 6})):
        batch = states[7 * i:7 * i + 7]
        x, blocked = _op_batch(metre, batch, rng, ties)
        n_blocked += sum(blocked)
        xd = torch.full((7, ldx), float("nan"), device=dev)
        xd[:, :V] = torch.from_numpy(x).to(dev)
        state = torch.tensor([st.s for _, st in batch], dtype=torch.int32, device=dev)
        rows = torch.tensor([st.ints() for _, st in batch], dtype=torch.int32, device=dev)
        y = torch.full((7, ldy), -7.0, device=dev) if with_y else None
        choice = hip.metre_argmax_rows(xd, table, state, metre, rows, y=y)
        torch.cuda.synchronize()
        got_id, got_s, got_m = choice.cpu().tolist(), state.cpu().tolist(), rows.cpu().tolist()
        for r, (label, st) in enumerate(batch):
            legal = metre.legal_tokens(st)
            mask = np.full(V, -np.inf, dtype=np.float32)
            mask[legal] = x[r, legal]
            want = int(mask.argmax())                                              # (first occurrence: the lowest index on ties)
            assert int(x[r].argmax()) != want, (label, "the row's unconstrained maximum is illegal")
            nx = metre.step(st, want)
            assert got_id[r] == want, (label, got_id[r], want)
            assert got_s[r] == nx.s and got_m[r] == nx.ints(), (label, got_s[r], nx.s, got_m[r], nx.ints())
            if st.L > 0:
                seen.update(r_ for r_ in (metre.violation(st, v) for v in range(V)) if r_)
        if with_y:
            x64 = x.astype(np.float64)
            ref = x64 - x64.max(1, keepdims=True) - np.log(np.exp(x64 - x64.max(1, keepdims=True)).sum(1, keepdims=True))
            got = y.cpu().numpy()
            worst = max(worst, float(np.abs(got[:, :V] - ref).max()))
            assert (got[:, V:] == -7.0).all(), "columns behind V are not the kernel's"
    from piano_a2s_amd.kern_grammar import METRE_RULES
    assert seen == set(METRE_RULES), f"rules never met: {set(METRE_RULES) - seen}"
    assert n_blocked >= 14, "the token on top is one the metre alone forbids in most rows"
    print(f"metre_argmax_rows: log_softmax max abs error {worst:.3e}")
    assert worst <= 1e-6


# ------------------------------------------------------------------------------------------- 2. scripted bars
def test_scripted_bars_through_the_op(dev, metre, lab):
    """22 bars (three scoregen bars per time signature, one spine each, and the two-spine bar above) as the rows of one batch, one op call per
    step, syntax and metre state kept on the device.  The logits favour the bar's next token (+4 over noise in [-1, 1]) and carry a bonus of +8 on
    <eos>, withheld only where <eos> is legal although the bar goes on (step 0: the empty bar; the later members of a chord that closes the bar):
    the metre alone keeps <eos> away until the bar is full, and then nothing else is favoured."""
    from piano_a2s_amd import hip, scoregen, spec
    cfg = spec.default_cfg()
    eos, pad = metre.grammar.eos, metre.grammar.pad
    bars, ts = [], []
    for sig in range(7):
        found = 0
        for seed in range(40):
            clip = scoregen.make_clip(cfg, 1000 + seed, time_sig=sig)
            row = [int(t) for t in clip["ids"]["upper" if seed % 2 else "lower"][seed % cfg["max_bars"]]]
            if 4 <= len(row) <= 40:
                bars.append(row)
                ts.append(sig)
                found += 1
                if found == 3:
                    break
        assert found == 3
    bars.append(lab.encode(TWO_SPINES))
    ts.append(0)
    R, steps = len(bars), max(len(b) for b in bars) + 3
    assert R == 22 and all(metre.complete(b + [eos], t) for b, t in zip(bars, ts))
    rng = np.random.default_rng(11)
    X = rng.uniform(-1.0, 1.0, (steps, R, V)).astype(np.float32)
    X[:, :, eos] += 8.0
    withheld = 0
    for r, b in enumerate(bars):
        st = metre.start(ts[r])
        for t, tok in enumerate(b):
            X[t, r, tok] += 4.0
            if metre.violation(st, eos) is None:                 # <eos> is legal before the bar's end: the empty bar, a closing chord's later members
                X[t, r, eos] -= 8.0
                withheld += 1
            st = metre.step(st, tok)
    assert R <= withheld <= 3 * R
    Xd = torch.from_numpy(X).to(dev)
    table = metre.grammar.device_table(dev)
    state = torch.full((R,), metre.grammar.start, dtype=torch.int32, device=dev)
    rows = hip.metre_rows(metre, torch.tensor(ts, dtype=torch.int32, device=dev))
    assert rows.cpu().tolist() == [metre.start(t).ints() for t in ts]
    out = torch.stack([hip.metre_argmax_rows(Xd[t], table, state, metre, rows) for t in range(steps)], dim=1).cpu().tolist()
    torch.cuda.synchronize()
    for r, b in enumerate(bars):
        assert out[r][:len(b)] == b, (r, ts[r])
        assert out[r][len(b)] == eos and out[r].count(eos) == 1 and all(t == pad for t in out[r][len(b) + 1:]), (r, out[r][len(b):])
        assert sum(X[t, r].argmax() == eos for t in range(len(b))) >= len(b) // 2, "the bonus did put <eos> on top inside the bar"
    assert state.cpu().tolist() == [metre.grammar.done] * R
    assert rows.cpu().tolist() == [metre.walk(b + [eos], t)[0].ints() for b, t in zip(bars, ts)]


# ------------------------------------------------------------------------------------------- 3. / 4. the small model
@pytest.fixture(scope="module")
def g1(golden_dir):
    meta = json.load(open(os.path.join(golden_dir, "g1_small.json")))
    return meta


def _small(meta, seed, max_length):
    from piano_a2s_amd import spec, synthetic
    cfg = spec.default_cfg(**dict(meta["cfg"], max_length=max_length))
    batch = synthetic.make_batch(3, cfg, meta["batch_seed"], **SMALL_BATCH)
    case = meta["cases"][f"greedy_s{seed}"]
    return cfg, batch, spec.procedural_state(cfg, case["weights_seed"], eos_bias=case["eos_bias"], lively=True)


def _run(cfg, S, spectrogram, gram, metre, graph=False, **attrs):
    from piano_a2s_amd import engine
    eng = engine.Engine(cfg)
    eng.kern_grammar, eng.kern_metre, eng.greedy_graph = gram, metre, graph
    for k, v in attrs.items():
        setattr(eng, k, v)
    outs = eng.forward(S, spectrogram, inference=True)
    torch.cuda.synchronize()
    return eng, outs


def _calls(eng):
    return [seg["staff"][k][2] for g in eng.saved["groups"] for seg in g["segments"] for k in ("up", "lo")]


@pytest.mark.parametrize("seed", [11, 18])
def test_unmetred_rows_equal_the_grammar_entry(g1, dev, metre, seed):
    from piano_a2s_amd import hip
    from piano_a2s_amd.kern_grammar import KernMetre
    cfg, batch, state = _small(g1, seed, tuple(g1["cfg"]["max_length"]))
    assert tuple(cfg["max_length"]) == (12, 8)
    S = {k: v.to(dev) for k, v in state.items()}
    eng0, ref = _run(cfg, S, batch[0].to(dev), metre.grammar, None)
    flat = KernMetre(metre.grammar)
    flat.bar_ticks = np.zeros_like(flat.bar_ticks)                              # every time signature: L = 0
    g0, m0 = hip.grammar_launches(), hip.metre_launches()
    eng, outs = _run(cfg, S, batch[0].to(dev), metre.grammar, flat)
    steps = sum(sv["launched"] for sv in _calls(eng))
    assert steps > 0 and hip.metre_launches() - m0 == steps and hip.grammar_launches() == g0
    for n, a, b in zip(("ts", "key", "up", "lo"), outs, ref):
        assert torch.equal(a, b), n
    for k in ("up", "lo"):
        assert torch.equal(eng.decoded[k][0], eng0.decoded[k][0]) and torch.equal(eng.decoded[k][1], eng0.decoded[k][1]), k
    for sv in _calls(eng):
        assert (sv["row_metre"][:, 0] == 0).all() and (sv["row_metre"][:, 3:] == 0).all(), "an unmetred row's ints are never written"


_ORACLE = {}


def _oracle(meta, metre, seed, max_length):
    """The metrical CPU oracle of one case: computed once, shared, never modified."""
    key = (seed, max_length)
    if key not in _ORACLE:
        from piano_a2s_amd import spec
        from tests import metre_oracle
        cfg, batch, state = _small(meta, seed, max_length)
        P, B = spec.split_state(state)
        _ORACLE[key] = metre_oracle.forward(P, B, cfg, batch[0], metre_oracle.MetreChoice(metre))
    return _ORACLE[key]


@pytest.mark.parametrize("max_length", [(12, 8), (48, 32)])
@pytest.mark.parametrize("seed", [11, 18])
def test_small_model_against_metre_oracle(g1, dev, metre, seed, max_length):
    """CPU-measured with tests/metre_oracle.py, smallest legal top-2 gap / smallest time-signature top-2 gap: (12, 8): 1.37e-2 / 4.56e-1 (greedy_s11),
    1.26e-3 / 7.30e-3 (greedy_s18); (48, 32): printed by this test."""
    cfg, batch, state = _small(g1, seed, max_length)
    ref_outs, ref_dec, gaps = _oracle(g1, metre, seed, max_length)
    min_gap, ts_gap = min(float(gaps[k].min()) for k in ("up", "lo")), float(gaps["ts"].min())
    print(f"greedy_s{seed} {max_length}: oracle's smallest legal top-2 gap {min_gap:.3e}, time-signature top-2 gap {ts_gap:.3e}")
    assert min_gap >= 1e-3 and ts_gap >= 1e-3, "fixture precondition: no near-tie among the legal candidates or the time signatures"
    S = {k: v.to(dev) for k, v in state.items()}
    eng, outs = _run(cfg, S, batch[0].to(dev), metre.grammar, metre)
    assert torch.equal(outs[0].argmax(-1).cpu(), ref_outs[0].argmax(-1)), "time signatures"
    for k in ("up", "lo"):
        ids, lengths = (t.cpu() for t in eng.decoded[k])
        want = ref_dec[k][0]
        assert ids.dtype == torch.int32 and lengths.dtype == torch.int64 and ids.shape == want.shape
        if not torch.equal(ids.long(), want):
            bad = tuple(int(i) for i in (ids.long() != want).nonzero()[0])
            raise AssertionError(f"{k} ids differ first at (clip,bar,step)={bad}: got {int(ids[bad])} ref {int(want[bad])}; the oracle's legal top-2 gap "
                                 f"there = {float(gaps[k][bad]):.3e}; {int((ids.long() != want).sum())} of {want.numel()} differ")
        assert torch.equal(lengths, ref_dec[k][1]), k
    for n, o, r in zip(("ts", "key", "up", "lo"), outs, ref_outs):
        err = float((o.cpu() - r).abs().max()) / max(1.0, float(r.abs().max()))
        print(f"greedy_s{seed} {max_length}.{n}: {err:.3e}")
        assert err <= TOL, f"{n}: {err:.3e} > {TOL}"
    # graph replay equals eager
    eng_g, graph = _run(cfg, S, batch[0].to(dev), metre.grammar, metre, graph=True)
    for a, b in zip(outs, graph):
        assert torch.equal(a, b)
    for k in ("up", "lo"):
        assert torch.equal(eng.decoded[k][0], eng_g.decoded[k][0]) and torch.equal(eng.decoded[k][1], eng_g.decoded[k][1])
    assert [sv["steps"] for sv in _calls(eng)] == [sv["steps"] for sv in _calls(eng_g)]


# ------------------------------------------------------------------------------------------- 5. full width
def test_full_width_rows_are_accepted_and_best_legal(golden_dir, dev, metre):
    from piano_a2s_amd import hip, spec, synthetic
    meta = json.load(open(os.path.join(golden_dir, "g2_full.json")))
    cfg = spec.default_cfg()
    st = spec.procedural_state(cfg, meta["weights_seed"], eos_bias=meta["eos_bias"], lively=meta["lively"])
    kw = dict(meta["batch_kwargs"])
    kw["upper_range"], kw["lower_range"] = tuple(kw["upper_range"]), tuple(kw["lower_range"])
    batch = synthetic.make_batch(2, cfg, meta["batch_seed"], **kw)
    S = {k: v.to(dev) for k, v in st.items()}
    m0, e0 = hip.lib().a2s_debug_get(b"dec_mid_launches"), hip.metre_launches()
    eng, outs = _run(cfg, S, batch[0].to(dev), metre.grammar, metre)
    assert hip.lib().a2s_debug_get(b"dec_mid_launches") > m0 and hip.metre_launches() > e0, "the mid-size kernels and the metre epilogue ran"
    eos, pad = metre.grammar.eos, metre.grammar.pad
    ts_ids = outs[0].argmax(-1).cpu().numpy()
    n_eos = n_steps = n_metre_only = 0
    for k, o in (("up", outs[2]), ("lo", outs[3])):
        ids, lengths = (t.cpu().numpy() for t in eng.decoded[k])
        logp = o.cpu().numpy()
        ran = np.abs(logp).sum(-1) > 0
        for b in range(ids.shape[0]):
            for bar in range(ids.shape[1]):
                row, lp, ts = ids[b, bar].tolist(), logp[b, bar], int(ts_ids[b, bar])
                assert metre.length(ts) > 0
                assert metre.accepts(row, ts), (k, b, bar, metre.first_violation(row, ts))
                n_exec = int(ran[b, bar].sum())
                assert ran[b, bar, :n_exec].all() and n_exec >= 1
                state = metre.start(ts)
                for t in range(n_exec):
                    legal = metre.legal_tokens(state)
                    assert row[t] in legal and lp[t, row[t]] == lp[t][legal].max(), (k, b, bar, t)
                    n_metre_only += lp[t, row[t]] < lp[t][metre.grammar.table[state.s] >= 0].max()
                    state = metre.step(state, row[t])
                n_steps += n_exec
                assert all(tok == pad for tok in row[n_exec:])
                if eos in row:
                    n_eos += 1
                    first = row.index(eos)
                    assert lengths[b, bar] == first + 1 and all(tok == pad for tok in row[first + 1:])
                    assert first == 0 or metre.complete(row, ts)
                else:
                    assert lengths[b, bar] == len(row) == n_exec
    print(f"full width: {n_steps} steps, {n_metre_only} of them chose below the best syntax-legal token, {n_eos} rows reached <eos>")
    assert n_metre_only > 0, "the metre never changed a choice: the test shows nothing beyond the grammar"


# ------------------------------------------------------------------------------------------- 6. argument errors
def test_metre_entry_points_refuse_bad_arguments(g1, dev, metre):
    from piano_a2s_amd import hip
    L = hip.lib()
    table = metre.grammar.device_table(dev)
    x, st = torch.zeros(2, V, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    rows = hip.metre_rows(metre, torch.zeros(2, dtype=torch.int32, device=dev))
    ref = hip.metre_ref(metre, rows)
    before = hip.metre_launches()
    with pytest.raises(hip.A2SError):                                                                       # V > 256
        hip.metre_argmax_rows(torch.zeros(2, 300, device=dev), torch.zeros(1, 300, dtype=torch.int8, device=dev), st, metre, rows)
    args = (hip.stream(), hip._p(x), C.c_long(V), None, C.c_long(0), hip._p(table), metre.grammar.n_states, hip._p(st))
    a = hip.NoteDecArgs()
    a.R, a.V = 2, V
    fwd = lambda a_, m_: L.a2s_note_decoder_fwd_metre(hip.stream(), C.byref(a_), hip._p(table), metre.grammar.n_states, hip._p(st), *m_, None)
    for i in range(5):                                                                                      # a null table, no rows, an empty `fillable`
        broken = list(ref)
        broken[i] = 0 if i == 3 else None
        assert L.a2s_metre_argmax_rows(*args, *broken, None, 2, V) == -1 and b"metre" in L.a2s_last_error(), i
        assert fwd(a, broken) == -1 and b"metre" in L.a2s_last_error(), i
    assert L.a2s_metre_argmax_rows(hip.stream(), hip._p(x), C.c_long(V), None, C.c_long(0), None, metre.grammar.n_states, hip._p(st), *ref, None, 2, V) == -1
    a.gt = x.data_ptr()                                                                                     # ground truth given
    assert fwd(a, ref) == -1 and b"greedy" in L.a2s_last_error()
    a.gt, a.gates = None, x.data_ptr()                                                                      # a training buffer
    assert fwd(a, ref) == -1 and b"inference only" in L.a2s_last_error()
    a.gates = None
    a.V = 300
    assert fwd(a, ref) == -1                                                                                # V > 256
    torch.cuda.synchronize()
    assert hip.metre_launches() == before and rows.cpu().tolist() == [metre.start(0).ints()] * 2
    # the engine: the metre needs the grammar, and neither a beam nor the alignment
    cfg, batch, state = _small(g1, 11, (12, 8))
    S = {k: v.to(dev) for k, v in state.items()}
    for kw, word in ((dict(beam_size=2), "beam"), (dict(alignment=True), "alignment")):
        with pytest.raises(hip.A2SError, match=word):
            _run(cfg, S, batch[0].to(dev), metre.grammar, metre, **kw)
    with pytest.raises(hip.A2SError, match="kern_grammar"):
        _run(cfg, S, batch[0].to(dev), None, metre)
    assert hip.metre_launches() == before


# ------------------------------------------------------------------------------------------- 7. the recipe
def _pretrain(tmp_path, name, extra):
    import pretrain
    ws = os.path.join(str(tmp_path), name)
    os.makedirs(ws)
    args = [os.path.join(ROOT, "hparams", "pretrain.yaml"), "--device=cuda:0", f"--workspace={ws}", "--soundfont_folder=/none",
            "--synthetic_clips=8", "--hidden_size=32", "--conv_feature_size=32", "--bins_per_octave=24", "--n_octaves=1", "--max_length=(12, 8)",
            "--synthetic_frames=41", "--synthetic_lengths=[[3, 10], [2, 7]]", "--batch_size=4", "--number_of_epochs=1", "--seed=1234"] + extra
    brain = pretrain.main(args)
    res = os.path.join(ws, "1234", "pretrain.epr", "results", "test")
    recs = {f: json.load(open(os.path.join(res, f))) for f in sorted(os.listdir(res))}
    return brain, recs


def test_recipe_with_and_without_metrical_decoding(tmp_path, dev, metre):
    from piano_a2s_amd import hip, scoregen
    sigs = scoregen.time_signatures()
    m0 = hip.metre_launches()
    brain, recs = _pretrain(tmp_path, "on", ["--metrical_decoding=true"])
    model = brain.modules.transcription
    assert hip.metre_launches() > m0 and model.metrical_decoding and model.last_decoded is not None
    bars = [(bar, sigs.index(rec[1])) for r in recs.values() for rec in r["pred"] for bar in rec[2:4]]
    assert bars and all(metre.accepts(bar, ts) for bar, ts in bars), [metre.first_violation(bar, ts) for bar, ts in bars]
    assert 0.0 <= brain.last_stats["complete_bars"] <= 1.0
    print(f"metrical recipe run: complete_bars {brain.last_stats['complete_bars']:.3f} over {len(bars)} bars")
    m1 = hip.metre_launches()
    brain_0, recs_0 = _pretrain(tmp_path, "off", ["--metrical_decoding=false"])          # the default decoder, scored the same way
    assert hip.metre_launches() == m1 and not brain_0.modules.transcription.metrical_decoding and brain_0.modules.transcription.last_decoded is None
    assert 0.0 <= brain_0.last_stats["complete_bars"] <= 1.0
    assert set(brain.last_stats) == set(brain_0.last_stats)
    # the default run's records are what they were: the same clips, the same keys
    assert list(recs_0) == list(recs) and all(set(recs_0[f]) == set(recs[f]) == {"pred", "wer_upper", "wer_lower", "key_f1", "time_f1", "style", "soundfont",
                                                                                "composer", "target_path"} for f in recs)
    illegal = sum(1 for r in recs_0.values() for rec in r["pred"] for bar in rec[2:4] if not metre.accepts(bar, sigs.index(rec[1])))
    print(f"default recipe run: {illegal} recorded bars are not legal under their time signature; complete_bars {brain_0.last_stats['complete_bars']:.3f}")
    assert illegal >= 1, "the default run wrote no bar the metre rejects: the option shows nothing at this seed"
