"""Grammar-constrained greedy decoding on the MI355X (csrc/a2s_grammar.hip, Engine.kern_grammar, --constrained_decoding):

1. the op a2s_grammar_argmax_rows against numpy;
2. the small model against the constrained CPU oracle (tests/constrained_oracle.py): emitted ids and lengths exact, log-probs within TOL;
3. with the permissive table the constrained entry point IS the launch-per-step greedy decoder, bit for bit (small and full width);
4. full width with the real grammar: every row accepted; every emitted token is the best legal one by the run's own log-probs; the run
   replayed through the teacher-forced eval path gives the same log-probs; graph replay equals eager;
5. the recipe with and without --constrained_decoding=true."""
import contextlib
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


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gram():
    from piano_a2s_amd.kern_grammar import KernGrammar
    return KernGrammar()


@contextlib.contextmanager
def launch_per_step():
    """The unconstrained decoder forced onto the launch-per-step loop (no persistent launch, no few-row kernels), as the `decoder_path` fixture does."""
    from piano_a2s_amd import hip
    L = hip.lib()
    for key, env in ((b"dec_persist", "A2S_DEC_PERSIST"), (b"dec_fused", "A2S_DEC_FUSED")):
        os.environ[env] = "0"
        hip.check(L.a2s_debug_set(key, 0), "a2s_debug_set")
    try:
        yield
    finally:
        for key, env in ((b"dec_persist", "A2S_DEC_PERSIST"), (b"dec_fused", "A2S_DEC_FUSED")):
            os.environ[env] = "1"
            hip.check(L.a2s_debug_set(key, 1), "a2s_debug_set")


# ------------------------------------------------------------------------------------------- 1. the op
def _op_batches(gram):
    """Batches of R = 7 rows (a partial workgroup of four-row workgroups; the last one holds three waves): logits in [-1, 1], every row with an
    ILLEGAL token (<sos>) on top at 1.5, some rows with an exact tie of three legal tokens at 1.25 (first, middle and last legal id: different
    lanes and different registers of a lane).  Every automaton state occurs, DONE several times."""
    rng = np.random.default_rng(5)
    sos = gram.classes.index("SOS")
    states = [[0, 1, 2, 3, 4, 5, 6], [7, 8, 9, 9, 5, 0, 9], [4, 4, 3, 8, 9, 1, 7]]
    tie_rows = [{1, 4, 6}, {0, 1, 3, 5}, {0, 2, 6}]
    out = []
    for st, ties in zip(states, tie_rows):
        x = rng.uniform(-1.0, 1.0, (7, V)).astype(np.float32)
        x[:, sos] = 1.5
        for r in ties:
            legal = np.nonzero(gram.table[st[r]] >= 0)[0]
            x[r, [legal[0], legal[len(legal) // 2], legal[-1]]] = 1.25
        out.append((np.array(st, dtype=np.int32), x))
    return out


@pytest.mark.parametrize("with_y", [True, False])
def test_grammar_argmax_rows_against_numpy(dev, gram, with_y):
    """Choices and new states exact; y = log_softmax within 1e-6 (absolute).  The logits are kept in [-1, 1.5] so that every log-probability is
    below 8 in magnitude, where half an ulp of fp32 is 2.4e-7: the tolerance leaves room for the rounding of the sum, the logarithm and the
    subtraction."""
    from piano_a2s_amd import hip
    table = gram.device_table(dev)
    ldx, ldy = 192, 181
    seen, worst = set(), 0.0
    for st, x in _op_batches(gram):
        seen.update(st.tolist())
        xd = torch.full((7, ldx), float("nan"), device=dev)
        xd[:, :V] = torch.from_numpy(x).to(dev)
        state = torch.from_numpy(st).to(dev)
        y = torch.full((7, ldy), -7.0, device=dev) if with_y else None
        choice = hip.grammar_argmax_rows(xd, table, state, y=y)
        torch.cuda.synchronize()
        masked = np.where(gram.table[st] >= 0, x, -np.inf)
        want = masked.argmax(axis=1)                                       # (first occurrence: the lowest index on ties)
        assert (x.argmax(axis=1) != want).all(), "every row's unconstrained maximum is illegal"
        assert np.array_equal(choice.cpu().numpy(), want), (st, choice.cpu().numpy(), want)
        assert np.array_equal(state.cpu().numpy(), gram.table[st, want].astype(np.int32))
        done = st == gram.done
        assert (want[done] == gram.pad).all() and (state.cpu().numpy()[done] == gram.done).all()
        if with_y:
            x64 = x.astype(np.float64)
            ref = x64 - x64.max(1, keepdims=True) - np.log(np.exp(x64 - x64.max(1, keepdims=True)).sum(1, keepdims=True))
            got = y.cpu().numpy()
            worst = max(worst, float(np.abs(got[:, :V] - ref).max()))
            assert (got[:, V:] == -7.0).all(), "columns behind V are not the kernel's"
    assert seen == set(range(gram.n_states))
    print(f"grammar_argmax_rows: log_softmax max abs error {worst:.3e}")
    assert worst <= 1e-6


def test_grammar_entry_points_refuse_bad_arguments(dev, gram):
    from piano_a2s_amd import hip
    L = hip.lib()
    table = gram.device_table(dev)
    x, st = torch.zeros(2, V, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    with pytest.raises(hip.A2SError):
        hip.grammar_argmax_rows(torch.zeros(2, 300, device=dev), torch.zeros(1, 300, dtype=torch.int8, device=dev), st)     # V > 256
    import ctypes as C
    assert L.a2s_grammar_argmax_rows(hip.stream(), hip._p(x), C.c_long(V), None, C.c_long(0), hip._p(table), 0, hip._p(st), None, 2, V) != 0       # no state
    a = hip.NoteDecArgs()
    a.gt = x.data_ptr()                                                     # ground truth given: an argument error, nothing is launched
    a.R, a.V = 2, V
    before = hip.grammar_launches()
    assert L.a2s_note_decoder_fwd_grammar(hip.stream(), C.byref(a), hip._p(table), gram.n_states, hip._p(st), None) == -1
    assert b"greedy" in L.a2s_last_error() and hip.grammar_launches() == before


# ------------------------------------------------------------------------------------------- 2. / 3. / 4d. the small model
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


_ORACLE = {}


def _oracle(g1, gram, seed):
    """The constrained CPU oracle of one case: computed once, shared, never modified."""
    if seed not in _ORACLE:
        from piano_a2s_amd import spec
        from tests import constrained_oracle
        meta, cfg, batch = g1
        P, B = spec.split_state(_small_state(cfg, meta["cases"][f"greedy_s{seed}"]))
        _ORACLE[seed] = constrained_oracle.forward(P, B, cfg, batch[0], constrained_oracle.GrammarChoice(gram))
    return _ORACLE[seed]


def _run(cfg, S, spectrogram, grammar, graph=False):
    from piano_a2s_amd import engine
    eng = engine.Engine(cfg)
    eng.kern_grammar = grammar
    eng.greedy_graph = graph
    outs = eng.forward(S, spectrogram, inference=True)
    torch.cuda.synchronize()
    return eng, outs


def _calls(eng):
    return [seg["staff"][k][2] for g in eng.saved["groups"] for seg in g["segments"] for k in ("up", "lo")]


@pytest.mark.parametrize("seed", [11, 18])
def test_small_model_against_constrained_oracle(g1, dev, gram, seed):
    """CPU-measured smallest top-2 gap among legal tokens: 3.67e-2 (greedy_s11), 1.26e-3 (greedy_s18)."""
    meta, cfg, batch = g1
    ref_outs, ref_dec, gaps = _oracle(g1, gram, seed)
    min_gap = min(float(g.min()) for g in gaps.values())
    print(f"greedy_s{seed}: smallest legal top-2 gap of the oracle {min_gap:.3e}")
    assert min_gap >= 1e-3, "fixture precondition: no near-tie among the legal candidates"
    S = {k: v.to(dev) for k, v in _small_state(cfg, meta["cases"][f"greedy_s{seed}"]).items()}
    eng, outs = _run(cfg, S, batch[0].to(dev), gram)
    assert eng.decoded is not None
    for k in ("up", "lo"):
        ids, lengths = (t.cpu() for t in eng.decoded[k])
        assert ids.dtype == torch.int32 and lengths.dtype == torch.int64 and ids.shape == ref_dec[k][0].shape and lengths.shape == ref_dec[k][1].shape
        want = ref_dec[k][0]
        if not torch.equal(ids.long(), want):
            bad = tuple(int(i) for i in (ids.long() != want).nonzero()[0])
            raise AssertionError(f"{k} ids differ first at (clip,bar,step)={bad}: got {int(ids[bad])} ref {int(want[bad])}; the oracle's legal top-2 gap "
                                 f"there = {float(gaps[k][bad]):.3e}; {int((ids.long() != want).sum())} of {want.numel()} differ")
        assert torch.equal(lengths, ref_dec[k][1]), k
    for n, o, r in zip(("ts", "key", "up", "lo"), outs, ref_outs):
        err = float((o.cpu() - r).abs().max()) / max(1.0, float(r.abs().max()))
        print(f"greedy_s{seed}.{n}: {err:.3e}")
        assert err <= TOL, f"{n}: {err:.3e} > {TOL}"
    for o, r in zip(outs[2:], ref_outs[2:]):
        assert torch.equal((o.abs().sum(-1) == 0).cpu(), r.abs().sum(-1) == 0), "rows never decoded stay exactly zero"


def _assert_permissive_equals_stepwise(cfg, S, spectrogram, full):
    from piano_a2s_amd import hip
    from piano_a2s_amd.kern_grammar import KernGrammar
    L = hip.lib()
    with launch_per_step():
        eng0, ref = _run(cfg, S, spectrogram, None)
        assert eng0.decoded is None and all(sv.get("persist_ws") is None for sv in _calls(eng0))
    g0, m0 = hip.grammar_launches(), L.a2s_debug_get(b"dec_mid_launches")
    eng, outs = _run(cfg, S, spectrogram, KernGrammar.permissive(V))
    steps = sum(sv["launched"] for sv in _calls(eng))
    assert steps > 0 and hip.grammar_launches() - g0 == steps, f"{hip.grammar_launches() - g0} grammar epilogues for {steps} launched steps"
    if full:
        assert L.a2s_debug_get(b"dec_mid_launches") - m0 >= steps, "the mid-size kernels did not run"
    for n, a, b in zip(("ts", "key", "up", "lo"), outs, ref):
        assert torch.equal(a, b), n
    assert [sv["steps"] for sv in _calls(eng)] == [sv["steps"] for sv in _calls(eng0)]
    for k, o in (("up", outs[2]), ("lo", outs[3])):
        ran = o.abs().sum(-1) > 0
        assert torch.equal(eng.decoded[k][0][ran].long(), o.argmax(-1)[ran]), k
        for seg0, seg in zip(eng0.saved["segments"], eng.saved["segments"]):
            assert torch.equal(seg0["staff"][k][1], seg["staff"][k][1]), "lengths"
    return outs


@pytest.mark.parametrize("seed", [11, 18])
def test_permissive_table_is_the_stepwise_decoder_small(g1, dev, seed):
    meta, cfg, batch = g1
    S = {k: v.to(dev) for k, v in _small_state(cfg, meta["cases"][f"greedy_s{seed}"]).items()}
    _assert_permissive_equals_stepwise(cfg, S, batch[0].to(dev), full=False)


def test_graph_replay_equals_eager(g1, dev, gram):
    meta, cfg, batch = g1
    S = {k: v.to(dev) for k, v in _small_state(cfg, meta["cases"]["greedy_s11"]).items()}
    eng_e, eager = _run(cfg, S, batch[0].to(dev), gram)
    eng_g, graph = _run(cfg, S, batch[0].to(dev), gram, graph=True)
    for a, b in zip(eager, graph):
        assert torch.equal(a, b)
    for k in ("up", "lo"):
        assert torch.equal(eng_e.decoded[k][0], eng_g.decoded[k][0]) and torch.equal(eng_e.decoded[k][1], eng_g.decoded[k][1])
    assert [sv["steps"] for sv in _calls(eng_e)] == [sv["steps"] for sv in _calls(eng_g)]


# ------------------------------------------------------------------------------------------- 3. / 4. full width
@pytest.fixture(scope="module")
def g2(golden_dir, dev):
    """The set-up of test_full_size_greedy_ids_exact: 16.36 M parameters, 2 clips, 1201 frames."""
    from piano_a2s_amd import spec, synthetic
    data = np.load(os.path.join(golden_dir, "g2_full.npz"))
    meta = json.load(open(os.path.join(golden_dir, "g2_full.json")))
    cfg = spec.default_cfg()
    st = spec.procedural_state(cfg, meta["weights_seed"], eos_bias=meta["eos_bias"], lively=meta["lively"])
    kw = dict(meta["batch_kwargs"])
    kw["upper_range"], kw["lower_range"] = tuple(kw["upper_range"]), tuple(kw["lower_range"])
    batch = synthetic.make_batch(2, cfg, meta["batch_seed"], **kw)
    return data, meta, cfg, {k: v.to(dev) for k, v in st.items()}, batch[0].to(dev)


def test_permissive_table_is_the_stepwise_decoder_full(g2):
    data, meta, cfg, S, spectrogram = g2
    assert min(meta["min_margin"].values()) >= 1e-3, "fixture precondition: no near-tie argmax"
    outs = _assert_permissive_equals_stepwise(cfg, S, spectrogram, full=True)
    for nm, t in (("up", outs[2]), ("lo", outs[3])):
        assert np.array_equal(t.argmax(-1).cpu().numpy(), data[f"greedy.{nm}_ids"]), f"{nm} ids differ from the reference's"


@pytest.fixture(scope="module")
def full_constrained(g2, gram):
    data, meta, cfg, S, spectrogram = g2
    from piano_a2s_amd import hip
    m0 = hip.lib().a2s_debug_get(b"dec_mid_launches")
    eng, outs = _run(cfg, S, spectrogram, gram)
    assert hip.lib().a2s_debug_get(b"dec_mid_launches") > m0
    return eng, outs


def test_full_width_rows_are_accepted_and_best_legal(full_constrained, gram):
    eng, outs = full_constrained
    eos, pad = gram.eos, gram.pad
    n_eos = 0
    for k, o in (("up", outs[2]), ("lo", outs[3])):
        ids, lengths = (t.cpu().numpy() for t in eng.decoded[k])
        logp = o.cpu().numpy()
        ran = np.abs(logp).sum(-1) > 0
        for b in range(ids.shape[0]):
            for bar in range(ids.shape[1]):
                row, lp = ids[b, bar].tolist(), logp[b, bar]
                assert gram.accepts(row), (k, b, bar, gram.first_violation(row))                       # (a)
                n_exec = int(ran[b, bar].sum())
                assert ran[b, bar, :n_exec].all() and n_exec >= 1
                state = gram.start
                for t in range(n_exec):                                                                  # (b)
                    legal = gram.table[state] >= 0
                    assert legal[row[t]] and lp[t, row[t]] == lp[t][legal].max(), (k, b, bar, t)
                    state = gram.step(state, row[t])
                assert all(tok == pad for tok in row[n_exec:])
                if eos in row:
                    n_eos += 1
                    first = row.index(eos)
                    assert lengths[b, bar] == first + 1 and all(tok == pad for tok in row[first + 1:])
                else:
                    assert lengths[b, bar] == len(row) == n_exec
    assert n_eos > 0


def test_full_width_replay_through_the_teacher_forced_path(full_constrained, g2):
    """The constrained run's own ids as ground truth of the eval-mode teacher-forced path: the same log-probs, the same step counts."""
    from piano_a2s_amd import engine
    eng, outs = full_constrained
    data, meta, cfg, S, spectrogram = g2
    gt = [outs[0].argmax(-1), outs[1].argmax(-1), eng.decoded["up"][0].long(), eng.decoded["up"][1].clone(), eng.decoded["lo"][0].long(),
          eng.decoded["lo"][1].clone()]
    eng_tf = engine.Engine(cfg)
    replay = eng_tf.forward(S, spectrogram, inference=False, ground_truth=gt, teacher_forcing_ratio=1.0, training=False)
    torch.cuda.synchronize()
    assert eng_tf.decoded is None
    for n, a, b in zip(("ts", "key", "up", "lo"), outs, replay):
        err = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
        print(f"replay {n}: {err:.3e}")
        assert err <= TOL, f"{n}: {err:.3e} > {TOL}"
    assert [sv["steps"] for sv in _calls(eng)] == [sv["steps"] for sv in _calls(eng_tf)]


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


def test_recipe_with_and_without_constrained_decoding(tmp_path, dev, gram):
    brain, bars = _pretrain(tmp_path, "on", ["--constrained_decoding=true"])
    assert bars and all(gram.accepts(bar) for bar in bars), [gram.first_violation(bar) for bar in bars]
    assert brain.modules.transcription.constrained_decoding and brain.modules.transcription.last_decoded is not None
    brain, bars = _pretrain(tmp_path, "off", [])
    illegal = sum(1 for bar in bars if not gram.accepts(bar))
    print(f"unconstrained recipe run: {illegal} of {len(bars)} recorded bars are ill-formed")
    assert illegal >= 1, "the unconstrained run wrote no ill-formed bar: the option shows nothing at this seed"
    assert not brain.modules.transcription.constrained_decoding and brain.modules.transcription.last_decoded is None
