"""Audio alignment from the attention weights on the MI355X (csrc/a2s_align.hip, Engine.alignment, --alignment):

1. the op a2s_attn_align_rows against numpy;
2. alignment does not change decoding: a greedy run with it equals the launch-per-step decoder without it, bit for bit (small and full width), the
   launch counter is the launched steps plus the bar steps, and with the option off a forward launches what it launched before the option existed;
3. the small model against the CPU oracle (tests/align_oracle.py): greedy, greedy under the kern grammar, teacher-forced, K = 2 beam;
4. full width, independent of the new kernel: the weights recomputed with a2s_attn_step_fwd from the call's saved query and key image, reduced in numpy;
5. beam search: the alignment is that of a teacher-forced alignment run over the winners, and the beam's own results are untouched;
6. refusals;
7. the recipe with and without --alignment=true."""
import contextlib
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # as tests/test_gpu_forward.py: max |dev - ref| relative to max(1, |ref|max)
SMALL_BATCH = dict(frames=41, upper_range=(3, 10), lower_range=(2, 7), full_tail=0.1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 173
FIELDS = ("peak", "weight", "centroid")
PREFIX = {"up": "decoder.upper_decoder", "lo": "decoder.lower_decoder"}


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
    """The decoder forced onto the launch-per-step loop (no persistent launch, no few-row kernels): the arrangement of tests/test_gpu_kern_grammar.py."""
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


def _reduce_np(a):
    """Rows of fp32 weights (R, T) -> peak (lowest index of the maximum), the fp32 weight there, the float64 centroid and its summation bound
    (T + 2) * 2^-24 * sum t a[t]: T products-and-adds in any order, each within half an ulp of a partial sum that never exceeds the (non-negative) total."""
    a64 = a.astype(np.float64)
    T = a.shape[1]
    peak = a.argmax(axis=1)
    cen = (a64 * np.arange(T)).sum(axis=1)
    return peak, a[np.arange(a.shape[0]), peak], cen, (T + 2) * 2.0 ** -24 * cen


# ------------------------------------------------------------------------------------------- 1. the op
OP_SHAPES = [(7, 41, 41), (9, 64, 70), (3, 65, 65), (1, 1, 1), (5, 1201, 1216)]


def _op_rows(R, T, seed):
    """Softmax rows of seeded logits; in every second row the maximum is planted EXACTLY at the first, a middle and the last frame (different lanes);
    the last row (of more than one) is all zeros."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 2.0, (R, T)).astype(np.float32)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    a = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    for r in range(0, R, 2):
        a[r, [0, T // 2, T - 1]] = np.float32(2.0) * a[r].max()
    if R > 1:
        a[R - 1] = 0.0
    return a


@pytest.mark.parametrize("R,T,ld", OP_SHAPES)
def test_attn_align_rows_against_numpy(dev, R, T, ld):
    from piano_a2s_amd import hip
    a = _op_rows(R, T, 100 + R + T)
    buf = torch.full((R + 1, ld), 7.0, device=dev)                       # 7: larger than any weight -- a read beyond T or beyond row R - 1 would win the maximum
    buf[:R, :T] = torch.from_numpy(a).to(dev)
    before = buf.clone()
    peak = torch.full((R + 1, 3), -5, dtype=torch.int32, device=dev)
    weight = torch.full((R + 1, 3), -5.0, device=dev)
    cen = torch.full((R + 1, 3), -5.0, device=dev)
    n0 = hip.align_launches()
    hip.attn_align_rows(buf, peak[:, 1], weight[:, 1], cen[:, 1], T=T, R=R)
    torch.cuda.synchronize()
    assert hip.align_launches() == n0 + 1
    want_peak, want_w, want_c, bound = _reduce_np(a)
    got_p, got_w, got_c = peak.cpu().numpy(), weight.cpu().numpy(), cen.cpu().numpy()
    assert np.array_equal(got_p[:R, 1], want_peak), (got_p[:R, 1], want_peak)
    for r in range(0, R, 2):
        assert want_peak[r] == 0, "planted ties: the lowest index wins"
    assert np.array_equal(got_w[:R, 1].view(np.uint32), want_w.view(np.uint32)), "weight is the input at the peak, bit for bit"
    err = np.abs(got_c[:R, 1].astype(np.float64) - want_c)
    print(f"attn_align_rows R={R} T={T}: centroid max error {err.max():.3e}, bound at that row {bound[err.argmax()]:.3e}")
    assert (err <= bound).all(), (err, bound)
    if R > 1:
        assert (got_p[R - 1, 1], got_w[R - 1, 1], got_c[R - 1, 1]) == (0, 0.0, 0.0), "a row of zeros: nothing ran"
    for out in (got_p, got_w, got_c):
        assert (out[:, [0, 2]] == -5).all() and (out[R] == -5).all(), "the other columns and the row behind R are not the kernel's"
    assert torch.equal(buf, before), "the weights, the padding of the row stride and the row behind R are only read"


def test_attn_align_rows_refuses_bad_arguments(dev):
    from piano_a2s_amd import hip
    L = hip.lib()
    a = torch.zeros(4, 8, device=dev)
    p, w, c = torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4, device=dev), torch.zeros(4, device=dev)
    n0, k0 = hip.align_launches(), L.a2s_launch_count()
    st = hip.stream()
    ok = (hip._p(a), C.c_long(8), 4, 8, hip._p(p), hip._p(w), hip._p(c), C.c_long(1))
    for i, bad in ((0, None), (4, None), (5, None), (6, None), (2, -1), (3, 0), (1, C.c_long(7)), (7, C.c_long(0))):
        args = list(ok)
        args[i] = bad
        assert L.a2s_attn_align_rows(st, *args) == -1, i
        assert b"attn_align_rows" in L.a2s_last_error()
    args = list(ok)
    args[2] = 0                                                            # no rows: fine, and nothing to launch
    assert L.a2s_attn_align_rows(st, *args) == 0
    assert hip.align_launches() == n0 and L.a2s_launch_count() == k0, "nothing was launched"
    with pytest.raises(hip.A2SError):
        hip.attn_align_rows(a, p.float(), w, c)


# ------------------------------------------------------------------------------------------- fixtures of the model tests
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
    data = np.load(os.path.join(golden_dir, "g2_full.npz"))
    meta = json.load(open(os.path.join(golden_dir, "g2_full.json")))
    cfg = spec.default_cfg()
    st = spec.procedural_state(cfg, meta["weights_seed"], eos_bias=meta["eos_bias"], lively=meta["lively"])
    kw = dict(meta["batch_kwargs"])
    kw["upper_range"], kw["lower_range"] = tuple(kw["upper_range"]), tuple(kw["lower_range"])
    batch = synthetic.make_batch(2, cfg, meta["batch_seed"], **kw)
    return data, meta, cfg, {k: v.to(dev) for k, v in st.items()}, batch[0].to(dev)


def _run(cfg, S, spectrogram, align, grammar=None, K=1, gt=None):
    """align None: the attribute is never touched."""
    from piano_a2s_amd import engine
    eng = engine.Engine(cfg)
    if align is not None:
        eng.alignment = align
    eng.kern_grammar, eng.beam_size = grammar, K
    if gt is None:
        outs = eng.forward(S, spectrogram, inference=True)
    else:
        outs = eng.forward(S, spectrogram, inference=False, ground_truth=gt, teacher_forcing_ratio=1.0, training=False)
    torch.cuda.synchronize()
    return eng, outs


def _calls(eng):
    return [seg["staff"][k][2] for g in eng.saved["groups"] for seg in g["segments"] for k in ("up", "lo")]


def _shapes_ok(eng, cfg, B):
    al = eng.alignment_out
    U, Lo = cfg["max_length"]
    for k, shape in (("bar", (B, cfg["max_bars"])), ("up", (B, cfg["max_bars"], U)), ("lo", (B, cfg["max_bars"], Lo))):
        assert set(al[k]) == set(FIELDS)
        assert al[k]["peak"].dtype == torch.int32 and al[k]["weight"].dtype == torch.float32 and al[k]["centroid"].dtype == torch.float32
        assert all(tuple(al[k][f].shape) == shape for f in FIELDS), k


# ------------------------------------------------------------------------------------------- 2. alignment does not change decoding
def _assert_alignment_keeps_decoding(cfg, S, spectrogram, full):
    from piano_a2s_amd import hip
    L = hip.lib()
    with launch_per_step():
        eng0, ref = _run(cfg, S, spectrogram, False)
        assert eng0.alignment_out is None and all(sv.get("persist_ws") is None and "align" not in sv for sv in _calls(eng0))
    a0, m0 = hip.align_launches(), L.a2s_debug_get(b"dec_mid_launches")
    eng, outs = _run(cfg, S, spectrogram, True)
    steps = sum(sv["launched"] for sv in _calls(eng))
    got = hip.align_launches() - a0
    assert steps > 0 and got == steps + cfg["max_bars"], f"{got} alignment launches for {steps} launched steps and {cfg['max_bars']} bar steps"
    if full:
        assert L.a2s_debug_get(b"dec_mid_launches") - m0 >= steps, "the mid-size kernels did not run"
    for n, a, b in zip(("ts", "key", "up", "lo"), outs, ref):
        assert torch.equal(a, b), n
    assert [sv["steps"] for sv in _calls(eng)] == [sv["steps"] for sv in _calls(eng0)]
    assert all(sv.get("persist_ws") is None for sv in _calls(eng))
    for seg0, seg in zip(eng0.saved["segments"], eng.saved["segments"]):
        for k in ("up", "lo"):
            assert torch.equal(seg0["staff"][k][0], seg["staff"][k][0]) and torch.equal(seg0["staff"][k][1], seg["staff"][k][1]), "ids, lengths"
    _shapes_ok(eng, cfg, spectrogram.shape[0])
    # a step ran exactly where the decoder wrote log-probabilities; everywhere else the fills
    for k, o in (("up", outs[2]), ("lo", outs[3])):
        ran = o.abs().sum(-1) > 0
        al = eng.alignment_out[k]
        assert torch.equal(al["peak"] >= 0, ran), k
        assert (al["weight"][ran] > 0).all() and (al["centroid"][ran] >= 0).all() and (al["centroid"][ran] <= spectrogram.shape[2] - 1).all()
        assert (al["peak"][~ran] == -1).all() and (al["weight"][~ran] == 0).all() and (al["centroid"][~ran] == -1).all()
    return eng, outs


@pytest.mark.parametrize("seed", [11, 18])
def test_alignment_keeps_decoding_small(g1, dev, seed):
    meta, cfg, batch = g1
    S = {k: v.to(dev) for k, v in _small_state(cfg, meta["cases"][f"greedy_s{seed}"]).items()}
    _assert_alignment_keeps_decoding(cfg, S, batch[0].to(dev), full=False)


@pytest.fixture(scope="module")
def full_align(g2):
    data, meta, cfg, S, spectrogram = g2
    assert min(meta["min_margin"].values()) >= 1e-3, "fixture precondition: no near-tie argmax"
    return _assert_alignment_keeps_decoding(cfg, S, spectrogram, full=True)


def test_alignment_keeps_decoding_full(g2, full_align):
    data = g2[0]
    eng, outs = full_align
    for nm, t in (("up", outs[2]), ("lo", outs[3])):
        assert np.array_equal(t.argmax(-1).cpu().numpy(), data[f"greedy.{nm}_ids"]), f"{nm} ids differ from the reference's"


def test_option_off_launches_what_it_launched_before(g1, dev):
    """One inference call with the attribute never touched and one with it set to False: the same number of kernel launches, nothing of the option's."""
    from piano_a2s_amd import hip
    L = hip.lib()
    meta, cfg, batch = g1
    S = {k: v.to(dev) for k, v in _small_state(cfg, meta["cases"]["greedy_s11"]).items()}
    x = batch[0].to(dev)
    _run(cfg, S, x, None)                                                  # (warm-up: what a first call sets up once is not counted)
    counts = []
    for align in (None, False):
        k0, a0 = L.a2s_launch_count(), hip.align_launches()
        eng, _ = _run(cfg, S, x, align)
        counts.append(L.a2s_launch_count() - k0)
        assert hip.align_launches() == a0 and eng.alignment_out is None and all("align" not in sv for sv in _calls(eng))
    print(f"launches per inference call: {counts}")
    assert counts[0] == counts[1] and counts[0] > 0


# ------------------------------------------------------------------------------------------- 3. against the oracle
_ORACLE = {}


def _compare(tag, dev_al, ref_al):
    """Every executed step of every attention layer against the oracle's float64 summaries."""
    diff = 0
    for k in ("bar", "up", "lo"):
        ref, got = ref_al[k], {f: dev_al[k][f].cpu() for f in FIELDS}
        ran = ref["ran"]
        assert torch.equal(got["peak"] >= 0, ran), f"{tag}.{k}: the executed steps differ from the oracle's"
        for f in ("centroid", "weight"):
            r = ref[f][ran]
            err = float((got[f][ran].to(torch.float64) - r).abs().max()) / max(1.0, float(r.abs().max()))
            print(f"{tag}.{k}.{f}: {err:.3e}")
            assert err <= TOL, f"{tag}.{k}.{f}: {err:.3e} > {TOL}"
        w = ref["weights"].to(torch.float64)
        at_peak = w.gather(-1, got["peak"].clamp(min=0).long().unsqueeze(-1)).squeeze(-1)
        assert (at_peak[ran] >= (1 - 2 * TOL) * ref["weight"][ran]).all(), f"{tag}.{k}: a device peak is not a maximum of the oracle's row within 2 TOL"
        diff += int((got["peak"][ran].long() != ref["peak"][ran]).sum())
        assert (got["peak"][~ran] == -1).all() and (got["weight"][~ran] == 0).all() and (got["centroid"][~ran] == -1).all(), "steps never run hold the fills"
    print(f"{tag}: {diff} peaks differ from the oracle's")
    return diff


@pytest.mark.parametrize("mode", ["greedy", "grammar", "teacher_forced", "beam2"])
def test_small_model_against_align_oracle(g1, dev, gram, mode):
    """Seeds 11 and 18 of the small fixture.  CPU-measured smallest relative gap between the two largest weights of an oracle row: 2.47e-4 (greedy_s18,
    upper staff) > 2 TOL, so on these fixtures the peak condition is an exact match (tests/test_align_oracle_cpu.py asserts the gap).
    Fixture precondition: per attention layer the oracle's centroids span at least 5 frames over the fixture's cases -- the test is not comparing
    near-constants.  (Over the two seeds together, as the ranges the feature was specified with: CPU-measured spans per layer bar / up / lo = greedy
    13.6 / 15.0 / 21.5, grammar 11.7 / 11.3 / 15.8, teacher-forced 10.5 / 17.4 / 27.6 frames.  A single (seed, mode) can fall below 5 in one layer:
    seed 11 under the grammar 2.89 in the upper staff, whose bars end after a step or two; seed 18 teacher-forced 4.35 at the bar level, 15 rows.)"""
    from piano_a2s_amd import spec
    from tests import align_oracle
    meta, cfg, batch = g1
    x = batch[0].to(dev)
    gt = list(batch[1:7])
    runs = []
    for seed in (11, 18):
        state = _small_state(cfg, meta["cases"][f"greedy_s{seed}"])
        P, Bf = spec.split_state(state)
        S = {k: v.to(dev) for k, v in state.items()}
        if mode == "beam2":
            eng, outs = _run(cfg, S, x, True, K=2)
            # the oracle forced along the device's own winning ids (and the heads' choices that went into the next bar's token)
            forced = [outs[0].argmax(-1).cpu(), outs[1].argmax(-1).cpu(), eng.decoded["up"][0].long().cpu(), eng.decoded["up"][1].cpu(),
                      eng.decoded["lo"][0].long().cpu(), eng.decoded["lo"][1].cpu()]
            ref = align_oracle.forward(P, Bf, cfg, batch[0], ground_truth=forced)
        else:
            key = (seed, mode)
            if key not in _ORACLE:                                             # computed once, shared, never modified
                choice = align_oracle.GrammarChoice(gram) if mode == "grammar" else None
                _ORACLE[key] = align_oracle.forward(P, Bf, cfg, batch[0], choice=choice, ground_truth=gt if mode == "teacher_forced" else None)
            ref = _ORACLE[key]
            eng, outs = _run(cfg, S, x, True, grammar=gram if mode == "grammar" else None, gt=[g.to(dev) for g in gt] if mode == "teacher_forced" else None)
        _shapes_ok(eng, cfg, 3)
        if mode in ("greedy", "grammar"):
            for k in ("up", "lo"):
                ids = eng.decoded[k][0].long().cpu() if mode == "grammar" else (outs[2] if k == "up" else outs[3]).argmax(-1).cpu()
                ran = ref[2][k]["ran"]
                assert torch.equal(ids[ran], ref[1][k][0][ran]), f"{k}: the device decoded other ids than the oracle"
        runs.append((f"s{seed}.{mode}", eng.alignment_out, ref[2]))
    for k in ("bar", "up", "lo"):
        cen = torch.cat([ref[k]["centroid"][ref[k]["ran"]] for _, _, ref in runs])
        span = float(cen.max() - cen.min())
        print(f"{mode}.{k}: the oracle's centroids span {span:.2f} frames over {cen.numel()} rows")
        assert span >= 5, f"fixture precondition: the oracle's {k} centroids span {span:.2f} frames"
    for tag, dev_al, ref_al in runs:
        _compare(tag, dev_al, ref_al)


# ------------------------------------------------------------------------------------------- 4. full width, independent of the new kernel
def test_full_width_against_the_existing_attention_op(g2, full_align, dev):
    """The weights of a handful of (bar, staff, step) recomputed by a2s_attn_step_fwd from the call's saved query and the key image, reduced in numpy."""
    from piano_a2s_amd import hip
    L = hip.lib()
    data, meta, cfg, S, spectrogram = g2
    eng, outs = full_align
    B, T, H = spectrogram.shape[0], eng.saved["enc_out"].shape[1], cfg["hidden_size"]
    enc = eng.saved["enc_out"]
    ws = hip.attn_workspace(B, T, H, dev)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)                  # a done counter at zero: the kernels the greedy loop takes
    checked = 0
    for bar, k in ((0, "up"), (2, "lo"), (4, "up")):
        sv = eng.saved["segments"][bar]["staff"][k][2]
        for step in sorted({0, 1, sv["steps"] // 2, sv["steps"] - 1}):
            q = sv["q"][step]
            ctx, attw = torch.empty(B, 2 * H, device=dev), torch.full((B, T), -1.0, device=dev)
            hip.check(L.a2s_attn_step_fwd(hip.stream(), hip._p(eng.saved["keys"][PREFIX[k]]), hip._p(enc), hip._p(q), C.c_long(H), hip._p(S[PREFIX[k] + ".attn.v.weight"]),
                                          hip._p(ctx), C.c_long(2 * H), None, C.c_long(0), hip._p(attw), B, T, H, hip._p(zero), B, hip._p(ws)), "a2s_attn_step_fwd")
            torch.cuda.synchronize()
            a = attw.cpu().numpy()
            assert (a >= 0).all() and abs(a.sum(axis=1) - 1).max() < 1e-4
            peak, w, cen, bound = _reduce_np(a)
            al = {f: eng.alignment_out[k][f][:, bar, step].cpu().numpy() for f in FIELDS}
            assert np.array_equal(al["peak"], peak), (bar, k, step, al["peak"], peak)
            assert np.array_equal(al["weight"].view(np.uint32), w.view(np.uint32)), (bar, k, step)
            err = np.abs(al["centroid"].astype(np.float64) - cen)
            assert (err <= bound).all(), (bar, k, step, err, bound)
            checked += 1
    assert checked >= 9


# ------------------------------------------------------------------------------------------- 5. beam
@pytest.mark.parametrize("with_grammar", [False, True])
def test_beam_alignment_is_the_forced_alignment_of_the_winners(g1, dev, gram, with_grammar):
    from piano_a2s_amd import hip
    meta, cfg, batch = g1
    S = {k: v.to(dev) for k, v in _small_state(cfg, meta["cases"]["greedy_s11"]).items()}
    x = batch[0].to(dev)
    grammar = gram if with_grammar else None
    eng0, ref = _run(cfg, S, x, False, grammar=grammar, K=2)
    b0 = hip.beam_launches()
    eng, outs = _run(cfg, S, x, True, grammar=grammar, K=2)
    assert hip.beam_launches() > b0 and eng0.alignment_out is None
    for n, a, b in zip(("ts", "key", "up", "lo"), outs, ref):
        assert torch.equal(a, b), n
    for k in ("up", "lo"):
        assert torch.equal(eng.decoded[k][0], eng0.decoded[k][0]) and torch.equal(eng.decoded[k][1], eng0.decoded[k][1]), k
        assert torch.equal(eng.beam_scores[k], eng0.beam_scores[k]), k
    gt = [outs[0].argmax(-1), outs[1].argmax(-1), eng.decoded["up"][0].long(), eng.decoded["up"][1].clone(), eng.decoded["lo"][0].long(), eng.decoded["lo"][1].clone()]
    eng_tf, _ = _run(cfg, S, x, True, gt=gt)
    _shapes_ok(eng, cfg, 3)
    for k in ("bar", "up", "lo"):
        a, b = eng.alignment_out[k], eng_tf.alignment_out[k]
        assert torch.equal(a["peak"] >= 0, b["peak"] >= 0), k
        ran = b["peak"] >= 0
        assert ran.any()
        for f in ("centroid", "weight"):
            err = float((a[f][ran] - b[f][ran]).abs().max()) / max(1.0, float(b[f][ran].abs().max()))
            print(f"beam grammar={with_grammar} {k}.{f}: {err:.3e}")
            assert err <= TOL, f"{k}.{f}: {err:.3e} > {TOL}"
        assert (a["peak"][~ran] == -1).all() and (a["weight"][~ran] == 0).all() and (a["centroid"][~ran] == -1).all()


def test_module_reports_last_alignment(g1, dev):
    """models.ScoreTranscription.alignment: `last_alignment` is the engine's result in evaluation mode, None without the option and in training mode."""
    import models
    meta, cfg, batch = g1
    model = models.ScoreTranscription(**cfg)
    model.load_state_dict(_small_state(cfg, meta["cases"]["greedy_s11"]))
    model = model.to(dev).eval()
    x = batch[0].to(dev)
    with torch.no_grad():
        ref = model(x)
        assert model.last_alignment is None
        model.alignment = True
        outs = model(x)
    al = model.last_alignment
    assert al is not None and set(al) == {"bar", "up", "lo"} and tuple(al["up"]["centroid"].shape) == (3, cfg["max_bars"], cfg["max_length"][0])
    for a, b in zip(outs[2:], ref[2:]):
        assert torch.equal(a.argmax(-1), b.argmax(-1))


# ------------------------------------------------------------------------------------------- 6. refusals
def test_alignment_entry_refuses_what_it_cannot_align(g1, dev, gram):
    from piano_a2s_amd import engine, hip
    L = hip.lib()
    meta, cfg, batch = g1
    x = torch.zeros(2, V, device=dev)
    st = torch.zeros(2, dtype=torch.int32, device=dev)
    table = gram.device_table(dev)
    host = (C.c_int * 4)(1, 1, 1, 1)

    def args(**kw):
        a = hip.NoteDecArgs()
        a.R, a.V, a.T, a.steps = 2, V, 8, 4
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    g, keep = hip.align_buffers(2, 4, 8, dev)
    gg, keep2 = hip.align_buffers(2, 4, 8, dev)
    gg.next_state, gg.n_states, gg.row_state = table.data_ptr(), gram.n_states, st.data_ptr()
    n0, k0 = hip.align_launches(), L.a2s_launch_count()
    for a, blk, word in ((args(attw=x.data_ptr()), g, b"training buffers"), (args(gates=x.data_ptr()), g, b"training buffers"), (args(drop=x.data_ptr()), g, b"training buffers"),
                         (args(n_active=C.cast(host, C.c_void_p).value), g, b"row bookkeeping"), (args(row_list=st.data_ptr()), g, b"row bookkeeping"),
                         (args(row_until=st.data_ptr()), g, b"row bookkeeping"), (args(clip_order=st.data_ptr()), g, b"row bookkeeping"),
                         (args(m_active=C.cast(host, C.c_void_p).value), g, b"row bookkeeping"),
                         (args(gt=x.data_ptr(), tf_flags=C.cast(host, C.c_void_p).value), gg, b"grammar"),
                         (args(gt=x.data_ptr()), g, b"tf_flags"), (args(gt=x.data_ptr(), tf_flags=C.cast(host, C.c_void_p).value, poll=16), g, b"poll")):
        assert L.a2s_note_decoder_fwd_align(hip.stream(), C.byref(a), C.byref(blk), None) == -1
        assert word in L.a2s_last_error(), (word, L.a2s_last_error())
    assert L.a2s_note_decoder_fwd_align(hip.stream(), None, C.byref(g), None) == -1
    assert L.a2s_note_decoder_fwd_align(hip.stream(), C.byref(args()), None, None) == -1
    assert hip.align_launches() == n0 and L.a2s_launch_count() == k0, "nothing was launched"
    S = {k: v.to(dev) for k, v in _small_state(cfg, meta["cases"]["greedy_s11"]).items()}
    eng = engine.Engine(cfg)
    eng.alignment = True
    with pytest.raises(ValueError, match="alignment"):
        eng.forward(S, batch[0].to(dev), inference=False, ground_truth=[g_.to(dev) for g_ in batch[1:7]], teacher_forcing_ratio=1.0, training=True)


# ------------------------------------------------------------------------------------------- 7. the recipe
PARENT_KEYS = {"pred", "wer_upper", "wer_lower", "key_f1", "time_f1", "style", "soundfont", "composer", "target_path"}


def _pretrain(tmp_path, name, extra):
    """The harness of tests/test_gpu_kern_grammar.py: 8 synthetic clips, hidden 32, 41 frames -> the TEST stage's result records."""
    import pretrain
    ws = os.path.join(str(tmp_path), name)
    os.makedirs(ws)
    args = [os.path.join(ROOT, "hparams", "pretrain.yaml"), "--device=cuda:0", f"--workspace={ws}", "--soundfont_folder=/none",
            "--synthetic_clips=8", "--hidden_size=32", "--conv_feature_size=32", "--bins_per_octave=24", "--n_octaves=1", "--max_length=(12, 8)",
            "--synthetic_frames=41", "--synthetic_lengths=[[3, 10], [2, 7]]", "--batch_size=4", "--number_of_epochs=1", "--seed=1234"] + extra
    brain = pretrain.main(args)
    res = os.path.join(ws, "1234", "pretrain.epr", "results", "test")
    return brain, [json.load(open(os.path.join(res, f))) for f in sorted(os.listdir(res))]


def test_recipe_with_and_without_alignment(tmp_path, dev):
    frames = 41
    brain, records = _pretrain(tmp_path, "on", ["--alignment=true"])
    assert records and brain.modules.transcription.alignment and brain.modules.transcription.last_alignment is not None
    tokens = 0
    for rec in records:
        assert set(rec) == PARENT_KEYS | {"alignment"}
        al = rec["alignment"]
        assert set(al) == {"frames_per_second", "bar", "bar_weight", "upper", "upper_weight", "lower", "lower_weight"}
        assert al["frames_per_second"] == 100
        assert len(al["bar"]) == len(al["bar_weight"]) == len(rec["pred"]) == 5
        assert all(0 <= c <= frames - 1 for c in al["bar"]) and all(0 < w <= 1 for w in al["bar_weight"])
        for i, bar in enumerate(rec["pred"]):
            for key, kept in (("upper", bar[3]), ("lower", bar[2])):
                assert len(al[key][i]) == len(al[key + "_weight"][i]) == len(kept), "one centroid per kept token"
                assert all(0 <= c <= frames - 1 for c in al[key][i]) and all(0 < w <= 1 for w in al[key + "_weight"][i])
                tokens += len(kept)
    assert tokens > 0
    brain, records = _pretrain(tmp_path, "off", [])
    assert records and all(set(rec) == PARENT_KEYS for rec in records), "without the flag the records have the parent's keys"
    assert not brain.modules.transcription.alignment and brain.modules.transcription.last_alignment is None
