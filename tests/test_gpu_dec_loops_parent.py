"""The note decoder's host loops against a recording of the commit before they were merged into one (csrc/a2s_seq.hip: note_decoder_run and the
step descriptor NoteStepMode / NoteStep; csrc/a2s_bwd.hip: the reverse loops): the refactor reorders no sum and changes no launch, so what two runs
of that commit reproduce bit for bit must come out bit-identical now.

tests/golden/dec_loops_parent.json is merge_recordings(record(dev), record(dev)) of two processes run on that commit: only entries on which the
two recordings agree are kept, the list "unstable" in the file names what did not (only the parameter tensors' norms, asserted with a margin).  Per decode mode: the decoded ids and lengths of every
bar and staff in full, a SHA-256 of the bytes of every output tensor (staff log-probabilities, alignment peak / weight / centroid, beam scores; for
the training-mode forward also of what every call saves for the backward pass) and the deltas of the library's launch counters over the call.  The
modes of the small fixture (3 clips, tests/golden/g1_small.json, hidden size 32, lively weights) all run the generic step or the few-row kernels:
at that width neither the mid-size kernels nor the persistent decoder are taken, so "eager_persistent" is there the few-row run and "eager_bulk" the
generic one.  The h64_ modes (hidden size 64) reach the mid-size kernels, the wide_ modes (hidden 256, the set-up of
tests/test_gpu_dec_persist.py) the persistent decoder; EXPECT names the launch counter that has to move in the parent's recording of a mode.
Two fused training steps: 12 clips, the smallest shape of tests/test_gpu_pair_staves.py that still takes the pair loop, and 4 clips, which the
persistent decoder takes in both directions.  Loss terms and counters exact; the backward sums some gradients with float atomics (bench.py:
dump_outputs), so the gradient norm and the updated parameters are not bit-stable from run to run and carry the margins of
tests/test_gpu_pair_staves.py -- 2e-5 relative on the norm, 5e-6 of max |p| on the parameters: on a fixed strided sample of them, and on every
parameter tensor's largest magnitude and norm (bounds that follow from it, see the test)."""
import contextlib
import hashlib
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SMALL_BATCH = dict(frames=41, upper_range=(3, 10), lower_range=(2, 7), full_tail=0.1)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "dec_loops_parent.json")
COUNTERS = ("dec_persist_launches", "dec_mid_launches", "attn_pair_launches")
# mode -> (what the Engine is given, the library switches set for the call)
MODES = {
    "eager_persistent": (dict(graph=False), {"dec_persist": 1, "dec_fused": 1}),
    "eager_few_row": (dict(graph=False), {"dec_persist": 0, "dec_fused": 1}),
    "eager_bulk": (dict(graph=False), {"dec_persist": 0, "dec_fused": 0}),
    "eager_generic": (dict(graph=False), {"dec_persist": 0, "dec_fused": 0, "dec_mid": 0}),      # the twelve-launch step
    "graph": (dict(graph=True), {}),
    "graph_grammar": (dict(graph=True, grammar=True), {}),
    "eager_grammar": (dict(graph=False, grammar=True), {}),
    "align_greedy": (dict(align=True), {}),
    "align_grammar": (dict(align=True, grammar=True), {}),
    "align_teacher_forced": (dict(align=True, forced=True), {}),
    "beam2": (dict(K=2), {}),
    "beam2_grammar": (dict(K=2, grammar=True), {}),
    "beam2_align": (dict(K=2, align=True), {}),
    # the same fixture at hidden_size 64, the smallest width the mid-size step kernels take (at 32 the launch-per-step loop runs the generic step):
    # here a step finds its query left behind by the step before it, and a beam re-parents that query
    "h64_eager_few_row": (dict(graph=False, hidden=64), {"dec_persist": 0, "dec_fused": 1}),
    "h64_eager_bulk": (dict(graph=False, hidden=64), {"dec_persist": 0, "dec_fused": 0}),
    "h64_graph": (dict(graph=True, hidden=64), {}),
    "h64_eager_grammar": (dict(graph=False, grammar=True, hidden=64), {}),
    "h64_align_greedy": (dict(align=True, hidden=64), {}),
    "h64_align_teacher_forced": (dict(align=True, forced=True, hidden=64), {}),
    "h64_beam2": (dict(K=2, hidden=64), {}),
    "h64_eager_generic": (dict(graph=False, hidden=64), {"dec_persist": 0, "dec_fused": 0, "dec_mid": 0}),
    "h64_beam2_grammar": (dict(K=2, grammar=True, hidden=64), {}),
    # the model's own widths (hidden 256), 3 clips: the whole call of a staff is one persistent launch (csrc/a2s_dec_persist.hip)
    "wide_persistent": (dict(graph=False, wide=True), {"dec_persist": 1, "dec_fused": 1}),
    "wide_persistent_train_forward": (dict(wide=True, train_forward=True, saved=True), {"dec_persist": 1, "dec_fused": 1}),
    "wide_few_row_train_forward": (dict(wide=True, train_forward=True), {"dec_persist": 0, "dec_fused": 1}),
}
# the counter that proves a mode took the path it is named for: > 0 in the parent's recording (ZERO: == 0)
EXPECT = {"graph_grammar": "grammar", "eager_grammar": "grammar", "align_greedy": "align", "align_grammar": "align", "align_teacher_forced": "align",
          "beam2": "beam", "beam2_grammar": "beam", "beam2_align": "beam", "h64_eager_bulk": "dec_mid_launches", "h64_eager_grammar": "dec_mid_launches",
          "h64_align_greedy": "dec_mid_launches", "h64_align_teacher_forced": "dec_mid_launches", "h64_beam2": "dec_mid_launches",
          "h64_beam2_grammar": "dec_mid_launches", "wide_persistent": "dec_persist_launches", "wide_persistent_train_forward": "dec_persist_launches"}
ZERO = {"h64_eager_generic": "dec_mid_launches", "h64_eager_few_row": "dec_mid_launches", "wide_few_row_train_forward": "dec_persist_launches"}
TRAIN_CASES = {12: "attn_pair_launches", 4: "dec_persist_launches"}       # clips -> the counter that has to move (see record_train)
PARAM_STRIDE = 8009             # the sample of the updated parameters: every 8009th element of the flat buffer (about 1500 values)


@contextlib.contextmanager
def _switches(values):
    """Library switches for one call, and the environment variables the conftest's `decoder_path` keeps beside two of them."""
    from piano_a2s_amd import hip
    L = hip.lib()
    env = {"dec_persist": "A2S_DEC_PERSIST", "dec_fused": "A2S_DEC_FUSED"}
    prev = {k: L.a2s_debug_get(k.encode()) for k in values}
    prev_env = {env[k]: os.environ.get(env[k]) for k in values if k in env}
    try:
        for k, v in values.items():
            if k in env:
                os.environ[env[k]] = str(v)
            hip.check(L.a2s_debug_set(k.encode(), v), "a2s_debug_set")
        yield
    finally:
        for k, v in prev.items():
            hip.check(L.a2s_debug_set(k.encode(), v), "a2s_debug_set")
        for name, v in prev_env.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v


def _counters():
    from piano_a2s_amd import hip
    L = hip.lib()
    c = {k: int(L.a2s_debug_get(k.encode())) for k in COUNTERS}
    c.update(grammar=hip.grammar_launches(), beam=hip.beam_launches(), align=hip.align_launches())
    return c


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().cpu().numpy()).tobytes()).hexdigest()


def small_setup(dev, hidden=None):
    """The g1_small set-up of tests/test_gpu_kern_grammar.py and tests/test_gpu_align.py (hidden: another hidden_size than the fixture's 32)."""
    from piano_a2s_amd import spec, synthetic
    from piano_a2s_amd.kern_grammar import KernGrammar
    meta = json.load(open(os.path.join(GOLDEN, "g1_small.json")))
    cfg = spec.default_cfg(**dict(meta["cfg"], **({"hidden_size": hidden} if hidden else {})))
    batch = synthetic.make_batch(3, cfg, meta["batch_seed"], **SMALL_BATCH)
    case = meta["cases"]["greedy_s11"]
    S = {k: v.to(dev) for k, v in spec.procedural_state(cfg, case["weights_seed"], eos_bias=case["eos_bias"], lively=True).items()}
    return cfg, S, batch[0].to(dev), [g.to(dev) for g in batch[1:7]], KernGrammar()


def wide_setup(dev):
    """The first case of tests/test_gpu_dec_persist.py::test_persistent_decoder_equals_stepwise: the model's widths, short bars, 3 clips of 97 frames."""
    from piano_a2s_amd import spec, synthetic
    from piano_a2s_amd.kern_grammar import KernGrammar
    cfg = spec.default_cfg(freq_bins=48, max_length=(40, 24))
    S = {k: v.to(dev) for k, v in spec.procedural_state(cfg, 43, eos_bias=2.0, lively="token").items()}
    batch = synthetic.make_batch(3, cfg, 10, frames=97, upper_range=(5, 30), lower_range=(3, 18), full_tail=0.15, spectrogram="ridges")
    return cfg, S, batch[0].to(dev), [g.to(dev) for g in batch[1:7]], KernGrammar()


_SETUPS = {}


def _setup(dev, opts):
    key = "wide" if opts.get("wide") else opts.get("hidden")
    if key not in _SETUPS:                       # built once, shared, never modified
        _SETUPS[key] = wide_setup(dev) if key == "wide" else small_setup(dev, key)
    return _SETUPS[key]


def record_mode(mode, dev):
    """One Engine.forward in `mode` -> its entry of the fixture."""
    from piano_a2s_amd import engine
    opts, switches = MODES[mode]
    cfg, S, x, gt, gram = _setup(dev, opts)
    eng = engine.Engine(cfg)
    if "graph" in opts:
        eng.greedy_graph = opts["graph"]
    eng.alignment = bool(opts.get("align"))
    eng.kern_grammar = gram if opts.get("grammar") else None
    eng.beam_size = opts.get("K", 1)
    with _switches(switches):
        c0 = _counters()
        if opts.get("train_forward"):            # (training mode: every call keeps its state, inputs, queries, outputs and gates for the backward pass)
            outs = eng.forward(S, x, inference=False, ground_truth=gt, teacher_forcing_ratio=1.0, training=True, dropout=False, rng=random.Random(3))
        elif opts.get("forced"):
            outs = eng.forward(S, x, inference=False, ground_truth=gt, teacher_forcing_ratio=1.0, training=False)
        else:
            outs = eng.forward(S, x, inference=True)
        torch.cuda.synchronize()
        c1 = _counters()
    segs = eng.saved["segments"]
    entry = {"counters": {k: c1[k] - c0[k] for k in c0}, "sha256": {"upper_logp": _sha(outs[2]), "lower_logp": _sha(outs[3])}}
    for k in ("up", "lo"):
        entry["ids_" + k] = [sg["staff"][k][0].cpu().tolist() for sg in segs]
        entry["lengths_" + k] = [sg["staff"][k][1].cpu().tolist() for sg in segs]
    if opts.get("saved"):
        # what the backward pass reads, rows and steps the call never wrote included: the persistent path zero-fills all of it before its launch
        # (the launch-per-step loop only for row_list tails: there the context columns behind the last step stay as allocated)
        for name in ("h", "x", "q", "o", "gates"):
            h = hashlib.sha256()
            for sg in segs:
                for k in ("up", "lo"):
                    h.update(np.ascontiguousarray(sg["staff"][k][2][name].cpu().numpy()).tobytes())
            entry["sha256"]["saved_" + name] = h.hexdigest()
    if eng.alignment_out is not None:
        for k in ("bar", "up", "lo"):
            for f in ("peak", "weight", "centroid"):
                entry["sha256"][f"align_{k}_{f}"] = _sha(eng.alignment_out[k][f])
    if eng.beam_scores is not None:
        for k in ("up", "lo"):
            entry["sha256"]["beam_score_" + k] = _sha(eng.beam_scores[k])
    return entry


def record_train(dev, B):
    """One fused training step, the (80, 1.0, False) set-up of tests/test_gpu_pair_staves.py at B clips.  B = 12: more than the 8 clips the persistent
    decoder takes, and the 60 rows of its five fused bars are more than the 32 ("attn_pair_fused_rows") at which the pair loop hands a step to the
    few-row kernels -- the parent's recording counts 9 joint sweeps in each direction (9 at 12 clips, 11 at 16, 10 at 24, 13 at 80).  B = 4: the
    persistent decoder, forward and backward."""
    import models
    from piano_a2s_amd import hip, spec, synthetic, train
    L = hip.lib()
    keys = ("attn_pair_launches", "attn_pair_bwd_launches", "dec_persist_launches")
    cfg = spec.default_cfg(freq_bins=48, max_length=(24, 14))
    batch = synthetic.make_batch(B, cfg, 63, frames=61, upper_range=(4, 22), lower_range=(3, 12), full_tail=0.05)
    dbatch = [t.to(dev) if torch.is_tensor(t) else t for t in batch]
    torch.manual_seed(11)
    m = models.ScoreTranscription(**cfg).to(dev).train()
    step = train.TrainStep(m, dropout=False, clip_groups=False)
    c0 = {k: int(L.a2s_debug_get(k.encode())) for k in keys}
    losses = step(dbatch, 1.0, rng=random.Random(7))
    torch.cuda.synchronize()
    ctl = step.opt.ctl.cpu()
    flat = step.flat.detach().cpu()
    tensors = {n: p.detach().double().cpu() for n, p in m.named_parameters()}
    return {"B": B, "losses_hex": [float(v).hex() for v in losses[:, 0].cpu().tolist()],
            "counters": {k: int(L.a2s_debug_get(k.encode())) - c0[k] for k in keys},
            "grad_norm": float(ctl[0]), "applied": float(ctl[2]), "param_absmax": float(flat.abs().max()),
            "params_sample": [float(v) for v in flat[::PARAM_STRIDE].tolist()],
            "param_tensors": {n: [int(t.numel()), float(t.abs().max()), float(t.norm())] for n, t in tensors.items()}}


def record(dev):
    """One recording, in the fixture's layout."""
    return {"modes": {m: record_mode(m, dev) for m in MODES}, "train": {str(B): record_train(dev, B) for B in TRAIN_CASES}}


TOLERANT = ("grad_norm", "params_sample", "param_absmax", "param_tensors")       # asserted with a margin: the first recording's values stay


def merge_recordings(a, b):
    """The fixture from two recordings of one commit: what differs between them is named in "unstable" and, unless asserted with a margin, left out."""
    unstable = []

    def merge(x, y, path):
        if isinstance(x, dict) and path[-1] not in TOLERANT:
            merged = {k: merge(x[k], y.get(k) if isinstance(y, dict) else None, path + [k]) for k in x}
            return {k: v for k, v in merged.items() if v is not None}
        if x == y:
            return x
        unstable.append(".".join(path))
        return x if path[-1] in TOLERANT else None
    return {"what": "tests/test_gpu_dec_loops_parent.py: merge_recordings of two record() runs on the commit before the decoder loops were merged",
            "modes": merge(a["modes"], b["modes"], ["modes"]), "train": merge(a["train"], b["train"], ["train"]), "unstable": unstable}


# ------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def parent():
    return json.load(open(FIXTURE))


def test_fixture_holds_every_mode(parent):
    """Nothing was dropped as unstable, and in the parent's recording every mode took the path it is named for."""
    assert set(parent["modes"]) == set(MODES) and set(parent["train"]) == {str(B) for B in TRAIN_CASES}
    for mode, e in parent["modes"].items():
        assert {"counters", "sha256", "ids_up", "ids_lo", "lengths_up", "lengths_lo"} <= set(e), mode
        assert {"upper_logp", "lower_logp"} <= set(e["sha256"]), mode
        assert set(e["counters"]) == set(COUNTERS) | {"grammar", "beam", "align"}, mode
        if MODES[mode][0].get("saved"):
            assert {"saved_h", "saved_x", "saved_q", "saved_o", "saved_gates"} <= set(e["sha256"]), mode
    for mode, key in EXPECT.items():
        assert parent["modes"][mode]["counters"][key] > 0, f"{mode}: {key} did not move in the parent's recording"
    for mode, key in ZERO.items():
        assert parent["modes"][mode]["counters"][key] == 0, f"{mode}: {key} moved in the parent's recording"
    for B, key in TRAIN_CASES.items():
        assert parent["train"][str(B)]["counters"][key] > 0, f"training step of {B} clips: {key} did not move in the parent's recording"
    assert not [u for u in parent["unstable"] if not u.rsplit(".", 1)[-1] in TOLERANT], parent["unstable"]


@pytest.mark.parametrize("mode", list(MODES))
def test_decode_mode_equals_the_parent_commit(parent, dev, mode):
    want = parent["modes"][mode]
    got = record_mode(mode, dev)
    print(f"{mode}: counters {got['counters']}")
    assert got["counters"] == want["counters"], (got["counters"], want["counters"])
    for k in ("ids_up", "ids_lo", "lengths_up", "lengths_lo"):
        assert got[k] == want[k], f"{mode}: {k} differ from the parent's"
    assert set(got["sha256"]) == set(want["sha256"])
    for k, h in want["sha256"].items():
        assert got["sha256"][k] == h, f"{mode}: the bytes of {k} differ from the parent's"


@pytest.mark.parametrize("B", list(TRAIN_CASES))
def test_training_step_equals_the_parent_commit(parent, dev, B):
    want = parent["train"][str(B)]
    got = record_train(dev, B)
    print(f"train B={B}: counters {got['counters']}, losses {got['losses_hex']}, gradient norm {got['grad_norm']!r} (parent {want['grad_norm']!r})")
    assert got["counters"] == want["counters"], (got["counters"], want["counters"])
    assert got["losses_hex"] == want["losses_hex"], (got["losses_hex"], want["losses_hex"])
    assert got["applied"] == want["applied"] == 1.0
    assert abs(got["grad_norm"] - want["grad_norm"]) <= 2e-5 * want["grad_norm"], (got["grad_norm"], want["grad_norm"])
    margin = 5e-6 * want["param_absmax"]                   # max |p - p'| <= margin over the whole parameter buffer is what is asked for
    a, b = np.array(got["params_sample"]), np.array(want["params_sample"])
    assert a.shape == b.shape and len(b) >= 1000
    err = float(np.abs(a - b).max())
    print(f"updated parameters: max |delta| over {len(b)} samples {err:.3e}, margin {margin:.3e}")
    assert err <= margin
    # ... and what it implies for EVERY tensor t of n elements: |max |t| - max |t'|| <= margin and |norm t - norm t'| <= norm (t - t') <= sqrt(n) * margin
    assert set(got["param_tensors"]) == set(want["param_tensors"])
    for name, (n, amax, norm) in want["param_tensors"].items():
        n1, amax1, norm1 = got["param_tensors"][name]
        assert n1 == n and abs(amax1 - amax) <= margin and abs(norm1 - norm) <= n ** 0.5 * margin, (name, (n, amax, norm), got["param_tensors"][name])
