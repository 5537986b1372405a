"""ONE encoder call -- Engine.encoder(S, x, training=True) and engine_bwd._encoder_bwd, exactly as Engine.forward and engine_bwd.backward issue them --
against the float64 oracle of tests/encoder_oracle.py, at the model's widths (hidden 256, 256 features: the only width at which the persistent
recurrences, the tall-K weight gradients and the two-term fp16 projections run), on every path the call can take, each forced by its switch and
proved by the library's launch counters.  Compared per tensor: the four input projections gi, both layers' outputs, the saved gates, the four final
states, `hidden`; then the returned dX and the 18 parameter gradients.  A failure names the tensor, the clip, the frame and the column.

Bars: per tensor, max(project bar, 3 x the deviation of the oracle's own float32 evaluation from its float64 one) -- the rule of
test_gpu_note_decoder_call.py; project bars 1e-5 forward, 2e-5 gradients (test_gpu_persist.py).  Every figure goes, with the float32 deviation and the
bar used, to the file test_gpu_ops.py::_report writes.

The inputs' preconditions (non-negative features, the saturated cases' share of exact +-1.0) are checked on the CPU by
tests/test_encoder_oracle_cpu.py, over CASES / SATURATED below."""
import functools

import pytest
import torch

from tests import encoder_oracle as oracle

pytestmark = pytest.mark.gpu

H, I = 256, 256
FWD_BAR, GRAD_BAR = 1e-5, 2e-5
WEIGHTS_SEED = 23

BIG = (126, 48)
# (clips, frames): the smallest shapes at which each mechanism can still go wrong
CASES = [
    (1, 1),                          # T < 2: no persistent launch; the first processed step is the only one, dgh_shift stays zero, db_hh is dgh_first's alone
    (1, 2),                          # the smallest persistent launch
    (5, 19), (7, 5), (8, 5),         # both sides of where gemm_workspace(B) alone stops holding W_hh^T (B <= 6) and the BPTT's granule buffers (B <= 7)
    (15, 5), (16, 5), (17, 5),       # a 16-row block not full, exactly full, full plus one row
    (37, 29),                        # three row blocks, the last partial
    (128, 4),                        # 8 row blocks: the block-index permutation of persist_block, both directions side by side on two streams
    (272, 3),                        # more than 256 clips: encoder_streams runs the directions one after the other and sets gru_persist_alone
    (2, 301),                        # a long chain: round-off over 4 x 301 dependent steps, both granule buffers alternating many times
    # 6048 rows: the smallest at which the GEMM hands the projections (768 columns: from 3969 rows) and layer 1's dX (512 columns: from 6017 rows) to
    # its 128 x 128 tiles, which alone run the two-term fp16 split (csrc/a2s_gemm.hip: at least 192 tiles); every case above keeps these products on
    # the small-tile fp32 kernels, where "two_term0" and "gemm_bf16x3_0" change the operand layout at most
    BIG,
]
PATH_CASES = [(5, 19), (17, 5), (37, 29), (128, 4)]
SATURATED = [(16, 5), (37, 29)]
# The saturated cases scale the features and both layers' weight_ih by these factors.  Chosen on the CPU (test_encoder_oracle_cpu.py asserts what they
# are for): gi of layer 0 grows by SAT_X * SAT_W = 64 (max |gi| ~ 250: many z gates below -17.4, where 1 - z rounds to 1, with candidates beyond
# +-9.02, where tanh rounds to +-1), layer 1's by SAT_W with inputs of which about half are then +-1.  Of the float32 oracle's outputs 46 % / 11 %
# (layer 0 / 1) are exactly +-1.0 at (16, 5) and 59 % / 20 % at (37, 29): well above the 1 % asked for, with unsaturated gates left beside them.
SAT_X, SAT_W = 4.0, 16.0

# every path but the default: the switches it sets (a2s_debug_set keys; "two_term" is engine._ENC_TWO_TERM)
PATHS = {
    "default": {},
    "gru_persist0": {"gru_persist": 0},                     # one launch per step, forward and BPTT
    # three launches per step.  (gru_fused = 0 alone takes the BPTT there; the forward asks for gru_persist only, so it is switched off with it)
    "gru_fused0": {"gru_fused": 0, "gru_persist": 0},
    "tallk_wgrad0": {"tallk_wgrad": 0},                     # split-K GEMM plus column sums; the unranged a2s_gru_seq_bwd
    "gemm_bf16x3_0": {"gemm_bf16x3": 0},                    # the other dX product
    "two_term0": {"two_term": False},
    "force_agent": {"persist_force_agent": 1},              # the write-through hand-off
}
COUNTERS = ("gru_persist_fwd_launches", "gru_persist_bwd_launches", "gru_step_fwd_launches", "gru_step_bwd_launches", "tallk_wgrad_launches")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def cfg():
    from piano_a2s_amd import spec
    return spec.default_cfg(freq_bins=48)          # the model's widths (hidden 256, 256 features); the ConvStack is not part of the call


@functools.lru_cache(maxsize=None)
def _weights():
    from piano_a2s_amd import spec
    return oracle.encoder_tensors(spec.procedural_state(cfg(), WEIGHTS_SEED))


@functools.lru_cache(maxsize=None)
def inputs(B, T, variant="plain"):
    """Everything one training call reads, on the CPU: the 18 tensors, features x >= 0 as the ConvStack's ReLU and dropout emit them (a fifth zeroed,
    the rest scaled by 1 / 0.8), seeded randn dEnc and d_hidden.  variant "saturated": x * SAT_X and both layers' weight_ih * SAT_W; "small": x at 1e-3,
    dEnc and d_hidden at 1e-6 of their usual size (the operand ranges the two-term products are scaled by are then far from 1)."""
    g = torch.Generator().manual_seed(1000 * B + T)
    x = torch.relu(torch.randn(B, T, I, generator=g)) * (torch.rand(B, T, I, generator=g) >= 0.2) / 0.8
    dEnc, d_hidden = torch.randn(B, T, 2 * H, generator=g), torch.randn(B, 2 * H, generator=g)
    W = dict(_weights())
    if variant == "saturated":
        x = x * SAT_X
        W.update({k: v * SAT_W for k, v in W.items() if ".weight_ih_" in k})
    elif variant == "small":
        x, dEnc, d_hidden = x * 1e-3, dEnc * 1e-6, d_hidden * 1e-6
    else:
        assert variant == "plain"
    return dict(W=W, x=x, dEnc=dEnc, d_hidden=d_hidden)


@functools.lru_cache(maxsize=None)
def reference(B, T, variant="plain"):
    """(f64 forward, f64 gradients, f32 forward, dev32) of oracle.reference: computed once per case, shared by every path, left unchanged."""
    i = inputs(B, T, variant)
    return oracle.reference(i["W"], i["x"], i["dEnc"], i["d_hidden"])


# ------------------------------------------------------------------------------------------- driving one call
class _path:
    """The switches of one path set, everything put back on the way out (gru_persist_alone included: encoder_streams leaves it as the last call set it)."""
    def __init__(self, name):
        self.kv = dict(PATHS[name])

    def __enter__(self):
        from piano_a2s_amd import engine, hip
        self.L = hip.lib()
        self.two_term = engine._ENC_TWO_TERM
        keys = [k for k in self.kv if k != "two_term"] + ["gru_persist_alone"]
        self.prev = {k: self.L.a2s_debug_get(k.encode()) for k in keys}
        for k, v in self.kv.items():
            if k == "two_term":
                engine._ENC_TWO_TERM = v
            else:
                hip.check(self.L.a2s_debug_set(k.encode(), v), "debug_set")
        return self

    def __exit__(self, *a):
        from piano_a2s_amd import engine
        engine._ENC_TWO_TERM = self.two_term
        for k, v in self.prev.items():
            self.L.a2s_debug_set(k.encode(), v)


def _counters(L):
    return {k: L.a2s_debug_get(k.encode()) for k in COUNTERS}


def _tallk_eligible(L, B, T):
    """How many of the call's eight weight-gradient products qualify for the tall-K kernel, by the library's own answer (the shapes of _encoder_bwd:
    per layer and direction dW_ih over (B*T, I_layer) x (B*T, 3H) and dW_hh over the (B*T, H) half of the 2H-wide outputs)."""
    n = 0
    for In in (I, 2 * H):
        n += 2 * int(L.a2s_tallk_wgrad_eligible(B * T, In, 3 * H, In, 3 * H, In, 1))
        n += 2 * int(L.a2s_tallk_wgrad_eligible(B * T, H, 3 * H, 2 * H, 3 * H, H, 1))
    return n


def _forward(dev, i, training=True):
    from piano_a2s_amd import engine
    S = {k: v.to(dev) for k, v in i["W"].items()}
    eng = engine.Engine(cfg())
    enc, hidden, saved = eng.encoder(S, i["x"].to(dev), training=training)
    torch.cuda.synchronize()
    return S, eng, enc, hidden, saved


def _backward(dev, i, S, eng, saved, B, T, prefill=None):
    from piano_a2s_amd import engine_bwd
    G = {k: (torch.zeros_like(v) if prefill is None else prefill[k].to(dev)) for k, v in S.items()}
    dX = engine_bwd._encoder_bwd(eng, S, G, saved, i["dEnc"].to(dev), i["d_hidden"].to(dev), B, T)
    torch.cuda.synchronize()                     # (the weight gradients land from another stream)
    return dict(dX=dX.cpu(), params={k: G[k].cpu() for k in oracle.PARAMS})


def _forward_tensors(enc, hidden, saved):
    got = {"hidden": hidden.cpu(), "out_l0": saved["layers"][0]["out"].cpu(), "out_l1": enc.cpu()}
    for n, sfx in enumerate(oracle.SUFFIXES):
        rec = saved["layers"][n // 2]["dirs"][n % 2]
        got[f"gi_{sfx}"] = rec["gi"].view(enc.shape[0], enc.shape[1], 3 * H).cpu()
        got[f"hn_{sfx}"] = rec["hn"].cpu()
        if rec["gates"] is not None:
            got[f"gates_{sfx}"] = rec["gates"].cpu()
    return got


def _report(label, name, err, dev32, bar):
    """One line per case and tensor -- "<case> <tensor> (float32 oracle <deviation>, bar <bar>): <error>" -- in the file the per-kernel tests of
    test_gpu_ops.py report to (one place names it)."""
    from tests import test_gpu_ops
    test_gpu_ops._report(f"encoder_call {label} {name} (float32 oracle {dev32:.3e}, bar {bar:.3e})", err)


def _compare(label, views, dev32, project_bar, bad, scale=None):
    """scale: name -> max |gradient| where `ref` holds more than the gradient (a pre-filled G): the error is then measured against that."""
    for name, ref, got in views:
        assert torch.isfinite(got).all(), f"{label} {name}: non-finite (a wait of a persistent launch timed out?)"
        err = oracle.rel_err(got, ref, None if scale is None else scale[name])
        bar = max(project_bar, 3 * dev32[name])
        _report(label, name, err, dev32[name], bar)
        print(f"{label} {name}: {err:.3e}  float32 oracle {dev32[name]:.3e}  bar {bar:.3e}")
        if not err <= bar:
            at, size = oracle.worst(got, ref)
            bad.append(f"{name}: {err:.3e} > {bar:.3e} (largest |got - ref| {size:.3e} at {oracle.where(name, at)})")


def _expected_counts(L, path, B, T):
    """(forward, backward) launch counts of the four recurrences of a call: every case from one clip upwards takes the persistent launches unless the
    path switches them off or T < 2 (a2s_gru_seq_fwd_persist_ok / _bwd_persist_ok refuse one step: there is nothing to hand on)."""
    kv = PATHS[path]
    persist = kv.get("gru_persist", 1) and T >= 2
    fused = kv.get("gru_fused", 1)
    fwd = dict(gru_persist_fwd_launches=4 if persist else 0, gru_persist_bwd_launches=0, gru_step_bwd_launches=0,
               gru_step_fwd_launches=0 if persist or not fused else 4 * T, tallk_wgrad_launches=0)
    bwd = dict(gru_persist_fwd_launches=0, gru_persist_bwd_launches=4 if persist else 0, gru_step_fwd_launches=0,
               gru_step_bwd_launches=0 if persist or not fused else 4 * (T - 1),         # (the last processed step is a plain gate backward)
               tallk_wgrad_launches=_tallk_eligible(L, B, T) if kv.get("tallk_wgrad", 1) else 0)
    return fwd, bwd


def _call_and_check(dev, B, T, path, variant="plain", label=None):
    """One training call on `path`: the counters prove the path, every tensor holds its bar.  Returns the forward tensors for further assertions."""
    from piano_a2s_amd import hip
    i = inputs(B, T, variant)
    f64, g64, _, dev32 = reference(B, T, variant)
    label = label or f"B{B}_T{T}-{path}" + ("" if variant == "plain" else f"-{variant}")
    L = hip.lib()
    with _path(path):
        want_fwd, want_bwd = _expected_counts(L, path, B, T)
        c0 = _counters(L)
        S, eng, enc, hidden, saved = _forward(dev, i)
        c1 = _counters(L)
        grads = _backward(dev, i, S, eng, saved, B, T)
        c2 = _counters(L)
    d1, d2 = {k: c1[k] - c0[k] for k in c0}, {k: c2[k] - c1[k] for k in c0}
    assert d1 == want_fwd, f"{label}: forward launches {d1}, expected {want_fwd}"
    assert d2 == want_bwd, f"{label}: backward launches {d2}, expected {want_bwd}"
    got = _forward_tensors(enc, hidden, saved)
    bad = []
    _compare(label, oracle.forward_views(f64, got), dev32, FWD_BAR, bad)
    assert not bad, f"{label} forward: " + "; ".join(bad)
    _compare(label, oracle.grad_views(g64, grads), dev32, GRAD_BAR, bad)
    assert not bad, f"{label} backward: " + "; ".join(bad)
    return got


@pytest.mark.parametrize("B,T", CASES, ids=[f"B{b}_T{t}" for b, t in CASES])
def test_default_path_against_the_oracle(dev, B, T):
    """Every case on the switches' defaults: four persistent forward and four persistent backward launches and no step launch from one clip upwards
    (T >= 2), the tall-K weight gradients wherever the library says the shapes qualify.  T = 1 is computed, on the step kernels: one
    gru_step_fwd_fused launch per recurrence, one plain gate backward."""
    _call_and_check(dev, B, T, "default")


SWITCHED = [(p, c) for p in PATHS if p != "default" for c in PATH_CASES] + [("two_term0", BIG), ("gemm_bf16x3_0", BIG)]


@pytest.mark.parametrize("path,case", SWITCHED, ids=[f"{p}-B{c[0]}_T{c[1]}" for p, c in SWITCHED])
def test_switched_path_against_the_oracle(dev, path, case):
    _call_and_check(dev, case[0], case[1], path)


@pytest.mark.parametrize("path", ["default", "gru_persist0"])
def test_eval_call_equals_training_call(dev, path):
    """training=False saves no gates and returns the bits of the training=True call on the same path."""
    B, T = 17, 5
    i = inputs(B, T)
    with _path(path):
        _, _, enc_t, hidden_t, saved_t = _forward(dev, i, training=True)
        _, _, enc_e, hidden_e, saved_e = _forward(dev, i, training=False)
    assert all(rec["gates"] is None for ls in saved_e["layers"] for rec in ls["dirs"])
    a, b = _forward_tensors(enc_t, hidden_t, saved_t), _forward_tensors(enc_e, hidden_e, saved_e)
    for k in ("out_l0", "out_l1", "hidden") + tuple(f"hn_{s}" for s in oracle.SUFFIXES):
        assert torch.equal(a[k], b[k]), f"{path} {k}: max diff {float((a[k] - b[k]).abs().max()):.3e}"


@pytest.mark.parametrize("path", ["default", "tallk_wgrad0"])
def test_parameter_gradients_accumulate(dev, path):
    """Every parameter gradient is added to what G holds: pre-filled with seeded randn, G ends as pre-fill plus gradient, within the gradient bars
    measured against the gradient's own maximum."""
    B, T = 17, 5
    i = inputs(B, T)
    _, g64, _, dev32 = reference(B, T)
    g = torch.Generator().manual_seed(99)
    prefill = {k: torch.randn(v.shape, generator=g) for k, v in i["W"].items()}
    with _path(path):
        S, eng, _, _, saved = _forward(dev, i)
        grads = _backward(dev, i, S, eng, saved, B, T, prefill=prefill)
    views = [(k, prefill[k].double() + g64["params"][k], grads["params"][k]) for k in oracle.PARAMS]
    scale = {k: float(g64["params"][k].abs().max()) for k in oracle.PARAMS}
    bad = []
    _compare(f"B{B}_T{T}-{path}-prefilled", views, dev32, GRAD_BAR, bad, scale)
    assert not bad, "; ".join(bad)


SAT_VARIANTS = [(p, c) for p in ("default", "gru_persist0") for c in SATURATED]


@pytest.mark.parametrize("path,case", SAT_VARIANTS, ids=[f"{p}-B{c[0]}_T{c[1]}" for p, c in SAT_VARIANTS])
def test_saturated_gates_keep_the_states_within_one(dev, path, case):
    """The engine vouches a bound of 1 (hip.one) for every GRU state -- layer 1's input projection, the attention key products, every dW_hh.  With
    the gates driven into saturation (a share of the float32 oracle's outputs is exactly +-1.0: test_encoder_oracle_cpu.py) no state exceeds 1.0."""
    got = _call_and_check(dev, case[0], case[1], path, "saturated")
    for k in ("out_l0", "out_l1") + tuple(f"hn_{s}" for s in oracle.SUFFIXES):
        m = float(got[k].abs().max())
        assert m <= 1.0, f"{k}: max |state| = 1 + {m - 1.0:.3e}"


def test_small_magnitudes(dev):
    _call_and_check(dev, 37, 29, "default", "small")
