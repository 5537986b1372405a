"""The key-image attention at LARGE pre-activations (VERDICT r6 weak spot 1(c), next-round item 4): every kernel that evaluates tanh(k + q) through
exp(2k) exp(2q) (csrc/a2s_common.h: exp2x_clamped, tanh_ek, sech2_ek) against float64 on the patterns of tests/attn_range_oracle.py, within that
oracle's a-priori fp32 bounds -- out to the edge of the domain piano_a2s_amd/attn_range.py states, in all four regimes -- and the guard that turns a
decode outside that domain into an error.  The key image always comes from the library (the key projection's GEMM epilogue, act 3, on K = enc [I | 0]:
every product has one non-zero term on a grid of 1/8, so it is exact); no host exp.  Every measurement is printed as a fraction of its bound and appended
to attn_range.txt in the tests' report directory (_log)."""
import ctypes as C
import os
import random
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import attn_range_oracle as oracle                     # noqa: E402

pytestmark = pytest.mark.gpu
NULL = C.c_void_p(0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _log(line):
    """Prints a measured figure and appends it to attn_range.txt in the directory A2S_TEST_REPORT_DIR names (default: test_reports/, ignored by git), as
    tests/test_gpu_operand_ranges.py does; profiles/attn_range_report.txt is that file from a run on the MI355X."""
    out = os.environ.get("A2S_TEST_REPORT_DIR", "test_reports")
    os.makedirs(out, exist_ok=True)
    print(line)
    with open(os.path.join(out, "attn_range.txt"), "a") as f:
        f.write(line + "\n")


class _switch:
    """Library switches for the body of a `with`, put back on the way out."""
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        from piano_a2s_amd import hip
        self.L = hip.lib()
        self.prev = {k: self.L.a2s_debug_get(k.encode()) for k in self.kv}
        for k, v in self.kv.items():
            hip.check(self.L.a2s_debug_set(k.encode(), v), "debug_set")

    def __exit__(self, *a):
        for k, v in self.prev.items():
            self.L.a2s_debug_set(k.encode(), v)


def _frac(name, got, ref, bound):
    """max |got - ref| / bound, logged; got: device tensor, ref / bound: float64 arrays."""
    got = got.detach().cpu().double().numpy()
    assert np.isfinite(got).all(), f"{name}: not finite"
    frac = float((np.abs(got - ref) / bound).max())
    _log(f"{name}: {frac:.2e} of the bound (max bound {float(np.max(bound)):.3e})")
    return frac


def _image(dev, x2d, splitk=1):
    """x2d (M, H) float64 on fp32 values -> the library's key image exp2x_clamped(x) (M, H): the key projection with enc = [x | 0], W_e = [I | 0]."""
    from piano_a2s_amd import hip
    M, H = x2d.shape
    enc = torch.zeros(M, 2 * H, device=dev)
    enc[:, :H] = torch.from_numpy(x2d).float().to(dev)
    W = torch.zeros(H, 4 * H, device=dev)
    W[:, 2 * H:3 * H] = torch.eye(H, device=dev)
    out = torch.full((M, H), float("nan"), device=dev)
    hip.gemm(enc, 2 * H, 1, W, 1, 4 * H, out, H, M, H, 2 * H, b_off=2 * H, act=3, splitk=splitk)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------- a. the image itself
@pytest.mark.parametrize("epilogue,splitk", [("tile", 1), ("splitk_reduce", 2)])
def test_key_image_of_both_gemm_epilogues(dev, epilogue, splitk):
    """exp2x_clamped as the two GEMM epilogues write it, x over [-70, 70] on a grid of 1/8 with +-43 and the floats next to them: inside the clamp within
    rho(x) of float64 exp(2x) (the oracle's derivation of how __expf rounds); beyond it bit-equal to the value at +-43, finite and normal."""
    f32 = np.float32
    edge = [np.nextafter(f32(s * 43), f32(0)) for s in (1, -1)] + [np.nextafter(f32(s * 43), f32(s * 99)) for s in (1, -1)]
    x = np.concatenate([np.arange(-70 * 8, 70 * 8 + 1) / 8.0, np.array(edge, dtype=np.float64)])
    H = 32
    M = -(-x.size // H)
    x2d = np.zeros(M * H)
    x2d[:x.size] = x
    x2d = x2d.reshape(M, H)
    img = _image(dev, x2d, splitk).cpu().numpy().reshape(-1)
    x, img32 = x2d.reshape(-1), img
    img = img32.astype(np.float64)
    assert np.isfinite(img).all() and (img >= np.finfo(np.float32).tiny).all(), "finite and normal"
    inside = np.abs(x) <= 43.0
    rel = np.abs(img[inside] / np.exp(2.0 * x[inside]) - 1.0)
    frac = rel / oracle.rho(x[inside])
    i = int(np.argmax(frac))
    _log(f"key image, {epilogue} epilogue: relative error {frac.max():.3f} of rho(x) at x = {x[inside][i]:g} ({rel[i]:.3e}); at |x| = 43: {rel[np.abs(x[inside]) == 43].max():.3e}")
    assert frac.max() <= 1.0, (float(x[inside][i]), float(rel[i]))
    at = {s: img32[x == s * 43.0][0] for s in (1, -1)}
    beyond = ~inside
    assert beyond.sum() > 400
    assert (img32[beyond] == np.where(x[beyond] > 0, at[1], at[-1])).all(), "beyond the clamp: the value at +-43, bit for bit"


def test_key_image_as_the_engine_forms_it(dev):
    """Engine._keys itself (the two-term fp16 product with ranges (1, max |W|), then act 3) with |enc| < 1 and W scaled so that |K| reaches 40: the image
    within rho(K) + 2 dK of float64, dK = 2e-6 sum |enc||W| the bar test_gpu_ops.py::test_gemm_two_term_fp16_path holds the raw product to (an absolute
    error dK of K is a relative error 2 dK of exp(2K)).  The logged number is what the two-term key product costs at this range."""
    from piano_a2s_amd import engine
    H, M = 256, 3 * 37
    g = torch.Generator().manual_seed(3)
    enc = (torch.rand(M, 2 * H, generator=g) * 2 - 1) * 0.999
    W = torch.randn(H, 4 * H, generator=g)
    K64 = enc.double() @ W[:, 2 * H:].double().t()
    W[:, 2 * H:] *= 40.0 / float(K64.abs().max())
    W = W.float()
    K64 = enc.double() @ W[:, 2 * H:].double().t()
    assert 39.99 < float(K64.abs().max()) < 40.01
    mag = enc.double().abs() @ W[:, 2 * H:].double().abs().t()
    eng = engine.Engine(dict(hidden_size=H))
    img = eng._keys({"a.attn.weight": W.to(dev)}, "a", enc.to(dev), H)
    torch.cuda.synchronize()
    rel = (img.cpu().double() / torch.exp(2 * K64) - 1.0).abs().numpy()
    bound = oracle.rho(K64.numpy()) + 2 * 2e-6 * mag.numpy()
    frac = float((rel / bound).max())
    _log(f"key image, Engine._keys (two-term product, max |K| = 40): relative error {rel.max():.3e}, {frac:.3f} of rho(K) + 2 dK "
         f"(rho alone {float(oracle.rho(40.0)):.3e}; {float((rel / oracle.rho(K64.numpy())).max()):.2f} of rho alone)")
    assert frac <= 1.0


# ---------------------------------------------------------------------------------------------------------------- b / c. the kernels
_CASES = {}


def _case(regime, H, T, rows, clips, S):
    """The data of one (regime, shape), built once and shared: patterns, float64 references of forward and backward, their bounds."""
    key = (regime, H, T, rows, clips, S)
    if key in _CASES:
        return _CASES[key]
    K, qs = oracle.patterns(regime, T, H, rows, clips, steps=S)
    rng = np.random.default_rng([H, T, rows, S])
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    v = f32(rng.standard_normal(H) * 0.1)
    enc = f32(rng.uniform(-1, 1, (clips, T, 2 * H)))
    dctx = f32(rng.standard_normal((S, rows, 2 * H)) * 0.02)
    fwd = [oracle.forward(K, qs[s], v, enc, with_bound=True) for s in range(S)]
    bwd = oracle.backward(K, qs, v, enc, dctx)
    # float64 autograd of tanh(K + q): the reference of the gradients (the oracle's closed forms carry the bounds and must agree with it)
    Kt, qt, vt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (K, qs, v))
    et, rows_of = torch.tensor(enc), torch.arange(rows) % clips
    scores, loss = [], 0
    for s in range(S):
        sc = (torch.tanh(Kt[rows_of] + qt[s].unsqueeze(1)) * vt).sum(-1)
        sc.retain_grad()
        scores.append(sc)
        ctx = torch.bmm(torch.softmax(sc, dim=1).unsqueeze(1), et[rows_of]).squeeze(1)
        loss = loss + (ctx * torch.tensor(dctx[s])).sum()
    loss.backward()
    auto = dict(dq=qt.grad.numpy(), dK=Kt.grad.numpy(), dv=vt.grad.numpy(), ds=np.stack([sc.grad.numpy() for sc in scores]))
    for name, a in auto.items():
        assert np.abs(a - bwd[name]).max() <= 1e-12 * max(1.0, np.abs(a).max()), name
    _CASES[key] = dict(K=K, qs=qs, v=v, enc=enc, dctx=dctx, fwd=fwd, bwd=bwd, auto=auto)
    return _CASES[key]


def _device_inputs(dev, c):
    clips, T, H = c["K"].shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)
    d = dict(keys=_image(dev, c["K"].reshape(clips * T, H)), enc=t(c["enc"]), v=t(c["v"]), qs=t(c["qs"]), dctx=t(c["dctx"]))
    assert torch.isfinite(d["keys"]).all()
    return d


def _fwd_plain(dev, d, s, rows, T, H, ws):
    from piano_a2s_amd import hip
    ctx, attw = torch.full((rows, 2 * H), 7.0, device=dev), torch.full((rows, T), 7.0, device=dev)
    hip.check(hip.lib().a2s_attn_step_fwd(hip.stream(), hip._p(d["keys"]), hip._p(d["enc"]), C.c_void_p(d["qs"][s].data_ptr()), H, hip._p(d["v"]), hip._p(ctx), 2 * H,
                                          NULL, 0, hip._p(attw), rows, T, H, NULL, 0, hip._p(ws)), "attn fwd")
    torch.cuda.synchronize()
    return attw, ctx


def _row_plan(dev, rows, clips):
    """Clip order and rank (the identity) and the step each row runs until (never finished): the row bookkeeping of a fused-bars call, all rows live."""
    ident = torch.arange(clips, dtype=torch.int32, device=dev)
    return ident, ident.clone(), torch.full((rows,), 1 << 20, dtype=torch.int32, device=dev)


def _fwd_rows(dev, d, s, rows, clips, T, H, ws):
    from piano_a2s_amd import hip
    plan = _row_plan(dev, rows, clips)
    ctx, attw = torch.full((rows, 2 * H), 7.0, device=dev), torch.full((rows, T), 7.0, device=dev)
    hip.check(hip.lib().a2s_attn_step_fwd_rows(hip.stream(), hip._p(d["keys"]), hip._p(d["enc"]), C.c_void_p(d["qs"][s].data_ptr()), H, hip._p(d["v"]), hip._p(ctx), 2 * H,
                                               NULL, 0, hip._p(attw), rows, T, H, hip._p(ws), clips, hip._p(plan[0]), hip._p(plan[1]), hip._p(plan[2]), clips, s), "attn fwd rows")
    torch.cuda.synchronize()
    return attw, ctx


def _check_fwd(name, c, s, attw, ctx):
    f = c["fwd"][s]
    assert not (attw == 7.0).any() and not (ctx == 7.0).any(), f"{name}: an output element was not written"
    fa = _frac(f"{name} attw", attw, f["attw"], f["attw_bound"])
    fc = _frac(f"{name} ctx", ctx, f["ctx"], f["ctx_bound"])
    assert fa <= 1.0 and fc <= 1.0, (name, fa, fc)


@pytest.mark.parametrize("regime", oracle.REGIMES)
@pytest.mark.parametrize("H,T,B,split", [(32, 41, 3, False), (256, 61, 5, False), (256, 61, 5, True)])
def test_attention_forward_step(dev, regime, H, T, B, split):
    """a2s_attn_step_fwd: one workgroup per clip (attn_step_fwd), and with the workspace the split-T sweep + combine."""
    from piano_a2s_amd import hip
    c = _case(regime, H, T, B, B, 3)
    d = _device_inputs(dev, c)
    ws = hip.attn_workspace(B, T, H, dev) if split else None
    for s in (0, 1):                                   # twice: the workspace's arrival counters are back at zero
        attw, ctx = _fwd_plain(dev, d, s, B, T, H, ws)
        _check_fwd(f"fwd {regime} H{H} T{T} B{B} split={split} step {s}", c, s, attw, ctx)


@pytest.mark.parametrize("regime", oracle.REGIMES)
@pytest.mark.parametrize("groups", [1, 3])
def test_attention_forward_fused_rows(dev, regime, groups):
    """a2s_attn_step_fwd_rows at hidden 256: attn_fwd_split256 (one row per clip) and attn_fwd_split256_mq (three), each as the one-round-trip `_deep` sweep
    (attn_deep 24: five active clips are below it) and as the plain sweep (attn_deep 0), the plain one also with non-temporal loads (attn_nt 1)."""
    from piano_a2s_amd import hip
    H, T, clips = 256, 61, 5
    rows = groups * clips
    c = _case(regime, H, T, rows, clips, 3)
    d = _device_inputs(dev, c)
    ws = hip.attn_workspace(clips, T, H, dev, groups=groups)
    for deep in (24, 0):
        for nt in (64, 1):
            with _switch(attn_deep=deep, attn_nt=nt):
                attw, ctx = _fwd_rows(dev, d, 0, rows, clips, T, H, ws)
            _check_fwd(f"fwd rows {regime} groups {groups} attn_deep={deep} attn_nt={nt}", c, 0, attw, ctx)


def _saturated_cap(c, which):
    """The a-priori size of a gradient through a saturated unit (the clamp fired, so |k~ + q~| >= 9 inside the domain): sech^2 <= 4 exp(-18) there, also as
    sech2_ek evaluates it (for P = exp(-18) the sum 1 + P rounds to 1 and the result is 0; for P = exp(18) it is 4 / P to a few ulp)."""
    K, qs, v, ds = c["K"], c["qs"], c["v"], np.abs(c["bwd"]["ds"])
    clips = K.shape[0]
    s2 = 4 * np.exp(-18.0) * (1 + 1e-3)
    if which == "dK":
        per_clip = np.zeros((clips, K.shape[1]))
        np.add.at(per_clip, np.arange(ds.shape[1]) % clips, ds.sum(axis=0))
        return (np.abs(K) > oracle.CLAMP), per_clip[:, :, None] * np.abs(v) * s2
    return (np.abs(qs) > oracle.CLAMP), ds.sum(axis=2)[:, :, None] * np.abs(v) * s2


def _check_bwd(name, regime, c, got):
    b, auto = c["bwd"], c["auto"]
    fr = {k: _frac(f"{name} {k}", got[k], auto[k], b[k + "_bound"]) for k in ("ds", "dq", "dK", "dv")}
    assert max(fr.values()) <= 1.0, (name, fr)
    if regime.endswith("_beyond"):
        which = "dK" if regime == "keys_beyond" else "dq"
        sat, cap = _saturated_cap(c, which)
        assert sat.any() and cap[sat].max() <= 1e-7, "the data keep the saturated gradients below 1e-7 a priori"
        g = got[which].detach().cpu().double().numpy()
        worst = float(np.abs(g[sat]).max())
        _log(f"{name} {which} through the {int(sat.sum())} saturated units: max {worst:.3e} (a-priori cap {cap[sat].max():.3e})")
        assert np.isfinite(g).all() and worst <= 1e-7


def _dk_dv(dev, d, q_all, ds_all, clips, T, S, H, groups, until=None):
    from piano_a2s_amd import hip
    L = hip.lib()
    dK = torch.zeros(clips, T, H, device=dev)
    nblk = L.a2s_attn_dk_blocks(clips, T)
    dvp = torch.zeros(nblk, H, device=dev)
    hip.check(L.a2s_attn_dk_accum(hip.stream(), hip._p(d["keys"]), hip._p(q_all), hip._p(ds_all), hip._p(d["v"]), hip._p(dK), hip._p(dvp), clips, T, S, H, hip._p(until), groups), "dk")
    dv = torch.zeros(H, device=dev)
    hip.check(L.a2s_col_sum(hip.stream(), hip._p(dvp), H, hip._p(dv), nblk, H, hip.f32(1.0), hip.f32(0.0), NULL, 0), "col_sum")
    torch.cuda.synchronize()
    return dK, dv


@pytest.mark.parametrize("regime", oracle.REGIMES)
@pytest.mark.parametrize("H,T,B,split", [(32, 41, 3, False), (256, 61, 5, False), (256, 61, 5, True)])
def test_attention_backward_step_and_deferred_keys(dev, regime, H, T, B, split):
    """a2s_attn_step_bwd over S = 3 steps (dq, ds), then a2s_attn_dk_accum on the ds it wrote (dK, dv) as attn_dk_accum_ahead and as attn_dk_accum."""
    from piano_a2s_amd import hip
    L = hip.lib()
    S = 3
    c = _case(regime, H, T, B, B, S)
    d = _device_inputs(dev, c)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)
    attw, ctx = t(c["bwd"]["attw"]), t(c["bwd"]["ctx"])
    ws = hip.attn_workspace(B, T, H, dev) if split else None
    dq, ds = torch.full((S, B, H), 7.0, device=dev), torch.full((S, B, T), 7.0, device=dev)
    for s in range(S):
        hip.check(L.a2s_attn_step_bwd(hip.stream(), hip._p(d["keys"]), hip._p(d["enc"]), C.c_void_p(d["qs"][s].data_ptr()), H, hip._p(d["v"]),
                                      C.c_void_p(attw[s].data_ptr()), C.c_void_p(ctx[s].data_ptr()), 2 * H, C.c_void_p(d["dctx"][s].data_ptr()), 2 * H, NULL, 0, NULL, 0,
                                      C.c_void_p(dq[s].data_ptr()), H, C.c_void_p(ds[s].data_ptr()), B, T, H, hip._p(ws)), "attn bwd")
    torch.cuda.synchronize()
    assert not (dq == 7.0).any() and not (ds == 7.0).any()
    for fast in (1, 0):
        n0 = L.a2s_debug_get(b"attn_dk_ahead_launches")
        with _switch(attn_deferred_fast=fast):
            dK, dv = _dk_dv(dev, d, d["qs"], ds, B, T, S, H, 1)
        assert L.a2s_debug_get(b"attn_dk_ahead_launches") - n0 == fast, "which deferred kernel ran"
        _check_bwd(f"bwd {regime} H{H} T{T} B{B} split={split} deferred_fast={fast}", regime, c, dict(dq=dq, ds=ds, dK=dK, dv=dv))


@pytest.mark.parametrize("regime", oracle.REGIMES)
@pytest.mark.parametrize("groups", [1, 3])
def test_attention_backward_fused_rows(dev, regime, groups):
    """a2s_attn_step_bwd_rows at hidden 256 (attn_bwd_split256 and its several-rows form; with and without non-temporal loads), then the deferred dK / dv
    over the fused rows, both kernels."""
    from piano_a2s_amd import hip
    L = hip.lib()
    H, T, clips, S = 256, 61, 5, 3
    rows = groups * clips
    c = _case(regime, H, T, rows, clips, S)
    d = _device_inputs(dev, c)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)
    attw, ctx = t(c["bwd"]["attw"]), t(c["bwd"]["ctx"])
    ws = hip.attn_workspace(clips, T, H, dev, groups=groups)
    plan = _row_plan(dev, rows, clips)
    until = plan[2]
    for nt in (64, 1):
        dq, ds = torch.full((S, rows, H), 7.0, device=dev), torch.full((S, rows, T), 7.0, device=dev)
        dctx_out = torch.full((S, rows, 2 * H), 7.0, device=dev)
        with _switch(attn_nt=nt):
            for s in range(S):
                hip.check(L.a2s_attn_step_bwd_rows(hip.stream(), hip._p(d["keys"]), hip._p(d["enc"]), C.c_void_p(d["qs"][s].data_ptr()), H, hip._p(d["v"]),
                                                   C.c_void_p(attw[s].data_ptr()), C.c_void_p(ctx[s].data_ptr()), 2 * H, C.c_void_p(d["dctx"][s].data_ptr()), 2 * H, NULL, 0,
                                                   C.c_void_p(dctx_out[s].data_ptr()), 2 * H, C.c_void_p(dq[s].data_ptr()), H, C.c_void_p(ds[s].data_ptr()), rows, T, H,
                                                   hip._p(ws), clips, hip._p(plan[0]), hip._p(plan[1]), hip._p(plan[2]), clips, s), "attn bwd rows")
            torch.cuda.synchronize()
        assert not (dq == 7.0).any() and not (ds == 7.0).any()
        for fast in (1, 0):
            with _switch(attn_deferred_fast=fast):
                dK, dv = _dk_dv(dev, d, d["qs"], ds, clips, T, S, H, groups, until)
            _check_bwd(f"bwd rows {regime} groups {groups} attn_nt={nt} deferred_fast={fast}", regime, c, dict(dq=dq, ds=ds, dK=dK, dv=dv))


# ---------------------------------------------------------------------------------------------------------------- d. through the decoders
_LAYERS = ("decoder.attn", "decoder.upper_decoder.attn", "decoder.lower_decoder.attn")
_MODEL = dict(freq_bins=24, conv_feature_size=48, hidden_size=256, max_length=(12, 8))
# regime -> (max |K| of the float64 oracle, limit on attn_range.query_bound)
_TARGETS = {"both": (40.0, 43.0), "keys_beyond": (60.0, 34.0), "outside": (60.0, 50.0)}


def _model_batch(cfg):
    from piano_a2s_amd import synthetic
    return synthetic.make_batch(3, cfg, 6, frames=37, upper_range=(3, 10), lower_range=(2, 7), full_tail=0.1)


def _oracle_keys(st, cfg, spectrogram, training):
    """{layer: K (B, T, H) float64} of the float64 oracle's encoder on these weights."""
    from oracle import model_ref
    from piano_a2s_amd import spec
    P, Bf = spec.split_state(st)
    P = {k: v.double() for k, v in P.items()}
    Bf = {k: (v.clone().double() if v.is_floating_point() else v.clone()) for k, v in Bf.items()}
    H = cfg["hidden_size"]
    with torch.no_grad():
        enc, _ = model_ref.encoder_forward(model_ref.convstack_forward(spectrogram.double(), P, Bf, training, dropout=False), P)
        return {p: enc @ P[p + ".attn.weight"][:, 2 * H:].t() for p in _LAYERS}


def _range_state(cfg, spectrogram, regime, training, exact_query_bound=False):
    """The procedural weights with the three attention Linears rescaled: the key half so that the float64 oracle's max |K| on this input is the regime's
    target, the query half and the bias so that attn_range.query_bound is just below (exact_query_bound: at) its limit."""
    from piano_a2s_amd import attn_range, spec
    k_target, q_limit = _TARGETS[regime]
    st = spec.procedural_state(cfg, 31, eos_bias=2.0, lively=True)
    H = cfg["hidden_size"]
    K = _oracle_keys(st, cfg, spectrogram, training)
    for p in _LAYERS:
        W, b = st[p + ".attn.weight"], st[p + ".attn.bias"]
        W[:, 2 * H:] *= k_target / float(K[p].abs().max())
        f = (1.0 if exact_query_bound else 0.999) * q_limit / float(attn_range.query_bound(W.double(), b.double(), H))
        W[:, :2 * H] *= f
        b *= f
    got = {p: float(k.abs().max()) for p, k in _oracle_keys(st, cfg, spectrogram, training).items()}
    assert all(abs(v - k_target) < 1e-3 * k_target for v in got.values()), got
    assert all(float(attn_range.query_bound(st[p + ".attn.weight"].double(), st[p + ".attn.bias"].double(), H)) <= q_limit * (1 + 1e-6) for p in _LAYERS)
    return st


_MODEL_REF = {}


def _model_reference(regime):
    """Outputs and all gradients of the CPU oracle in float64, and the deviation of its float32 evaluation from them (what an fp32 evaluation may lose by
    itself), teacher forcing 1.0, train mode, no dropout; computed once per regime."""
    if regime in _MODEL_REF:
        return _MODEL_REF[regime]
    from oracle import model_ref, recipe_ref
    from piano_a2s_amd import spec
    cfg = spec.default_cfg(**_MODEL)
    batch = _model_batch(cfg)
    st = _range_state(cfg, batch[0], regime, training=True)
    res = {}
    for dt in (torch.float64, torch.float32):
        P, Bf = spec.split_state(st)
        P = {k: v.to(dt).clone().requires_grad_(True) for k, v in P.items()}
        Bf = {k: (v.clone().to(dt) if v.is_floating_point() else v.clone()) for k, v in Bf.items()}
        outs = model_ref.forward(P, Bf, cfg, batch[0].to(dt), inference=False, ground_truth=[batch[i] for i in range(1, 7)], teacher_forcing_ratio=1.0,
                                 training=True, rng=random.Random(5), dropout=False)
        loss = recipe_ref.objectives(outs, (batch[1], batch[2], batch[3], batch[5]))[0]
        loss.backward()
        res[dt] = ([o.detach().double() for o in outs], {k: p.grad.double() for k, p in P.items()}, float(loss.detach()))
    o64, g64, l64 = res[torch.float64]
    o32, g32, _ = res[torch.float32]
    dev_out = max(float((a - b).abs().max()) for a, b in zip(o64, o32))
    dev_grad = max(float((g32[k] - g64[k]).abs().max()) / max(float(g64[k].abs().max()), 1e-12) for k in g64)
    _log(f"model {regime}: float32 CPU oracle against float64: outputs {dev_out:.3e}, gradients {dev_grad:.3e} (relative to each tensor's max)")
    _MODEL_REF[regime] = dict(cfg=cfg, batch=batch, st=st, outs=o64, grads=g64, loss=l64, out_bar=max(1e-4, 3 * dev_out), grad_bar=max(2e-4, 3 * dev_grad))
    return _MODEL_REF[regime]


def _loss_grads(outs, batch, dev):
    """d(total loss)/d(outputs) with the reference's objective (pretrain.py:72-88), evaluated by torch on the device."""
    leaves = [o.detach().clone().requires_grad_(True) for o in outs]
    nll, nll_pad = torch.nn.NLLLoss(), torch.nn.NLLLoss(ignore_index=147)
    ts_t, key_t, up_t, lo_t = batch[1].to(dev), batch[2].to(dev), batch[3].to(dev), batch[5].to(dev)
    ts_o, key_o, up_o, lo_o = leaves
    total = (nll(ts_o.permute(0, 2, 1), ts_t) + nll(key_o.permute(0, 2, 1), key_t)
             + nll_pad(up_o.view(-1, up_o.shape[2], up_o.shape[3]).permute(0, 2, 1), up_t.view(-1, up_t.shape[2]))
             + nll_pad(lo_o.view(-1, lo_o.shape[2], lo_o.shape[3]).permute(0, 2, 1), lo_t.view(-1, lo_t.shape[2])))
    total.backward()
    return float(total.detach()), [l.grad for l in leaves]


def _compare_model(tag, ref, outs, grads, live=None):
    """outs: the four device outputs (B, bars, ...); grads: {name: device gradient}; live: optional masks of the staff outputs' rows that reach the loss."""
    worst_o = 0.0
    for i, (name, o, r) in enumerate(zip(("ts", "key", "up", "lo"), outs, ref["outs"])):
        d = (o.detach().cpu().double() - r).abs()
        if live is not None and i >= 2:
            d = d[live[i - 2]]
        assert torch.isfinite(d).all(), name
        worst_o = max(worst_o, float(d.max()))
    errs = {k: float((grads[k].detach().cpu().double() - rg).abs().max()) / max(float(rg.abs().max()), 1e-12) for k, rg in ref["grads"].items()}
    worst_k = max(errs, key=errs.get)
    _log(f"model {tag}: outputs {worst_o:.3e} (bar {ref['out_bar']:.3e}), gradients {errs[worst_k]:.3e} at {worst_k} (bar {ref['grad_bar']:.3e}); "
         f"attention Linears: " + ", ".join(f"{errs[p + '.attn.weight']:.2e}" for p in _LAYERS))
    assert worst_o <= ref["out_bar"], (tag, worst_o)
    bad = [(k, e) for k, e in errs.items() if not e <= ref["grad_bar"]]
    assert not bad, (tag, bad[:6])


@pytest.mark.parametrize("regime", ["both", "keys_beyond"])
def test_decoders_at_large_pre_activations(dev, regime, decoder_path):
    """The whole model at hidden 256 with max |K| = 40 / 60 (3 clips, 37 frames, teacher forcing 1.0, train mode, no dropout) against the float64 oracle,
    outputs and all 83 gradients, through the persistent decoder, the few-row step kernels and the bulk loop."""
    from piano_a2s_amd import engine, engine_bwd
    ref = _model_reference(regime)
    cfg, batch = ref["cfg"], ref["batch"]
    S = {k: v.to(dev) for k, v in ref["st"].items()}
    eng = engine.Engine(cfg)
    outs = eng.forward(S, batch[0].to(dev), inference=False, ground_truth=[b.to(dev) for b in batch[1:7]], teacher_forcing_ratio=1.0, training=True,
                       dropout=False, rng=random.Random(5))
    decoder_path(eng)
    loss, gouts = _loss_grads(outs, batch, dev)
    assert abs(loss - ref["loss"]) <= ref["out_bar"] * abs(ref["loss"])
    G = engine_bwd.backward(eng, S, gouts)
    torch.cuda.synchronize()
    _compare_model(f"{regime} [{decoder_path.name}]", ref, outs, G)


@pytest.mark.parametrize("regime", ["both", "keys_beyond"])
def test_fused_step_with_pair_sweeps_at_large_pre_activations(dev, regime):
    """The same model and batch through the fused training step with ONE attention sweep per decode step for both staves (attn_fwd_split256_pair /
    attn_bwd_split256_pair; the library's pair counters prove it): the 15 rows of the five teacher-forced bars are one segment, the few-row hand-over is
    lowered to 1 row and the persistent decoder is off so that the pair loop takes every step.  Outputs where they reach the loss, all gradients."""
    import models
    from piano_a2s_amd import hip, train
    from piano_a2s_amd.spec import PAD
    L = hip.lib()
    ref = _model_reference(regime)
    cfg, batch = ref["cfg"], ref["batch"]
    m = models.ScoreTranscription(**cfg)
    m.load_state_dict(ref["st"])
    m = m.to(dev).train()
    with _switch(attn_pair_fused_rows=1, dec_persist=0):
        step = train.TrainStep(m, dropout=False, clip_groups=False)
        step.keep_grads = True
        n0, nb0 = L.a2s_debug_get(b"attn_pair_launches"), L.a2s_debug_get(b"attn_pair_bwd_launches")
        step([b.to(dev) if torch.is_tensor(b) else b for b in batch], 1.0, rng=random.Random(5))
        torch.cuda.synchronize()
        pair = (L.a2s_debug_get(b"attn_pair_launches") - n0, L.a2s_debug_get(b"attn_pair_bwd_launches") - nb0)
    _log(f"model {regime} [fused step]: pair sweeps forward / backward {pair}")
    assert pair[0] > 0 and pair[1] == pair[0], pair
    live = [(batch[3] != PAD), (batch[5] != PAD)]
    _compare_model(f"{regime} [fused step, pair sweeps]", ref, step.last_outputs, step.last_grads, live)


# ---------------------------------------------------------------------------------------------------------------- e. the guard
@pytest.fixture(scope="module")
def outside():
    """The model of (d) in eval mode with max |K| = 60 and attn_range.query_bound = 50 in all three attention layers: outside the domain."""
    from piano_a2s_amd import spec
    cfg = spec.default_cfg(**_MODEL)
    batch = _model_batch(cfg)
    return cfg, batch, _range_state(cfg, batch[0], "outside", training=False, exact_query_bound=True)


@pytest.fixture()
def raising(monkeypatch):
    """attn_range in its default mode, whatever an earlier test left."""
    from piano_a2s_amd import attn_range
    monkeypatch.setattr(attn_range, "on_violation", "raise")
    monkeypatch.setattr(attn_range, "_warned", False)
    return attn_range


# the image saturates at the clamp, so a layer whose keys reach 60 reads 43, "this or more"; the query bound is the number the weights give
_MESSAGE = r"decoder\.attn: max \|k\| = 43 \(saturated: this or more\), bound on \|q\| = 50\b"


@pytest.mark.parametrize("entry", ["greedy", "beam", "grammar", "align"])
def test_guard_raises_outside_the_domain(dev, outside, raising, entry):
    from piano_a2s_amd import engine, hip
    from piano_a2s_amd.kern_grammar import KernGrammar
    cfg, batch, st = outside
    eng = engine.Engine(cfg)
    if entry == "beam":
        eng.beam_size = 2
    elif entry == "grammar":
        eng.kern_grammar = KernGrammar()
    elif entry == "align":
        eng.alignment = True
    with pytest.raises(hip.A2SError, match=_MESSAGE) as info:
        eng.forward({k: v.to(dev) for k, v in st.items()}, batch[0].to(dev), inference=True)
    torch.cuda.synchronize()
    assert "upper_decoder.attn" in str(info.value) and "lower_decoder.attn" in str(info.value)
    k, q = eng.attn_ranges["decoder.attn"]
    assert abs(k - 43.0) < 1e-3 and abs(q - 50.0) < 1e-3


def test_guard_raises_in_the_teacher_forced_eval_pass(dev, outside, raising):
    """Engine.forward with training=False and ground truth: no decoder call reads anything back, the pass reads its ranges at its end."""
    from piano_a2s_amd import engine, hip
    cfg, batch, st = outside
    with pytest.raises(hip.A2SError, match=_MESSAGE):
        engine.Engine(cfg).forward({k: v.to(dev) for k, v in st.items()}, batch[0].to(dev), inference=False, ground_truth=[b.to(dev) for b in batch[1:7]],
                                   teacher_forcing_ratio=1.0, training=False)
    torch.cuda.synchronize()


def test_guard_raises_in_the_recipe_validation_stage_and_in_transcribe(dev, outside, raising):
    import types
    import models
    from piano_a2s_amd import hip, recipe, spec, transcribe
    cfg, batch, st = outside
    m = models.ScoreTranscription(**cfg)
    m.load_state_dict(st)
    brain = object.__new__(recipe.ASR)                                   # the stage's forward alone: no run, no loaders
    brain.device, brain.modules, brain.hparams, brain._synthetic_room = str(dev), types.SimpleNamespace(transcription=m.to(dev).eval()), types.SimpleNamespace(), None
    with pytest.raises(hip.A2SError, match=_MESSAGE):
        with torch.no_grad():
            brain.compute_forward(list(batch), recipe.sb.Stage.VALID)
    # transcribe: the small model at the VQT's 480 bins; the key halves scaled until the image saturates on any input, the query bound set to 50
    small = dict(conv_feature_size=32, hidden_size=32, max_length=(12, 8))
    scfg = spec.default_cfg(**small)
    sst = spec.procedural_state(scfg, 11, eos_bias=3.0, lively=True)
    H = 32
    for p in _LAYERS:
        W, b = sst[p + ".attn.weight"], sst[p + ".attn.bias"]
        W[:, 2 * H:] *= 1e3
        f = 50.0 / float(raising.query_bound(W.double(), b.double(), H))
        W[:, :2 * H] *= f
        b *= f
    sm = models.ScoreTranscription(**small)
    sm.load_state_dict(sst)
    hp = dict(sample_rate=16000, hop_length=160, max_frame_num=1201, max_bars=5, bins_per_octave=60, n_octaves=8, gamma=20)
    tt = np.arange(16000 * 3) / 16000.0
    x = (0.3 * np.sin(2 * np.pi * 220.0 * tt) * np.exp(-tt)).astype(np.float32)[:, None]
    with pytest.raises(hip.A2SError, match=r"max \|k\| = 43 \(saturated: this or more\), bound on \|q\| = 50\b"):
        transcribe.transcribe_waveform(sm.to(dev).eval(), x, 16000, hparams=hp)
    torch.cuda.synchronize()


@pytest.mark.parametrize("regime", ["both", "keys_beyond"])
def test_guard_passes_inside_the_domain(dev, raising, regime):
    """The weights of (d), rescaled on the eval-mode encoder (BatchNorm's running statistics give other keys than the batch's): max |K| = 40 with the query
    bound just below 43, max |K| = 60 with it just below 34 -- both inside; the readings are what the float64 oracle says."""
    from piano_a2s_amd import engine, spec
    cfg = spec.default_cfg(**_MODEL)
    batch = _model_batch(cfg)
    st = _range_state(cfg, batch[0], regime, training=False)
    eng = engine.Engine(cfg)
    outs = eng.forward({k: v.to(dev) for k, v in st.items()}, batch[0].to(dev), inference=True)
    torch.cuda.synchronize()
    assert all(torch.isfinite(o).all() for o in outs)
    k_target, q_limit = _TARGETS[regime]
    for p in _LAYERS:
        k, q = eng.attn_ranges[p]
        _log(f"guard {regime} {p}: max |k| read {k:.4f} (float64 oracle {k_target:g}), bound on |q| {q:.4f}")
        assert abs(k - min(k_target, 43.0)) <= 1e-3 * k_target + 2 * 2e-6 * 256 * k_target and 0.99 * q_limit <= q <= q_limit


def test_guard_passes_the_small_fixture(golden_dir, dev, raising):
    import json
    from piano_a2s_amd import engine, spec, synthetic
    meta = json.load(open(os.path.join(golden_dir, "g1_small.json")))
    cfg = spec.default_cfg(**meta["cfg"])
    case = meta["cases"]["greedy_s11"]
    batch = synthetic.make_batch(3, cfg, meta["batch_seed"], frames=41, upper_range=(3, 10), lower_range=(2, 7), full_tail=0.1)
    S = {k: v.to(dev) for k, v in spec.procedural_state(cfg, case["weights_seed"], eos_bias=case["eos_bias"], lively=True).items()}
    eng = engine.Engine(cfg)
    eng.forward(S, batch[0].to(dev), inference=True)
    torch.cuda.synchronize()
    assert set(eng.attn_ranges) == set(_LAYERS) and all(raising.in_domain(k, q) for k, q in eng.attn_ranges.values()), eng.attn_ranges
    # a training pass is not guarded: nothing is enqueued, nothing is read
    eng.attn_ranges = None
    eng.forward(S, batch[0].to(dev), inference=False, ground_truth=[b.to(dev) for b in batch[1:7]], teacher_forcing_ratio=1.0, training=True, dropout=False)
    torch.cuda.synchronize()
    assert eng.attn_ranges is None and eng._attn_range_pending is None


def test_warning_mode_returns_outputs_and_warns_once(dev, outside, raising, monkeypatch):
    from piano_a2s_amd import engine
    cfg, batch, st = outside
    monkeypatch.setattr(raising, "on_violation", "warn")
    S = {k: v.to(dev) for k, v in st.items()}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(2):
            outs = engine.Engine(cfg).forward(S, batch[0].to(dev), inference=True)
            torch.cuda.synchronize()
            assert len(outs) == 4 and all(torch.isfinite(o).all() for o in outs)
    mine = [w for w in caught if "key image's domain" in str(w.message)]
    assert len(mine) == 1 and issubclass(mine[0].category, RuntimeWarning) and "bound on |q| = 50" in str(mine[0].message)
