"""The additive attention tanh(K + q) in float64 with the a-priori fp32 error bounds of its key-image evaluation (csrc/a2s_common.h: exp2x_clamped,
tanh_ek, sech2_ek), the data patterns that take it to the edges of its domain (piano_a2s_amd/attn_range.py), and an fp32 numpy emulation of the
three-instruction formula that tests/test_attn_range_cpu.py holds against the bounds.  numpy only.

The bounds.  k~, q~ are the values after the clamp to +-43, P = exp(2 (k~ + q~)), U = 2^-24.
  image entry     rho(x) = 2^-23 + |x| 2^-22  relative, |x| <= 43:  __expf(y) is exp2(y * log2e); the constant and the product each round by U, a relative error
                  d of exp2's argument a is a relative error a d ln2 of its value, a ln2 = y, so at most |y| 2^-23; v_exp_f32 adds one ulp (2^-23); y = 2 x
                  (the doubling itself is exact).
  energy          |tanh_ek - tanh(k + q)| <= 0.5 (rho(k~) + rho(q~) + U) + 7 U + 2 exp(-2 |k~ + q~|) [clamp fired]:  tanh = 1 - 2 / (1 + P) and
                  |P d/dP| of it is 2 P / (1 + P)^2 <= 0.5; 7 U covers the fma rounding of 1 + p and the 1-ulp rcp (both scaled by 2 / (1 + P) <= 2) and
                  the final fma; where the clamp fired both tanh(k + q) and tanh(k~ + q~) are within 2 exp(-2 |k~ + q~|) of the same +-1 inside the domain.
  sech2_ek        0.4 (rho(k~) + rho(q~) + U) + 2^-20:  |P d/dP (4 P / (1 + P)^2)| <= 0.39; 2^-20 covers the rcp, the subtraction from 1 and the two
                  products (and 4 exp(-18) = 6.1e-8 where the clamp fired).
  scores          ds = sum_j |v_j| (energy bound) + H U sum_j |v_j|  (an fp32 dot product of H terms of magnitude <= |v_j|, any order).
  weights         a_ref expm1(2 max_t ds) + 2e-5 max a_ref:  a softmax whose scores move by at most ds moves by that factor; the second term is the bar
                  test_gpu_ops.py::test_attention_step applies to the softmax and context arithmetic, which nothing here touches.
  context         the weight bound through sum_t |enc|.
  ds, dq, dK, dv  the same propagation with the sech2 bound (dv: the energy bound), each plus 5e-5 max |reference|, the bar the backward tests of
                  test_gpu_bwd_ops.py apply to their reductions."""
import numpy as np

U = 2.0 ** -24
CLAMP, ONE_SIDED = 43.0, 34.0
SOFTMAX_BAR, REDUCTION_BAR = 2e-5, 5e-5


def clamp(x):
    return np.clip(np.asarray(x, dtype=np.float64), -CLAMP, CLAMP)


def rho(x):
    """Bound on the relative error of exp2x_clamped at a pre-activation x, |x| <= 43."""
    return 2.0 ** -23 + np.abs(np.asarray(x, dtype=np.float64)) * 2.0 ** -22


def _fired(k, q):
    return (np.abs(k) > CLAMP) | (np.abs(q) > CLAMP)


def energy(k, q, with_bound=False):
    """tanh(k + q) in float64 (k, q broadcast); with_bound: also the bound on |tanh_ek(E_K, E_q) - tanh(k + q)|."""
    k, q = np.asarray(k, dtype=np.float64), np.asarray(q, dtype=np.float64)
    e = np.tanh(k + q)
    if not with_bound:
        return e
    kc, qc = clamp(k), clamp(q)
    b = 0.5 * (rho(kc) + rho(qc) + U) + 7 * U + 2.0 * np.exp(-2.0 * np.abs(kc + qc)) * _fired(k, q)
    return e, b


def sech2(k, q, with_bound=False):
    """1 - tanh^2(k + q) in float64; with_bound: also the bound on |sech2_ek(E_K, E_q) - it|."""
    k, q = np.asarray(k, dtype=np.float64), np.asarray(q, dtype=np.float64)
    s = 1.0 / np.cosh(np.minimum(np.abs(k + q), 350.0)) ** 2
    if not with_bound:
        return s
    kc, qc = clamp(k), clamp(q)
    return s, 0.4 * (rho(kc) + rho(qc) + U) + 2.0 ** -20 + 0.0 * s


def in_domain(k, q):
    k, q = np.abs(k), np.abs(q)
    return ((k <= CLAMP) & (q <= CLAMP)) | (np.minimum(k, q) <= ONE_SIDED)


# ---- the kernels' arithmetic, emulated in numpy float32 (each operation computed in float64 and rounded once: the products of two fp32 numbers are
# exact in float64, so this is an fma)
def image_fp32(x):
    """exp2x_clamped with a correctly rounded exp."""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(2.0 * clamp(np.asarray(x, dtype=np.float32))).astype(np.float32)


def tanh_ek_fp32(ek, eq):
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        p = (ek.astype(np.float64) * eq.astype(np.float64) + 1.0).astype(np.float32)
        r = (1.0 / p.astype(np.float64)).astype(np.float32)                 # rcp(inf) = 0
        return (1.0 - 2.0 * r.astype(np.float64)).astype(np.float32)


def sech2_ek_fp32(ek, eq):
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        p = (ek.astype(np.float64) * eq.astype(np.float64) + 1.0).astype(np.float32)
        r = (1.0 / p.astype(np.float64)).astype(np.float32)
        return ((np.float32(4.0) * r) * (np.float32(1.0) - r)).astype(np.float32)


# ---- one attention layer over fused rows: row r reads clip r % clips
def forward(K, q, v, enc, with_bound=False):
    """K (clips, T, H), q (R, H), v (H,), enc (clips, T, C) -> dict(attw (R, T), ctx (R, C)) in float64; with_bound: also attw_bound, ctx_bound."""
    K, q, v, enc = (np.asarray(a, dtype=np.float64) for a in (K, q, v, enc))
    clips, T, H = K.shape
    R = q.shape[0]
    Kr, encr = K[np.arange(R) % clips], enc[np.arange(R) % clips]
    e, eb = energy(Kr, q[:, None, :], with_bound=True)
    s = e @ v
    a = np.exp(s - s.max(axis=1, keepdims=True))
    a /= a.sum(axis=1, keepdims=True)
    out = dict(attw=a, ctx=np.einsum("rt,rtc->rc", a, encr), energy=e)
    if with_bound:
        ds = eb @ np.abs(v) + H * U * np.abs(v).sum()
        out["score_bound"] = ds
        out["attw_bound"] = a * np.expm1(2.0 * ds.max(axis=1, keepdims=True)) + SOFTMAX_BAR * a.max(axis=1, keepdims=True)
        out["ctx_bound"] = np.einsum("rt,rtc->rc", out["attw_bound"], np.abs(encr))
    return out


def backward(K, qs, v, enc, dctxs, live=None):
    """S steps through one layer, loss = sum_s sum_r live[s, r] <ctx_s[r], dctx_s[r]>.  qs (S, R, H), dctxs (S, R, C), live (S, R) 0/1 or None.
    -> float64 dict: attw, ctx (S, R, .) (zero on dead rows), ds (S, R, T) the score gradients, dq (S, R, H), dK (clips, T, H), dv (H,), and the
    bound of each gradient as name + "_bound" -- for kernels that take attw and ctx of the reference (rounded to fp32) and, in the deferred dK / dv
    kernels, the ds the step kernel wrote."""
    K, qs, v, enc, dctxs = (np.asarray(a, dtype=np.float64) for a in (K, qs, v, enc, dctxs))
    S, R, H = qs.shape
    clips, T, _ = K.shape
    live = np.ones((S, R)) if live is None else np.asarray(live, dtype=np.float64)
    rows = np.arange(R) % clips
    encr, Kr = enc[rows], K[rows]
    av = np.abs(v)
    o = {k: [] for k in ("attw", "ctx", "ds", "ds_bound", "dq", "dq_bound")}
    dK, dKb, dv, dvb = np.zeros((clips, T, H)), np.zeros((clips, T, H)), np.zeros(H), np.zeros(H)
    per_step = []
    for s in range(S):
        f = forward(K, qs[s], v, enc)
        a, e = f["attw"], f["energy"]
        g = np.einsum("rc,rtc->rt", dctxs[s], encr)
        ds = a * (g - (a * g).sum(axis=1, keepdims=True)) * live[s][:, None]
        per_step.append((ds, e))
        o["attw"].append(a * live[s][:, None]); o["ctx"].append(f["ctx"] * live[s][:, None]); o["ds"].append(ds)
    ds_all = np.stack(o["ds"])
    eds = REDUCTION_BAR * np.abs(ds_all).max()                     # bound on every entry of ds: one bar over the whole tensor, as the tests measure it
    for s in range(S):
        ds, e = per_step[s]
        s2, s2b = sech2(Kr, qs[s][:, None, :], with_bound=True)
        _, eb = energy(Kr, qs[s][:, None, :], with_bound=True)
        ads = np.abs(ds)
        o["dq"].append(np.einsum("rt,rth->rh", ds, s2) * v)
        o["dq_bound"].append((np.einsum("rt,rth->rh", ads, s2b) + eds * s2.sum(axis=1) * live[s][:, None]) * av)
        o["ds_bound"].append(np.full_like(ds, eds))
        lv = live[s][:, None, None]
        np.add.at(dK, rows, ds[:, :, None] * s2 * v)
        np.add.at(dKb, rows, (ads[:, :, None] * s2b + eds * s2 * lv) * av)
        dv += np.einsum("rt,rth->h", ds, e)
        dvb += np.einsum("rt,rth->h", ads, eb) + eds * (np.abs(e) * lv).sum(axis=(0, 1))
    out = {k: np.stack(val) for k, val in o.items()}
    out["dq_bound"] += REDUCTION_BAR * np.abs(out["dq"]).max()
    out.update(dK=dK, dK_bound=dKb + REDUCTION_BAR * np.abs(dK).max(), dv=dv, dv_bound=dvb + REDUCTION_BAR * np.abs(dv).max())
    return out


# ---- data
REGIMES = ("both", "keys_beyond", "queries_beyond", "benign")


def _grid(rng, lo, hi, shape):
    """Multiples of 1/8 in [lo, hi]: exact in fp32 and in three bf16 terms (|x| * 8 < 2^9)."""
    return rng.integers(int(lo * 8), int(hi * 8) + 1, size=shape).astype(np.float64) / 8.0


def patterns(regime, T, H, rows, clips=None, steps=1, seed=0):
    """K (clips, T, H) and q (rows, H) (steps > 1: (steps, rows, H)) on a grid of 1/8; row r reads clip r % clips (clips defaults to rows).
      both            |k|, |q| <= 43 with +-43 exactly on both sides; per (t, j) either an opposite-sign pair with k + q in [-3, 3] (about half, a different
                      set for every t, so the softmax is not flat) or an independent draw (equal and opposite signs: the product E_K E_q overflows to inf,
                      underflows to 0, or is exp(0) formed as exp(86) exp(-86))
      keys_beyond     |k| up to 60 of both signs (+-60 present), |q| <= 34 (+-34 present); a quarter of the units stay within +-4
      queries_beyond  the mirror image
      benign          |x| <= 4, the control
    The generator itself asserts that every pair lies in the domain and, for `both` and `benign`, that at least a quarter of each row's (t, j) energies are
    unsaturated (|k + q| < 4): otherwise a test compares +-1 with +-1."""
    assert regime in REGIMES, regime
    clips = rows if clips is None else clips
    assert rows % clips == 0
    rng = np.random.default_rng([seed, REGIMES.index(regime), T, H, rows, clips, steps])
    S = steps
    clip_of = np.arange(rows) % clips
    if regime == "benign":
        K, q = _grid(rng, -4, 4, (clips, T, H)), _grid(rng, -4, 4, (S, rows, H))
    elif regime == "both":
        qbase = _grid(rng, -43, 43, (clips, H))
        qbase[:, 0::8] = 43.0
        qbase[:, 1::8] = -43.0
        q = np.clip(qbase[clip_of][None] + _grid(rng, -1, 1, (S, rows, H)), -43, 43)
        q[:, :, 0:2] = qbase[clip_of][None][:, :, 0:2]                             # +-43 exactly in every row
        near = np.clip(-qbase[:, None, :] + _grid(rng, -2, 2, (clips, T, H)), -43, 43)
        far = _grid(rng, -43, 43, (clips, T, H))
        far[:, 0::3, 0:2] = np.array([43.0, -43.0])                                # equal signs at the clamp: exp(86) exp(86)
        far[:, 1::3, 0:2] = np.array([-43.0, 43.0])                                # opposite signs at the clamp: exp(86) exp(-86) for tanh(0)
        pick = rng.random((clips, T, H)) < (0.35 + 0.3 * rng.random((clips, T, 1)))
        pick[:, :, 0:2] = False
        K = np.where(pick, near, far)
    else:
        big = _grid(rng, -60, 60, (clips, T, H))
        big[:, 0, 0], big[:, 0, 1] = 60.0, -60.0
        small = _grid(rng, -34, 34, (S, rows, H))
        small[:, :, 0], small[:, :, 1] = 34.0, -34.0
        quarter = (np.arange(H) % 4) == 3                                          # units that stay benign on both sides
        big[:, :, quarter] = _grid(rng, -4, 4, (clips, T, int(quarter.sum())))
        small[:, :, quarter] = _grid(rng, -4, 4, (S, rows, int(quarter.sum())))
        if regime == "keys_beyond":
            K, q = big, small
        else:
            # the mirror image: queries take the wide draw (per row and step), keys the narrow one
            wide = _grid(rng, -60, 60, (S, rows, H))
            wide[:, :, 0], wide[:, :, 1] = 60.0, -60.0
            wide[:, :, quarter] = _grid(rng, -4, 4, (S, rows, int(quarter.sum())))
            narrow = _grid(rng, -34, 34, (clips, T, H))
            narrow[:, 0, 0], narrow[:, 0, 1] = 34.0, -34.0
            narrow[:, :, quarter] = _grid(rng, -4, 4, (clips, T, int(quarter.sum())))
            K, q = narrow, wide
    for s in range(S):
        ksum = K[clip_of] + q[s][:, None, :]
        assert in_domain(K[clip_of], q[s][:, None, :]).all(), regime
        if regime in ("both", "benign"):
            frac = (np.abs(ksum) < 4).mean(axis=(1, 2))
            assert frac.min() >= 0.25, (regime, float(frac.min()))
    assert (K * 8 == np.round(K * 8)).all() and (q * 8 == np.round(q * 8)).all()
    return K, (q if steps > 1 else q[0])
