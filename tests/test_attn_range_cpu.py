"""piano_a2s_amd/attn_range.py (the domain of the key-image attention, the query bound, the key reading, the guard's report) and tests/attn_range_oracle.py
(its a-priori fp32 bounds, its data patterns), without a GPU: the float64 grid check of the domain against the module's constants, and the oracle's bounds
against an fp32 numpy emulation of the three-instruction formula on the very patterns the GPU tests run."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import attn_range_oracle as oracle                     # noqa: E402

from piano_a2s_amd import attn_range                   # noqa: E402


def test_constants_agree_with_the_oracle_and_say_why():
    assert attn_range.CLAMP == oracle.CLAMP == 43.0 and attn_range.ONE_SIDED == oracle.ONE_SIDED == 34.0
    assert attn_range.ONE_SIDED == attn_range.CLAMP - 9.0
    # exp(+-2 CLAMP) is finite and normal in fp32, and 1 - tanh(9) is what one clamped side may cost
    hi, lo = np.float32(np.exp(2 * 43.0)), np.float32(np.exp(-2 * 43.0))
    assert np.isfinite(hi) and lo >= np.finfo(np.float32).tiny
    assert abs((1 - np.tanh(9.0)) - 3.05e-8) < 1e-10


def test_float64_grid_inside_the_domain_is_exact_and_outside_is_not():
    x = np.arange(-70 * 4, 70 * 4 + 1) / 4.0
    k, q = np.meshgrid(x, x, indexing="ij")
    clamped = np.tanh(np.clip(k, -attn_range.CLAMP, attn_range.CLAMP) + np.clip(q, -attn_range.CLAMP, attn_range.CLAMP))
    err = np.abs(clamped - np.tanh(k + q))
    inside = oracle.in_domain(k, q)
    assert inside.any() and (~inside).any()
    assert err[inside].max() <= 4e-8, err[inside].max()
    assert err[~inside].max() > 0.5
    # the same split for sech2: inside, both sides are below 4 exp(-18) wherever the clamp changes anything
    s_err = np.abs(oracle.sech2(np.clip(k, -43, 43), np.clip(q, -43, 43)) - oracle.sech2(k, q))
    assert s_err[inside].max() <= 4 * np.exp(-18.0) and s_err[~inside].max() > 0.5
    # the module's scalar predicate is the oracle's array one
    for kk, qq in ((50.0, -45.0), (43.0, 43.0), (60.0, 34.0), (34.0, 70.0), (43.25, 34.25), (0.0, 0.0)):
        assert attn_range.in_domain(abs(kk), abs(qq)) == bool(oracle.in_domain(kk, qq))
    assert abs(np.tanh(43.0 - 43.0) - np.tanh(50.0 - 45.0)) > 0.99                    # the issue's example


def test_in_domain_edges():
    nxt = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))
    D = attn_range.in_domain
    assert D(43.0, 43.0) and D(0.0, 0.0) and D(43.0, 0.0)
    assert not D(nxt(43.0), 43.0) and not D(43.0, nxt(43.0))                          # both sides matter once the smaller one is above 34
    assert D(1e30, 34.0) and D(34.0, 1e30) and D(float("inf"), 34.0)                  # one side at most 34: the other one is free
    assert not D(nxt(43.0), nxt(34.0)) and not D(nxt(34.0), nxt(43.0))
    assert D(43.0, nxt(34.0)) and D(nxt(34.0), 43.0)                                  # just beyond 34 is fine while the other side is inside the clamp
    assert not D(float("nan"), 1.0) and not D(1.0, float("nan"))


def test_query_bound_and_key_range():
    g = torch.Generator().manual_seed(0)
    H = 8
    W, b = torch.randn(H, 4 * H, generator=g), torch.randn(H, generator=g)
    qb = attn_range.query_bound(W, b, H)
    assert qb.dim() == 0 and float(qb) == pytest.approx(float((W[:, :2 * H].abs().sum(1) + b.abs()).max()))
    h = torch.rand(1000, 2 * H, generator=g) * 2 - 1                                  # GRU states
    assert float((h @ W[:, :2 * H].t() + b).abs().max()) <= float(qb)
    W2 = W.clone(); W2[:, 2 * H:] *= 100                                              # the key half does not enter
    assert float(attn_range.query_bound(W2, b, H)) == float(qb)
    k = torch.tensor([[-7.5, 3.0], [0.0, 12.25]])
    assert float(attn_range.key_range(torch.exp(2 * k.double()))) == pytest.approx(12.25)
    assert float(attn_range.key_range(torch.exp(2 * k.double().neg()))) == pytest.approx(12.25)
    sat = torch.from_numpy(oracle.image_fp32(np.array([-60.0, 1.0, 50.0])))
    assert float(attn_range.key_range(sat)) == pytest.approx(43.0, abs=1e-4)          # 43 reads "43 or more"
    assert not attn_range.in_domain(float(attn_range.key_range(torch.tensor([0.0, 1.0]))), 40.0)     # a zero in the image: no reading, no pass


def test_report_raises_by_default_and_warns_once(monkeypatch):
    class Err(Exception):
        pass
    bad = attn_range.violations(["a", "b", "c"], [60.0, 43.0, 10.0], [50.0, 30.0, 100.0])
    assert [n for n, _, _ in bad] == ["a"]
    monkeypatch.setattr(attn_range, "on_violation", "raise")
    attn_range.report([], Err)
    with pytest.raises(Err, match=r"a: max \|k\| = 60.*bound on \|q\| = 50"):
        attn_range.report(bad, Err)
    monkeypatch.setattr(attn_range, "on_violation", "warn")
    monkeypatch.setattr(attn_range, "_warned", False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        attn_range.report(bad, Err)
        attn_range.report(bad, Err)
    assert len(w) == 1 and "60" in str(w[0].message) and "50" in str(w[0].message)
    monkeypatch.setattr(attn_range, "on_violation", "ignore")
    with pytest.raises(ValueError):
        attn_range.report(bad, Err)


def test_image_bound_holds_for_a_correctly_rounded_exp():
    x = np.concatenate([np.arange(-70 * 8, 70 * 8 + 1) / 8.0, [np.nextafter(np.float32(43), np.float32(0)), np.nextafter(np.float32(43), np.float32(99))]])
    img = oracle.image_fp32(x).astype(np.float64)
    ref = np.exp(2.0 * oracle.clamp(x))
    assert (np.abs(img / ref - 1.0) <= oracle.rho(oracle.clamp(x))).all()
    assert (img[np.abs(x) > 43] == np.where(x[np.abs(x) > 43] > 0, img[x == 43.0][0], img[x == -43.0][0])).all()
    assert np.isfinite(img).all() and (img >= np.finfo(np.float32).tiny).all()


# (H, T, rows, clips): the shapes of the GPU tests
SHAPES = [(32, 41, 3, 3), (256, 61, 5, 5), (256, 61, 15, 5)]


@pytest.mark.parametrize("regime", oracle.REGIMES)
@pytest.mark.parametrize("H,T,rows,clips", SHAPES)
def test_emulated_fp32_formula_stays_inside_the_bounds(regime, H, T, rows, clips):
    K, q = oracle.patterns(regime, T, H, rows, clips)
    assert K.shape == (clips, T, H) and q.shape == (rows, H)
    lim = {"both": (43, 43), "keys_beyond": (60, 34), "queries_beyond": (34, 60), "benign": (4, 4)}[regime]
    assert np.abs(K).max() == lim[0] and np.abs(q).max() == lim[1]                    # the edges themselves are present
    Kr = K[np.arange(rows) % clips]
    ek, eq = oracle.image_fp32(Kr), oracle.image_fp32(q)[:, None, :]
    e, eb = oracle.energy(Kr, q[:, None, :], with_bound=True)
    s, sb = oracle.sech2(Kr, q[:, None, :], with_bound=True)
    e32, s32 = oracle.tanh_ek_fp32(ek, eq).astype(np.float64), oracle.sech2_ek_fp32(ek, eq).astype(np.float64)
    assert np.isfinite(e32).all() and np.isfinite(s32).all()
    assert (np.abs(e32 - e) <= eb).all(), float((np.abs(e32 - e) / eb).max())
    assert (np.abs(s32 - s) <= sb).all(), float((np.abs(s32 - s) / sb).max())
    # the bounds say something: far below the 1e-4 parity budget everywhere, and the softmax of the patterns is not flat
    assert eb.max() < 2.5e-5 and sb.max() < 2.5e-5
    rng = np.random.default_rng(1)
    v = np.round(rng.standard_normal(H) * 0.1 * 64) / 64
    f = oracle.forward(K, q, v, rng.uniform(-1, 1, (clips, T, 2 * H)), with_bound=True)
    assert (f["attw"].max(axis=1) > 1.5 / T).all()
    # an fp32 evaluation of the scores from the emulated energies stays inside the score bound
    s32 = (e32.astype(np.float32) * v.astype(np.float32)).astype(np.float32).sum(axis=2, dtype=np.float32)
    assert (np.abs(s32 - e @ v) <= f["score_bound"]).all()
    assert (f["attw_bound"] < 2e-3 * f["attw"].max(axis=1, keepdims=True)).all()


def test_patterns_are_deterministic_and_steps_share_the_keys():
    K1, q1 = oracle.patterns("both", 61, 256, 15, 5, steps=3)
    K2, q2 = oracle.patterns("both", 61, 256, 15, 5, steps=3)
    assert (K1 == K2).all() and (q1 == q2).all() and q1.shape == (3, 15, 256)
    assert (q1[0] != q1[1]).any()


def test_backward_oracle_matches_autograd():
    K, qs = oracle.patterns("benign", 7, 8, 6, 3, steps=2)
    rng = np.random.default_rng(0)
    v, enc, dctx = rng.standard_normal(8) * 0.3, rng.uniform(-1, 1, (3, 7, 16)), rng.standard_normal((2, 6, 16))
    live = np.array([[1, 1, 1, 0, 1, 1], [1, 0, 1, 0, 1, 1]], dtype=np.float64)
    o = oracle.backward(K, qs, v, enc, dctx, live)
    Kt, qt, vt, et = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (K, qs, v, enc))
    rows = torch.arange(6) % 3
    loss = 0
    for s in range(2):
        a = torch.softmax((torch.tanh(Kt[rows] + qt[s].unsqueeze(1)) * vt).sum(-1), dim=1)
        ctx = torch.bmm(a.unsqueeze(1), et[rows]).squeeze(1)
        loss = loss + (ctx * torch.tensor(dctx[s]) * torch.tensor(live[s]).unsqueeze(1)).sum()
    loss.backward()
    for name, t in (("dq", qt), ("dK", Kt), ("dv", vt)):
        assert np.abs(o[name] - t.grad.numpy()).max() < 1e-12, name
        assert (o[name + "_bound"] > 0).all()
