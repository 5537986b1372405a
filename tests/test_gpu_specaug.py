"""Spectrogram augmentation on the MI355X (csrc/a2s_specaug.hip, piano_a2s_amd/augment.py):

1. a2s_specaug_plan: content, mask plan and x_min of hand-built clips exactly, M within the parity tolerance, counters, one launch of its own counter;
2. a2s_specaug_apply against the float64 oracle, F = 480 and F = 37, aligned and not, every combination of gain, noise and masks, with guards;
3. neutral parameters return the input;
4. a clip's bits do not depend on the batch or on the run;
5. refusals launch nothing; the typed wrappers name the argument;
6. one SpecAugment call is two launches of its own counter;
7. physics, as an inequality: a two-tap filter of the rendered waveform against its gain table on the feature rows;
8. the training step reads the augmented features with no synchronisation in between;
9. the recipe with and without the flags, through pretrain.py and finetune.py.

Measured on the MI355X (the figures the tests print): max |device - float64| of a2s_specaug_apply over all cases of test 2 1.727e-07 (PARITY_MEASURED;
asserted TOL = 2^-21 = 4.77e-07, the smallest power of two that is at least twice it), of M 8.9e-09 on the features' scale, of neutral parameters against
the input 8.9e-08; the physics ratio 0.030 - 0.050 (asserted < 0.5); see DESIGN.md section 20 and profiles/specaug.json."""
import json
import os
import random

import numpy as np
import pytest
import torch

from piano_a2s_amd import scoregen, spec
from piano_a2s_amd.augment import SpecAugment, TempoAugment, TransposeAugment
from tests import specaug_oracle as oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FGUARD = 123.0
IGUARD = -77
PARITY_MEASURED = 1.727e-07          # max |device - float64| over test 2's cases, as measured on the MI355X
TOL = 2.0 ** -21          # 4.77e-07 >= 2 * 1.727e-07 > 2^-22
ROWS = [1, 5, 16, 17, 1201]          # below, at and above one chunk of the content scan and one row tile of the apply; the training window


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _guarded(values, dev, guard, lead=8, tail=8):
    """`values` (a host tensor) in the middle of a device buffer of guard values: -> (the whole buffer, the view on the middle)."""
    flat = torch.full((lead + values.numel() + tail,), guard, dtype=values.dtype, device=dev)
    view = flat[lead:lead + values.numel()].view(values.shape)
    view.copy_(values)
    return flat, view


def _guards_intact(flat, n, guard, lead=8):
    host = flat.cpu()
    return bool((host[:lead] == guard).all() and (host[lead + n:] == guard).all())


def _words(draws):
    """uint32 draws (host) -> the int32 tensor of the same bits."""
    return torch.from_numpy(np.ascontiguousarray(draws, dtype=np.uint32).view(np.int32).copy())


def _tables(B, F, rng, eq=True, noise=True):
    return np.stack([oracle.table(F, rng.uniform(-4, 4, 3), rng.random(2), rng.uniform(20, 60), rng.uniform(-3, 3), 60, eq=eq, noise=noise) for _ in range(B)])


def _unit(M):
    """A peak power on the features' scale (1 + log10(M) / 8): where M is compared within the parity tolerance."""
    return 1.0 + np.log10(np.asarray(M, dtype=np.float64)) / 8.0


# ------------------------------------------------------------------------------------------- 1. the plan
def _plan_clips(rows, F):
    """Five clips: all zero; only -0.0; content of one row; content that ends mid-window with 40 % of its cells at one floor value; a full window
    of one constant value."""
    rng = np.random.default_rng(rows * 1000 + F)
    x = torch.zeros(5, rows, F)
    x[1] = -0.0
    x[2, 0] = torch.from_numpy(0.3 + 0.7 * rng.random(F)).float()
    n_mid = (rows + 1) // 2
    c = 0.5 + 0.5 * rng.random((n_mid, F))
    c[rng.random((n_mid, F)) < 0.4] = 0.4531
    c[n_mid - 1, F - 1] = 0.9                                             # (the last content row holds a value)
    x[3, :n_mid] = torch.from_numpy(c).float()
    x[4] = 0.625
    return x, [0, 0, 1, n_mid, rows]


@pytest.mark.parametrize("F", [480, 37])
@pytest.mark.parametrize("rows", ROWS)
def test_specaug_plan_content_masks_stats_and_counters(dev, F, rows):
    from piano_a2s_amd import hip
    N, Wt, Wf, m = 64, 100, 60, 3
    x, want_content = _plan_clips(rows, F)
    rng = np.random.default_rng(7 * rows + F)
    tab = _tables(5, F, rng)
    draws = rng.integers(0, 2 ** 32, size=(N, 5, 16), dtype=np.uint32)
    draws[0], draws[1] = 0, 0xFFFFFFFF
    xflat, xv = _guarded(x, dev, 7.0, lead=64, tail=F + 5)                # non-zero values before and behind the clips: never taken for content
    t_dev, d_dev = torch.from_numpy(tab).to(dev), _words(draws).to(dev)
    cflat, cv = _guarded(torch.full((N, 5), IGUARD, dtype=torch.int32), dev, IGUARD)
    pflat, pv = _guarded(torch.full((N, 5, 16), IGUARD, dtype=torch.int32), dev, IGUARD)
    sflat, sv = _guarded(torch.full((N, 5, 2), FGUARD), dev, FGUARD)
    kflat, kv = _guarded(torch.tensor([10, 20, 30], dtype=torch.int32), dev, IGUARD)
    n0, t0, a0, k0 = hip.specaug_launches(), hip.tempo_launches(), hip.augment_launches(), hip.lib().a2s_launch_count()
    hip.specaug_plan(xv, t_dev, d_dev[0], Wt, Wf, m, cv[0], pv[0], sv[0], kv)
    assert hip.specaug_launches() == n0 + 1 and hip.lib().a2s_launch_count() == k0 + 1, "exactly one launch, of the library's count and of this counter"
    assert hip.tempo_launches() == t0 and hip.augment_launches() == a0, "not of the tempo or the transposition counter"
    for i in range(1, N):
        hip.specaug_plan(xv, t_dev, d_dev[i], Wt, Wf, m, cv[i], pv[i], sv[i], kv)
    torch.cuda.synchronize()
    content, plan, stats, counters = cv.cpu().numpy(), pv.cpu().numpy(), sv.cpu().numpy(), kv.cpu().tolist()
    assert all(_guards_intact(flat, n, g) for flat, n, g in ((cflat, 5 * N, IGUARD), (pflat, 80 * N, IGUARD), (sflat, 10 * N, FGUARD), (kflat, 3, IGUARD)))
    assert (content == np.array(want_content, dtype=np.int32)[None, :]).all(), content[0]
    ref = [oracle.apply(x[b].numpy(), tab[b]) for b in range(5)]
    assert [r["n"] for r in ref] == want_content
    time_masked = freq_masked = 0
    for i in range(N):
        for b in range(5):
            want = oracle.mask_plan(want_content[b], F, draws[i, b], Wt, Wf, m)
            assert plan[i, b].tolist() == want, (i, b, plan[i, b].tolist(), want)
            time_masked += any(w > 0 for w in want[1:8:2])
            freq_masked += any(w > 0 for w in want[9:16:2])
    worst = 0.0
    for b, r in enumerate(ref):
        assert (stats[:, b, 0] == r["x_min"]).all(), (b, stats[0, b, 0], r["x_min"])
        assert (stats[:, b, 1] == stats[0, b, 1]).all(), "the same M from run to run"
        if r["n"] == 0:
            assert stats[0, b, 1] == 0.0
        else:
            worst = max(worst, float(abs(_unit(stats[0, b, 1]) - _unit(r["M"]))))
    print(f"specaug_plan rows = {rows}, F = {F}: max |M - float64| on the features' scale = {worst:.3e} (asserted {TOL:.3e})")
    assert worst <= TOL
    assert counters == [10 + 5 * N, 20 + time_masked, 30 + freq_masked], (counters, time_masked, freq_masked)
    assert freq_masked > 0 and (time_masked > 0 or rows < 5)


# ------------------------------------------------------------------------------------------- 2. the apply
def _floor_clips(B, rows, F, seed):
    """Random features with a floor: x = max(x_floor, uniform noise), about a third of the cells at the floor; clip 0 is all zero, the others end
    at different rows."""
    rng = np.random.default_rng(seed)
    x = np.maximum(np.float32(0.33), rng.random((B, rows, F)).astype(np.float32))
    content = []
    for b in range(B):
        n = 0 if b == 0 else rows - ((b - 1) % 3) * (rows // 4)
        x[b, n:] = 0
        content.append(n)
    return x, content


_COMBOS = [(eq, noise, masks) for eq in (False, True) for noise in (False, True) for masks in (False, True)]
_CASES = [(F, lead, lead, rows) for F in (480, 37) for lead in (64, 3) for rows in ROWS] + [(480, 3, 64, 17)]
_WORST = {}


@pytest.mark.parametrize("F,xlead,ylead,rows", _CASES, ids=[f"F{F}-x{xl}-y{yl}-rows{rows}" for F, xl, yl, rows in _CASES])
def test_specaug_apply_against_the_float64_oracle(dev, F, xlead, ylead, rows):
    """Nine clips: an all-zero one, then E in {0, 12} x noise on / off x masks on / off.  lead 64 / 3: the buffer starts 16-byte aligned (vector loads and
    stores when F % 4 == 0) / does not (the scalar instance; x3-y64: unaligned 16-byte loads beside aligned stores).  |device - float64| <= TOL on
    every cell; exactly: padding rows and masked cells 0.0, the all-zero clip zero, maximum 1.0 wherever no mask lies over the peak, guards intact.
    TOL = 2^-21 is the smallest power of two that is at least twice the largest |device - float64| measured over all of these cases on the MI355X,
    1.727e-07 (PARITY_MEASURED; per case 0.9e-07 - 1.7e-07)."""
    from piano_a2s_amd import hip
    B, Wt, Wf, m = 9, 100, 60, 4
    x, content = _floor_clips(B, rows, F, seed=F + rows + xlead)
    rng = np.random.default_rng(F * rows + ylead)
    tab = np.stack([oracle.table(F, rng.uniform(-4, 4, 3) * (1.0 if eq else 0.0), rng.random(2), rng.uniform(20, 60), rng.uniform(-3, 3), 60, eq=eq, noise=noise)
                    for eq, noise, _ in [(True, True, True)] + _COMBOS])          # (e in +- 4 dB each: E = 12)
    draws = rng.integers(0, 2 ** 32, size=(B, 16), dtype=np.uint32)
    draws[:, 0] = 0xFFFFFFFF                                               # (the first mask of each kind at its full width)
    draws[:, 2] = 0xFFFFFFFF
    for b, (_, _, masks) in enumerate(_COMBOS, start=1):
        if not masks:
            draws[b, 0::4], draws[b, 2::4] = 0, 0                          # masks off: every width word 0
    xflat, xv = _guarded(torch.from_numpy(x), dev, float("nan"), lead=xlead, tail=F + 5)          # NaN before and behind the input: never read into a result
    yflat, yv = _guarded(torch.full((B, rows, F), FGUARD), dev, FGUARD, lead=ylead, tail=F + 5)
    t_dev, d_dev = torch.from_numpy(tab).to(dev), _words(draws).to(dev)
    cont, plan, stats = torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, 16), dtype=torch.int32, device=dev), torch.empty((B, 2), device=dev)
    counters = torch.zeros(3, dtype=torch.int32, device=dev)
    n0, t0, a0 = hip.specaug_launches(), hip.tempo_launches(), hip.augment_launches()
    hip.specaug_plan(xv, t_dev, d_dev, Wt, Wf, m, cont, plan, stats, counters)
    hip.specaug_apply(xv, t_dev, cont, plan, stats, y=yv)
    torch.cuda.synchronize()
    assert hip.specaug_launches() == n0 + 2 and hip.tempo_launches() == t0 and hip.augment_launches() == a0
    got = yv.cpu().numpy()
    assert _guards_intact(yflat, B * rows * F, FGUARD, lead=ylead), "the guards before and behind the output"
    assert np.isfinite(got).all() and cont.cpu().tolist() == content
    assert torch.equal(xv.cpu(), torch.from_numpy(x)), "the input is as it was"
    plan_h = plan.cpu().numpy()
    worst = 0.0
    for b in range(B):
        want_plan = oracle.mask_plan(content[b], F, draws[b], Wt, Wf, m)
        assert plan_h[b].tolist() == want_plan
        r = oracle.apply(x[b], tab[b], want_plan)
        n, ref, masked = r["n"], r["out"], r["masked"]
        if b == 0:
            assert n == 0 and (got[b] == 0).all(), "an all-zero clip stays zero"
            continue
        assert (got[b][n:] == 0).all() and (got[b][masked] == 0).all(), "padding rows and masked cells are exactly 0.0"
        if b >= 1 and _COMBOS[b - 1][2] and rows >= 5 and F >= 5:
            assert masked.any()
        err = float(np.abs(got[b].astype(np.float64) - ref).max())
        worst = max(worst, err)
        assert err <= TOL, (b, err)
        near_peak = r["y"] >= r["M"] * (1.0 - 1e-4)
        if not masked[:n][near_peak].any():                                # no mask over the peak (or over a cell that fp32 cannot tell from it)
            assert got[b].max() == 1.0, (b, got[b].max())
        assert got[b].max() <= 1.0 and got[b].min() >= 0.0
    _WORST[(F, xlead, ylead, rows)] = worst
    print(f"specaug_apply F = {F}, rows = {rows}, leads = ({xlead}, {ylead}): max |device - float64| = {worst:.3e}; over the cases so far "
          f"{max(_WORST.values()):.3e} (asserted {TOL:.3e})")


# ------------------------------------------------------------------------------------------- 3. neutral parameters
def _unit_peak_clips(B, rows, F, seed):
    """Clips whose maximum is 1.0: content in [0.5, 1) with a third of the cells at one floor value 0.4531 and one cell at 1.0; clip b ends b rows early."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, rows, F), dtype=np.float32)
    for b in range(B):
        n = max(1, rows - b)
        c = (0.5 + 0.4999 * rng.random((n, F))).astype(np.float32)
        c[rng.random((n, F)) < 0.33] = np.float32(0.4531)
        c[n - 1, 0] = 0.75
        c[n // 2, F // 2] = 1.0
        x[b, :n] = c
    return x


@pytest.mark.parametrize("F,rows", [(480, 17), (37, 5), (480, 1201)])
def test_neutral_parameters_return_the_input(dev, F, rows):
    from piano_a2s_amd import hip
    B = 3
    x = _unit_peak_clips(B, rows, F, seed=rows)
    xd = torch.from_numpy(x).to(dev)
    tab = torch.stack([torch.ones(B, F), torch.zeros(B, F)], dim=1).contiguous().to(dev)
    cont, plan, stats = torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, 16), dtype=torch.int32, device=dev), torch.empty((B, 2), device=dev)
    hip.specaug_plan(xd, tab, torch.full((B, 16), -1, dtype=torch.int32, device=dev), 0, 0, 4, cont, plan, stats, torch.zeros(3, dtype=torch.int32, device=dev))
    y = hip.specaug_apply(xd, tab, cont, plan, stats)
    torch.cuda.synchronize()
    assert (plan.cpu()[:, 1::2] == 0).all(), "Wt = Wf = 0: every width is 0"
    assert stats.cpu()[:, 1].tolist() == [1.0] * B and (stats.cpu()[:, 0] == np.float32(0.4531)).all()
    err = float((y.cpu().double() - torch.from_numpy(x).double()).abs().max())
    print(f"neutral parameters F = {F}, rows = {rows}: max |device - input| = {err:.3e} (asserted {TOL:.3e})")
    assert err <= TOL
    assert (y.cpu().amax(dim=(1, 2)) == 1.0).all()


# ------------------------------------------------------------------------------------------- 4. the same bits
def test_a_clips_bits_do_not_depend_on_the_batch_or_the_run(dev):
    from piano_a2s_amd import hip
    rows, F = 37, 480
    x, _ = _floor_clips(6, rows, F, seed=5)
    x = x[1:]                                                              # five clips with content
    rng = np.random.default_rng(11)
    tab, draws = _tables(5, F, rng), rng.integers(0, 2 ** 32, size=(5, 16), dtype=np.uint32)

    def run(sel):
        xd, td, dd = torch.from_numpy(x[sel]).to(dev), torch.from_numpy(tab[sel]).to(dev), _words(draws[sel]).to(dev)
        B = xd.shape[0]
        cont, plan, stats = torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, 16), dtype=torch.int32, device=dev), torch.empty((B, 2), device=dev)
        hip.specaug_plan(xd, td, dd, 10, 20, 2, cont, plan, stats, torch.zeros(3, dtype=torch.int32, device=dev))
        y = hip.specaug_apply(xd, td, cont, plan, stats)
        torch.cuda.synchronize()
        return y.cpu().view(torch.int32), stats.cpu().view(torch.int32), plan.cpu()

    whole, again, alone = run(slice(0, 5)), run(slice(0, 5)), run(slice(3, 4))
    assert all(torch.equal(a, b) for a, b in zip(whole, again)), "the same bits from run to run"
    assert all(torch.equal(w[3:4], a) for w, a in zip(whole, alone)), "B = 1 against position 3 of B = 5"
    assert (whole[0] != 0).any()


# ------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_launch_nothing(dev):
    from piano_a2s_amd import hip
    Lib, st = hip.lib(), hip.stream()
    B, rows, F = 2, 5, 480
    x, y = torch.rand(B, rows, F, device=dev), torch.zeros(B, rows, F, device=dev)
    tab, draws = torch.ones(B, 2, F, device=dev), torch.zeros((B, 16), dtype=torch.int32, device=dev)
    content, plan = torch.full((B,), IGUARD, dtype=torch.int32, device=dev), torch.full((B, 16), IGUARD, dtype=torch.int32, device=dev)
    stats, counters = torch.full((B, 2), FGUARD, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)
    n0, k0 = hip.specaug_launches(), Lib.a2s_launch_count()
    ok = (hip._p(x), B, rows, F, hip._p(tab), hip._p(draws), 10, 10, 2, hip._p(content), hip._p(plan), hip._p(stats), hip._p(counters))
    bad_plan = [(0, None), (4, None), (5, None), (9, None), (10, None), (11, None), (12, None), (1, -1), (1, 65536), (2, 0), (2, -3), (3, 0), (6, -1), (7, -1),
                (8, 5), (8, -1)]
    for i, bad in bad_plan:
        args = list(ok)
        args[i] = bad
        assert Lib.a2s_specaug_plan(st, *args) == -1, (i, bad)
        assert b"specaug_plan" in Lib.a2s_last_error()
    args = list(ok)
    args[1] = 0
    assert Lib.a2s_specaug_plan(st, *args) == 0
    ok2 = (hip._p(x), hip._p(y), hip._p(tab), hip._p(content), hip._p(plan), hip._p(stats), B, rows, F)
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (1, hip._p(x)), (6, -1), (6, 65536), (7, 0), (8, 0)):
        args = list(ok2)
        args[i] = bad
        assert Lib.a2s_specaug_apply(st, *args) == -1, (i, bad)
        assert b"specaug_apply" in Lib.a2s_last_error()
    args = list(ok2)
    args[6] = 0
    assert Lib.a2s_specaug_apply(st, *args) == 0
    torch.cuda.synchronize()
    assert hip.specaug_launches() == n0 and Lib.a2s_launch_count() == k0, "nothing was launched"
    assert (y == 0).all() and (content == IGUARD).all() and (plan == IGUARD).all() and (stats == FGUARD).all() and counters.tolist() == [0, 0, 0]
    # the typed wrappers name the argument
    plan_ok = dict(x=x, table=tab, draws=draws, Wt=10, Wf=10, m=2, content=content, plan=plan, stats=stats, counters=counters)
    for name, value in (("x", x.transpose(1, 2)), ("x", x.double()), ("x", x.cpu()), ("table", tab[:, :1]), ("table", tab.half()), ("table", tab.cpu()),
                        ("draws", draws[:, :8]), ("draws", draws.long()), ("draws", draws.cpu()), ("Wt", -1), ("Wt", 2.5), ("Wf", -2), ("m", 5), ("m", -1),
                        ("content", content.long()), ("content", content[:1]), ("plan", plan[:, :8]), ("stats", stats.double()), ("stats", stats.cpu()),
                        ("counters", counters[:2]), ("counters", counters.cpu())):
        with pytest.raises(hip.A2SError, match=f"`{name}`"):
            hip.specaug_plan(**{**plan_ok, name: value})
    apply_ok = dict(x=x, table=tab, content=content, plan=plan, stats=stats, y=y)
    for name, value in (("x", x[:, :, ::2]), ("x", x.cpu()), ("table", tab.transpose(1, 2)), ("content", content.float()), ("plan", plan.cpu()), ("stats", stats[:1]),
                        ("y", y[:, :4]), ("y", y.double()), ("y", y.cpu()), ("y", x)):
        with pytest.raises(hip.A2SError, match=f"`{name}`"):
            hip.specaug_apply(**{**apply_ok, name: value})
    torch.cuda.synchronize()
    assert hip.specaug_launches() == n0 and Lib.a2s_launch_count() == k0


# ------------------------------------------------------------------------------------------- 6. launches
def test_one_call_is_two_launches_of_its_own_counter(dev):
    from piano_a2s_amd import hip
    Lib = hip.lib()
    cfg = spec.default_cfg()
    rows = 37
    x = torch.rand(4, 1, rows, 480, device=dev)
    x[1, :, 20:] = 0                                                               # a padded clip: content 20 of 37 rows
    key, upper, lower = torch.full((4, 5), 6, device=dev), torch.ones(4, 5, 9, dtype=torch.long, device=dev), torch.ones(4, 5, 6, dtype=torch.long, device=dev)
    batch = [x, None, key, upper, None, lower]
    aug = SpecAugment(cfg, 6, (30, 50), 7, 20, 2, seed=7, device=dev)
    keep = x.clone()
    n0, t0, a0, k0 = hip.specaug_launches(), hip.tempo_launches(), hip.augment_launches(), Lib.a2s_launch_count()
    out = aug(batch)
    torch.cuda.synchronize()
    assert hip.specaug_launches() == n0 + 2 and Lib.a2s_launch_count() == k0 + 2 and hip.tempo_launches() == t0 and hip.augment_launches() == a0
    assert out[0] is not x and out[0].shape == x.shape and torch.equal(x, keep) and all(out[i] is batch[i] for i in (1, 2, 3, 4, 5)), "a new feature tensor, nothing else touched"
    content, plan, stats = (t.cpu() for t in aug.last_plan)
    assert content.tolist() == [37, 20, 37, 37]
    again = SpecAugment(cfg, 6, (30, 50), 7, 20, 2, seed=7, device=dev)
    tab, draws = again.draw(4)
    want = [oracle.mask_plan(n, 480, d, 7, 20, 2) for n, d in zip(content.tolist(), draws)]
    assert plan.tolist() == want
    got = out[0].cpu().numpy()
    for b in range(4):
        ref = oracle.apply(x[b, 0].cpu().numpy(), tab[b], want[b])["out"]
        assert np.abs(got[b, 0] - ref).max() <= TOL
    assert aug.counts() == dict(clips=4, time_masked=sum(any(w > 0 for w in p[1:8:2]) for p in want), freq_masked=sum(any(w > 0 for w in p[9:16:2]) for p in want))
    # beside the other two: two launches each, each on its own counter
    transposer, tempo = TransposeAugment(cfg, 2, 1.0, seed=7, device=dev), TempoAugment(cfg, 0.2, seed=7, device=dev)
    n0, t0, a0, k0 = hip.specaug_launches(), hip.tempo_launches(), hip.augment_launches(), Lib.a2s_launch_count()
    out = aug(tempo(transposer(batch)))
    torch.cuda.synchronize()
    assert hip.specaug_launches() == n0 + 2 and hip.tempo_launches() == t0 + 2 and hip.augment_launches() == a0 + 2 and Lib.a2s_launch_count() == k0 + 6
    assert aug.counts()["clips"] == 8 and tempo.counts()["clips"] == 4 and transposer.counts()["clips"] == 4


# ------------------------------------------------------------------------------------------- 7. physics
FILTERS = (-0.9, -0.5, 0.5, 0.9)


@pytest.mark.parametrize("seed", [3, 7, 11])
def test_a_filter_on_the_waveform_is_the_gain_table_on_the_feature_rows(dev, seed):
    """mean |augmented dry features - features of the filtered waveform| < 0.5 * mean |dry features - features of the filtered waveform| for
    y[n] = x[n] + c x[n - 1], c in {-0.9, -0.5, 0.5, 0.9}: the GPU renderer, the filter in torch, the GPU VQT, the gain table from its closed form.
    With the host renderer and the direct-form VQT the ratio is 0.006 - 0.253 for these seeds and filters (tests/test_specaug_cpu.py); 0.5 is twice the
    worst of them.  Measured on the MI355X: 0.030 - 0.050 for all twelve cases (DESIGN.md section 20 has the table and why the figures are not the host's)."""
    from piano_a2s_amd import hip
    from piano_a2s_amd.render import render
    from piano_a2s_amd.vqt import VQT
    clip = scoregen.make_clip(spec.default_cfg(max_bars=2), seed, frames=301)
    prog = scoregen.pack_program(clip, rows=len(clip["events"]))
    wave = render(torch.from_numpy(prog[None]).to(dev))
    waves = [wave]
    for c in FILTERS:
        w = wave.clone()
        w[..., 1:] += c * wave[..., :-1]
        waves.append(w)
    feat = VQT(dev)(torch.cat(waves, dim=0))
    B, F = len(FILTERS), feat.shape[-1]
    dry = feat[:1].expand(B, *feat.shape[1:]).contiguous()
    tab = torch.from_numpy(np.stack([oracle.filter_gain_table(c, F) for c in FILTERS])).to(dev)
    print(f"seed {seed}: {feat.shape[-2]} frames, {100 * float((feat[0] - feat[0].min() <= 2.0 ** -18).float().mean()):.1f} % of the dry cells at the floor value "
          f"{float(feat[0].min()):.4f}")
    cont, plan, stats = torch.empty(B, dtype=torch.int32, device=dev), torch.empty((B, 16), dtype=torch.int32, device=dev), torch.empty((B, 2), device=dev)
    hip.specaug_plan(dry, tab, torch.zeros((B, 16), dtype=torch.int32, device=dev), 0, 0, 1, cont, plan, stats, torch.zeros(3, dtype=torch.int32, device=dev))
    aug = hip.specaug_apply(dry, tab, cont, plan, stats)
    for i, c in enumerate(FILTERS):
        with_aug, without = float((aug[i] - feat[1 + i]).abs().mean()), float((dry[i] - feat[1 + i]).abs().mean())
        print(f"seed {seed}, c = {c}: mean |augmented - filtered| = {with_aug:.5f}, mean |dry - filtered| = {without:.5f}, ratio {with_aug / without:.3f}")
        assert with_aug < 0.5 * without, (seed, c, with_aug, without)


# ------------------------------------------------------------------------------------------- 8. the step reads the augmented features
def test_step_reads_the_augmented_features_without_a_synchronisation(dev):
    import models
    from datasets.syn import RenderedClips
    from piano_a2s_amd import recipe, train
    cfg = spec.default_cfg(hidden_size=32, conv_feature_size=32, max_length=(48, 32))
    ds = RenderedClips(cfg, 2, seed=4321, frames=201)
    host = torch.utils.data.default_collate([ds[i] for i in range(2)])
    torch.manual_seed(11)
    init = models.ScoreTranscription(**cfg).state_dict()
    aug = SpecAugment(cfg, 9, (30, 40), 20, 30, 2, seed=99, device=dev)
    tab, draws = aug.draw(2)
    res = []
    for mode in ("plain", "racy", "beforehand"):
        m = models.ScoreTranscription(**cfg)
        m.load_state_dict(init)
        m = m.to(dev).train()
        step = train.TrainStep(m, dropout=False)
        batch = recipe._features(list(host), dev)
        torch.cuda.synchronize()
        if mode != "plain":
            batch = aug.apply(batch, tab, draws)                 # two launches on the current stream ...
        if mode == "beforehand":
            torch.cuda.synchronize()
        losses = step(batch, 0.7, rng=random.Random(3))          # ... and the step right behind them
        torch.cuda.synchronize()
        res.append((losses[:, 0].clone().cpu(), [t.cpu() for t in batch[2:7]], batch[0].cpu()))
    (l_plain, t_plain, f_plain), (l_racy, t_racy, f_racy), (l_before, t_before, f_before) = res
    assert torch.isfinite(l_racy).all()
    assert torch.equal(f_racy, f_before) and torch.equal(l_racy, l_before), (l_racy, l_before)
    assert not torch.equal(f_racy, f_plain) and not torch.equal(l_racy, l_plain), "the clips were changed and the loss shows it"
    assert all(torch.equal(a, b) for a, b in zip(t_racy, t_plain)), "no target was touched"


# ------------------------------------------------------------------------------------------- 9. the recipe
def _run(module, tmp_path, name, extra):
    ws = os.path.join(str(tmp_path), name)
    os.makedirs(ws)
    common = ["--device=cuda:0", f"--workspace={ws}", "--synthetic_clips=8", "--synthetic_scores=rendered", "--synthetic_frames=201", "--batch_size=2",
              "--number_of_epochs=1", "--hidden_size=32", "--conv_feature_size=32", "--max_length=(48, 32)", "--seed=1234"]
    if module.__name__ == "pretrain":
        args, out = [os.path.join(ROOT, "hparams", "pretrain.yaml"), "--soundfont_folder=/none"], "pretrain.epr"
    else:
        args, out = [os.path.join(ROOT, "hparams", "finetune.yaml"), "--asap_folder=/none", "--mv2h_bin=/none"], "finetune.epr"
    brain = module.main(args + common + extra)
    with open(os.path.join(ws, "1234", out, "run_summary.json")) as f:
        return brain, json.load(f)


@pytest.fixture
def train_features(monkeypatch):
    """The feature tensors that reach the training step, batch by batch."""
    from piano_a2s_amd import recipe
    seen, orig = [], recipe.ASR._train_features

    def spy(self, batch):
        out = orig(self, batch)
        seen.append(out[0].detach().cpu().clone())
        return out

    monkeypatch.setattr(recipe.ASR, "_train_features", spy)
    return seen


def _seed_host_generators():
    """Two runs are compared loss for loss: both start from the same state of the generators the training step draws from."""
    random.seed(5), np.random.seed(6), torch.manual_seed(7)


def test_recipe_with_every_flag_off_is_the_run_without_them(tmp_path, dev, train_features):
    """Flags absent against flags at their off values: no augmenter is built, nothing is launched, and the tensors that reach the training step are the
    same bits, batch for batch -- everything the feature could touch."""
    import pretrain
    from piano_a2s_amd import hip
    n0 = hip.specaug_launches()
    _seed_host_generators()
    brain, summary = _run(pretrain, tmp_path, "absent", [])
    plain, plain_stats = list(train_features), dict(brain.train_stats)
    del train_features[:]
    _seed_host_generators()
    brain2, summary2 = _run(pretrain, tmp_path, "off", ["--eq_augment_db=0", "--mask_time=0", "--mask_freq=0", "--mask_count=3"])
    assert hip.specaug_launches() == n0, "with every component off nothing is launched"
    for b, s in ((brain, summary), (brain2, summary2)):
        assert "spec_augment" not in s and b._spec_augment() is None and s["optimizer_steps"] == 4 and "specaug_clips" not in b.train_stats
    assert len(plain) == 4 and len(train_features) == 4 and all(torch.equal(a, b) for a, b in zip(plain, train_features)), "the same features reach the step"
    # the losses themselves are printed, not compared: from the same generator states and on identical features, with no augmenter built and nothing
    # launched, the two runs' mean losses differed by 1.6e-8 relative when this test was written (some terms equal, some not, and which changes from run
    # to run): the training step does not repeat its own fp32 sums bit for bit
    print("train stats without the flags:", plain_stats, "with every flag at its off value:", brain2.train_stats)


def test_recipe_with_the_flags(tmp_path, dev, train_features):
    import pretrain
    from piano_a2s_amd import hip
    n0, t0, a0 = hip.specaug_launches(), hip.tempo_launches(), hip.augment_launches()
    brain, summary = _run(pretrain, tmp_path, "on", ["--eq_augment_db=6", "--noise_augment_db=(30, 50)", "--mask_time=20", "--mask_freq=30"])
    assert hip.specaug_launches() == n0 + 2 * 4, "two launches for each of the 4 training batches, none in VALID or TEST"
    assert hip.tempo_launches() == t0 and hip.augment_launches() == a0
    assert summary["fused_hip_step"] and summary["optimizer_steps"] == 4 and summary["nonfinite_steps"] == 0
    block = summary["spec_augment"]
    assert block["eq_db"] == 6 and block["noise_db"] == [30, 50] and (block["mask_time"], block["mask_freq"], block["mask_count"]) == (20, 30, 2)
    assert block["clips"] == 8 and 0 <= block["time_masked"] <= 8 and 0 < block["freq_masked"] <= 8
    assert "transpose_augment" not in summary and "tempo_augment" not in summary
    assert all(np.isfinite(brain.last_stats[k]) for k in ("loss", "time_loss", "key_loss", "upper_loss", "lower_loss", "WER", "WER_upper", "WER_lower")), brain.last_stats
    assert all(np.isfinite(v) for v in brain.train_stats.values()), brain.train_stats
    assert brain.train_stats["specaug_clips"] == 8
    assert len(train_features) == 4 and all(float(f.amax()) <= 1.0 and float(f.amin()) >= 0.0 for f in train_features)
    assert any(float(f.amax()) == 1.0 for f in train_features), "re-normalised: a clip whose peak no mask covers has maximum 1.0"
    assert any((f == 0).all(dim=-2).any() for f in train_features), "a frequency mask shows as a bin that is zero in every row"


def test_recipe_refuses_a_value_out_of_range_before_training(tmp_path, dev):
    import pretrain
    from piano_a2s_amd import hip
    n0 = hip.specaug_launches()
    for i, (flag, extra) in enumerate((("noise_augment_db", ["--noise_augment_db=(10, 50)"]), ("mask_count", ["--mask_freq=10", "--mask_count=5"]))):
        with pytest.raises(ValueError, match=flag):
            _run(pretrain, tmp_path, f"refused{i}", extra)
        assert not os.path.exists(os.path.join(str(tmp_path), f"refused{i}", "1234", "pretrain.epr", "results")), "refused before the first epoch"
    assert hip.specaug_launches() == n0


def test_finetune_applies_it_after_transposition_and_tempo(tmp_path, dev, monkeypatch):
    import finetune
    from piano_a2s_amd import hip
    order = []
    for cls in (TransposeAugment, TempoAugment, SpecAugment):
        def logged(self, batch, _orig=cls.__call__, _name=cls.__name__):
            order.append(_name)
            return _orig(self, batch)
        monkeypatch.setattr(cls, "__call__", logged)
    n0, t0, a0 = hip.specaug_launches(), hip.tempo_launches(), hip.augment_launches()
    brain, summary = _run(finetune, tmp_path, "fine", ["--transpose_augment=2", "--detune_bins=0.5", "--tempo_augment=0.25", "--mask_time=30", "--mask_count=1"])
    assert hip.specaug_launches() == n0 + 2 * 4 and hip.tempo_launches() == t0 + 2 * 4 and hip.augment_launches() == a0 + 2 * 4
    assert order == ["TransposeAugment", "TempoAugment", "SpecAugment"] * 4
    assert summary["spec_augment"]["clips"] == 8 and summary["spec_augment"]["mask_time"] == 30 and summary["spec_augment"]["eq_db"] == 0
    assert summary["spec_augment"]["noise_db"] is None and summary["spec_augment"]["freq_masked"] == 0
    assert summary["tempo_augment"]["clips"] == 8 and summary["transpose_augment"]["clips"] == 8
    assert brain.finetune and np.isfinite(brain.last_stats["WER"])
