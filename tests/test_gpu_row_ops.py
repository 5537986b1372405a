"""Op-by-op parity of the row, loss and optimizer kernels on the MI355X -- the oldest entry points, which every training step and every
decode goes through and which the suite otherwise reaches only end to end: a2s_log_softmax_rows, a2s_embed_rows (+ the remaining forms of
a2s_embed_scatter_add), a2s_nll_loss / a2s_nll_grad, a2s_clip_adadelta, a2s_bn_relu_apply, a2s_bn1d_relu_dropout, a2s_ew_act_bwd and the two
halves of the synchronised BatchNorm backward with two emulated ranks.

Every reference is float64 on the CPU from the same fp32 inputs, written out here; every bound is stated where it is asserted and comes from
the number formats and the operation, never from what the kernel gives.  Shapes are odd on purpose: not a multiple of the 64 lanes, of the 4
rows or 256 threads of a workgroup, grids larger than their cap.  Output buffers are wider than what a kernel may write and pre-filled with
a sentinel that must come back bit for bit.  NB raw pointers do not keep tensors alive: every device operand is bound to a local name."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SENT = 12345.0                    # what the unwritten part of every output buffer holds before and after a call
U24, U23 = 2.0 ** -24, 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _report(name, err):
    """One line "row <name>: <figure>" in the file the per-kernel tests of test_gpu_ops.py report to (one place names it)."""
    from tests import test_gpu_ops
    test_gpu_ops._report(f"row {name}", err)


def _bits(t):
    """The bit patterns of a float32 tensor (on the CPU): equality of these is equality bit for bit (-0.0 != 0.0, NaN == the same NaN)."""
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _padded(x, width, dev):
    """x (R, n) as the leading columns of a (R, width) device buffer whose other columns hold the sentinel."""
    buf = torch.full((x.shape[0], width), SENT)
    buf[:, :x.shape[1]] = x
    return buf.to(dev)


def _tail(n, dev, extra=5, dtype=torch.float32):
    """A flat device buffer of n + extra elements, all sentinel."""
    return torch.full((n + extra,), SENT, dtype=dtype, device=dev)


def _flat(x, dev, extra=5):
    """x (flat) followed by `extra` sentinel elements, on the device."""
    buf = torch.full((x.numel() + extra,), SENT, dtype=x.dtype)
    buf[:x.numel()] = x.reshape(-1)
    return buf.to(dev)


def _tail_untouched(buf, n):
    t = buf[n:].cpu()
    return bool((t == SENT).all())


# ------------------------------------------------------------------------------------------------------------------ a2s_log_softmax_rows
LSM_ROWS = (1, 3, 4, 5, 9)                       # the kernel handles 4 rows per workgroup
LSM_VOCAB = (1, 2, 5, 63, 64, 65, 173, 200)


def _log_softmax_rows(dev, x):
    """One call with and one without argmax_out on x (R, V) placed in a row window: ldx = V + 3 (the three columns behind a row hold the
    sentinel, which is larger than every logit: a lane that reads past V would make it the maximum), ldy = 2 V + 1.  Returns y (R, V) and
    the argmax (R,), after checking that nothing outside the window was written and that both calls give the same bits."""
    from piano_a2s_amd import hip
    L = hip.lib()
    R, V = x.shape
    ldx, ldy = V + 3, 2 * V + 1
    xd = _padded(x, ldx, dev)
    got = []
    for want_argmax in (True, False):
        yd = torch.full((R, ldy), SENT, device=dev)
        am = torch.full((R + 3,), -7, dtype=torch.int32, device=dev)
        hip.check(L.a2s_log_softmax_rows(hip.stream(), hip._p(xd), ldx, hip._p(yd), ldy, hip._p(am) if want_argmax else None, R, V), "log_softmax_rows")
        torch.cuda.synchronize()
        y, a = yd.cpu(), am.cpu()
        assert bool((y[:, V:] == SENT).all()), "log_softmax_rows wrote outside its column window"
        assert bool((a[R:] == -7).all()) and (want_argmax or bool((a == -7).all())), "log_softmax_rows wrote outside argmax_out"
        got.append((y[:, :V].clone(), a[:R].clone()))
    assert _same_bits(got[0][0], got[1][0]), "argmax_out = NULL changes the log-probabilities"
    return got[0]


def _lsm_fraction_of_bound(y, x):
    """max over the finite entries of |y - ref| / (8 * 2^-24 * max(1, max|x| + ln V)), ref = float64 log_softmax of the same fp32 logits
    (max|x| over the row's finite logits).  The bound covers the rounding of expf and logf, the sum of at most V terms in [0, 1] and the two
    subtractions; torch's fp32 log_softmax reaches 0.34 of it on these inputs.  Entries that are -inf in the reference must be -inf."""
    V = x.shape[1]
    ref = torch.log_softmax(x.double(), dim=1)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(y), fin) and bool((y[~fin] == ref[~fin].float()).all()), "-inf logits must give -inf log-probabilities"
    xmax = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)).double().amax(dim=1, keepdim=True)
    bound = 8 * U24 * torch.clamp(xmax + np.log(V), min=1.0)
    err = torch.where(fin, (y.double() - ref).abs(), torch.zeros_like(ref))
    return float((err / bound).max())


@pytest.mark.parametrize("V", LSM_VOCAB)
def test_log_softmax_rows_values_and_argmax(dev, V):
    g = torch.Generator().manual_seed(100 + V)
    worst = 0.0
    for R in LSM_ROWS:
        base = torch.randn(R, V, generator=g)
        holes = base.clone()                                        # some -inf entries among finite ones (one finite logit per row at least)
        holes[torch.rand(R, V, generator=g) < 0.3] = float("-inf")
        holes[torch.arange(R), torch.arange(R) % V] = base[torch.arange(R), torch.arange(R) % V]
        for name, x in (("x1", base), ("x30", base * 30), ("x1e-3", base * 1e-3), ("+80", base + 80), ("-80", base - 80), ("-inf", holes)):
            y, am = _log_softmax_rows(dev, x)
            frac = _lsm_fraction_of_bound(y, x)
            worst = max(worst, frac)
            assert frac <= 1.0, (R, V, name, frac)
            assert np.array_equal(am.numpy(), np.argmax(x.numpy(), axis=1)), (R, V, name)
    _report(f"log_softmax_rows V{V} (fraction of 8 * 2^-24 * max(1, max|x| + ln V))", worst)


@pytest.mark.parametrize("V", LSM_VOCAB)
def test_log_softmax_rows_argmax_is_the_lowest_index_among_the_maxima(dev, V):
    """Planted maxima: at index 0, at V - 1, ties inside one lane (3, 67), across lanes (5, 70), across the 64-lane boundary (63, 64) and an
    all-equal row -- each where V has those indices."""
    g = torch.Generator().manual_seed(200 + V)
    plants = [(0,), (V - 1,)] + [p for p in ((3, 67), (5, 70), (63, 64)) if p[1] < V]
    x = torch.randn(len(plants) + 1, V, generator=g)
    for r, idx in enumerate(plants):
        x[r, list(idx)] = 50.0
    x[-1, :] = 0.25
    want = np.array([p[0] for p in plants] + [0])
    assert np.array_equal(np.argmax(x.numpy(), axis=1), want)
    y, am = _log_softmax_rows(dev, x)
    assert np.array_equal(am.numpy(), want), (am.tolist(), want.tolist())
    assert _lsm_fraction_of_bound(y, x) <= 1.0


@pytest.mark.parametrize("V", LSM_VOCAB)
def test_log_softmax_rows_argmax_stays_in_the_row_without_an_ordered_value(dev, V):
    """The contract of include/a2s.h: the index written is in [0, V) whatever the logits; a row that is all NaN or all -inf gives 0.  (Before the
    arg-maximum epilogues mapped their "no candidate yet" index to 0 such a row gave 2147483647, and the decoder epilogues gathered an embedding
    row by it.)  This kernel only stores the index."""
    g = torch.Generator().manual_seed(300 + V)
    x = torch.randn(5, V, generator=g)
    x[0, :] = float("nan")
    x[1, :] = float("-inf")
    x[2, ::2] = float("nan")                                    # NaN mixed with finite values (V = 1: all NaN)
    x[3, 1::2] = float("nan")
    from piano_a2s_amd import hip
    L = hip.lib()
    ldx, ldy = V + 3, 2 * V + 1
    xd = _padded(x, ldx, dev)
    yd = torch.full((5, ldy), SENT, device=dev)
    am = torch.full((8,), -7, dtype=torch.int32, device=dev)
    hip.check(L.a2s_log_softmax_rows(hip.stream(), hip._p(xd), ldx, hip._p(yd), ldy, hip._p(am), 5, V), "log_softmax_rows")
    torch.cuda.synchronize()
    a = am.cpu().tolist()
    assert all(0 <= i < V for i in a[:5]), a
    assert a[0] == 0 and a[1] == 0, a
    assert a[5:] == [-7, -7, -7]
    y = yd.cpu()
    assert bool(torch.isnan(y[:2, :V]).all()), "a row without an ordered value must keep non-finite log-probabilities (the update is skipped)"
    assert bool((y[:, V:] == SENT).all())


# ------------------------------------------------------------------------------------------------------------------ a2s_embed_rows
EMB_TABLE_ROWS = 173


def _ids_for(R, g):
    ids = torch.randint(0, EMB_TABLE_ROWS, (R,), generator=g)
    ids[-1] = EMB_TABLE_ROWS - 1                                 # the last row of the table ...
    if R > 1:
        ids[0] = 0                                              # ... and the first
    return ids


@pytest.mark.parametrize("source", ["ids64", "ids64_stride5", "ids32", "const_id"])
def test_embed_rows(dev, source):
    """out[r, col0 : col0 + E] = table[id_r] bit for bit, or with a keep mask the fp32 product e * inv_keep / exact 0.0; R * E below and above
    256 and no multiple of it; the row buffer is wider than the window (ldo = col0 + E + 2)."""
    from piano_a2s_amd import hip
    L = hip.lib()
    g = torch.Generator().manual_seed(17)
    inv_keep = 1.25
    for R in (1, 7, 300):
        for E in (1, 16, 20, 65):
            table = torch.randn(EMB_TABLE_ROWS, E, generator=g)
            tabd = table.to(dev)
            for col0 in (0, 3):
                ids = _ids_for(R, g)
                stride, const_id, ids64d, ids32d = 1, -1, None, None
                if source == "ids64":
                    ids64d = ids.to(dev)
                elif source == "ids64_stride5":
                    stride = 5
                    spread = torch.randint(0, EMB_TABLE_ROWS, (R, 5), generator=g)        # the entries between two ids: other valid rows
                    spread[:, 0] = ids
                    ids64d = spread.reshape(-1).to(dev)
                elif source == "ids32":
                    ids32d = ids.to(torch.int32).to(dev)
                else:
                    const_id = EMB_TABLE_ROWS - 1 if col0 == 0 else 0
                    ids = torch.full((R,), const_id, dtype=torch.int64)
                for masked in (False, True):
                    keep = (torch.rand(R, E, generator=g) > 0.3).to(torch.uint8)
                    keepd = keep.to(dev) if masked else None
                    ldo = col0 + E + 2
                    out = torch.full((R, ldo), SENT, device=dev)
                    hip.check(L.a2s_embed_rows(hip.stream(), hip._p(tabd), hip._p(ids64d), hip._p(ids32d), stride, const_id, hip._p(out), ldo, col0, R, E,
                                               hip._p(keepd), inv_keep), "embed_rows")
                    torch.cuda.synchronize()
                    want = torch.full((R, ldo), SENT)
                    rows = table[ids]
                    if masked:
                        rows = torch.where(keep.bool(), rows * torch.tensor(inv_keep, dtype=torch.float32), torch.zeros_like(rows))
                    want[:, col0:col0 + E] = rows
                    assert _same_bits(out, want), (source, R, E, col0, masked)


@pytest.mark.parametrize("source", ["ids32", "const_id"])
def test_embed_scatter_add_remaining_forms(dev, source):
    """a2s_embed_scatter_add with 32-bit ids and with const_id (every row lands on ONE table row: the worst collision), on a table that is
    not zero (it accumulates), against float64 index_add_.  The order of the atomic additions is free: the error is measured per element against
    2^-23 * sum |terms| (the terms being the start value and the g * mask * inv_keep that land there); the bar is stated at the assertion."""
    from piano_a2s_amd import hip
    L = hip.lib()
    g = torch.Generator().manual_seed(23)
    R, E, col0, inv_keep = 300, 20, 3, 1.25
    ldg = col0 + E + 2
    gt = torch.randn(R, ldg, generator=g)
    tab0 = torch.randn(EMB_TABLE_ROWS, E, generator=g)
    masked = source == "ids32"
    keep = (torch.rand(R, E, generator=g) > 0.3).to(torch.uint8)
    ids = torch.randint(0, 9, (R,), generator=g) if source == "ids32" else torch.full((R,), 41, dtype=torch.int64)      # duplicates on purpose
    terms = gt[:, col0:col0 + E].double() * (keep.double() * inv_keep if masked else 1.0)
    ref = tab0.double().index_add_(0, ids, terms)
    mag = tab0.double().abs().index_add_(0, ids, terms.abs())
    tab = tab0.to(dev)
    gtd, keepd = gt.to(dev), keep.to(dev) if masked else None
    ids32d = ids.to(torch.int32).to(dev) if source == "ids32" else None
    hip.check(L.a2s_embed_scatter_add(hip.stream(), hip._p(tab), None, hip._p(ids32d), 1, 41 if source == "const_id" else -1, hip._p(gtd), ldg, col0, R, E,
                                      hip._p(keepd), inv_keep), "scatter")
    torch.cuda.synchronize()
    frac = float(((tab.cpu().double() - ref).abs() / (U23 * mag)).max())
    _report(f"embed_scatter_add {source} (fraction of 2^-23 * sum |terms|)", frac)
    # 2^-23 * sum |terms| alone is too tight for fp32 accumulation itself: on exactly these inputs torch's fp32 index_add_ on the CPU (row order)
    # is off from float64 by 1.17 (ids32) / 0.85 (const_id) of it, and sequential fp32 accumulation over 1000 random row orders reaches
    # 1.65 / 1.72 (above 1 in 19 % / 8 % of the orders).  The order of the atomics is free, so the bar is twice what fp32 on the CPU shows.
    allowed = {"ids32": 2 * 1.65, "const_id": 2 * 1.72}[source]
    assert frac <= allowed, (frac, allowed)
    untouched = torch.ones(EMB_TABLE_ROWS, dtype=torch.bool)
    untouched[ids] = False
    assert _same_bits(tab.cpu()[untouched], tab0[untouched]), "rows no id names must not change"


# ------------------------------------------------------------------------------------------------------------------ a2s_nll_loss / a2s_nll_grad
def _nll_case(rows, V, ignore_index, g):
    """logp (rows, V) and targets; with an ignore_index about a third of the targets are ignored, the first and the last row among them (a single
    row stays valid: the mean over no target is out of scope), and the logp rows of ignored targets are NaN: they must not be read."""
    logp = torch.log_softmax(torch.randn(rows, V, generator=g), dim=1)
    target = torch.randint(0, V, (rows,), generator=g)
    if ignore_index >= 0:
        target[target == ignore_index] = (ignore_index + 1) % V
        ign = torch.rand(rows, generator=g) < 1 / 3
        if rows >= 3:
            ign[0] = ign[-1] = True
            ign[1] = False
        else:
            ign[:] = False
        target[ign] = ignore_index
        logp[ign] = float("nan")
    return logp, target


def _nll_reference(logp, target, ignore_index):
    valid = target != ignore_index
    picked = logp.double()[torch.arange(logp.shape[0])[valid], target[valid]]
    count = int(valid.sum())
    return float(-picked.sum() / count), count, valid


def _nll_grad_expected(rows, V, target, valid, gscale, inv_count_f32, lo=0, hi=None):
    """dlogp: np.float32(-gscale) * loss_out[1] (one fp32 product) at (r, target[r]) of the valid rows in [lo, hi), 0.0 elsewhere."""
    hi = rows if hi is None else hi
    want = torch.zeros(rows, V)
    value = float(np.float32(-gscale) * np.float32(inv_count_f32))
    sel = valid.clone()
    sel[:lo] = False
    sel[hi:] = False
    want[torch.arange(rows)[sel], target[sel]] = value
    return want


@pytest.mark.parametrize("V", [3, 173])
def test_nll_loss_and_gradient(dev, V):
    from piano_a2s_amd import hip
    L = hip.lib()
    g = torch.Generator().manual_seed(31 + V)
    worst = 0.0
    for rows in (1, 255, 256, 257, 1000):
        for ignore_index in (147 if V == 173 else V - 1, -1):
            logp, target = _nll_case(rows, V, ignore_index, g)
            ref, count, valid = _nll_reference(logp, target, ignore_index)
            logpd, targetd = logp.to(dev), target.to(dev)
            for nblocks in (1, 2, 64):
                for gscale in (1.0, 0.25):
                    loss_out = _tail(2, dev, extra=2)
                    partial = _tail(2 * nblocks, dev, extra=2, dtype=torch.float64)
                    dlogp = _flat(torch.zeros(rows, V), dev)
                    hip.check(L.a2s_nll_loss(hip.stream(), hip._p(logpd), hip._p(targetd), rows, V, ignore_index, hip._p(loss_out), hip._p(dlogp), gscale,
                                             hip._p(partial), nblocks), "nll_loss")
                    torch.cuda.synchronize()
                    lo, pa = loss_out.cpu(), partial.cpu()
                    key = (rows, V, ignore_index, nblocks, gscale)
                    # the device sums in double and rounds once to fp32
                    err = abs(float(lo[0]) - ref) / abs(ref)
                    worst = max(worst, err / U23)
                    assert err <= U23, (key, float(lo[0]), ref)
                    assert np.float32(lo[1].item()).tobytes() == np.float32(1.0 / count).tobytes(), (key, float(lo[1]), count)
                    assert _tail_untouched(loss_out, 2) and _tail_untouched(partial, 2 * nblocks), key
                    empty = [b for b in range(nblocks) if b * 256 >= rows]                # blocks without rows: their partials are zero
                    assert all(pa[2 * b] == 0 and pa[2 * b + 1] == 0 for b in empty), key
                    assert float(pa[1:2 * nblocks:2].sum()) == count, key
                    want = _nll_grad_expected(rows, V, target, valid, gscale, lo[1].item())
                    assert _same_bits(dlogp[:rows * V].view(rows, V), want), key
                    assert _tail_untouched(dlogp, rows * V), key
    _report(f"nll_loss V{V} (fraction of 2^-23 |ref|)", worst)


def test_nll_grad_alone_and_loss_without_gradient(dev):
    """a2s_nll_grad over a sub-range of the rows with the caller's loss_out; rows = 0 launches nothing; a2s_nll_loss with dlogp = NULL gives the
    same loss bits in two launches instead of three."""
    from piano_a2s_amd import hip
    L = hip.lib()
    g = torch.Generator().manual_seed(37)
    rows, V, ignore_index, gscale = 1000, 173, 147, 0.25
    logp, target = _nll_case(rows, V, ignore_index, g)
    _, count, valid = _nll_reference(logp, target, ignore_index)
    logpd, targetd = logp.to(dev), target.to(dev)
    inv = np.float32(1.0 / count)
    loss_in = torch.tensor([float("nan"), float(inv)], dtype=torch.float32).to(dev)          # loss_out[0] is not looked at
    lo_row, hi_row = 257, 771
    dlogp = _flat(torch.zeros(rows, V), dev)
    sub = dlogp[lo_row * V:]
    tsub = targetd[lo_row:]
    hip.check(L.a2s_nll_grad(hip.stream(), hip._p(sub), hip._p(tsub), hip._p(loss_in), gscale, hi_row - lo_row, V, ignore_index), "nll_grad")
    torch.cuda.synchronize()
    want = _nll_grad_expected(rows, V, target, valid, gscale, inv, lo_row, hi_row)
    assert _same_bits(dlogp[:rows * V].view(rows, V), want)
    assert _tail_untouched(dlogp, rows * V)
    # rows = 0: success, nothing launched, nothing written
    before = L.a2s_launch_count()
    before_bits = _bits(dlogp).clone()
    assert L.a2s_nll_grad(hip.stream(), hip._p(dlogp), hip._p(targetd), hip._p(loss_in), gscale, 0, V, ignore_index) == 0
    assert L.a2s_launch_count() == before
    torch.cuda.synchronize()
    assert torch.equal(_bits(dlogp), before_bits)
    # dlogp = NULL: the loss alone
    outs = []
    for with_grad in (True, False):
        loss_out = _tail(2, dev, extra=2)
        partial = _tail(2 * 7, dev, extra=2, dtype=torch.float64)
        grad = _flat(torch.zeros(rows, V), dev)
        before = L.a2s_launch_count()
        hip.check(L.a2s_nll_loss(hip.stream(), hip._p(logpd), hip._p(targetd), rows, V, ignore_index, hip._p(loss_out), hip._p(grad) if with_grad else None, gscale,
                                 hip._p(partial), 7), "nll_loss")
        launches = L.a2s_launch_count() - before
        torch.cuda.synchronize()
        assert launches == (3 if with_grad else 2)
        outs.append((loss_out.cpu(), partial.cpu(), grad.cpu()))
    assert _same_bits(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert bool((outs[1][2][:rows * V] == 0).all()) and bool(torch.isfinite(outs[1][0][:2]).all())


# ------------------------------------------------------------------------------------------------------------------ a2s_clip_adadelta
ADA = dict(lr=1.0, rho=0.95, eps=1e-8, max_norm=5.0)
ADA_BIG = 2048 * 256 + 3                         # more elements than the capped grid has threads: the stride loop and its tail


def _ada_gradient(n, scale, g):
    """scale * r with |r| >= 0.2 (so that even a single element at scale 50 has a norm above max_norm)."""
    r = torch.randn(n, generator=g)
    return scale * torch.where(r >= 0, r + 0.2, r - 0.2)


def _ada_call(dev, p, gr, sq, acc, n, loss, ctl, nblocks, zero_grad):
    from piano_a2s_amd import hip
    L = hip.lib()
    partial = _tail(nblocks, dev, extra=2, dtype=torch.float64)
    hip.check(L.a2s_clip_adadelta(hip.stream(), hip._p(p), hip._p(gr), hip._p(sq), hip._p(acc), n, hip._p(loss), ADA["max_norm"], ADA["lr"], ADA["rho"],
                                  ADA["eps"], hip._p(ctl), hip._p(partial), nblocks, zero_grad), "clip_adadelta")
    torch.cuda.synchronize()
    assert _tail_untouched(partial, nblocks)


@pytest.mark.parametrize("scale", [1e-4, 50.0])
@pytest.mark.parametrize("n", [1, 255, 256, 257, ADA_BIG])
def test_clip_adadelta_three_steps(dev, n, scale):
    """Three steps in a row with fresh gradients against clip_grad_norm_ + torch.optim.Adadelta on a float64 CPU parameter: the second and the
    third step start from non-zero square_avg / acc_delta.  Scale 1e-4: never clipped (coefficient exactly 1); scale 50: clipped every step."""
    g = torch.Generator().manual_seed(41 + n % 1000)
    p0 = torch.randn(n, generator=g)
    grads = [_ada_gradient(n, scale, g) for _ in range(3)]
    ref_p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adadelta([ref_p], lr=ADA["lr"], rho=ADA["rho"], eps=ADA["eps"])
    ref_ctl = []
    for gr in grads:
        ref_p.grad = gr.double().clone()
        norm = float(ref_p.grad.norm())
        torch.nn.utils.clip_grad_norm_([ref_p], ADA["max_norm"])
        opt.step()
        ref_ctl.append((norm, min(1.0, ADA["max_norm"] / (norm + 1e-6))))
    ref_sq, ref_acc = opt.state[ref_p]["square_avg"], opt.state[ref_p]["acc_delta"]
    assert all((c < 1.0) == (scale == 50.0) for _, c in ref_ctl)
    ref_p = ref_p.detach()
    worst = dict.fromkeys(("norm", "coef", "square_avg", "acc_delta", "param"), 0.0)
    for nblocks in (1, 7, 1024):
        p, sq, acc = _flat(p0, dev), _flat(torch.zeros(n), dev), _flat(torch.zeros(n), dev)
        loss = torch.tensor([0.75], device=dev)
        for step, gr in enumerate(grads):
            grd, ctl = _flat(gr, dev), _tail(3, dev, extra=2)
            _ada_call(dev, p, grd, sq, acc, n, loss, ctl, nblocks, 1)
            c = ctl.cpu().double()
            norm, coef = ref_ctl[step]
            e_norm, e_coef = abs(float(c[0]) - norm) / norm, abs(float(c[1]) - coef) / coef
            worst["norm"], worst["coef"] = max(worst["norm"], e_norm / U23), max(worst["coef"], e_coef / (4 * U24))
            assert e_norm <= U23, (n, nblocks, step, float(c[0]), norm)
            assert e_coef <= 4 * U24, (n, nblocks, step, float(c[1]), coef)
            assert scale == 50.0 or float(c[1]) == 1.0
            assert float(c[2]) == 1.0 and _tail_untouched(ctl, 3)
            assert bool((grd[:n] == 0).all()) and _tail_untouched(grd, n), "zero_grad = 1 clears every gradient element and nothing else"
        for buf in (p, sq, acc):
            assert _tail_untouched(buf, n)
        pc, sqc, accc = p[:n].cpu().double(), sq[:n].cpu().double(), acc[:n].cpu().double()
        # 2e-6: the suite's fp32 round-off constant; both accumulators are sums of non-negative terms (no cancellation)
        e_sq = float(((sqc - ref_sq).abs() / ref_sq.abs()).max())
        e_acc = float(((accc - ref_acc).abs() / ref_acc.abs()).max())
        # |p - ref| <= 3 * 2^-23 * max(1, |p|) + 2e-6 * |ref - p0|: three subtractions in fp32 plus the relative error of the three updates
        bound_p = 3 * U23 * torch.clamp(ref_p.abs(), min=1.0) + 2e-6 * (ref_p - p0.double()).abs()
        e_p = float(((pc - ref_p).abs() / bound_p).max())
        worst["square_avg"], worst["acc_delta"], worst["param"] = max(worst["square_avg"], e_sq), max(worst["acc_delta"], e_acc), max(worst["param"], e_p)
        assert e_sq <= 2e-6 and e_acc <= 2e-6, (n, nblocks, e_sq, e_acc)
        assert e_p <= 1.0, (n, nblocks, e_p)
    _report(f"clip_adadelta n{n} scale{scale:g} norm (fraction of 2^-23)", worst["norm"])
    _report(f"clip_adadelta n{n} scale{scale:g} coefficient (fraction of 4 * 2^-24)", worst["coef"])
    _report(f"clip_adadelta n{n} scale{scale:g} square_avg after 3 steps (relative, bound 2e-6)", worst["square_avg"])
    _report(f"clip_adadelta n{n} scale{scale:g} acc_delta after 3 steps (relative, bound 2e-6)", worst["acc_delta"])
    _report(f"clip_adadelta n{n} scale{scale:g} parameters after 3 steps (fraction of 3 * 2^-23 max(1, |p|) + 2e-6 |ref - p0|)", worst["param"])


@pytest.mark.parametrize("n", [257, ADA_BIG])
def test_clip_adadelta_flags_and_skipped_steps(dev, n):
    """zero_grad = 0 leaves the gradients bit for bit; loss = NULL applies the step; a NaN or inf loss, or one inf gradient element, skips it:
    ctl[2] == 0, parameters and both accumulators bit-identical, the gradients still cleared when asked (the tail of the large n included)."""
    g = torch.Generator().manual_seed(43)
    p0, sq0, acc0 = torch.randn(n, generator=g), torch.rand(n, generator=g) + 0.1, torch.rand(n, generator=g) * 1e-3 + 1e-6
    gr0 = _ada_gradient(n, 1e-3, g)                               # norm ~ 1e-3 sqrt(n) < max_norm at both sizes: never clipped

    def run(gr, loss_value, zero_grad):
        p, sq, acc, grd, ctl = _flat(p0, dev), _flat(sq0, dev), _flat(acc0, dev), _flat(gr, dev), _tail(3, dev, extra=2)
        loss = None if loss_value is None else torch.tensor([loss_value], device=dev)
        _ada_call(dev, p, grd, sq, acc, n, loss, ctl, 7, zero_grad)
        for buf in (p, sq, acc, grd):
            assert _tail_untouched(buf, n)
        return p[:n].cpu(), sq[:n].cpu(), acc[:n].cpu(), grd[:n].cpu(), ctl[:3].cpu()

    p, sq, acc, grd, ctl = run(gr0, None, 0)                       # loss = NULL, zero_grad = 0
    assert float(ctl[2]) == 1.0 and float(ctl[1]) == 1.0
    assert _same_bits(grd, gr0), "zero_grad = 0 must leave the gradients bit for bit"
    assert not torch.equal(p, p0) and not torch.equal(sq, sq0) and not torch.equal(acc, acc0)
    applied = (p, sq, acc)
    p, sq, acc, grd, ctl = run(gr0, 0.5, 1)                        # the same step with a finite loss: same bits
    assert all(_same_bits(a, b) for a, b in zip((p, sq, acc), applied))
    assert bool((grd == 0).all())
    inf_grad = gr0.clone()
    inf_grad[n - 1] = float("inf")                                  # the very last element: the tail of the stride loop
    for gr, loss_value in ((gr0, float("nan")), (gr0, float("inf")), (inf_grad, 0.5)):
        for zero_grad in (0, 1):
            p, sq, acc, grd, ctl = run(gr, loss_value, zero_grad)
            assert float(ctl[2]) == 0.0, (loss_value, zero_grad)
            assert _same_bits(p, p0) and _same_bits(sq, sq0) and _same_bits(acc, acc0), "a skipped step must not touch parameters or accumulators"
            assert bool((grd == 0).all()) if zero_grad else _same_bits(grd, gr)


# ------------------------------------------------------------------------------------------------------------------ elementwise BatchNorm / activation kernels
def _fraction_of_one_ulp(got, ref):
    """max |got - ref| / (2^-23 * max(1, |ref|)): each result is one FMA, or two roundings.  The kernels meet it because the compiler
    contracts x * scale + shift and 1 - y * y into one FMA each; the same formulas evaluated WITHOUT contraction (plain fp32 torch on the CPU,
    inputs of these tests at the largest sizes) reach 1.03 (BatchNorm + ReLU), 1.38 (with the dropout scale) and 1.14 (tanh backward) of it."""
    return float(((got.double() - ref).abs() / (U23 * torch.clamp(ref.abs(), min=1.0))).max())


@pytest.mark.parametrize("rows,Cc,F", [(3, 20, 24), (5, 40, 7), (2, 3, 1)])
def test_bn_relu_apply(dev, rows, Cc, F):
    from piano_a2s_amd import hip
    L = hip.lib()
    g = torch.Generator().manual_seed(51 + F)
    x = torch.randn(rows, Cc, F, generator=g) * 1.5 + 0.5
    scale, shift = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    ref = torch.relu(x.double() * scale.double().view(1, -1, 1) + shift.double().view(1, -1, 1))
    n = x.numel()
    xd, scd, shd, y = x.to(dev), scale.to(dev), shift.to(dev), _tail(n, dev)
    hip.check(L.a2s_bn_relu_apply(hip.stream(), hip._p(xd), hip._p(y), hip._p(scd), hip._p(shd), n, Cc, F), "bn_relu_apply")
    torch.cuda.synchronize()
    frac = _fraction_of_one_ulp(y[:n].cpu().view(rows, Cc, F), ref)
    _report(f"bn_relu_apply ({rows}, {Cc}, {F}) (fraction of 2^-23 * max(1, |ref|))", frac)
    assert frac <= 1.0, frac
    assert _tail_untouched(y, n)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("rows,Cc", [(1, 256), (37, 20), (300, 3)])
def test_bn1d_relu_dropout(dev, rows, Cc, masked):
    from piano_a2s_amd import hip
    L = hip.lib()
    g = torch.Generator().manual_seed(53 + Cc)
    inv_keep = 1.25
    x = torch.randn(rows, Cc, generator=g) * 1.5 + 0.5
    scale, shift = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    keep = (torch.rand(rows, Cc, generator=g) > 0.2).to(torch.uint8)
    ref = torch.relu(x.double() * scale.double() + shift.double())
    if masked:
        ref = ref * keep.double() * inv_keep
    n = x.numel()
    xd, scd, shd, y = x.to(dev), scale.to(dev), shift.to(dev), _tail(n, dev)
    keepd = keep.to(dev) if masked else None
    hip.check(L.a2s_bn1d_relu_dropout(hip.stream(), hip._p(xd), hip._p(y), hip._p(scd), hip._p(shd), hip._p(keepd), inv_keep, n, Cc), "bn1d_relu_dropout")
    torch.cuda.synchronize()
    got = y[:n].cpu().view(rows, Cc)
    frac = _fraction_of_one_ulp(got, ref)
    _report(f"bn1d_relu_dropout ({rows}, {Cc}) mask={masked} (fraction of 2^-23 * max(1, |ref|))", frac)
    assert frac <= 1.0, frac
    if masked:
        assert bool((_bits(got)[keep == 0] == 0).all()), "dropped elements are exact 0.0"
    assert _tail_untouched(y, n)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("n", [1, 257, ADA_BIG])
def test_ew_act_bwd(dev, n, act, in_place):
    """dx = g * [y > 0] (act 1; y == 0.0 and y == -0.0 give 0) or g * (1 - y^2) (act 2), out of place and in place (dx == g), more elements
    than the capped grid has threads."""
    from piano_a2s_amd import hip
    L = hip.lib()
    g = torch.Generator().manual_seed(57 + act)
    gy = torch.randn(n, generator=g)
    if act == 1:
        y = torch.randn(n, generator=g)
        y[::5] = 0.0
        y[2::7] = -0.0
        if n == 1:
            y[0] = -0.0
        ref = torch.where(y.double() > 0, gy.double(), torch.zeros(n, dtype=torch.float64))
    else:
        y = torch.tanh(torch.randn(n, generator=g) * 1.5)
        ref = gy.double() * (1 - y.double() ** 2)
    gd, yd = _flat(gy, dev), y.to(dev)
    dx = gd if in_place else _tail(n, dev)
    hip.check(L.a2s_ew_act_bwd(hip.stream(), hip._p(gd), hip._p(yd), hip._p(dx), n, act), "ew_act_bwd")
    torch.cuda.synchronize()
    got = dx[:n].cpu()
    frac = _fraction_of_one_ulp(got, ref)
    _report(f"ew_act_bwd n{n} act{act} in_place={in_place} (fraction of 2^-23 * max(1, |ref|))", frac)
    assert frac <= 1.0, frac
    if act == 1:
        assert _same_bits(got, ref.float()), "relu backward passes g through or gives exact 0.0"
    assert _tail_untouched(dx, n)
    if not in_place:
        assert _same_bits(gd[:n], gy) and _tail_untouched(gd, n)


# ------------------------------------------------------------------------------------------------------------------ synchronised BatchNorm backward, two emulated ranks
@pytest.mark.parametrize("layout", ["planes", "cols"])
def test_sync_bn_backward_two_emulated_ranks(dev, layout):
    """The layouts and the autograd reference of test_gpu_bwd_ops.test_bn_relu_dropout_backward over the WHOLE batch, computed in two uneven
    parts as two ranks would: a2s_bn_bwd_stats per part, the sums added (the all-reduce), a2s_bn_bwd_apply per part with its own local sums,
    the global sums and the global element count."""
    from oracle import model_ref
    from piano_a2s_amd import hip
    L = hip.lib()
    g = torch.Generator().manual_seed(8)
    Cc = 20
    if layout == "planes":
        rows, F, split = 14, 24, 5
        x = (torch.randn(rows, Cc, F, generator=g) * 1.5 + 0.5).requires_grad_(True)
        mask = None
    else:
        rows, F, split = 300, 1, 100
        x = (torch.randn(rows, Cc, generator=g) * 1.5 + 0.5).requires_grad_(True)
        mask = (torch.rand(rows, Cc, generator=g) > 0.2).to(torch.uint8)
    P = {"bn.weight": (torch.rand(Cc, generator=g) + 0.5).requires_grad_(True), "bn.bias": (torch.randn(Cc, generator=g) * 0.3).requires_grad_(True)}
    Bf = {"bn.running_mean": torch.zeros(Cc), "bn.running_var": torch.ones(Cc), "bn.num_batches_tracked": torch.tensor(0)}
    y = torch.relu(model_ref.batch_norm(x, P, Bf, "bn", True, channel_dim=1))
    if mask is not None:
        y = y * mask / 0.8
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    dims = [d for d in range(x.dim()) if d != 1]
    mean = x.detach().mean(dims); var = x.detach().var(dims, unbiased=False)
    invstd = 1 / torch.sqrt(var + 1e-5)
    scale = P["bn.weight"].detach() * invstd; shift = P["bn.bias"].detach() - mean * scale
    bn = [t.to(dev) for t in (mean, invstd, scale, shift)]
    xd, gyd = x.detach().to(dev), gy.to(dev)
    maskd = mask.to(dev) if mask is not None else None
    inv_keep = 1 / 0.8
    # the one-rank call over the whole batch: what c12 must come out as
    dgam_w, dbet_w, dx_w = torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev), torch.empty_like(xd)
    part_w = torch.empty(L.a2s_bn_bwd_partial_floats(rows, Cc, F), device=dev)
    c12_w = torch.empty(2 * Cc, device=dev)
    hip.check(L.a2s_bn_bwd(hip.stream(), hip._p(gyd), hip._p(xd), *map(hip._p, bn), hip._p(maskd), inv_keep, hip._p(dgam_w), hip._p(dbet_w), hip._p(dx_w),
                           hip._p(part_w), hip._p(c12_w), rows, Cc, F), "bn_bwd")
    parts = [(0, split), (split, rows)]
    xs, gs = [xd[a:b].contiguous() for a, b in parts], [gyd[a:b].contiguous() for a, b in parts]
    ms = [maskd[a:b].contiguous() if maskd is not None else None for a, b in parts]
    sums = []
    for (a, b), xp, gp, mp in zip(parts, xs, gs, ms):
        part = torch.empty(L.a2s_bn_bwd_partial_floats(b - a, Cc, F), device=dev)
        s = torch.full((2 * Cc + 2,), SENT, device=dev)
        hip.check(L.a2s_bn_bwd_stats(hip.stream(), hip._p(gp), hip._p(xp), *map(hip._p, bn), hip._p(mp), inv_keep, hip._p(part), hip._p(s), b - a, Cc, F), "bn_bwd_stats")
        torch.cuda.synchronize()
        assert bool((s[2 * Cc:] == SENT).all())
        sums.append(s[:2 * Cc].contiguous())
    glob = sums[0] + sums[1]                                   # the all-reduce
    dxs, dgams, dbets, c12s = [], [], [], []
    for (a, b), xp, gp, mp, local in zip(parts, xs, gs, ms, sums):
        dgam, dbet, c12 = torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev), torch.empty(2 * Cc, device=dev)
        dx = torch.full((xp.numel() + 5,), SENT, device=dev)
        hip.check(L.a2s_bn_bwd_apply(hip.stream(), hip._p(gp), hip._p(xp), *map(hip._p, bn), hip._p(mp), inv_keep, hip._p(local), hip._p(glob), float(rows * F),
                                     hip._p(dgam), hip._p(dbet), hip._p(dx), hip._p(c12), b - a, Cc, F), "bn_bwd_apply")
        torch.cuda.synchronize()
        assert _tail_untouched(dx, xp.numel())
        dxs.append(dx[:xp.numel()].view(xp.shape)); dgams.append(dgam); dbets.append(dbet); c12s.append(c12)
    errs = {"dx": _rel(torch.cat(dxs), x.grad), "dgamma": _rel(dgams[0] + dgams[1], P["bn.weight"].grad), "dbeta": _rel(dbets[0] + dbets[1], P["bn.bias"].grad)}
    c12_err = max(_rel(c, c12_w) for c in c12s)
    for k, e in errs.items():
        _report(f"sync bn_bwd two ranks {layout} {k}", e)
    _report(f"sync bn_bwd two ranks {layout} c12 vs one rank", c12_err)
    assert max(errs.values()) < 2e-5, errs
    assert c12_err < 2e-6, c12_err


def test_sync_bn_backward_from_partials_two_emulated_ranks(dev):
    """The statistics-only pair a2s_bn_bwd_sums_from_partial + a2s_bn_bwd_c12_from_sums, as hip.bn_bwd_sync wires it: each rank's partials come
    from the epilogue of its own data-gradient convolution (a2s_conv3x3_dgrad_bnstats, 40 -> 20 channels, clips 1 + 2 of T = 5, F = 24);
    c12, dgamma and dbeta must be those of a2s_bn_bwd_from_partial over the whole batch."""
    from piano_a2s_amd import hip
    L = hip.lib()
    g = torch.Generator().manual_seed(61)
    B, T, F, Cin, Cout = 3, 5, 24, 40, 20
    dy = torch.randn(B, T, Cin, F, generator=g)
    w = torch.randn(Cin, Cout, 3, 3, generator=g) * 0.2
    yl = torch.randn(B, T, Cout, F, generator=g)
    mean, invstd = torch.randn(Cout, generator=g) * 0.1, torch.rand(Cout, generator=g) + 0.5
    bsc, bsh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.3
    bn = [t.to(dev) for t in (mean, invstd, bsc, bsh)]
    wd, cws = w.to(dev), hip.conv_workspace(Cin, dev)

    def dgrad(dy_part, yl_part):
        b = dy_part.shape[0]
        dyd, yld = dy_part.contiguous().to(dev), yl_part.contiguous().to(dev)
        gout = torch.empty(b, T, Cout, F, device=dev)
        nblk = L.a2s_conv3x3_stat_blocks(b, T, F, Cin)
        part = torch.zeros(nblk, Cout, 2, device=dev)
        hip.check(L.a2s_conv3x3_dgrad_bnstats(hip.stream(), hip._p(dyd), hip._p(wd), hip._p(gout), hip._p(yld), *map(hip._p, bn), hip._p(part), b, T, F, Cin, Cout,
                                              hip._p(cws)), "dgrad_bnstats")
        torch.cuda.synchronize()
        return gout, yld, part, nblk

    count = float(B * T * F)
    gw, ylw, partw, nblkw = dgrad(dy, yl)
    dgam_w, dbet_w, c12_w = torch.zeros(Cout, device=dev), torch.zeros(Cout, device=dev), torch.empty(2 * Cout, device=dev)
    hip.check(L.a2s_bn_bwd_from_partial(hip.stream(), hip._p(gw), hip._p(ylw), *map(hip._p, bn), hip._p(dgam_w), hip._p(dbet_w), None, hip._p(partw), nblkw,
                                        hip._p(c12_w), B * T, Cout, F), "bn_bwd_from_partial")
    halves = [dgrad(dy[:1], yl[:1]), dgrad(dy[1:], yl[1:])]
    sums = []
    for _, _, part, nblk in halves:
        s = torch.full((2 * Cout + 2,), SENT, device=dev)
        hip.check(L.a2s_bn_bwd_sums_from_partial(hip.stream(), hip._p(part), nblk, Cout, hip._p(s)), "sums_from_partial")
        torch.cuda.synchronize()
        assert bool((s[2 * Cout:] == SENT).all())
        sums.append(s[:2 * Cout].contiguous())
    glob = sums[0] + sums[1]                                   # the all-reduce
    dgams, dbets, c12s = [], [], []
    for local in sums:
        dgam, dbet, c12 = torch.zeros(Cout, device=dev), torch.zeros(Cout, device=dev), torch.full((2 * Cout + 2,), SENT, device=dev)
        hip.check(L.a2s_bn_bwd_c12_from_sums(hip.stream(), hip._p(local), hip._p(glob), count, hip._p(dgam), hip._p(dbet), hip._p(c12), Cout), "c12_from_sums")
        torch.cuda.synchronize()
        assert bool((c12[2 * Cout:] == SENT).all())
        dgams.append(dgam); dbets.append(dbet); c12s.append(c12[:2 * Cout])
    errs = {"c12": max(_rel(c, c12_w) for c in c12s), "dgamma": _rel(dgams[0] + dgams[1], dgam_w), "dbeta": _rel(dbets[0] + dbets[1], dbet_w)}
    for k, e in errs.items():
        _report(f"sync bn_bwd from partials two ranks {k}", e)
    assert max(errs.values()) < 2e-5, errs
