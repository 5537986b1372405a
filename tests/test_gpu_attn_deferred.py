"""The deferred attention gradients on their live-pair kernels (a2s_debug_set("attn_deferred_fast", 1), the default): attn_dk_accum_ahead must
give the bits of attn_dk_accum, a2s_attn_denc_accum the batched GEMM's dEnc within the noise of two correct fp32 sums, and neither may read
a row of a finished (step, bar) pair -- those rows hold NaN here.  NB raw pointers do not keep tensors alive: every operand has a local name."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

H, CLIPS = 256, 3
# (T, groups, S): frames that are no multiple of 16 or 64, one and several frame tiles; fewer pairs than one block of the dK kernel and a count
# that is no multiple of it; the last case has more candidate pairs (540) than one compaction round of the kernels takes (512)
SHAPES = [(T, g, S) for T in (37, 130) for g in (1, 3) for S in (5, 21)] + [(37, 3, 180)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def fast_switch():
    from piano_a2s_amd import hip
    L = hip.lib()

    def set_(on):
        hip.check(L.a2s_debug_set(b"attn_deferred_fast", 1 if on else 0), "a2s_debug_set")
    yield set_
    set_(True)


def _until(S, groups):
    """Steps each (bar, clip) row ran: 0 (never), S (to the end) and values in between, different for the bars of one clip."""
    base = [0, S, S // 2, S, 1, S - 1, 2, 0, S]
    return torch.tensor(base[:groups * CLIPS], dtype=torch.int32)


def _inputs(dev, T, groups, S, masked):
    g = torch.Generator().manual_seed(1000 * T + 10 * S + groups)
    R = groups * CLIPS
    d = {"K": torch.exp(2 * 0.5 * torch.randn(CLIPS, T, H, generator=g)),          # the kernels take the key image exp(2K)
         "q": torch.randn(S, R, H, generator=g), "ds": torch.randn(S, R, T, generator=g) * 0.1, "v": torch.randn(H, generator=g),
         "attw": torch.rand(S, R, T, generator=g) / 8, "dctx": torch.randn(S, R, 2 * H, generator=g),
         "dK0": torch.randn(CLIPS, T, H, generator=g), "dEnc0": torch.randn(CLIPS, T, 2 * H, generator=g)}
    d = {k: t.to(dev) for k, t in d.items()}
    until = _until(S, groups).to(dev) if masked else None
    live = (torch.arange(S, device=dev).unsqueeze(1) < until.unsqueeze(0)) if masked else torch.ones(S, R, dtype=torch.bool, device=dev)
    return d, until, live


def _finished(t, live, value):
    return torch.where(live.unsqueeze(-1), t, torch.full_like(t, value))


@pytest.mark.parametrize("masked", [True, False], ids=["row_until", "no_row_until"])
@pytest.mark.parametrize("T,groups,S", SHAPES)
def test_dk_and_dv_partials_are_bit_equal(dev, fast_switch, T, groups, S, masked):
    from piano_a2s_amd import hip
    L = hip.lib()
    d, until, live = _inputs(dev, T, groups, S, masked)
    ds = _finished(d["ds"], live, float("nan"))
    nblk = L.a2s_attn_dk_blocks(CLIPS, T)
    got = {}
    for on in (True, False):
        fast_switch(on)
        n0 = L.a2s_debug_get(b"attn_dk_ahead_launches")
        dK, dvp = d["dK0"].clone(), torch.full((nblk, H), 3.0, device=dev)
        hip.check(L.a2s_attn_dk_accum(hip.stream(), hip._p(d["K"]), hip._p(d["q"]), hip._p(ds), hip._p(d["v"]), hip._p(dK), hip._p(dvp),
                                      CLIPS, T, S, H, hip._p(until), groups), "a2s_attn_dk_accum")
        torch.cuda.synchronize()
        assert L.a2s_debug_get(b"attn_dk_ahead_launches") - n0 == (1 if on else 0)
        got[on] = (dK, dvp)
    assert torch.isfinite(got[False][0]).all() and torch.isfinite(got[False][1]).all()
    assert not torch.equal(got[False][0], d["dK0"]) or not bool(live.any())
    assert torch.equal(got[True][0], got[False][0]), "dK differs from attn_dk_accum"
    assert torch.equal(got[True][1], got[False][1]), "dv partials differ from attn_dk_accum"


@pytest.mark.parametrize("masked", [True, False], ids=["row_until", "no_row_until"])
@pytest.mark.parametrize("T,groups,S", SHAPES)
def test_denc_against_float64_and_the_batched_gemm(dev, fast_switch, T, groups, S, masked):
    """Reference: the sum over the live pairs in float64.  The new kernel's maximum error relative to max |dEnc| may be at most twice the
    batched GEMM's on the same inputs (two correct fp32 sums in different orders).  Both figures are printed and appended to
    attn_deferred_check.txt in the directory A2S_TEST_REPORT_DIR names (default: test_reports/, ignored by git); profiles/attn_deferred_check.txt
    keeps the lines of a run on the MI355X."""
    from piano_a2s_amd import engine_bwd, hip
    L = hip.lib()
    d, until, live = _inputs(dev, T, groups, S, masked)
    R = groups * CLIPS
    a0, c0 = _finished(d["attw"], live, 0.0), _finished(d["dctx"], live, 0.0)
    ref = d["dEnc0"].double() + torch.einsum("sgbt,sgbd->btd", a0.double().view(S, groups, CLIPS, T), c0.double().view(S, groups, CLIPS, 2 * H))
    scale = float(ref.abs().max())
    Sd, active = {"a.v.weight": d["v"]}, ({"until": until} if masked else None)
    err = {}
    for on in (True, False):
        fast_switch(on)
        n0 = L.a2s_debug_get(b"attn_denc_launches")
        # the new kernel gets NaN in every row of a finished pair; the GEMM reads those rows, so it gets the zeros a real run leaves there
        attw, dctx = (_finished(d["attw"], live, float("nan")), _finished(d["dctx"], live, float("nan"))) if on else (a0, c0)
        ds = _finished(d["ds"], live, float("nan"))
        dK, dEnc, G = d["dK0"].clone(), d["dEnc0"].clone(), {"a.v.weight": torch.zeros(H, device=dev)}
        engine_bwd._attn_deferred(None, Sd, G, "a", d["K"], d["K"], d["q"], ds, attw, dctx, dK, dEnc, CLIPS, T, H, S, active, groups)
        torch.cuda.synchronize()
        assert L.a2s_debug_get(b"attn_denc_launches") - n0 == (1 if on else 0), "the live-pair dEnc kernel ran exactly when the switch is on"
        assert torch.isfinite(dEnc).all() and torch.isfinite(dK).all() and torch.isfinite(G["a.v.weight"]).all()
        err[on] = float((dEnc.double() - ref).abs().max()) / scale
    line = f"dEnc T{T} groups{groups} S{S} {'row_until' if masked else 'all live'}: live-pair kernel {err[True]:.3e}  batched GEMM {err[False]:.3e}  (of max |dEnc| = {scale:.3e})"
    print(line)
    out = os.environ.get("A2S_TEST_REPORT_DIR", "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "attn_deferred_check.txt"), "a") as f:
        f.write(line + "\n")
    assert R == live.shape[1]
    assert err[True] <= 2 * err[False], line


def test_denc_entry_refuses_other_widths(dev):
    from piano_a2s_amd import hip
    L = hip.lib()
    x = torch.zeros(16, device=dev)
    assert L.a2s_attn_denc_accum(hip.stream(), hip._p(x), hip._p(x), hip._p(x), 1, 1, 1, 256, C.c_void_p(0), 1) != 0
    assert b"512" in L.a2s_last_error()
