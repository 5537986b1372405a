"""conv3x3_rows16 with the input rows staged by the narrow-group waves alone (csrc/a2s_conv_rows.hip, template flag SN; a2s_debug_set
("conv_rows_stage", 1); on by default, which is 3) against the form in which every thread stages ("conv_rows_stage" = 0) and against
torch.nn.functional.conv2d in float64 on the CPU, through the C entry points the engine uses:

  fwd2020 / fwd2040 / fwd4040        forward with input affine, batch statistics and out_absmax   (a2s_conv3x3_ranged)
  dgrad4040 / dgrad4020              data gradient with BatchNorm-backward statistics and out_absmax   (a2s_conv3x3_dgrad_bnstats_ranged)
  dgrad2020                          data gradient with BatchNorm-backward statistics, no out_absmax   (a2s_conv3x3_dgrad_bnstats_scaled)
  flip4020 / flip4040                plain flip launch   (a2s_conv3x3, flip = 1)

under "conv_rows" = 7 and 15 (two accumulator sets for the forward; for the data gradient too).  Only the thread that converts an element
differs between the two settings, so y, the statistics partials and out_absmax must be BIT-equal; the counter "conv_rows_stage_launches"
proves the path.  Bars against float64 and shapes: those of tests/test_gpu_conv_rows16_c20.py (one column tile with most staging columns
masked and clip offsets; strips shorter than the ring prologue; a second column tile of a single quad; four column tiles with two row
strips, the first starting at t = 0; a ragged last tile with B > 1).  Inputs: randn * exp(randn); outputs pre-filled with NaN."""
import ctypes as C
import functools

import pytest
import torch

NULL = C.c_void_p(0)
pytestmark = pytest.mark.gpu

SHAPES = [(2, 9, 24), (1, 1, 120), (1, 2, 120), (1, 6, 124), (1, 41, 480), (2, 33, 244)]
# mode -> (kind, Cin, Cout) of the launch (data gradient: channels of dy -> channels of dx)
MODES = {"fwd2020": ("fwd", 20, 20), "fwd2040": ("fwd", 20, 40), "fwd4040": ("fwd", 40, 40),
         "dgrad4040": ("dgrad_ranged", 40, 40), "dgrad4020": ("dgrad_ranged", 40, 20), "dgrad2020": ("dgrad_scaled", 20, 20),
         "flip4020": ("flip", 40, 20), "flip4040": ("flip", 40, 40)}
COUNTER = b"conv_rows_stage_launches"


def _ships(mode, conv_rows):
    """The launcher keeps the all-thread form, and builds no other, for the instances whose narrow-staging form did not measure faster
    (rows16_stage_narrow, csrc/a2s_conv_rows.hip): the 20 -> 20 data gradient and the two-set 40 -> 20 data gradient."""
    return not (mode == "dgrad2020" or (mode == "dgrad4020" and conv_rows & 8))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ch(t):
    return t.double().view(1, -1, 1, 1)          # per-channel vector over (B, C, T, F)


@functools.lru_cache(maxsize=None)
def _case(mode, B, T, F):
    """Inputs and the float64 reference of one (mode, shape): built once, shared by the conv_rows values, never modified."""
    kind, Cin, Cout = MODES[mode]
    g = torch.Generator().manual_seed(Cin * 100 + Cout + 7 * T + F + len(kind))
    x = torch.randn(B, T, Cin, F, generator=g) * torch.exp(torch.randn(B, T, Cin, F, generator=g))
    fwd = kind == "fwd"
    w = torch.randn((Cout, Cin, 3, 3) if fwd else (Cin, Cout, 3, 3), generator=g) * 0.2
    scale, shift = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.3
    yl = torch.randn(B, T, Cout, F, generator=g)
    mean, invstd = torch.randn(Cout, generator=g) * 0.1, torch.rand(Cout, generator=g) + 0.5
    bsc, bsh = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.3
    x64 = x.double().permute(0, 2, 1, 3)
    if fwd:
        x64 = torch.relu(x64 * _ch(scale) + _ch(shift))
    w64 = w.double() if fwd else w.double().transpose(0, 1).flip(2, 3)
    ref = torch.nn.functional.conv2d(x64, w64, padding=1).permute(0, 2, 1, 3).contiguous()
    mag = torch.nn.functional.conv2d(x64.abs(), w64.abs(), padding=1).permute(0, 2, 1, 3) + 1e-30
    return dict(x=x, w=w, scale=scale, shift=shift, yl=yl, mean=mean, invstd=invstd, bsc=bsc, bsh=bsh, ref=ref, mag=mag)


def _launch(L, hip, dev, mode, d, B, T, F):
    """One launch of `mode` on the device tensors d; returns (y, statistics partials or None, out_absmax or None)."""
    kind, Cin, Cout = MODES[mode]
    y = torch.full((B, T, Cout, F), float("nan"), device=dev)
    part = torch.full((L.a2s_conv3x3_stat_blocks(B, T, F, Cin), Cout, 2), float("nan"), device=dev)
    amax = torch.full((Cout,), 1e30, device=dev)
    cws = hip.conv_workspace(Cin, dev)
    p = hip._p
    bn = (p(d["yl"]), p(d["mean"]), p(d["invstd"]), p(d["bsc"]), p(d["bsh"]))
    if kind == "fwd":
        hip.check(L.a2s_conv3x3_ranged(hip.stream(), p(d["x"]), p(d["w"]), p(y), p(d["scale"]), p(d["shift"]), NULL, p(part), p(amax),
                                       B, T, F, Cin, Cout, p(cws)), "conv3x3_ranged")
    elif kind == "dgrad_ranged":
        xmax = hip.absmax(d["x"])
        hip.check(L.a2s_conv3x3_dgrad_bnstats_ranged(hip.stream(), p(d["x"]), p(d["w"]), p(y), *bn, p(part), B, T, F, Cin, Cout, p(cws), p(xmax),
                                                     p(amax)), "dgrad_bnstats_ranged")
    elif kind == "dgrad_scaled":
        xmax = hip.absmax(d["x"])
        hip.check(L.a2s_conv3x3_dgrad_bnstats_scaled(hip.stream(), p(d["x"]), p(d["w"]), p(y), *bn, p(part), B, T, F, Cin, Cout, p(cws), p(xmax)),
                  "dgrad_bnstats_scaled")
        amax = None
    else:
        hip.check(L.a2s_conv3x3(hip.stream(), p(d["x"]), p(d["w"]), p(y), NULL, NULL, NULL, B, T, F, Cin, Cout, 1, p(cws)), "conv3x3 flip")
        part = amax = None
    torch.cuda.synchronize()
    return y, part, amax


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("conv_rows", [7, 15])
@pytest.mark.parametrize("B,T,F", SHAPES)
@pytest.mark.parametrize("mode", list(MODES))
def test_narrow_staging_bit_equal_and_against_float64(dev, mode, B, T, F, conv_rows):
    from piano_a2s_amd import hip
    L = hip.lib()
    kind = MODES[mode][0]
    c = _case(mode, B, T, F)
    ref, mag = c["ref"], c["mag"]
    d = {k: c[k].to(dev) for k in ("x", "w", "scale", "shift", "yl", "mean", "invstd", "bsc", "bsh")}
    prev_rows, prev_stage = L.a2s_debug_get(b"conv_rows"), L.a2s_debug_get(b"conv_rows_stage")
    assert prev_stage & 1, prev_stage                                   # the default keeps the narrow-staging form on
    hip.check(L.a2s_debug_set(b"conv_rows", conv_rows), "debug_set")
    try:
        res, launched = {}, {}
        for stage in (0, 1):
            hip.check(L.a2s_debug_set(b"conv_rows_stage", stage), "debug_set")
            assert L.a2s_debug_get(b"conv_rows_stage") == stage
            before = L.a2s_debug_get(COUNTER)
            res[stage] = _launch(L, hip, dev, mode, d, B, T, F)
            launched[stage] = L.a2s_debug_get(COUNTER) - before
    finally:
        hip.check(L.a2s_debug_set(b"conv_rows", prev_rows), "debug_set")
        hip.check(L.a2s_debug_set(b"conv_rows_stage", prev_stage), "debug_set")
    assert launched == {0: 0, 1: int(_ships(mode, conv_rows))}, launched   # the narrow-staging instance ran once, and only when asked for
    (y0, part0, amax0), (y, part, amax) = res[0], res[1]
    assert not torch.isnan(y).any() and not torch.isnan(y0).any()       # every element of the NaN-filled outputs was written
    assert torch.equal(_bits(y), _bits(y0))
    if part is not None:
        assert torch.equal(_bits(part), _bits(part0))
    if amax is not None:
        assert torch.equal(_bits(amax), _bits(amax0))
    y64 = y.cpu().double()
    err = float(((y64 - ref).abs() / mag).max())
    rel = float((y64 - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    print(f"rows16 stage {mode} B{B} T{T} F{F} conv_rows {conv_rows}: err {err:.2e} (vs sum|a||b|), rel {rel:.2e}")
    assert err < 2e-6, err
    assert rel < 5e-6, rel
    if amax is not None:
        assert torch.equal(amax, y.abs().amax(dim=(0, 1, 3))), (amax, y.abs().amax(dim=(0, 1, 3)))
    if part is None:
        return
    assert torch.isfinite(part).all()
    sums = part.cpu().double().sum(0)
    if kind == "fwd":
        ref_s, ref_s2 = ref.sum(dim=(0, 1, 3)), (ref ** 2).sum(dim=(0, 1, 3))
        e1, e2 = float((sums[:, 0] - ref_s).abs().max()), float((sums[:, 1] - ref_s2).abs().max())
        print(f"    statistics: sum {e1:.2e} (bar {1e-3 * float(ref_s.abs().max().clamp_min(1.0)):.2e}), sumsq {e2:.2e} (bar {1e-4 * float(ref_s2.abs().max()):.2e})")
        assert e1 < 1e-3 * float(ref_s.abs().max().clamp_min(1.0))
        assert e2 < 1e-4 * float(ref_s2.abs().max())
    else:
        yl = c["yl"].double()
        on = (yl * c["bsc"].double().view(1, 1, -1, 1) + c["bsh"].double().view(1, 1, -1, 1)) > 0
        gm = torch.where(on, ref, torch.zeros_like(ref))
        xhat = (yl - c["mean"].double().view(1, 1, -1, 1)) * c["invstd"].double().view(1, 1, -1, 1)
        ref_s, ref_s2 = gm.sum(dim=(0, 1, 3)), (gm * xhat).sum(dim=(0, 1, 3))
        scale_s = float(torch.where(on, mag, torch.zeros_like(mag)).sum(dim=(0, 1, 3)).max())
        e1, e2 = float((sums[:, 0] - ref_s).abs().max()), float((sums[:, 1] - ref_s2).abs().max())
        print(f"    statistics: sum g' {e1 / scale_s:.2e}, sum g' xhat {e2 / (scale_s * float(xhat.abs().max())):.2e} (bar 1e-5)")
        assert e1 < 1e-5 * scale_s
        assert e2 < 1e-5 * scale_s * float(xhat.abs().max())


def test_bit1_runs_the_two_set_data_gradient_at_40_40(dev):
    """"conv_rows_stage" = 3 (the default) under "conv_rows" = 7 launches the same instance for the 40 -> 40 data gradient as
    "conv_rows" = 15 with "conv_rows_stage" = 1: two accumulator sets, rows staged by the narrow waves."""
    from piano_a2s_amd import hip
    L = hip.lib()
    B, T, F = 1, 41, 480
    c = _case("dgrad4040", B, T, F)
    d = {k: c[k].to(dev) for k in ("x", "w", "scale", "shift", "yl", "mean", "invstd", "bsc", "bsh")}
    prev_rows, prev_stage = L.a2s_debug_get(b"conv_rows"), L.a2s_debug_get(b"conv_rows_stage")
    assert prev_stage == 3, prev_stage
    try:
        res = []
        for rows, stage in ((7, 3), (15, 1), (7, 1)):
            hip.check(L.a2s_debug_set(b"conv_rows", rows), "debug_set")
            hip.check(L.a2s_debug_set(b"conv_rows_stage", stage), "debug_set")
            before = L.a2s_debug_get(COUNTER)
            res.append(_launch(L, hip, dev, "dgrad4040", d, B, T, F))
            assert L.a2s_debug_get(COUNTER) - before == 1
    finally:
        hip.check(L.a2s_debug_set(b"conv_rows", prev_rows), "debug_set")
        hip.check(L.a2s_debug_set(b"conv_rows_stage", prev_stage), "debug_set")
    for a, b in zip(res[0], res[1]):
        assert torch.equal(_bits(a), _bits(b))
    # the one-set form computes the same outputs (the epilogue's arithmetic per element is the same); its statistics add in another order
    assert torch.equal(_bits(res[0][0]), _bits(res[2][0]))
    assert torch.equal(_bits(res[0][2]), _bits(res[2][2]))
