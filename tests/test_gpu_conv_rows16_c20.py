"""conv3x3_rows16 with 20 output channels (csrc/a2s_conv_rows.hip: one group of 16 channels + a narrow group of 4 in one n-tile) against
torch.nn.functional.conv2d in float64 on the CPU, through the C entry points the engine uses:

  fwd        20 -> 20 forward with input affine, batch statistics and out_absmax   (a2s_conv3x3_ranged)
  dgrad      40 -> 20 data gradient with BatchNorm-backward statistics and out_absmax   (a2s_conv3x3_dgrad_bnstats_ranged)
  dgrad2020  20 -> 20 data gradient with BatchNorm-backward statistics, no out_absmax   (a2s_conv3x3_dgrad_bnstats_scaled)
  flip       40 -> 20 plain flip launch   (a2s_conv3x3, flip = 1)

under "conv_rows" = 3 / 7 / 15 (one accumulator set; two sets for the forward; two sets for the data gradient too).  Bars: those of
tests/test_gpu_ops.py::test_conv3x3_split_operand_kernel for the values and the statistics, tests/test_gpu_operand_ranges.py's exact
equality for out_absmax.  Shapes: one column tile with most columns masked and clip offsets; strips shorter than the ring prologue; a
second column tile of a single quad; four column tiles with two row strips (22 + 19 rows: both strip boundaries, both parities of the
two-set tail); a ragged last tile with B > 1.  Inputs: randn * exp(randn)."""
import ctypes as C
import functools

import pytest
import torch

NULL = C.c_void_p(0)
pytestmark = pytest.mark.gpu

SHAPES = [(2, 9, 24), (1, 1, 120), (1, 2, 120), (1, 6, 124), (1, 41, 480), (2, 33, 244)]
MODES = {"fwd": (20, 20), "dgrad": (40, 20), "dgrad2020": (20, 20), "flip": (40, 20)}
COUNTER = b"conv_rows16_c20_launches"


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
    Cin, Cout = MODES[mode]
    g = torch.Generator().manual_seed(Cin * 100 + Cout + 7 * T + F + len(mode))
    x = torch.randn(B, T, Cin, F, generator=g) * torch.exp(torch.randn(B, T, Cin, F, generator=g))
    fwd = mode == "fwd"
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


def _launch(L, hip, dev, mode, c, B, T, F):
    """One launch of `mode`; returns (y, statistics partials or None, out_absmax or None)."""
    Cin, Cout = MODES[mode]
    d = {k: c[k].to(dev) for k in ("x", "w", "scale", "shift", "yl", "mean", "invstd", "bsc", "bsh")}
    y = torch.full((B, T, Cout, F), float("nan"), device=dev)
    part = torch.full((L.a2s_conv3x3_stat_blocks(B, T, F, Cin), Cout, 2), float("nan"), device=dev)
    amax = torch.full((Cout,), 1e30, device=dev)
    cws = hip.conv_workspace(Cin, dev)
    p = hip._p
    bn = (p(d["yl"]), p(d["mean"]), p(d["invstd"]), p(d["bsc"]), p(d["bsh"]))
    if mode == "fwd":
        hip.check(L.a2s_conv3x3_ranged(hip.stream(), p(d["x"]), p(d["w"]), p(y), p(d["scale"]), p(d["shift"]), NULL, p(part), p(amax),
                                       B, T, F, Cin, Cout, p(cws)), "conv3x3_ranged")
    elif mode == "dgrad":
        xmax = hip.absmax(d["x"])
        hip.check(L.a2s_conv3x3_dgrad_bnstats_ranged(hip.stream(), p(d["x"]), p(d["w"]), p(y), *bn, p(part), B, T, F, Cin, Cout, p(cws), p(xmax),
                                                     p(amax)), "dgrad_bnstats_ranged")
    elif mode == "dgrad2020":
        xmax = hip.absmax(d["x"])
        hip.check(L.a2s_conv3x3_dgrad_bnstats_scaled(hip.stream(), p(d["x"]), p(d["w"]), p(y), *bn, p(part), B, T, F, Cin, Cout, p(cws), p(xmax)),
                  "dgrad_bnstats_scaled")
        amax = None
    else:
        hip.check(L.a2s_conv3x3(hip.stream(), p(d["x"]), p(d["w"]), p(y), NULL, NULL, NULL, B, T, F, Cin, Cout, 1, p(cws)), "conv3x3 flip")
        part = amax = None
    torch.cuda.synchronize()
    return y, part, amax


@pytest.mark.parametrize("conv_rows", [3, 7, 15])
@pytest.mark.parametrize("B,T,F", SHAPES)
@pytest.mark.parametrize("mode", list(MODES))
def test_rows16_c20_against_float64(dev, mode, B, T, F, conv_rows):
    from piano_a2s_amd import hip
    L = hip.lib()
    c = _case(mode, B, T, F)
    ref, mag = c["ref"], c["mag"]
    previous = L.a2s_debug_get(b"conv_rows")
    hip.check(L.a2s_debug_set(b"conv_rows", conv_rows), "debug_set")
    try:
        before = L.a2s_debug_get(COUNTER)
        y, part, amax = _launch(L, hip, dev, mode, c, B, T, F)
        launched = L.a2s_debug_get(COUNTER) - before
    finally:
        hip.check(L.a2s_debug_set(b"conv_rows", previous), "debug_set")
    assert launched == 1, launched                                      # the 20-channel rows16 instance ran, once
    assert not torch.isnan(y).any()                                     # every element of the NaN-filled output was written
    y64 = y.cpu().double()
    err = float(((y64 - ref).abs() / mag).max())
    rel = float((y64 - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    print(f"rows16 c20 {mode} B{B} T{T} F{F} conv_rows {conv_rows}: err {err:.2e} (vs sum|a||b|), rel {rel:.2e}")
    assert err < 2e-6, err
    assert rel < 5e-6, rel
    if amax is not None:
        assert torch.equal(amax, y.abs().amax(dim=(0, 1, 3))), (amax, y.abs().amax(dim=(0, 1, 3)))
    if part is None:
        return
    assert torch.isfinite(part).all()
    sums = part.cpu().double().sum(0)
    if mode == "fwd":
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


def test_first_generation_switch_does_not_take_the_rows16_path(dev):
    """"conv_rows" = 1 keeps every 20-channel launch on conv3x3_rows: the counter does not move."""
    from piano_a2s_amd import hip
    L = hip.lib()
    B, T, F = SHAPES[0]
    previous = L.a2s_debug_get(b"conv_rows")
    hip.check(L.a2s_debug_set(b"conv_rows", 1), "debug_set")
    try:
        before = L.a2s_debug_get(COUNTER)
        for mode in MODES:
            y, _, _ = _launch(L, hip, dev, mode, _case(mode, B, T, F), B, T, F)
            assert not torch.isnan(y).any()
        assert L.a2s_debug_get(COUNTER) == before
    finally:
        hip.check(L.a2s_debug_set(b"conv_rows", previous), "debug_set")
