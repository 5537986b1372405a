"""The VQT front end on the MI355X kernel by kernel (csrc/a2s_vqt.hip, the framed form of a2s_gemm_f32, the host glue of piano_a2s_amd/vqt.py), each
against its float64 restatement in tests/vqt_ops_oracle.py (pinned to oracle/vqt_ref.py by tests/test_vqt_ops_oracle_cpu.py):

1. a2s_vqt_decimate: the workgroup edges, tap counts, rows shorter than the last window (nothing of a neighbouring clip is read), refusals;
2. a2s_vqt_logmag and a2s_vqt_logmag_octaves: each clip's own maximum, the floor, the clamp, both layouts, refusals;
3. the framed GEMM as VQT.__call__ launches it: overlapping rows, a shared row-contiguous bank, a column block of a wider row, on every tile;
4. the host glue: VQT._decimate against the oracle's decimator, the whole front end at the shortest inputs.

Outputs are poisoned with NaN and have NaN guards around them; every measured error goes, beside its bound, to the report
tests/test_gpu_vqt.py writes (vqt_errors.txt), through that module's own _log."""
import numpy as np
import pytest
import torch

from tests import vqt_ops_oracle as O
from tests.test_gpu_vqt import _log                     # one report of the front end's errors, one place that names it

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC00000
GUARD = 64                                              # floats of NaN in front of and behind every output

# 1. n sequential fp32 FMAs: |out - exact| <= n 2^-24 sum |y||h| (to first order; the three zero taps of the padded product filter leave room for the
# rounding of its taps to float32).  A dropped or shifted O(1) tap costs about 1 / ntaps of that sum: 3e-3 at 364 taps, against 2.2e-5.
# Measured on the MI355X: at most 2.6e-7 with random taps (n_out 2052, 62 taps), 8.1e-7 with the product filter, 8.3e-7 through VQT._decimate.
# 2. both 20 log10f terms are at most 100 in magnitude, so one unit of the result is ulp(128) / 80 = 2^-17 / 80 = 9.5e-8.  The bound is (2 E + 3)
# units: two logarithms E units off each, and the roundings of the magnitude, the difference and the final sum.  The ROCm installation documents no
# ulp bound for the device's log10f, so E = 4 x 1.8: a float32 numpy restatement of the formula (vqt_ops_oracle.logmag_f32 -- an emulation, not the
# code under test) is 1.8 units from float64 on inputs of this kind.  (2 * 7.2 + 3) units = 17.4 units = 1.66e-6.  Measured on the MI355X: at most
# 2.74 units (2.6e-7), both entry points, all cases below.
LOGMAG_UNIT = 2.0 ** -17 / 80.0
LOG10F_UNITS = 4 * 1.8
LOGMAG_TOL = (2 * LOG10F_UNITS + 3) * LOGMAG_UNIT
# 3. the project's own bound for its GEMMs against sum |a||b| (tests/test_gpu_ops.py::test_gemm_split_operand_path).  Measured on the MI355X: at most
# 4.2e-7 (128 x 128 fp32-input tile, hop 20, K = 128); the three-term bf16 path 2.4e-7 / 2.8e-7 beside the fp32-input tile's 3.1e-7 at K = 512 / 256.
GEMM_TOL = 2e-6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def front(dev):
    from piano_a2s_amd.vqt import VQT
    return VQT(dev)


def _guarded(n, dev):
    """n floats of NaN between two guards of NaN -> (the flat buffer, the address of the n floats)."""
    buf = torch.full((GUARD + n + GUARD,), float("nan"), device=dev)
    return buf, buf.data_ptr() + 4 * GUARD


def _payload(buf, n):
    """-> the n floats as float32 numpy, after checking that the guards still hold the NaN they were filled with."""
    bits = buf.view(torch.int32).cpu().numpy()
    assert np.all(bits[:GUARD] == NAN_BITS) and np.all(bits[GUARD + n:] == NAN_BITS), "written outside the output"
    return bits[GUARD:GUARD + n].view(np.float32)


# ------------------------------------------------------------------------------------------- 1. the decimator
def _decimate(dev, ypad, taps, n_out):
    """a2s_vqt_decimate on numpy operands (ypad (B, padded_len) float32 with any padded_len) -> (B, n_out) float32."""
    from piano_a2s_amd import hip
    B, plen = ypad.shape
    yd, td = torch.from_numpy(np.ascontiguousarray(ypad)).to(dev), torch.from_numpy(np.ascontiguousarray(taps)).to(dev)
    buf, out = _guarded(B * n_out, dev)
    hip.check(hip.lib().a2s_vqt_decimate(hip.stream(), hip._p(yd), plen, hip._p(td), len(taps), hip._p(out), n_out, B), "a2s_vqt_decimate")
    torch.cuda.synchronize()
    return _payload(buf, B * n_out).reshape(B, n_out).copy()


DEC_N_OUT = [1, 2, 255, 1023, 1024, 1025, 2049 + 3]              # around DEC_OUT_PER_WG = 1024 and the 256-thread stride of a thread's 4 outputs


@pytest.mark.parametrize("ntaps", [2, 4, 62, 364])
@pytest.mark.parametrize("n_out", DEC_N_OUT)
def test_decimate_against_float64(dev, n_out, ntaps):
    for B in (1, 3):
        g = np.random.default_rng(1000 * n_out + 10 * ntaps + B)
        taps = g.standard_normal(ntaps).astype(np.float32)                              # O(1): every tap matters
        ypad = g.standard_normal((B, 2 * n_out + ntaps)).astype(np.float32)
        ref, mag = O.decimate_ref(ypad, taps, n_out)
        out = _decimate(dev, ypad, taps, n_out)
        assert np.all(np.isfinite(out))
        err, bound = float((np.abs(out - ref) / mag).max()), ntaps * 2.0 ** -24
        _log(f"decimate n_out {n_out} ntaps {ntaps} B {B}: |out - ref| / sum|y||h| {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (err, bound)


def test_decimate_with_the_product_filter(dev):
    from piano_a2s_amd.vqt import decimation_filter, decimator_taps
    h, half = decimation_filter()
    taps = decimator_taps(h).astype(np.float32)
    assert len(taps) == 364
    n_out, B = 1025, 3
    g = np.random.default_rng(361)
    ypad = np.zeros((B, 2 * n_out + 364), dtype=np.float32)
    ypad[:, half:half + 2 * n_out - 1] = g.standard_normal((B, 2 * n_out - 1))
    ref, mag = O.decimate_ref(ypad, taps, n_out)
    out = _decimate(dev, ypad, taps, n_out)
    err, bound = float((np.abs(out - ref) / mag).max()), 364 * 2.0 ** -24
    _log(f"decimate product filter n_out {n_out} B {B}: |out - ref| / sum|y||h| {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("n_out,ntaps", [(1, 2), (2, 4), (255, 62), (1024, 364), (1025, 364), (2049 + 3, 62)])
def test_decimate_reads_nothing_beyond_a_clips_row(dev, n_out, ntaps):
    """Rows shorter than the last output's window (include/a2s.h: any padded_len >= 1, what lies at or beyond it is zero): with every other clip's
    row full of NaN, a read past the end of clip b's row -- into clip b + 1's -- shows in clip b's output."""
    B = 3
    g = np.random.default_rng(7 * n_out + ntaps)
    taps = g.standard_normal(ntaps).astype(np.float32)
    S = 2 * n_out + ntaps // 2 - 1                                                         # the signal: the last outputs' windows reach beyond it
    full = 2 * n_out + ntaps
    full += (-full) % 4
    sig = g.standard_normal(S).astype(np.float32)
    for short in (S + (-S) % 4, S):                                                        # the smallest multiple of 4 that holds it; and no multiple of anything
        for b in range(B):
            rows = np.full((B, short), np.nan, dtype=np.float32)
            rows[b] = 0.0
            rows[b, :S] = sig
            ref, mag = O.decimate_ref(rows[b:b + 1], taps, n_out)                          # zero-extended
            out = _decimate(dev, rows, taps, n_out)
            assert np.all(np.isfinite(out[b])), "clip %d read a neighbour's row" % b
            err = float((np.abs(out[b] - ref[0]) / np.maximum(mag[0], 1e-30)).max())
            assert err <= ntaps * 2.0 ** -24, err
            long_rows = np.full((B, full + 4), np.nan, dtype=np.float32)                   # the same clip in a row that holds every window, zero-filled
            long_rows[b] = 0.0
            long_rows[b, :S] = sig
            again = _decimate(dev, long_rows, taps, n_out)
            assert np.array_equal(again[b].view(np.int32), out[b].view(np.int32)), "zero-extension is bit for bit the zero-filled row"
    _log(f"decimate short rows n_out {n_out} ntaps {ntaps}: finite, within {ntaps} * 2^-24, bit-identical to the zero-filled row")


def test_decimate_refusals_launch_nothing(dev):
    from piano_a2s_amd import hip
    L = hip.lib()
    y, taps, out = torch.zeros(2, 64, device=dev), torch.ones(4100, device=dev), torch.full((2, 8), float("nan"), device=dev)
    st = hip.stream()
    # a2s_vqt_decimate(stream, ypad, padded_len, taps, ntaps, out, n_out, B)
    ok = (hip._p(y), 64, hip._p(taps), 4, hip._p(out), 8, 2)
    k0 = L.a2s_launch_count()
    for i, bad in ((0, None), (2, None), (4, None), (3, 3), (3, 363), (3, 4098), (3, 0), (3, -2), (6, 0), (6, -1), (5, 0), (5, -1), (1, 0)):
        args = list(ok)
        args[i] = bad
        assert L.a2s_vqt_decimate(st, *args) == -1, (i, bad)
        assert b"vqt_decimate" in L.a2s_last_error()
    assert L.a2s_launch_count() == k0, "nothing was launched"
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    args = list(ok)
    args[3] = 4096                                                                         # the largest tap count is taken
    assert L.a2s_vqt_decimate(st, *args) == 0 and L.a2s_vqt_decimate(st, *ok) == 0
    torch.cuda.synchronize()
    assert L.a2s_launch_count() == k0 + 2, "one launch per call"
    assert bool((out == torch.tensor(0.0, device=dev)).all())


# ------------------------------------------------------------------------------------------- 2. the epilogues
def _logmag(dev, re, im, bpo, top_db):
    """Both entry points on the same planes, each in its own layout -> (plain, octaves), (B, rows, bins) float32 each."""
    from piano_a2s_amd import hip
    B, rows, bins = re.shape
    L, outs = hip.lib(), []
    for octaves in (False, True):
        Cd = torch.from_numpy(np.ascontiguousarray(O.pack_octaves(re, im, bpo) if octaves else O.pack_plain(re, im))).to(dev)
        partial = torch.full((B * 64 + GUARD,), float("inf"), device=dev)                  # (an entry left unwritten would become the clip maximum)
        buf, out = _guarded(B * rows * bins, dev)
        if octaves:
            hip.check(L.a2s_vqt_logmag_octaves(hip.stream(), hip._p(Cd), hip._p(out), hip._p(partial), B, rows, bins, bpo, top_db), "a2s_vqt_logmag_octaves")
        else:
            hip.check(L.a2s_vqt_logmag(hip.stream(), hip._p(Cd), hip._p(out), hip._p(partial), B, rows, bins, top_db), "a2s_vqt_logmag")
        torch.cuda.synchronize()
        assert bool(torch.isinf(partial[B * 64:]).all()), "the scratch is B * 64 floats"
        outs.append(_payload(buf, B * rows * bins).reshape(B, rows, bins).copy())
    return outs


@pytest.mark.parametrize("place", O.PEAK_PLACES)
@pytest.mark.parametrize("shape", O.LOGMAG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_logmag_against_float64(dev, shape, place):
    """Per-clip maxima four decades apart, an ulp apart, a silent clip and one below the floor; the cell that holds the maximum in the first row,
    in the last row's last bin, or owned by a high-numbered partial-maximum block; top_db 80 and 60.  Measured on the MI355X: the largest error of a
    case is logged in units of LOGMAG_UNIT beside the bound of 17.4."""
    B, rows, bins, bpo = shape
    r, k = O.peak_cell(place, rows, bins)
    worst = 0.0
    for name, peaks in O.PEAK_SETS.items():
        if name == "floor" and B > 1:
            continue                                                                        # (the special set has that clip already)
        re, im = O.logmag_case(shape, peaks, place, O.LOGMAG_SHAPES.index(shape) * 10 + O.PEAK_PLACES.index(place))
        for top_db in (80.0, 60.0):
            ref, db = O.logmag_ref(re, im, top_db)
            plain, octs = _logmag(dev, re, im, bpo, top_db)
            low = (80.0 - top_db) / 80.0
            for what, out in (("logmag", plain), ("logmag_octaves", octs)):
                assert np.all(np.isfinite(out)), (what, name)
                for b in range(B):
                    if np.float32(peaks[b]) < 1e-5:
                        assert np.all(out[b] == 1.0), (what, name, b, "silence, or a clip below the floor")
                    else:
                        assert out[b, r, k] == 1.0, (what, name, b, float(out[b, r, k]))
                clamped = db < -top_db - 0.01
                assert np.all(out[clamped] == np.float32(low)), (what, name, top_db)
                assert out.min() >= np.float32(low) and out.max() <= 1.0
                err = float(np.abs(out - ref).max())
                worst = max(worst, err)
                assert err <= LOGMAG_TOL, (what, name, top_db, err / LOGMAG_UNIT)
            both = float(np.abs(plain.astype(np.float64) - octs).max())
            assert both <= LOGMAG_TOL, (name, top_db, both / LOGMAG_UNIT)
    _log(f"logmag {shape} peak at {place} ({r}, {k}): max |out - ref| {worst / LOGMAG_UNIT:.2f} units of 2^-17 / 80 (bound {LOGMAG_TOL / LOGMAG_UNIT:.1f} units = "
         f"{LOGMAG_TOL:.3e}; log10f taken as {LOG10F_UNITS} units = 4 x the float32 emulation's 1.8)")


@pytest.mark.parametrize("B,rows,bins,bpo,db_per_octave", [(2, 5, 480, 60, 10.0), (3, 7, 24, 4, 20.0)])
def test_logmag_layouts_cell_by_cell(dev, B, rows, bins, bpo, db_per_octave):
    """Every (octave, bin) cell a magnitude of its own, 10 dB (8 octaves: all inside the 80 dB above the clamp) or 20 dB (6 octaves: the lowest two
    at the clamp) from octave to octave and monotone inside: neighbouring cells are 1.8e-3 or more apart, a thousand times the tolerance, so any
    permutation of bins, octaves or parts shows."""
    re, im = O.layout_case(B, rows, bins, bpo, db_per_octave)
    ref, db = O.logmag_ref(re, im, 80.0)
    plain, octs = _logmag(dev, re, im, bpo, 80.0)
    for what, out in (("logmag", plain), ("logmag_octaves", octs)):
        err = float(np.abs(out - ref).max())
        _log(f"{what} layout {(B, rows, bins, bpo)} {db_per_octave} dB per octave: max |out - ref| {err / LOGMAG_UNIT:.2f} units (bound {LOGMAG_TOL / LOGMAG_UNIT:.1f})")
        assert err <= LOGMAG_TOL, (what, err / LOGMAG_UNIT)
        assert np.all(out[db < -80.01] == 0.0)
        free = db[0, 0] > -79.9
        assert np.all(np.diff(out[0, 0][free]) > 1e-3), "rising with the bin, as the input does"


def test_logmag_refusals_launch_nothing(dev):
    from piano_a2s_amd import hip
    L = hip.lib()
    Cd, out, partial = torch.ones(2, 3, 48, device=dev), torch.full((2, 3, 24), float("nan"), device=dev), torch.zeros(128, device=dev)
    st = hip.stream()
    # a2s_vqt_logmag(stream, C, out, partial, B, rows, bins, top_db);  a2s_vqt_logmag_octaves(stream, C, out, partial, B, rows, bins, bins_per_octave, top_db)
    ok = (hip._p(Cd), hip._p(out), hip._p(partial), 2, 3, 24, 80.0)
    ok_oct = ok[:6] + (4, 80.0)
    k0 = L.a2s_launch_count()
    bad_common = ((0, None), (1, None), (2, None), (3, 0), (3, -1), (4, 0), (4, -1), (5, 0), (5, -4))
    for fn, good, bads, tag in ((L.a2s_vqt_logmag, ok, bad_common, b"vqt_logmag"),
                                (L.a2s_vqt_logmag_octaves, ok_oct, bad_common + ((6, 0), (6, -4), (6, 5), (6, 48)), b"vqt_logmag_octaves")):
        for i, bad in bads:
            args = list(good)
            args[i] = bad
            assert fn(st, *args) == -1, (tag, i, bad)
            assert tag in L.a2s_last_error()
    assert L.a2s_launch_count() == k0, "nothing was launched"
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert L.a2s_vqt_logmag(st, *ok) == 0 and L.a2s_vqt_logmag_octaves(st, *ok_oct) == 0
    torch.cuda.synchronize()
    assert L.a2s_launch_count() == k0 + 4, "two launches per call: the partial maxima and the epilogue"
    assert bool((out == torch.tensor(1.0, device=dev)).all())


# ------------------------------------------------------------------------------------------- 3. the framed GEMM
FORMS = [(160, 512), (80, 256), (20, 128), (10, 64), (5, 32)]           # (hop, n_fft) of octaves 0, 1, 3, 4 and 5-7: 16-byte loads of A possible above hop 10
# (frames, clips) -> the tile a2s_gemm_f32 picks for M = frames, N = 120: 2 x 1 x 96 = 192 tiles of 128 x 128 (the three-term bf16 path at K >= 256),
# 64 x 64 (M > 64, few tiles), 64 x 32 (M <= 64), 32 x 64 (M <= 32), 16 x 64 (M <= 16)
TILES = [(129, 96), (70, 2), (38, 2), (20, 2), (9, 1)]
N_OCT, LDC = 120, 960


@pytest.fixture(scope="module")
def framed_cases():
    return {}


def _framed_case(cache, hop, n_fft, frames, B):
    """Operands and float64 reference of one case, computed once: random bank (O(0.05)), random signals with a per-clip gain spread."""
    key = (hop, n_fft, frames, B)
    if key not in cache:
        g = np.random.default_rng(hop * 1000 + frames)
        plen = (frames - 1) * hop + n_fft
        plen += (-plen) % 4
        padded = (g.standard_normal((B, plen)) * np.exp(g.standard_normal((B, 1)))).astype(np.float32)
        bank = (0.05 * g.standard_normal((n_fft, N_OCT))).astype(np.float32)
        ref, mag = O.framed_gemm_ref(padded, hop, bank, frames)
        cache[key] = padded, bank, ref, mag + 1e-30
    return cache[key]


@pytest.mark.parametrize("frames,B", TILES)
@pytest.mark.parametrize("hop,n_fft", FORMS)
def test_framed_gemm_as_the_front_end_calls_it(dev, framed_cases, hop, n_fft, frames, B):
    """hip.gemm with the arguments of VQT.__call__: A(n, m) = padded[n * hop + m] (row stride hop < K: rows overlap), B row-contiguous and shared by
    the batch (bsB = 0), C at a column offset into rows of 960.  Everything but the octave's 120 columns stays the NaN it was filled with."""
    from piano_a2s_amd import hip
    L = hip.lib()
    padded, bank, ref, mag = _framed_case(framed_cases, hop, n_fft, frames, B)
    plen = padded.shape[1]
    pd, bd = torch.from_numpy(padded).to(dev), torch.from_numpy(bank).to(dev)
    refd, magd = torch.from_numpy(ref).to(dev), torch.from_numpy(mag).to(dev)
    split = frames == 129 and n_fft >= 256                                                # the 128 x 128 tile takes the three-term bf16 path there
    previous = L.a2s_debug_get(b"gemm_bf16x3")
    errs = {}
    try:
        for mode in ((0, 1) if split else (previous,)):
            hip.check(L.a2s_debug_set(b"gemm_bf16x3", mode), "debug_set")
            for c_off in (0, 240, 840):
                buf = torch.full((LDC + B * frames * LDC + LDC,), float("nan"), device=dev)
                hip.gemm(pd, hop, 1, bd, N_OCT, 1, buf, LDC, frames, N_OCT, n_fft, batch=B, bsA=plen, bsB=0, bsC=frames * LDC, c_off=LDC + c_off)
                torch.cuda.synchronize()
                Cc = buf[LDC:LDC + B * frames * LDC].view(B, frames, LDC)
                got = Cc[:, :, c_off:c_off + N_OCT]
                assert bool(torch.isfinite(got).all())
                errs[mode] = max(errs.get(mode, 0.0), float(((got.double() - refd).abs() / magd).max()))
                bits = buf.view(torch.int32)
                outside = torch.ones(LDC, dtype=torch.bool, device=dev)
                outside[c_off:c_off + N_OCT] = False
                assert bool((bits[:LDC] == NAN_BITS).all()) and bool((bits[LDC + B * frames * LDC:] == NAN_BITS).all()), "written outside C"
                assert bool((Cc.view(torch.int32)[:, :, outside] == NAN_BITS).all()), "written outside the octave's columns"
    finally:
        hip.check(L.a2s_debug_set(b"gemm_bf16x3", previous), "debug_set")
    for mode, err in errs.items():
        _log(f"framed gemm hop {hop} n_fft {n_fft} frames {frames} clips {B} gemm_bf16x3 {mode}: |C - ref| / sum|a||b| {err:.3e} (bound {GEMM_TOL:.0e})")
        assert err < GEMM_TOL, errs
    if split:
        assert errs[1] < 3 * errs[0] + 1e-7, errs                                          # at the fp32-input kernel's level


# ------------------------------------------------------------------------------------------- 4. the host glue
@pytest.mark.parametrize("N", [1, 2, 161, 5121])
def test_host_decimation_is_the_oracles(dev, front, N):
    """VQT._decimate (the tap reversal, the offset `half`, n_out = (N + 1) // 2) against oracle.vqt_ref._decimate2 on the same float32 samples, at the
    decimator's bound: 361 FMAs and the rounding of the taps to float32 stay below 364 * 2^-24 sum |y||h|."""
    from oracle import vqt_ref as V
    from piano_a2s_amd.vqt import decimation_filter
    y = np.random.default_rng(N).standard_normal((2, N)).astype(np.float32)
    out = front._decimate(torch.from_numpy(y).to(dev))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert out.shape == (2, (N + 1) // 2)
    h, half = decimation_filter()
    for b in range(2):
        ref = V._decimate2(y[b].astype(np.float64))
        mag = np.convolve(np.abs(y[b].astype(np.float64)), np.abs(h))[half:half + 2 * len(ref):2]
        err, bound = float((np.abs(out[b] - ref) / mag).max()), 364 * 2.0 ** -24
        _log(f"VQT._decimate N {N} clip {b}: |out - ref| / sum|y||h| {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (err, bound)


@pytest.mark.parametrize("N,frames", [(1, 1), (159, 1), (160, 2), (161, 2), (321, 3), (5121, 33)])
def test_front_end_at_the_shortest_inputs(dev, front, N, frames):
    """The whole front end against the multirate oracle where the frame count and the decimation chain are at their edges; the asserts of
    tests/test_gpu_vqt.py::test_matches_the_multirate_oracle."""
    from oracle import vqt_ref as V
    y = np.random.default_rng(N).standard_normal(N).astype(np.float32)
    ref = V.vqt_features_librosa(y.astype(np.float64))
    out = front(torch.from_numpy(y).to(dev).unsqueeze(0))
    torch.cuda.synchronize()
    assert out.shape == (1, 1, frames, 480) == (1, 1) + ref.shape
    d = np.abs(out[0, 0].cpu().numpy() - ref)
    audible = ref > 0.05
    worst = d[audible].max() if audible.any() else float("nan")
    _log(f"front end N {N}: max {d.max() * 80:.4f} dB, audible max {worst * 80:.4f} dB, mean {d.mean() * 80:.5f} dB")
    if audible.any():
        assert d[audible].max() < 2.5e-3, d[audible].max()
    assert d.mean() < 2e-4, d.mean()
