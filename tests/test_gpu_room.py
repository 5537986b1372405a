"""The room acoustics of the rendered corpus on the MI355X (csrc/a2s_room.hip, piano_a2s_amd/room.py):

1. fir_rows, exact: small integers, every sum below 2^24, equal to np.convolve; NaN behind every clip's taps, guards around x and y; aligned and unaligned rows;
2. the identity room;
3. fir_rows against the float64 oracle on an oracle-rendered generator clip;
4. room_ir against the oracle;
5. determinism and independence of the other clips and of the grid;
6. refusals and the launch counter;
7. Room.apply against the oracle chain, and the recipe with and without --synthetic_room."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from piano_a2s_amd import scoregen, spec
from tests import render_oracle, room_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 123.0
NAN_BITS = np.array([0x7FC00000], dtype=np.uint32).view(np.int32)[0]
ORACLE_SEEDS = (0x0BADCAFE ^ 0x524F4F4D, 0x12345678 ^ 0x524F4F4D)
# 3. max |device - oracle| over the two clips of `_oracle_case`, measured on the MI355X: 2.032e-7 in clip 0 (1.6e-6 of its peak 0.128), 2.440e-7 in clip 1 (2.5e-6
# of its peak 0.096); through Room.apply (the device's own impulse responses) 2.107e-7 and 2.440e-7
MEASURED_MAX_ERR = 2.440e-7
# ... and what is asserted: four times that (other inputs of the same length); it has to stay below 1e-4 of the clip's peak (-80 dB, the VQT's own floor)
TOL = 4 * MEASURED_MAX_ERR
# 4. max over the clips of `test_room_ir_against_the_oracle` of |device - oracle| / wet in the tail, measured on the MI355X: 1.113e-7 (clip 2; the
# others 7.0e-8 .. 9.6e-8)
MEASURED_IR_ERR_OF_WET = 1.113e-7
# ... asserted: four times that, which has to stay below 1e-6 (of wet)
IR_TOL_OF_WET = 4 * MEASURED_IR_ERR_OF_WET


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dims():
    from piano_a2s_amd import hip
    T, Cc = hip.fir_tile_samples(), hip.fir_tap_chunk()
    assert T >= 64 and Cc >= 8
    return T, Cc, 2 * T + 37


def _table(rows):
    """(B, 4) int32 from rows of (pre, L, wet, decay)."""
    t = np.zeros((len(rows), 4), dtype=np.int32)
    for b, (pre, L, wet, decay) in enumerate(rows):
        t[b, :2] = pre, L
        t[b, 2:] = np.array([wet, decay], dtype=np.float32).view(np.int32)
    return t


def _fir_guarded(x, ir, table, L_max, dev, lead, pad, n_samples=None):
    """fir_rows with x, y in flat buffers of guard values: `lead` floats in front, row stride N + pad, a row of guards behind.  -> (B, n) float32."""
    from piano_a2s_amd import hip
    B, N = x.shape
    n = N if n_samples is None else n_samples
    stride = N + pad
    xf = torch.full((lead + (B + 1) * stride,), GUARD, device=dev)
    xv = xf[lead:lead + B * stride].view(B, stride)
    xv[:, :N] = torch.tensor(x).to(dev)
    yf = torch.full((lead + (B + 1) * stride,), GUARD, device=dev)
    yv = yf[lead:lead + B * stride].view(B, stride)
    hip.fir_rows(xv, torch.tensor(ir).to(dev), torch.tensor(table).to(dev), L_max, y=yv, n_samples=n)
    torch.cuda.synchronize()
    out = yf.cpu().numpy()
    rows = out[lead:lead + B * stride].reshape(B, stride)
    assert (out[:lead] == GUARD).all() and (out[lead + B * stride:] == GUARD).all(), "the guards before and after the output"
    assert (rows[:, n:] == GUARD).all(), "the padding of the row stride"
    assert (xf.cpu().numpy()[:lead] == GUARD).all(), "x is not written"
    return rows[:, :n].copy()


# ------------------------------------------------------------------------------------------- 1. exact
_EXACT = {}


def _exact_case(dims):
    """x in -3 .. 3, h in -2 .. 2, per-clip L in {1, C + 1, 3 C + 5, N + 9}: |sum| <= 6 (N + 9) < 2^24, exact in fp32 in any order.  Computed once."""
    if not _EXACT:
        T, Cc, N = dims
        rng = np.random.default_rng(20)
        Ls = (1, Cc + 1, 3 * Cc + 5, N + 9)
        L_max = N + 9
        assert 6 * L_max < 2 ** 24
        x = rng.integers(-3, 4, (4, N)).astype(np.float32)
        h = rng.integers(-2, 3, (4, L_max)).astype(np.float32)
        h[:, 0] = (1, 2, -1, 2)                                            # (a first tap that is not 0, so that L = 1 is not silence)
        want = np.stack([np.convolve(x[b].astype(np.float64), h[b, :L].astype(np.float64))[:N] for b, L in enumerate(Ls)]).astype(np.float32)
        ir = np.full((4, L_max + 3), np.float32(0)).view(np.int32)
        ir[:] = NAN_BITS                                                   # NaN behind every clip's own L, and in the padding of the stride
        ir = ir.view(np.float32)
        for b, L in enumerate(Ls):
            ir[b, :L] = h[b, :L]
        assert np.isnan(ir[0, 1:]).all() and np.isnan(ir[3, L_max:]).all() and np.abs(want).max() > 50
        _EXACT.update(x=x, ir=ir, table=_table([(1, L, 0.0, 0.0) for L in Ls]), L_max=L_max, want=want)
        for v in _EXACT.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _EXACT


def test_fir_is_exact_on_small_integers(dev, dims):
    from piano_a2s_amd import hip
    c = _exact_case(dims)
    n0 = hip.room_launches()
    got = _fir_guarded(c["x"], c["ir"], c["table"], c["L_max"], dev, lead=64, pad=11)          # 16-byte aligned rows: the vector loads and stores
    assert hip.room_launches() == n0 + 1
    got_u = _fir_guarded(c["x"], c["ir"], c["table"], c["L_max"], dev, lead=3, pad=6)          # unaligned rows: the 4-byte ones
    assert np.isfinite(got).all(), "nothing behind a clip's L reached the result"
    wrong = np.argwhere(got != c["want"])
    assert wrong.size == 0, f"{len(wrong)} samples differ from np.convolve, the first at (clip, sample) {wrong[0]}: {got[tuple(wrong[0])]} != {c['want'][tuple(wrong[0])]}"
    assert np.array_equal(got.view(np.uint32), got_u.view(np.uint32)), "aligned and unaligned rows give the same bits"


# ------------------------------------------------------------------------------------------- 2. identity
def test_identity_room_returns_x(dev, dims):
    _, _, N = dims
    rng = np.random.default_rng(21)
    x = rng.standard_normal((2, N)).astype(np.float32)
    ir = np.full((2, 8), np.nan, dtype=np.float32)
    ir[:, 0] = 1.0
    got = _fir_guarded(x, ir, _table([(1, 1, 0.0, 0.0)] * 2), 8, dev, lead=64, pad=3)
    assert np.array_equal(got, x)


# ------------------------------------------------------------------------------------------- 3. against the oracle
_ORACLE = {}


def _oracle_case(dims):
    """Two generator clips (test_gpu_render.py's kind) rendered by the float64 synthesiser oracle, each through the oracle's room of its seed, the rooms
    of Room's defaults capped to L_max = 3 C + 5.  Computed once, shared, never modified."""
    if not _ORACLE:
        T, Cc, N = dims
        L_max = 3 * Cc + 5
        frames = N // 160 + 5
        waves, rooms, irs, refs = [], [], [], []
        for clip_seed, seed in zip((4321, 137), ORACLE_SEEDS):
            prog = scoregen.pack_program(scoregen.make_clip(spec.default_cfg(), clip_seed, frames=frames), rows=300)
            assert prog[0, 1] >= 20 and prog[0, 0] >= N
            prog[0, 0] = N
            x = render_oracle.render(prog).astype(np.float32)             # the device's input: the oracle's waveform as float32
            p = room_oracle.params(seed, L_max=L_max)
            h = room_oracle.impulse_response(seed, p["pre"], p["L"], p["wet"], p["decay"], L_max=L_max)
            assert p["L"] == L_max and 80 <= p["pre"] <= 400
            waves.append(x), rooms.append(p), irs.append(h), refs.append(room_oracle.fir(x, h, L=p["L"]))
        _ORACLE.update(x=np.stack(waves), rooms=rooms, ir=np.stack(irs), ref=np.stack(refs), L_max=L_max,
                       table=np.stack([room_oracle.table_row(p) for p in rooms]))
        for v in _ORACLE.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _ORACLE


def _report_against_oracle(what, got, c):
    peaks = np.abs(c["ref"]).max(axis=1)
    errs = np.abs(got.astype(np.float64) - c["ref"]).max(axis=1)
    for b in range(len(peaks)):
        print(f"{what} clip {b}: peak {peaks[b]:.4f}, max |device - oracle| {errs[b]:.3e} ({errs[b] / peaks[b]:.3e} of the peak)")
    print(f"{what}: max error {errs.max():.3e}, asserted {TOL:.3e}")
    assert peaks.min() > 0.05, "the reference is not near silence"
    assert TOL <= 1e-4 * peaks.min(), "the asserted tolerance is below -80 dB of either clip's peak"
    assert errs.max() <= TOL, f"{errs.max():.3e} > {TOL:.3e}"


def test_fir_against_the_float64_oracle(dev, dims):
    """Measured on the MI355X: see MEASURED_MAX_ERR."""
    c = _oracle_case(dims)
    dry = np.abs(c["x"].astype(np.float64) - c["ref"]).max(axis=1)
    assert (dry > 100 * TOL).all(), "the room is audible: the reference is not the dry clip"
    got = _fir_guarded(c["x"], c["ir"].astype(np.float32), c["table"], c["L_max"], dev, lead=64, pad=7)
    _report_against_oracle("fir_rows", got, c)


# ------------------------------------------------------------------------------------------- 4. room_ir
def test_room_ir_against_the_oracle(dev):
    """Measured on the MI355X: see MEASURED_IR_ERR_OF_WET."""
    from piano_a2s_amd import hip
    from piano_a2s_amd.room import Room
    room = Room()
    L_max = room.L_max
    seeds = np.array([0, 1, 0xFFFFFFFF, 0xC0FFEE11, 0x524F4F4D, 77, 78], dtype=np.uint32)
    table = room.params(seeds)
    table[5] = (1, L_max + 500, *_table([(0, 0, 0.05, 1e-3)])[0, 2:])       # pre = 1 and an L behind L_max: clamped, the tail fills the row
    table[6] = (3, 0, *_table([(0, 0, 0.05, 1e-3)])[0, 2:])                 # L = 0: clamped to 1, the direct path alone
    B, stride = len(seeds), L_max + 5
    flat = torch.full((64 + (B + 1) * stride,), GUARD, device=dev)
    ir = flat[64:64 + B * stride].view(B, stride)
    n0 = hip.room_launches()
    hip.room_ir(torch.from_numpy(seeds.view(np.int32)).to(dev), torch.from_numpy(table).to(dev), L_max, ir=ir)
    torch.cuda.synchronize()
    assert hip.room_launches() == n0 + 1
    out = flat.cpu().numpy()
    assert (out[:64] == GUARD).all() and (out[64 + B * stride:] == GUARD).all(), "the guards before and after the buffer"
    got = out[64:64 + B * stride].reshape(B, stride)
    assert (got[:, L_max:] == GUARD).all(), "the padding of the row stride"
    got = got[:, :L_max]
    worst = 0.0
    for b in range(B):
        pre, L = int(table[b, 0]), min(max(int(table[b, 1]), 1), L_max)
        wet, decay = (float(v) for v in table[b, 2:].view(np.float32))
        want = room_oracle.impulse_response(int(seeds[b]), pre, L, wet, decay, L_max=L_max)
        assert got[b, 0] == 1.0, "the direct path"
        assert (got[b, 1:max(pre, 1)] == 0).all() and not np.signbit(got[b, 1:max(pre, 1)]).any(), "exact zeros in the pre-delay"
        assert (got[b, L:] == 0).all() and not np.signbit(got[b, L:]).any(), "exact zeros behind L"
        assert (want[1:pre] == 0).all() and (want[L:] == 0).all()
        err = np.abs(got[b].astype(np.float64) - want).max() / wet
        print(f"room_ir clip {b}: pre {pre}, L {L}, wet {wet:.5f}, max |device - oracle| {err * wet:.3e} = {err:.3e} of wet")
        worst = max(worst, err)
        if L > pre:
            assert np.abs(want[pre:L]).max() > 0.5 * wet and (got[b, pre:L] != 0).mean() > 0.99
    assert table[6, 1] == 0 and (got[6, 1:] == 0).all()
    print(f"room_ir: max error {worst:.3e} of wet, asserted {IR_TOL_OF_WET:.3e}")
    assert IR_TOL_OF_WET < 1e-6, "the asserted tolerance is below 1e-6 of wet"
    assert worst <= IR_TOL_OF_WET, f"{worst:.3e} > {IR_TOL_OF_WET:.3e}"


# ------------------------------------------------------------------------------------------- 5. determinism, independence
def test_launches_are_bit_equal_and_clips_and_grids_independent(dev, dims):
    from piano_a2s_amd import hip
    T, Cc, N = dims
    c = _oracle_case(dims)
    x, ir, table = (torch.tensor(a).to(dev) for a in (c["x"], c["ir"].astype(np.float32), c["table"]))
    a, b = hip.fir_rows(x, ir, table, c["L_max"]), hip.fir_rows(x, ir, table, c["L_max"])
    assert a.shape == (2, N) and a.dtype == torch.float32 and a.data_ptr() != b.data_ptr()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    alone = hip.fir_rows(x[1:2].clone(), ir[1:2].clone(), table[1:2].clone(), c["L_max"])
    assert torch.equal(alone[0].view(torch.int32), a[1].view(torch.int32)), "clip 1 processed alone"
    shorter = hip.fir_rows(x, ir, table, c["L_max"], n_samples=T + 5)          # another grid: the samples it shares are the same bits
    assert shorter.shape == (2, T + 5)
    assert torch.equal(shorter.view(torch.int32), a[:, :T + 5].contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------- 6. refusals, launch counter
def test_refusals_launch_nothing(dev, dims):
    from piano_a2s_amd import hip
    from piano_a2s_amd.room import Room
    L = hip.lib()
    _, _, N = dims
    c = _oracle_case(dims)
    L_max = c["L_max"]
    x, ir, table = (torch.tensor(a).to(dev) for a in (c["x"], c["ir"].astype(np.float32), c["table"]))
    seeds = torch.from_numpy(np.array(ORACLE_SEEDS, dtype=np.uint32).view(np.int32)).to(dev)
    y = torch.zeros(2, N, device=dev)
    st = hip.stream()
    n0, k0 = hip.room_launches(), L.a2s_launch_count()
    lN, lL = C.c_long(N), C.c_long(L_max)
    # a2s_fir_rows(stream, x, x_bstride, ir, ir_bstride, params, y, y_bstride, B, n_samples, L_max)
    ok = (hip._p(x), lN, hip._p(ir), lL, hip._p(table), hip._p(y), lN, 2, N, L_max)
    for i, bad in ((0, None), (2, None), (4, None), (5, None), (7, -1), (7, 65536), (8, 0), (9, 0), (1, C.c_long(N - 1)), (6, C.c_long(N - 1)),
                   (3, C.c_long(L_max - 1)), (5, hip._p(x))):
        args = list(ok)
        args[i] = bad
        assert L.a2s_fir_rows(st, *args) == -1, i
        assert b"fir_rows" in L.a2s_last_error()
    # a2s_room_ir(stream, room_seed, params, B, ir, ir_bstride, L_max)
    ok_ir = (hip._p(seeds), hip._p(table), 2, hip._p(ir), lL, L_max)
    for i, bad in ((0, None), (1, None), (3, None), (2, -1), (2, 65536), (5, 0), (4, C.c_long(L_max - 1))):
        args = list(ok_ir)
        args[i] = bad
        assert L.a2s_room_ir(st, *args) == -1, i
        assert b"room_ir" in L.a2s_last_error()
    for fn, good, at in ((L.a2s_fir_rows, ok, 7), (L.a2s_room_ir, ok_ir, 2)):
        args = list(good)
        args[at] = 0                                                        # no clips: fine, and nothing to launch
        assert fn(st, *args) == 0
    assert hip.room_launches() == n0 and L.a2s_launch_count() == k0, "nothing was launched"
    assert L.a2s_room_ir(st, *ok_ir) == 0 and L.a2s_fir_rows(st, *ok) == 0
    torch.cuda.synchronize()
    assert hip.room_launches() == n0 + 2 and L.a2s_launch_count() == k0 + 2, "one launch per call"
    with pytest.raises(hip.A2SError):
        Room().apply(torch.from_numpy(c["x"].copy()), ORACLE_SEEDS)         # a CPU waveform
    with pytest.raises(hip.A2SError):
        hip.fir_rows(x, ir, table, L_max, y=x)
    with pytest.raises(hip.A2SError):
        hip.fir_rows(x.double(), ir, table, L_max)
    with pytest.raises(hip.A2SError):
        hip.fir_rows(x, ir, table.float(), L_max)
    with pytest.raises(hip.A2SError):
        hip.room_ir(seeds[:1], table, L_max)
    assert hip.room_launches() == n0 + 2


# ------------------------------------------------------------------------------------------- 7. Python and the recipe
def test_room_apply_is_the_oracle_chain_and_reuses_its_buffers(dev, dims):
    from piano_a2s_amd import hip
    from piano_a2s_amd.room import Room
    c = _oracle_case(dims)
    room = Room(L_max=c["L_max"])
    assert np.array_equal(room.params(ORACLE_SEEDS), c["table"]), "the product's table is the oracle's"
    wave = torch.from_numpy(c["x"].copy()).to(dev)
    n0 = hip.room_launches()
    y = room.apply(wave, ORACLE_SEEDS)
    assert hip.room_launches() == n0 + 2 and room.clips == 2 and tuple(y.shape) == tuple(wave.shape)
    _report_against_oracle("Room.apply", y.cpu().numpy(), c)
    ir, params = room.impulse_responses(ORACLE_SEEDS, dev)
    assert tuple(ir.shape) == (2, c["L_max"]) and np.array_equal(params.cpu().numpy(), c["table"])
    first, ptr = y.clone(), y.data_ptr()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(dev)
    again = room.apply(wave, ORACLE_SEEDS)
    torch.cuda.synchronize()
    assert again.data_ptr() == ptr and torch.cuda.memory_allocated(dev) == before, "the second call of a shape allocates nothing on the device"
    assert torch.equal(again.view(torch.int32), first.view(torch.int32)) and room.clips == 4


def _pretrain(tmp_path, name, extra):
    import pretrain
    ws = os.path.join(str(tmp_path), name)
    os.makedirs(ws)
    args = [os.path.join(ROOT, "hparams", "pretrain.yaml"), "--device=cuda:0", f"--workspace={ws}", "--soundfont_folder=/none", "--synthetic_clips=8",
            "--synthetic_frames=201", "--batch_size=2", "--number_of_epochs=1", "--hidden_size=32", "--conv_feature_size=32", "--max_length=(48, 32)",
            "--seed=1234"] + extra
    brain = pretrain.main(args)
    with open(os.path.join(ws, "1234", "pretrain.epr", "run_summary.json")) as f:
        return brain, json.load(f)


def _finite(brain):
    stats = brain.last_stats
    assert all(np.isfinite(stats[k]) for k in ("loss", "time_loss", "key_loss", "upper_loss", "lower_loss", "WER")), stats
    assert all(np.isfinite(v) for v in brain.train_stats.values()), brain.train_stats


def test_recipe_with_rooms_in_every_stage(tmp_path, dev):
    from piano_a2s_amd import hip
    n0 = hip.room_launches()
    brain, summary = _pretrain(tmp_path, "all", ["--synthetic_scores=rendered", "--synthetic_room=all", "--room_rt60=(0.2, 0.3)"])
    assert hip.room_launches() == n0 + 2 * (4 + 1 + 1), "4 training batches, validation and test: room_ir and fir_rows each"
    _finite(brain)
    assert summary["room"] == dict(stages="all", clips=8 + 1 + 1, rt60=[0.2, 0.3], drr_db=[0.0, 12.0], predelay_ms=[5.0, 25.0], sample_rate=16000, L_max=5200)
    assert summary["fused_hip_step"] and summary["optimizer_steps"] == 4 and summary["nonfinite_steps"] == 0


def test_recipe_with_rooms_in_training_only_and_without(tmp_path, dev):
    from piano_a2s_amd import hip
    n0 = hip.room_launches()
    brain, summary = _pretrain(tmp_path, "train", ["--synthetic_scores=rendered", "--synthetic_room=train"])
    assert hip.room_launches() == n0 + 2 * 4, "the 4 training batches alone"
    _finite(brain)
    assert summary["room"]["stages"] == "train" and summary["room"]["clips"] == 8 and summary["room"]["L_max"] == 10_000
    n1, r1 = hip.room_launches(), hip.render_launches()
    brain, summary = _pretrain(tmp_path, "dry", ["--synthetic_scores=rendered"])
    assert hip.room_launches() == n1 and hip.render_launches() >= r1 + 6, "without the override nothing of the room runs"
    assert "room" not in summary
    _finite(brain)
    with pytest.raises(ValueError, match="synthetic_scores=rendered"):
        _pretrain(tmp_path, "refused", ["--synthetic_room=all"])
    assert hip.room_launches() == n1


def test_features_of_a_batch_with_and_without_the_room(dev):
    from piano_a2s_amd import hip, recipe
    from piano_a2s_amd.render import render
    from piano_a2s_amd.room import Room, room_seeds
    from piano_a2s_amd.vqt import VQT
    cfg = spec.default_cfg(max_bars=2)
    progs = torch.from_numpy(np.stack([scoregen.pack_program(scoregen.make_clip(cfg, s, frames=201)) for s in (137, 197)]))
    want = VQT(dev)(render(progs.to(dev)))
    n0 = hip.room_launches()
    dry = recipe._features([progs, "rest"], dev)
    assert hip.room_launches() == n0 and dry[1] == "rest"
    assert torch.equal(dry[0].view(torch.int32), want.view(torch.int32)), "without a room: VQT(render(programs)), bit for bit"
    room = Room()
    wet = recipe._features([progs, "rest"], dev, room=room)
    assert hip.room_launches() == n0 + 2 and room.clips == 2 and wet[0].shape == want.shape
    assert torch.isfinite(wet[0]).all() and not torch.equal(wet[0], want), "with a room the features differ"
    seeds = room_seeds(progs)
    assert seeds[0] != seeds[1] and not np.array_equal(room.params(seeds)[0], room.params(seeds)[1]), "every clip has a room of its own"
    change = (wet[0] - want).abs()
    print(f"features, dry against room: mean |change| {float(change.mean()):.4f}, largest {float(change.max()):.4f} (feature units)")
