"""The note synthesiser of the rendered synthetic corpus on the MI355X (csrc/a2s_render.hip, piano_a2s_amd/render.py):

1. the kernel against the float64 definition (tests/render_oracle.py), with guard values around the output;
2. determinism and independence of the other clips;
3. the noise against the hash formula in numpy float32;
4. refusals and the launch counter;
5. score -> audio -> features: the notes of generator clips land on their VQT bins;
6. the recipe with and without --synthetic_scores=rendered."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from piano_a2s_amd import scoregen, spec
from tests import render_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2 * 1024 + 37
ROWS = 300
GUARD = 123.0
NAN_BITS = np.array([0x7FC00000], dtype=np.uint32).view(np.int32)[0]
# max |device - oracle| over the three clips below, measured on the MI355X: 1.023e-7 in clip 0 (1.4e-7 of its peak 0.734), 1.6e-8 in clip 2 (1.8e-7 of its peak 0.092) ...
MEASURED_MAX_ERR = 1.023e-7
# ... and what is asserted: four times that (other inputs of the same polyphony); it has to stay below 1e-4 of the clip's peak (-80 dB, the VQT's own floor)
TOL = 4 * MEASURED_MAX_ERR


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _programs():
    """Clip 0: hand-placed notes, spread over the row chunks (rows 1 .. 300: more than one scan of 256) between padding rows.  Clip 1: nothing but
    padding rows of NaN bit patterns, no noise.  Clip 2: a generator clip."""
    decay, g = 1.0 / 900, 0.7
    notes = {1: (0, 500, 60, 0.8, decay, g, 8),                       # a note at sample 0
             7: (900, 400, 64, 0.6, decay, g, 6),                     # across the tile boundary at 1024
             40: (1100, 300, 60, 0.5, decay, 0.5, 8),                 # a three-note chord on one onset ...
             41: (1100, 300, 64, 0.5, decay, 0.5, 8),
             258: (1100, 300, 67, 0.5, decay, 0.5, 8),                # ... its third note in the second chunk of rows
             100: (1500, N - 200 - 1500, 72, 0.7, decay, g, 5),       # the release (rel_len 200) ends on the last sample
             259: (1900, 1000, 55, 0.9, decay, g, 10),                # runs past the end
             260: (300, 1200, 108, 0.6, decay, g, 8),                 # MIDI 108: every partial above the first lies beyond the Nyquist frequency
             300: (1300, 600, 96, 0.4, decay, 0.8, 16)}               # MIDI 96: partials 4 .. 16 do
    p0 = np.zeros((1 + ROWS, 8), dtype=np.int32)
    p0[0] = scoregen.pack_rows(N, [], attack=40, rel_len=200, rel_rate=1.0 / 60, gain=0.35, noise_level=0.003, noise_seed=0xC0FFEE11)[0]
    p0[0, 1] = ROWS
    for row, note in notes.items():
        p0[row] = scoregen.pack_rows(N, [note])[1]
    p0[2] = NAN_BITS                                                   # padding by its onset (>= n_samples), whatever else it holds
    p0[3, :] = (10, 0, 1 << 28, NAN_BITS, NAN_BITS, NAN_BITS, 8, 0)    # padding by its length
    p0[4, :] = (10, -5, 1 << 28, NAN_BITS, NAN_BITS, NAN_BITS, 8, 0)
    p0[5, :] = (N, 50, 1 << 28, NAN_BITS, NAN_BITS, NAN_BITS, 8, 0)    # onset == n_samples
    p1 = np.full((1 + ROWS, 8), NAN_BITS, dtype=np.int32)
    p1[0] = scoregen.pack_rows(N, [], noise_level=0.0)[0]
    p1[0, 1] = ROWS
    clip = scoregen.make_clip(spec.default_cfg(), 4321, frames=14)     # 2080 samples: every event lies inside N
    p2 = scoregen.pack_program(clip, rows=ROWS)
    assert p2[0, 1] >= 20 and p2[0, 0] == 2080
    p2[0, 0] = N
    return np.stack([p0, p1, p2])


_REF = {}


def _reference():
    """The oracle's three waveforms: computed once, shared, never modified."""
    if not _REF:
        progs = _programs()
        _REF["programs"] = progs
        _REF["wave"] = np.stack([render_oracle.render(p) for p in progs])
        _REF["wave"].setflags(write=False)
    return _REF["programs"], _REF["wave"]


def _render_guarded(progs, dev, lead, stride):
    """Render into a flat buffer of guard values: `lead` floats in front, row stride `stride` >= N, a row of guards behind."""
    from piano_a2s_amd import hip
    B = progs.shape[0]
    flat = torch.full((lead + (B + 1) * stride,), GUARD, device=dev)
    wave = flat[lead:lead + B * stride].view(B, stride)
    hip.render_notes(torch.from_numpy(progs).to(dev), N, wave=wave)
    torch.cuda.synchronize()
    out = flat.cpu().numpy()
    rows = out[lead:lead + B * stride].reshape(B, stride)
    assert (out[:lead] == GUARD).all() and (out[lead + B * stride:] == GUARD).all(), "the guards before and after the buffer"
    assert (rows[:, N:] == GUARD).all(), "the padding of the row stride"
    return rows[:, :N].copy()


# ------------------------------------------------------------------------------------------- 1. against the oracle
def test_kernel_against_the_float64_oracle(dev):
    """Measured on the MI355X: see MEASURED_MAX_ERR."""
    from piano_a2s_amd import hip
    progs, ref = _reference()
    assert len(render_oracle.live_rows(progs[0])) == 9 and render_oracle.live_rows(progs[1]) == []
    n0 = hip.render_launches()
    got = _render_guarded(progs, dev, lead=64, stride=N + 11)               # 16-byte aligned rows: the vector stores
    assert hip.render_launches() == n0 + 1
    got_u = _render_guarded(progs, dev, lead=3, stride=N + 6)               # unaligned: the scalar stores
    assert np.array_equal(got.view(np.uint32), got_u.view(np.uint32)), "the two store paths write the same bits"
    assert (got[1] == 0).all() and not np.signbit(got[1]).any(), "a clip of padding rows and no noise is exactly zero"
    assert np.isfinite(got).all()
    peaks = np.abs(ref).max(axis=1)
    errs = np.abs(got.astype(np.float64) - ref).max(axis=1)
    for b in range(3):
        print(f"render clip {b}: peak {peaks[b]:.4f}, max |device - oracle| {errs[b]:.3e} ({errs[b] / max(peaks[b], 1e-30):.3e} of the peak)")
    print(f"render: max error {errs.max():.3e}, asserted {TOL:.3e}")
    assert peaks[0] > 0.3 and peaks[2] > 0.05, "the reference is not near silence"
    assert TOL <= 1e-4 * min(peaks[0], peaks[2]), "the asserted tolerance is below -80 dB of either clip's peak"
    assert errs.max() <= TOL, f"{errs.max():.3e} > {TOL:.3e}"


# ------------------------------------------------------------------------------------------- 2. determinism, independence
def test_launches_are_bit_equal_and_clips_independent(dev):
    from piano_a2s_amd.render import render
    progs, _ = _reference()
    p = torch.from_numpy(progs).to(dev)
    a, b = render(p), render(p)
    assert a.shape == (3, N) and a.dtype == torch.float32
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    alone = render(p[2:3].clone())
    assert torch.equal(alone[0].view(torch.int32), a[2].view(torch.int32)), "clip 2 rendered alone"
    first = render(p[0:1].clone(), n_samples=N)
    assert torch.equal(first[0].view(torch.int32), a[0].view(torch.int32))
    shorter = render(p, n_samples=1024 + 5)                                  # another grid: the samples it shares are the same bits
    assert torch.equal(shorter.view(torch.int32), a[:, :1024 + 5].contiguous().view(torch.int32))


def test_clip_shorter_than_the_call_is_zero_behind_its_length(dev):
    from piano_a2s_amd.render import render
    progs, _ = _reference()
    q = progs.copy()
    q[0, 0, 0] = 1500
    out = render(torch.from_numpy(q).to(dev), n_samples=N).cpu().numpy()
    want = render_oracle.render(q[0], n_samples=N)
    assert (out[0, 1500:] == 0).all() and (want[1500:] == 0).all()
    assert np.abs(out[0] - want).max() <= TOL


# ------------------------------------------------------------------------------------------- 3. noise
def test_noise_is_the_hash_formula(dev):
    from piano_a2s_amd.render import render
    seed, level = 0x9ABCDEF1, 0.01
    p = scoregen.pack_rows(N, [], noise_level=level, noise_seed=seed, rows=4)[None]
    got = render(torch.from_numpy(p).to(dev)).cpu().numpy()[0]
    n = np.arange(N, dtype=np.uint64)
    h = render_oracle.hash32(np.uint64(seed) + n * np.uint64(0x9E3779B9))
    u = (h >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -23) - np.float32(1.0)
    want = np.float32(level) * u
    ulp = np.spacing(np.abs(want))
    assert np.abs(want).max() > 0.0099 and (np.abs(got - want) <= ulp).all()
    print(f"noise: {int((got != want).sum())} of {N} samples differ from numpy float32 (within 1 ulp)")


# ------------------------------------------------------------------------------------------- 4. refusals, launch counter
def test_refusals_launch_nothing(dev):
    from piano_a2s_amd import hip, render
    L = hip.lib()
    progs, _ = _reference()
    p = torch.from_numpy(progs).to(dev)
    w = torch.zeros(3, N, device=dev)
    st = hip.stream()
    n0, k0 = hip.render_launches(), L.a2s_launch_count()
    ok = (hip._p(p), 1 + ROWS, N, hip._p(w), C.c_long(N), 3)
    for i, bad in ((0, None), (3, None), (5, -1), (1, 0), (2, 0), (4, C.c_long(N - 1))):
        args = list(ok)
        args[i] = bad
        assert L.a2s_render_notes(st, *args) == -1, i
        assert b"render_notes" in L.a2s_last_error()
    args = list(ok)
    args[5] = 0                                                             # no clips: fine, and nothing to launch
    assert L.a2s_render_notes(st, *args) == 0
    assert hip.render_launches() == n0 and L.a2s_launch_count() == k0, "nothing was launched"
    assert L.a2s_render_notes(st, *ok) == 0
    torch.cuda.synchronize()
    assert hip.render_launches() == n0 + 1 and L.a2s_launch_count() == k0 + 1, "one launch per call"
    with pytest.raises(hip.A2SError):
        render.render(torch.from_numpy(progs))                              # a CPU tensor
    with pytest.raises(hip.A2SError):
        hip.render_notes(p.float(), N)
    q = progs.copy()
    q[1, 0, 0] = N - 1
    with pytest.raises(hip.A2SError):
        render.render(torch.from_numpy(q).to(dev))                          # the clips of a batch disagree about n_samples
    assert hip.render_launches() == n0 + 1


# ------------------------------------------------------------------------------------------- 5. score -> audio -> features
E2E_SEEDS = (137, 197, 95, 126)
E2E_BARS = 2


def test_generated_notes_land_on_their_vqt_bins(dev):
    """4 generator clips of 2 s -> render -> the product VQT (480 bins).  Every event of at least 0.1 s that no other event overlaps within 2 semitones
    with its fundamental, second or third partial (render_oracle.isolated_events): at the frame 50 ms after its onset the feature at bin
    5 (midi - 21) is the maximum of the bins within 7 of it."""
    from piano_a2s_amd.render import render
    from piano_a2s_amd.vqt import VQT
    cfg = spec.default_cfg(max_bars=E2E_BARS)
    clips = [scoregen.make_clip(cfg, s, frames=201) for s in E2E_SEEDS]
    progs = torch.from_numpy(np.stack([scoregen.pack_program(c) for c in clips])).to(dev)
    feat = VQT(dev)(render(progs))
    assert tuple(feat.shape) == (4, 1, 201, 480)
    feat = feat[:, 0].cpu().numpy()
    checked, worst = 0, np.inf
    for b, clip in enumerate(clips):
        for onset, length, midi in render_oracle.isolated_events(clip["events"]):
            frame, k = int(round((onset + 800) / 160)), 5 * (midi - 21)
            around = feat[b, frame, max(0, k - 7):k + 8].copy()
            here = around[k - max(0, k - 7)]
            around[k - max(0, k - 7)] = -1.0
            worst = min(worst, here - around.max())
            assert here >= around.max(), (E2E_SEEDS[b], onset, length, midi, int(around.argmax()) - 7, float(here - around.max()))
            checked += 1
    print(f"score -> audio -> features: {checked} events, smallest margin {worst:.4f}")
    assert checked >= 20


# ------------------------------------------------------------------------------------------- 6. the recipe
def _pretrain(tmp_path, name, extra):
    import pretrain
    ws = os.path.join(str(tmp_path), name)
    os.makedirs(ws)
    args = [os.path.join(ROOT, "hparams", "pretrain.yaml"), "--device=cuda:0", f"--workspace={ws}", "--soundfont_folder=/none", "--synthetic_clips=8",
            "--synthetic_frames=201", "--batch_size=2", "--number_of_epochs=1", "--hidden_size=32", "--conv_feature_size=32", "--max_length=(48, 32)",
            "--seed=1234"] + extra
    brain = pretrain.main(args)
    res = os.path.join(ws, "1234", "pretrain.epr", "results")
    records = {split: [json.load(open(os.path.join(res, split, f))) for f in sorted(os.listdir(os.path.join(res, split)))] for split in ("valid", "test")}
    return brain, records


def test_recipe_on_the_rendered_corpus(tmp_path, dev):
    from piano_a2s_amd import hip
    from piano_a2s_amd.kern_grammar import KernGrammar
    gram = KernGrammar()
    n0 = hip.render_launches()
    brain, records = _pretrain(tmp_path, "plain", [])
    assert hip.render_launches() == n0, "without --synthetic_scores nothing is rendered"
    brain, records = _pretrain(tmp_path, "rendered", ["--synthetic_scores=rendered"])
    n1 = hip.render_launches()
    assert n1 >= n0 + 4 + 1 + 1, "4 training batches, validation and test each render"
    assert len(records["valid"]) == 1 and len(records["test"]) == 1
    stats = brain.last_stats
    assert all(np.isfinite(stats[k]) for k in ("loss", "time_loss", "key_loss", "upper_loss", "lower_loss", "WER")), stats
    assert all(np.isfinite(v) for v in brain.train_stats.values()), brain.train_stats
    summary = json.load(open(os.path.join(str(tmp_path), "rendered", "1234", "pretrain.epr", "run_summary.json")))
    assert summary["fused_hip_step"] and summary["optimizer_steps"] == 4 and summary["nonfinite_steps"] == 0
    brain, records = _pretrain(tmp_path, "constrained", ["--synthetic_scores=rendered", "--constrained_decoding=true"])
    assert hip.render_launches() > n1
    bars = [bar for split in ("valid", "test") for rec in records[split] for pred in rec["pred"] for bar in pred[2:4]]
    assert len(bars) == 2 * 5 * 2 and all(gram.accepts(bar) for bar in bars), [gram.first_violation(bar) for bar in bars]
    assert all(np.isfinite(v) for v in brain.last_stats.values())
