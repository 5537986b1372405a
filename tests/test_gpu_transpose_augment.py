"""Transposition augmentation on the MI355X (csrc/a2s_augment.hip, piano_a2s_amd/augment.py):

6.  a2s_transpose_targets against kern_transpose.transpose_ids on a hand-built batch, with guard values around every buffer;
7.  a2s_shift_bins against the sliced input (whole shifts, bit for bit) and the float64 oracle (fractional shifts), F = 480 and F = 37;
8.  refusals launch nothing; two launches per TransposeAugment call;
9.  physics, as an inequality: shifted features are closer to the features of the transposed render than the unshifted ones are;
10. the training step sees what was augmented, with no synchronisation in between;
11. the recipe with and without --transpose_augment / --detune_bins, through pretrain.py and finetune.py."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

from data_processing.humdrum import LabelsMultiple
from piano_a2s_amd import kern_transpose as kt
from piano_a2s_amd import scoregen, spec
from piano_a2s_amd.augment import TransposeAugment
from tests import transpose_oracle as oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = LabelsMultiple(extended=True)
IDS = LABELS.labels_map
PAD, EOS = IDS["<pad>"], IDS["<eos>"]
GUARD = 1 << 40
FGUARD = 123.0


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


def _row(text, length):
    ids = LABELS.encode(text)
    assert len(ids) < length
    return ids + [EOS] + [PAD] * (length - len(ids) - 1)


# ------------------------------------------------------------------------------------------- 6. the targets
BARS, U, L = 3, 9, 6


def _hand_batch():
    c_major, g_major = 6, 7
    clips = [  # (s, detune, keys per bar, upper texts, lower texts)
        (0, 0.25, [c_major] * 3, ["4c 4e", "8f#\n8g", "2b-"], ["2C", "4r", "1GG"]),
        (-3, -1.5, [c_major, c_major, g_major], ["4c 4e", "8d\n8g", "4f# 4a"], ["2C", "4E", "2D"]),          # diatonic, two keys
        (2, 0.75, [c_major] * 3, ["4c 4e", "8d\n8g", "4f 4a"], ["2C", "4E", "2B#"]),                        # B# by (2, 2) needs two sharps
        (6, 2.0, [c_major] * 3, ["4CCC 4bbb", "8DDD\n8aaa", "4ccc"], ["2CCC", "4EEE", "2BBB"])]             # both ends of the range, staying inside
    key = torch.tensor([c[2] for c in clips], dtype=torch.long)
    upper = torch.tensor([[_row(t, U) for t in c[3]] for c in clips], dtype=torch.long)
    lower = torch.tensor([[_row(t, L) for t in c[4]] for c in clips], dtype=torch.long)
    return np.array([c[0] for c in clips], dtype=np.int32), np.array([c[1] for c in clips], dtype=np.float32), key, upper, lower


def _expected(s, d, key, upper, lower):
    """The batch under the draws by the pure-Python transposer: a clip with one unrepresentable bar stays as it is."""
    key2, upper2, lower2, eff, counts = key.clone(), upper.clone(), lower.clone(), np.array(d, dtype=np.float32), [0, 0, 0]
    for b in range(key.shape[0]):
        bars = [(kt.transpose_ids(upper[b, i].tolist(), int(key[b, i]), int(s[b])), kt.transpose_ids(lower[b, i].tolist(), int(key[b, i]), int(s[b])))
                for i in range(key.shape[1])]
        counts[0] += 1
        if any(u is None or l is None for u, l in bars):
            counts[2] += 1
            continue
        counts[1] += int(s[b] != 0)
        eff[b] = np.float32(5 * int(s[b])) + d[b]
        for i, (u, l) in enumerate(bars):
            upper2[b, i], lower2[b, i], key2[b, i] = torch.tensor(u[0]), torch.tensor(l[0]), u[1]
    return key2, upper2, lower2, eff, counts


def test_transpose_targets_against_the_python_transposer(dev):
    from piano_a2s_amd import hip
    s, d, key, upper, lower = _hand_batch()
    want_key, want_upper, want_lower, want_eff, want_counts = _expected(s, d, key, upper, lower)
    assert want_counts == [4, 2, 1] and want_eff.tolist() == [0.25, -16.5, 0.75, 32.0]
    assert torch.equal(want_upper[2], upper[2]) and not torch.equal(want_upper[1], upper[1]) and want_key[1].tolist() == [9, 9, 10]
    assert int(want_upper[3, 0, 1]) == IDS["FFF#"] and int(want_upper[3, 0, 4]) == IDS["eeee#"]
    tables = [torch.from_numpy(np.array(t)).to(dev) for t in kt.tables()]
    bufs = {name: _guarded(t, dev, guard) for name, t, guard in (("key", key, GUARD), ("upper", upper, GUARD), ("lower", lower, GUARD),
                                                                 ("eff", torch.full((4,), FGUARD), FGUARD), ("counters", torch.tensor([10, 20, 30], dtype=torch.int32), 77))}
    n0 = hip.augment_launches()
    hip.transpose_targets(*tables, torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev), bufs["key"][1], bufs["upper"][1], bufs["lower"][1], 5,
                          bufs["eff"][1], bufs["counters"][1])
    torch.cuda.synchronize()
    assert hip.augment_launches() == n0 + 1
    assert torch.equal(bufs["upper"][1].cpu(), want_upper) and torch.equal(bufs["lower"][1].cpu(), want_lower) and torch.equal(bufs["key"][1].cpu(), want_key)
    assert bufs["eff"][1].cpu().numpy().tolist() == want_eff.tolist()
    assert bufs["counters"][1].cpu().tolist() == [10 + 4, 20 + 2, 30 + 1]
    for name, (flat, view) in bufs.items():
        guard = {"eff": FGUARD, "counters": 77}.get(name, GUARD)
        assert _guards_intact(flat, view.numel(), guard), name
    # ids or keys out of range make the clip unrepresentable, nothing else
    bad_key, bad_tok = key.clone(), upper.clone()
    bad_key[1, 2], bad_tok[3, 1, 0] = 14, 173
    k2, u2, l2 = bad_key.to(dev), bad_tok.to(dev), lower.to(dev)
    eff, counters = torch.empty(4, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)
    hip.transpose_targets(*tables, torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev), k2, u2, l2, 5, eff, counters)
    assert counters.tolist() == [4, 0, 3] and eff.cpu().numpy().tolist() == [0.25, -1.5, 0.75, 2.0]
    assert torch.equal(k2.cpu(), bad_key) and torch.equal(u2.cpu(), bad_tok) and torch.equal(l2.cpu(), lower)


# ------------------------------------------------------------------------------------------- 7. the features
ROWS = 5


def _shifts(F):
    return [0.0, 5.0, -5.0, 30.0, -30.0, 0.5, 2.25, -31.75, float(F + 3), float(-(F + 3))]


@pytest.mark.parametrize("F", [480, 37])
@pytest.mark.parametrize("lead", [64, 3], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("ROWS", [5, 37])          # 37: workgroups whose 16 rows all exist (the loads of eight rows issued together) and a last one of 5
def test_shift_bins_against_slices_and_the_float64_oracle(dev, F, lead, ROWS):
    """Whole shifts: bit for bit.  Fractional shifts: |device - float64| <= 2^-22 (inputs in [0, 1]; two products and one sum, each rounded
    to within 2^-24 of a value <= 1).  lead 64 / 3: y starts 16-byte aligned (vector stores when F % 4 == 0) / does not (scalar stores)."""
    from piano_a2s_amd import hip
    g = torch.Generator().manual_seed(F)
    shifts = _shifts(F)
    n0 = hip.augment_launches()
    for call in range(4):
        ns = [shifts[(3 * call + i) % len(shifts)] for i in range(3)]
        x = torch.rand((3, ROWS, F), generator=g)
        xflat, xv = _guarded(x, dev, float("nan"), lead=lead, tail=F + 5)            # NaN before and behind the input: never read into a result
        yflat, yv = _guarded(torch.full((3, ROWS, F), FGUARD), dev, FGUARD, lead=lead, tail=F + 5)
        hip.shift_bins(xv, torch.tensor(ns, dtype=torch.float32, device=dev), y=yv)
        torch.cuda.synchronize()
        got = yv.cpu()
        assert _guards_intact(yflat, 3 * ROWS * F, FGUARD, lead=lead), "the guards before and behind the output"
        assert torch.isfinite(got).all()
        for b, n in enumerate(ns):
            if abs(n) >= F + 1:
                assert (got[b] == 0).all(), n
            elif n == int(n):
                m, want = int(n), torch.zeros(ROWS, F)
                if m >= 0:
                    want[:, m:] = x[b, :, :F - m]
                else:
                    want[:, :F + m] = x[b, :, -m:]
                assert torch.equal(got[b].view(torch.int32), want.view(torch.int32)), n
            else:
                want = oracle.shift_bins(x[b].numpy(), n)
                err = np.abs(got[b].numpy().astype(np.float64) - want).max()
                print(f"shift_bins F = {F}, n = {n}: max |device - float64| = {err:.3e} (asserted {2.0 ** -22:.3e})")
                assert err <= 2.0 ** -22, (n, err)
    assert hip.augment_launches() == n0 + 4


# ------------------------------------------------------------------------------------------- 8. refusals, launch counter
def test_refusals_launch_nothing(dev):
    from piano_a2s_amd import hip
    Lib = hip.lib()
    st = hip.stream()
    s, d, key, upper, lower = _hand_batch()
    tables = [torch.from_numpy(np.array(t)).to(dev) for t in kt.tables()]
    sd, dd, kd, ud, ld = torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev), key.to(dev), upper.to(dev), lower.to(dev)
    eff, counters = torch.zeros(4, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)
    n0, k0 = hip.augment_launches(), Lib.a2s_launch_count()
    ok = (hip._p(tables[0]), hip._p(tables[1]), hip._p(tables[2]), 25, 173, hip._p(sd), hip._p(dd), hip._p(kd), hip._p(ud), hip._p(ld), BARS, U, L, 5,
          hip._p(eff), hip._p(counters), 4)
    for i, bad in [(i, None) for i in (0, 1, 2, 5, 6, 7, 8, 9, 14, 15)] + [(3, 0), (4, 0), (10, 0), (11, -1), (12, 0), (13, 0), (16, -1)]:
        args = list(ok)
        args[i] = bad
        assert Lib.a2s_transpose_targets(st, *args) == -1, i
        assert b"transpose_targets" in Lib.a2s_last_error()
    args = list(ok)
    args[16] = 0
    assert Lib.a2s_transpose_targets(st, *args) == 0
    x, y = torch.rand(2, ROWS, 480, device=dev), torch.zeros(2, ROWS, 480, device=dev)
    e2 = torch.zeros(2, device=dev)
    ok2 = (hip._p(x), hip._p(y), hip._p(e2), 2, ROWS, 480)
    for i, bad in ((0, None), (1, None), (2, None), (3, -1), (3, 65536), (4, 0), (5, 0), (1, hip._p(x))):
        args = list(ok2)
        args[i] = bad
        assert Lib.a2s_shift_bins(st, *args) == -1, i
        assert b"shift_bins" in Lib.a2s_last_error()
    args = list(ok2)
    args[3] = 0
    assert Lib.a2s_shift_bins(st, *args) == 0
    torch.cuda.synchronize()
    assert hip.augment_launches() == n0 and Lib.a2s_launch_count() == k0, "nothing was launched"
    assert torch.equal(kd.cpu(), key) and torch.equal(ud.cpu(), upper) and (y == 0).all() and counters.tolist() == [0, 0, 0]
    # the typed wrappers name the argument
    with pytest.raises(hip.A2SError, match="upper"):
        hip.transpose_targets(*tables, sd, dd, kd, ud[:, :2].contiguous(), ld, 5, eff, counters)
    with pytest.raises(hip.A2SError, match="semitones"):
        hip.transpose_targets(*tables, sd.long(), dd, kd, ud, ld, 5, eff, counters)
    with pytest.raises(hip.A2SError, match="lower"):
        hip.transpose_targets(*tables, sd, dd, kd, ud, ld.transpose(1, 2), 5, eff, counters)
    with pytest.raises(hip.A2SError, match="eff_bins"):
        hip.shift_bins(x, torch.zeros(3, device=dev))
    with pytest.raises(hip.A2SError, match="`x`"):
        hip.shift_bins(x.transpose(1, 2), e2)
    with pytest.raises(hip.A2SError):
        hip.transpose_targets(*tables, sd, dd, key, ud, ld, 5, eff, counters)          # host memory
    with pytest.raises(hip.A2SError):
        hip.shift_bins(x.cpu(), e2)
    assert hip.augment_launches() == n0
    # one TransposeAugment call: exactly the two launches
    aug = TransposeAugment(spec.default_cfg(), 2, 1.0, seed=7, device=dev)
    batch = [torch.rand(4, 1, ROWS, 480, device=dev), None, kd, ud, None, ld]
    out = aug(batch)
    torch.cuda.synchronize()
    assert hip.augment_launches() == n0 + 2 and Lib.a2s_launch_count() == k0 + 2
    assert out[0] is not batch[0] and out[0].shape == batch[0].shape and out[2] is kd and out[3] is ud and out[5] is ld
    assert aug.counts()["clips"] == 4


# ------------------------------------------------------------------------------------------- 9. physics
def _transposed_program(clip, s):
    """The clip's program with every event's MIDI raised by s: same instrument, amplitudes and decays (those of the notes as drawn)."""
    prog = scoregen.pack_program(clip, rows=len(clip["events"]))
    head = prog[0]
    f = head[4:7].view(np.float32)
    inst = clip["instrument"]
    notes = [(int(o), int(l), int(m) + s, float(a), float(prog[i, 4:5].view(np.float32)[0]), inst["g"], inst["n_harm"])
             for i, ((o, l, m), a) in enumerate(zip(clip["events"], clip["amps"]), 1)]
    out = scoregen.pack_rows(int(head[0]), notes, attack=int(head[2]), rel_len=int(head[3]), rel_rate=float(f[0]), gain=float(f[1]), noise_level=float(f[2]),
                             noise_seed=int(np.array(head[7], dtype=np.int32).view(np.uint32)))
    same = scoregen.pack_rows(int(head[0]), [(n[0], n[1], n[2] - s) + n[3:] for n in notes], attack=int(head[2]), rel_len=int(head[3]), rel_rate=float(f[0]),
                              gain=float(f[1]), noise_level=float(f[2]), noise_seed=int(np.array(head[7], dtype=np.int32).view(np.uint32)))
    assert np.array_equal(same, prog), "the rebuilt program with s = 0 is the clip's own"
    return prog, out


@pytest.mark.parametrize("s", [2, -2])
def test_shifted_features_are_closer_to_the_transposed_render(dev, s):
    from piano_a2s_amd import hip
    from piano_a2s_amd.render import render
    from piano_a2s_amd.vqt import VQT
    cfg = spec.default_cfg(max_bars=2)
    clips = [scoregen.make_clip(cfg, seed, frames=201) for seed in (137, 197)]
    rows = max(len(c["events"]) for c in clips)
    assert rows >= 8
    progs = [_transposed_program(c, s) for c in clips]
    pad = lambda p: np.concatenate([p, np.zeros((1 + rows - p.shape[0], 8), dtype=np.int32)])
    stack = torch.from_numpy(np.stack([pad(p) for pair in progs for p in pair])).to(dev)          # [clip 0, clip 0 + s, clip 1, clip 1 + s]
    feat = VQT(dev)(render(stack))
    drawn, moved = feat[0::2].contiguous(), feat[1::2]
    shifted = hip.shift_bins(drawn, torch.full((2,), 5.0 * s, device=dev))
    lo, hi = (5 * s, 480) if s > 0 else (0, 480 + 5 * s)
    with_shift = float((shifted - moved)[..., lo:hi].abs().mean())
    without = float((drawn - moved)[..., lo:hi].abs().mean())
    print(f"s = {s:+d}: mean |shift(features) - transposed render| = {with_shift:.5f}, mean |features - transposed render| = {without:.5f}")
    assert with_shift < without


# ------------------------------------------------------------------------------------------- 10. the step sees the augmented batch
def test_step_reads_the_augmented_targets_without_a_synchronisation(dev):
    import models
    from datasets.syn import RenderedClips
    from piano_a2s_amd import recipe, train
    cfg = spec.default_cfg(hidden_size=32, conv_feature_size=32, max_length=(48, 32))
    ds = RenderedClips(cfg, 2, seed=4321, frames=201)
    host = torch.utils.data.default_collate([ds[i] for i in range(2)])
    torch.manual_seed(11)
    init = models.ScoreTranscription(**cfg).state_dict()
    aug = TransposeAugment(cfg, 3, 1.5, seed=99, device=dev)
    draws = (np.array([3, -2], dtype=np.int32), np.array([0.75, -1.25], dtype=np.float32))
    assert all(kt.transpose_ids(ids, ds.clip(b)["key"], int(draws[0][b])) is not None for b in range(2) for st in ("upper", "lower") for ids in ds.clip(b)["ids"][st])
    res = []
    for mode in ("plain", "racy", "synced"):
        m = models.ScoreTranscription(**cfg)
        m.load_state_dict(init)
        m = m.to(dev).train()
        step = train.TrainStep(m, dropout=False)
        batch = recipe._features(list(host), dev)
        torch.cuda.synchronize()
        if mode != "plain":
            batch = aug.apply(batch, *draws)                     # two launches on the current stream ...
            if mode == "synced":
                torch.cuda.synchronize()
        losses = step(batch, 0.7, rng=random.Random(3))          # ... and the step right behind them
        torch.cuda.synchronize()
        res.append((losses[:, 0].clone().cpu(), step.decode_steps, [t.cpu() for t in batch[2:7]]))
    (l_plain, steps_plain, t_plain), (l_racy, steps_racy, t_racy), (l_sync, steps_sync, t_sync) = res
    assert torch.isfinite(l_racy).all()
    assert torch.equal(l_racy, l_sync), (l_racy, l_sync)
    assert steps_racy == steps_sync == steps_plain and steps_plain > 0, "the host plan has the lengths of the un-augmented batch"
    assert torch.equal(t_racy[2], t_plain[2]) and torch.equal(t_racy[4], t_plain[4]), "the lengths are untouched"
    assert not torch.equal(t_racy[1], t_plain[1]) and not torch.equal(t_racy[0], t_plain[0]), "the score and the key were respelled"
    assert ((t_racy[1] == PAD) == (t_plain[1] == PAD)).all() and not torch.equal(l_racy, l_plain)


# ------------------------------------------------------------------------------------------- 11. the recipe
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


def test_recipe_without_the_flags_launches_nothing(tmp_path, dev):
    import pretrain
    from piano_a2s_amd import hip
    n0 = hip.augment_launches()
    brain, summary = _run(pretrain, tmp_path, "off", [])
    assert hip.augment_launches() == n0, "without the flags nothing is launched"
    assert "transpose_augment" not in summary and brain._transpose_augment() is None and summary["optimizer_steps"] == 4
    assert "augmented_clips" not in brain.train_stats


def test_recipe_with_the_flags(tmp_path, dev):
    import pretrain
    from piano_a2s_amd import hip
    n0 = hip.augment_launches()
    brain, summary = _run(pretrain, tmp_path, "on", ["--transpose_augment=3", "--detune_bins=1.5"])
    assert hip.augment_launches() == n0 + 2 * 4, "two launches for each of the 4 training batches, none in VALID or TEST"
    assert summary["fused_hip_step"] and summary["optimizer_steps"] == 4 and summary["nonfinite_steps"] == 0
    block = summary["transpose_augment"]
    assert block["max_semitones"] == 3 and block["detune_bins"] == 1.5 and block["clips"] == 8
    assert 0 <= block["transposed"] <= 8 and block["transposed"] + block["not_representable"] <= 8
    assert all(np.isfinite(brain.last_stats[k]) for k in ("loss", "time_loss", "key_loss", "upper_loss", "lower_loss", "WER", "WER_upper", "WER_lower")), brain.last_stats
    assert all(np.isfinite(v) for v in brain.train_stats.values()), brain.train_stats
    assert brain.train_stats["augmented_clips"] == 8


def test_recipe_refuses_values_out_of_range_before_training(tmp_path, dev):
    import pretrain
    from piano_a2s_amd import hip
    n0 = hip.augment_launches()
    for i, extra in enumerate((["--transpose_augment=9"], ["--transpose_augment=2", "--detune_bins=3.0"])):
        with pytest.raises(ValueError, match="transpose_augment|detune_bins"):
            _run(pretrain, tmp_path, f"refused{i}", extra)
        assert not os.path.exists(os.path.join(str(tmp_path), f"refused{i}", "1234", "pretrain.epr", "results")), "refused before the first epoch"
    assert hip.augment_launches() == n0


def test_finetune_takes_the_same_flags(tmp_path, dev):
    import finetune
    from piano_a2s_amd import hip
    n0 = hip.augment_launches()
    brain, summary = _run(finetune, tmp_path, "fine", ["--transpose_augment=2", "--detune_bins=0.5"])
    assert hip.augment_launches() == n0 + 2 * 4
    assert summary["transpose_augment"]["clips"] == 8 and summary["transpose_augment"]["max_semitones"] == 2
    assert brain.finetune and np.isfinite(brain.last_stats["WER"])
