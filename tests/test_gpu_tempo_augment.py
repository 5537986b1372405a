"""Tempo augmentation on the MI355X (csrc/a2s_tempo.hip, piano_a2s_amd/augment.py):

1. a2s_tempo_plan: the content of hand-built clips exactly, the planned step against the float32 restatement, counters, one launch;
2. a2s_stretch_frames against the input (step 65536, bit for bit) and the float64 oracle, F = 480 and F = 37, aligned and not, with guards;
3. refusals launch nothing; the typed wrappers name the argument;
4. one TempoAugment call is two launches of its own counter, beside the transposer two each;
5. physics, as an inequality: stretched features are closer to the features of the clip rendered slower or faster than the unstretched ones are;
6. the training step reads the stretched features with no synchronisation in between;
7. the recipe with and without --tempo_augment, through pretrain.py and finetune.py.

Measured on the MI355X (the figures the tests print): max |device - float64| of a2s_stretch_frames 7.4e-08 for step < 65536 (asserted 2^-22 = 2.38e-07) and
1.54e-07 for step > 65536 (asserted 2^-20 = 9.54e-07); the physics ratio 0.165 - 0.273 (asserted < 0.5); see DESIGN.md section 18."""
import json
import os
import random

import numpy as np
import pytest
import torch

from piano_a2s_amd import scoregen, spec
from piano_a2s_amd.augment import TempoAugment, TransposeAugment
from tests import tempo_oracle as oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FGUARD = 123.0
IGUARD = -77


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


# ------------------------------------------------------------------------------------------- 1. the plan
def _plan_clips(rows, F):
    """Five clips and their content: all zero; only -0.0; one value at the last column of row 0; one at the last column of a middle row; a NaN in the
    last row."""
    x = torch.zeros(5, rows, F)
    x[1] = -0.0
    x[2, 0, F - 1] = 0.5
    x[3, rows // 2, F - 1] = -1e-30
    x[4, rows - 1, F // 2] = float("nan")
    x[4, 0, 0] = 1.0
    return x, [0, 0, 1, rows // 2 + 1, rows]


@pytest.mark.parametrize("F", [480, 37])
@pytest.mark.parametrize("rows", [5, 16, 17, 37, 1201])          # below, at and above one chunk of 16 rows; several chunks; the training window
def test_tempo_plan_content_step_and_counters(dev, F, rows):
    from piano_a2s_amd import hip
    R, min_frames, N = (0.25 if F == 480 else 0.15), max(1, rows // 3), 64
    x, want_content = _plan_clips(rows, F)
    xflat, xv = _guarded(x, dev, 7.0, lead=64, tail=F + 5)              # non-zero values before and behind the clips: never taken for content
    us = np.random.default_rng(1000 * F + rows).random(size=N, dtype=np.float32)
    u_dev = torch.from_numpy(np.repeat(us[:, None], 5, axis=1).copy()).to(dev)
    cflat, cv = _guarded(torch.full((N, 5), IGUARD, dtype=torch.int32), dev, IGUARD)
    sflat, sv = _guarded(torch.full((N, 5), IGUARD, dtype=torch.int32), dev, IGUARD)
    kflat, kv = _guarded(torch.tensor([10, 20, 30], dtype=torch.int32), dev, IGUARD)
    n0, a0, k0 = hip.tempo_launches(), hip.augment_launches(), hip.lib().a2s_launch_count()
    hip.tempo_plan(xv, u_dev[0], R, min_frames, cv[0], sv[0], kv)
    assert hip.tempo_launches() == n0 + 1 and hip.lib().a2s_launch_count() == k0 + 1 and hip.augment_launches() == a0, "exactly one launch, of the tempo counter"
    for i in range(1, N):
        hip.tempo_plan(xv, u_dev[i], R, min_frames, cv[i], sv[i], kv)
    torch.cuda.synchronize()
    content, step, counters = cv.cpu().numpy(), sv.cpu().numpy(), kv.cpu().tolist()
    assert all(_guards_intact(flat, n, IGUARD) for flat, n in ((cflat, 5 * N), (sflat, 5 * N), (kflat, 3)))
    assert (content == np.array(want_content, dtype=np.int32)[None, :]).all(), content[0]
    left_out = planned = 0
    for i, u in enumerate(us):
        for b, n in enumerate(want_content):
            want, kept = oracle.plan(n, rows, u, R, min_frames)
            if kept:
                assert step[i, b] == oracle.ONE, (u, n)
                continue
            planned += 1
            q = oracle.quotient(n, rows, u, R, min_frames)
            if q is not None and abs(q - np.floor(q) - 0.5) < 0.01 and oracle.MIN_STEP < q < oracle.MAX_STEP:
                left_out += 1
                assert abs(int(step[i, b]) - want) <= 1, (u, n, step[i, b], want)
            else:
                assert step[i, b] == want, (u, n, step[i, b], want, q)
    print(f"tempo_plan rows = {rows}, F = {F}: {planned} planned steps, {left_out} within 0.01 of a rounding boundary")
    assert left_out <= 0.05 * max(planned, 1)
    kept_clips = sum(oracle.plan(n, rows, 0.5, R, min_frames)[1] for n in want_content)          # (whether a clip is kept does not depend on u)
    assert counters == [10 + 5 * N, 20 + int((step != oracle.ONE).sum()), 30 + kept_clips * N], counters
    assert kept_clips >= 2 and planned > 0


# ------------------------------------------------------------------------------------------- 2. the frames
STEPS = [65536, 52429, 87381, 65535, 65537, 60000, 75000, 0, 200000]
_CASES = [(F, lead, rows) for F in (480, 37) for lead in (64, 3) for rows in (5, 37)] + [(480, 64, 1201)]          # 1201 rows: the largest pos


@pytest.mark.parametrize("F,lead,rows", _CASES, ids=[f"F{F}-{'aligned' if lead == 64 else 'unaligned'}-rows{rows}" for F, lead, rows in _CASES])
def test_stretch_frames_against_the_input_and_the_float64_oracle(dev, F, lead, rows):
    """One clip per step.  65536: bit for bit (a -0.0 among the inputs included).  0 and 200000: zeros.  step < 65536: |device - float64| <= 2^-22 (inputs
    in [0, 1]; the weights w / 65536 are exact, then two products and one sum, each rounded to within 2^-24 of a value <= 1).  step > 65536: <= 2^-20
    (three weights, each w * (1 / W) with two roundings, then three products and two sums: under 11 * 2^-24).  lead 64 / 3: y starts 16-byte aligned
    (vector loads and stores when F % 4 == 0) / does not (the scalar instance)."""
    from piano_a2s_amd import hip
    B = len(STEPS)
    x = torch.rand((B, rows, F), generator=torch.Generator().manual_seed(F + rows))
    x[0, 1, 2] = -0.0
    xflat, xv = _guarded(x, dev, float("nan"), lead=lead, tail=F + 5)                # NaN before and behind the input: never read into a result
    yflat, yv = _guarded(torch.full((B, rows, F), FGUARD), dev, FGUARD, lead=lead, tail=F + 5)
    n0, a0 = hip.tempo_launches(), hip.augment_launches()
    hip.stretch_frames(xv, torch.tensor(STEPS, dtype=torch.int32, device=dev), y=yv)
    torch.cuda.synchronize()
    assert hip.tempo_launches() == n0 + 1 and hip.augment_launches() == a0
    got = yv.cpu()
    assert _guards_intact(yflat, B * rows * F, FGUARD, lead=lead), "the guards before and behind the output"
    assert torch.isfinite(got).all()
    worst = {"expand": 0.0, "compress": 0.0}
    for b, step in enumerate(STEPS):
        if step == oracle.ONE:
            assert torch.equal(got[b].view(torch.int32), x[b].view(torch.int32)), "step 65536 is a copy, bit for bit"
        elif not oracle.MIN_STEP <= step <= oracle.MAX_STEP:
            assert (got[b] == 0).all(), step
        else:
            err = float(np.abs(got[b].numpy().astype(np.float64) - oracle.stretch(x[b].numpy(), step)).max())
            kind, bound = ("expand", 2.0 ** -22) if step < oracle.ONE else ("compress", 2.0 ** -20)
            worst[kind] = max(worst[kind], err)
            print(f"stretch_frames F = {F}, rows = {rows}, step = {step}: max |device - float64| = {err:.3e} (asserted {bound:.3e})")
            assert err <= bound, (step, err)
    print(f"stretch_frames F = {F}, rows = {rows}, lead = {lead}: worst {worst}")


# ------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_launch_nothing(dev):
    from piano_a2s_amd import hip
    Lib, st = hip.lib(), hip.stream()
    rows, F = 5, 480
    x, y = torch.rand(2, rows, F, device=dev), torch.zeros(2, rows, F, device=dev)
    u, content, step = torch.rand(2, device=dev), torch.full((2,), IGUARD, dtype=torch.int32, device=dev), torch.full((2,), oracle.ONE, dtype=torch.int32, device=dev)
    counters = torch.zeros(3, dtype=torch.int32, device=dev)
    n0, a0, k0 = hip.tempo_launches(), hip.augment_launches(), Lib.a2s_launch_count()
    ok = (hip._p(x), 2, rows, F, hip._p(u), 0.15, 1, hip._p(content), hip._p(step), hip._p(counters))
    bad_plan = [(0, None), (4, None), (7, None), (8, None), (9, None), (1, -1), (1, 65536), (2, 0), (2, 16385), (3, 0), (5, -0.01), (5, 0.26), (5, float("nan")),
                (5, float("inf")), (6, 0)]
    for i, bad in bad_plan:
        args = list(ok)
        args[i] = bad
        assert Lib.a2s_tempo_plan(st, *args) == -1, (i, bad)
        assert b"tempo_plan" in Lib.a2s_last_error()
    args = list(ok)
    args[1] = 0
    assert Lib.a2s_tempo_plan(st, *args) == 0
    ok2 = (hip._p(x), hip._p(y), hip._p(step), 2, rows, F)
    for i, bad in ((0, None), (1, None), (2, None), (1, hip._p(x)), (3, -1), (3, 65536), (4, 0), (4, 16385), (5, 0)):
        args = list(ok2)
        args[i] = bad
        assert Lib.a2s_stretch_frames(st, *args) == -1, (i, bad)
        assert b"stretch_frames" in Lib.a2s_last_error()
    args = list(ok2)
    args[3] = 0
    assert Lib.a2s_stretch_frames(st, *args) == 0
    torch.cuda.synchronize()
    assert hip.tempo_launches() == n0 and Lib.a2s_launch_count() == k0 and hip.augment_launches() == a0, "nothing was launched"
    assert (y == 0).all() and (content == IGUARD).all() and counters.tolist() == [0, 0, 0]
    # the typed wrappers name the argument
    with pytest.raises(hip.A2SError, match="`u`"):
        hip.tempo_plan(x, torch.rand(3, device=dev), 0.15, 1, content, step, counters)
    with pytest.raises(hip.A2SError, match="`step`"):
        hip.tempo_plan(x, u, 0.15, 1, content, step.long(), counters)
    with pytest.raises(hip.A2SError, match="`R`"):
        hip.tempo_plan(x, u, 0.3, 1, content, step, counters)
    with pytest.raises(hip.A2SError, match="`min_frames`"):
        hip.tempo_plan(x, u, 0.15, 0, content, step, counters)
    with pytest.raises(hip.A2SError, match="`counters`"):
        hip.tempo_plan(x, u, 0.15, 1, content, step, counters[:2])
    with pytest.raises(hip.A2SError, match="`x`"):
        hip.stretch_frames(x.transpose(1, 2), step)
    with pytest.raises(hip.A2SError, match="`step`"):
        hip.stretch_frames(x, step.float())
    with pytest.raises(hip.A2SError, match="`y`"):
        hip.stretch_frames(x, step, y=y[:, :4])
    with pytest.raises(hip.A2SError):
        hip.tempo_plan(x.cpu(), u, 0.15, 1, content, step, counters)          # host memory
    with pytest.raises(hip.A2SError):
        hip.stretch_frames(x.cpu(), step)
    torch.cuda.synchronize()
    assert hip.tempo_launches() == n0 and Lib.a2s_launch_count() == k0


# ------------------------------------------------------------------------------------------- 4. launches
def test_one_call_is_two_launches_of_its_own_counter(dev):
    from piano_a2s_amd import hip
    from piano_a2s_amd import kern_transpose  # noqa: F401  (the transposer's tables)
    Lib = hip.lib()
    cfg = spec.default_cfg()
    rows = 37
    x = torch.rand(4, 1, rows, 480, device=dev)
    x[1, :, 20:] = 0                                                               # a padded clip: content 20 of 37 rows
    key, upper, lower = torch.full((4, 5), 6, device=dev), torch.ones(4, 5, 9, dtype=torch.long, device=dev), torch.ones(4, 5, 6, dtype=torch.long, device=dev)
    batch = [x, None, key, upper, None, lower]
    tempo = TempoAugment(cfg, 0.2, seed=7, device=dev)
    n0, a0, k0 = hip.tempo_launches(), hip.augment_launches(), Lib.a2s_launch_count()
    out = tempo(batch)
    torch.cuda.synchronize()
    assert hip.tempo_launches() == n0 + 2 and hip.augment_launches() == a0 and Lib.a2s_launch_count() == k0 + 2
    assert out[0] is not x and out[0].shape == x.shape and all(out[i] is batch[i] for i in (2, 3, 5)), "a new feature tensor, no target touched"
    content, step = (t.cpu().tolist() for t in tempo.last_plan)
    assert content == [37, 20, 37, 37] and all(s >= oracle.ONE for i, s in enumerate(step) if i != 1), "a full window is only ever compressed"
    want = [oracle.plan(n, rows, u, 0.2, 12)[0] for n, u in zip(content, TempoAugment(cfg, 0.2, seed=7, device=dev).draw(4))]
    assert all(abs(s - w) <= 1 for s, w in zip(step, want)), (step, want)
    assert tempo.counts() == dict(clips=4, stretched=sum(s != oracle.ONE for s in step), kept=0)
    # beside the transposer: two launches each, each on its own counter
    transposer = TransposeAugment(cfg, 2, 1.0, seed=7, device=dev)
    n0, a0, k0 = hip.tempo_launches(), hip.augment_launches(), Lib.a2s_launch_count()
    out = tempo(transposer(batch))
    torch.cuda.synchronize()
    assert hip.tempo_launches() == n0 + 2 and hip.augment_launches() == a0 + 2 and Lib.a2s_launch_count() == k0 + 4
    assert tempo.counts()["clips"] == 8 and transposer.counts()["clips"] == 4


# ------------------------------------------------------------------------------------------- 5. physics
def _scaled_program(clip, c):
    """The clip's render program without its noise floor, every event's onset and length multiplied by c (rounded to samples)."""
    p = scoregen.pack_program(clip, rows=len(clip["events"])).copy()
    p[0, 6] = np.array(0.0, dtype=np.float32).view(np.int32)
    p[1:, 0] = np.rint(p[1:, 0] * c).astype(np.int32)
    p[1:, 1] = np.rint(p[1:, 1] * c).astype(np.int32)
    return p


@pytest.mark.parametrize("seed", [137, 3])
def test_stretched_features_are_closer_to_the_render_at_the_other_tempo(dev, seed):
    """mean |stretch(features) - scaled render| < 0.5 * mean |features - scaled render| for c in {0.80, 0.90, 1.05, 1.10}.  With the host renderer and
    the librosa VQT the ratio is 0.16 - 0.27 for these seeds and factors; 0.5 leaves about 2 x over the worst of them."""
    from piano_a2s_amd import hip
    from piano_a2s_amd.render import render
    from piano_a2s_amd.vqt import VQT
    factors = (0.80, 0.90, 1.05, 1.10)
    clip = scoregen.make_clip(spec.default_cfg(max_bars=2), seed, frames=201)
    assert len(clip["events"]) >= 4
    progs = [_scaled_program(clip, c) for c in (1.0,) + factors]
    assert int(progs[0][0, 0]) == clip["n_samples"] and max(int((p[1:, 0] + p[1:, 1]).max()) for p in progs) <= clip["n_samples"], "the content stays in the window"
    feat = VQT(dev)(render(torch.from_numpy(np.stack(progs)).to(dev)))
    drawn = feat[:1].expand(len(factors), *feat.shape[1:]).contiguous()
    steps = [int(np.rint(65536 / c)) for c in factors]
    stretched = hip.stretch_frames(drawn, torch.tensor(steps, dtype=torch.int32, device=dev))
    for i, c in enumerate(factors):
        with_stretch = float((stretched[i] - feat[1 + i]).abs().mean())
        without = float((drawn[i] - feat[1 + i]).abs().mean())
        print(f"seed {seed}, c = {c}: mean |stretch(features) - scaled render| = {with_stretch:.5f}, mean |features - scaled render| = {without:.5f}, "
              f"ratio {with_stretch / without:.3f}")
        assert with_stretch < 0.5 * without, (c, with_stretch, without)


# ------------------------------------------------------------------------------------------- 6. the step reads the stretched features
def test_step_reads_the_stretched_features_without_a_synchronisation(dev):
    import models
    from datasets.syn import RenderedClips
    from piano_a2s_amd import hip, recipe, train
    cfg = spec.default_cfg(hidden_size=32, conv_feature_size=32, max_length=(48, 32))
    ds = RenderedClips(cfg, 2, seed=4321, frames=201)
    host = torch.utils.data.default_collate([ds[i] for i in range(2)])
    torch.manual_seed(11)
    init = models.ScoreTranscription(**cfg).state_dict()
    tempo = TempoAugment(cfg, 0.25, seed=99, device=dev)
    u = np.array([0.9, 0.2], dtype=np.float32)
    res, recorded = [], None
    for mode in ("plain", "racy", "beforehand"):
        m = models.ScoreTranscription(**cfg)
        m.load_state_dict(init)
        m = m.to(dev).train()
        step = train.TrainStep(m, dropout=False)
        batch = recipe._features(list(host), dev)
        torch.cuda.synchronize()
        if mode == "racy":
            batch = tempo.apply(batch, u)                        # two launches on the current stream ...
        elif mode == "beforehand":
            batch = list(batch)
            batch[0] = hip.stretch_frames(batch[0].contiguous(), recorded)
            torch.cuda.synchronize()
        losses = step(batch, 0.7, rng=random.Random(3))          # ... and the step right behind them
        torch.cuda.synchronize()
        if mode == "racy":
            recorded = tempo.last_plan[1].clone()
        res.append((losses[:, 0].clone().cpu(), [t.cpu() for t in batch[2:7]]))
    (l_plain, t_plain), (l_racy, t_racy), (l_before, t_before) = res
    assert torch.isfinite(l_racy).all()
    assert torch.equal(l_racy, l_before), (l_racy, l_before)
    assert (recorded.cpu() != oracle.ONE).any() and not torch.equal(l_racy, l_plain), "the clips were stretched and the loss shows it"
    assert all(torch.equal(a, b) for a, b in zip(t_racy, t_plain)), "no target was touched"


# ------------------------------------------------------------------------------------------- 7. the recipe
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


def test_recipe_without_the_flag_launches_nothing(tmp_path, dev):
    import pretrain
    from piano_a2s_amd import hip
    n0 = hip.tempo_launches()
    brain, summary = _run(pretrain, tmp_path, "off", [])
    assert hip.tempo_launches() == n0, "without the flag nothing is launched"
    assert "tempo_augment" not in summary and brain._tempo_augment() is None and summary["optimizer_steps"] == 4
    assert "tempo_clips" not in brain.train_stats


def test_recipe_with_the_flag(tmp_path, dev):
    import pretrain
    from piano_a2s_amd import hip
    n0, a0 = hip.tempo_launches(), hip.augment_launches()
    brain, summary = _run(pretrain, tmp_path, "on", ["--tempo_augment=0.15"])
    assert hip.tempo_launches() == n0 + 2 * 4 and hip.augment_launches() == a0, "two launches for each of the 4 training batches, none in VALID or TEST"
    assert summary["fused_hip_step"] and summary["optimizer_steps"] == 4 and summary["nonfinite_steps"] == 0
    block = summary["tempo_augment"]
    assert block["max_change"] == 0.15 and block["clips"] == 8 and 0 <= block["stretched"] <= 8 and 0 <= block["kept"] <= 8
    assert "transpose_augment" not in summary
    assert all(np.isfinite(brain.last_stats[k]) for k in ("loss", "time_loss", "key_loss", "upper_loss", "lower_loss", "WER", "WER_upper", "WER_lower")), brain.last_stats
    assert all(np.isfinite(v) for v in brain.train_stats.values()), brain.train_stats
    assert brain.train_stats["tempo_clips"] == 8


def test_recipe_refuses_a_value_out_of_range_before_training(tmp_path, dev):
    import pretrain
    from piano_a2s_amd import hip
    n0 = hip.tempo_launches()
    with pytest.raises(ValueError, match="tempo_augment"):
        _run(pretrain, tmp_path, "refused", ["--tempo_augment=0.4"])
    assert not os.path.exists(os.path.join(str(tmp_path), "refused", "1234", "pretrain.epr", "results")), "refused before the first epoch"
    assert hip.tempo_launches() == n0


def test_finetune_takes_both_flags(tmp_path, dev):
    import finetune
    from piano_a2s_amd import hip
    n0, a0 = hip.tempo_launches(), hip.augment_launches()
    brain, summary = _run(finetune, tmp_path, "fine", ["--transpose_augment=2", "--detune_bins=0.5", "--tempo_augment=0.25"])
    assert hip.tempo_launches() == n0 + 2 * 4 and hip.augment_launches() == a0 + 2 * 4
    assert summary["tempo_augment"]["clips"] == 8 and summary["tempo_augment"]["max_change"] == 0.25
    assert summary["transpose_augment"]["clips"] == 8 and summary["transpose_augment"]["max_semitones"] == 2
    assert brain.finetune and np.isfinite(brain.last_stats["WER"])
