"""The whole fused training step with the encoder GRU's weight / bias gradients and the attention key products on the tall-K kernel
(csrc/a2s_linear.hip, a2s_tallk_wgrad) against the same step on the generic split-K GEMM and the column-sum passes
(a2s_debug_set("tallk_wgrad", 0)): loss terms, gradient norm, updated parameters, at the model and batch -- and with the bars -- of
tests/test_gpu_pair_staves.py; the library-side launch counter proves which path ran."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("B,tf,groups", [(80, 1.0, False), (128, 0.7, True)])
def test_step_with_tallk_weight_gradients_equals_generic(dev, B, tf, groups):
    import models
    from piano_a2s_amd import hip, spec, synthetic, train
    L = hip.lib()
    if groups:
        cfg = spec.default_cfg(freq_bins=48, max_length=(40, 24))
        batch = synthetic.make_batch(B, cfg, 63, frames=61, upper_range=(3, 12), lower_range=(2, 8), full_tail=0.0, full_rows=((3, 1, "up"), (8, 3, "lo")))
    else:
        cfg = spec.default_cfg(freq_bins=48, max_length=(24, 14))
        batch = synthetic.make_batch(B, cfg, 63, frames=61, upper_range=(4, 22), lower_range=(3, 12), full_tail=0.05)
    dbatch = [t.to(dev) if torch.is_tensor(t) else t for t in batch]
    torch.manual_seed(11)
    init = models.ScoreTranscription(**cfg).state_dict()
    prev = L.a2s_debug_get(b"tallk_wgrad")
    res = []
    try:
        for on in (0, 1):
            hip.check(L.a2s_debug_set(b"tallk_wgrad", on), "debug_set")
            m = models.ScoreTranscription(**cfg)
            m.load_state_dict(init)
            m = m.to(dev).train()
            step = train.TrainStep(m, dropout=False, **(dict(group_plan={"step_cost": 4.0, "min_gain": 0.0}) if groups else dict(clip_groups=False)))
            n0 = L.a2s_debug_get(b"tallk_wgrad_launches")
            losses = step(dbatch, tf, rng=random.Random(7))
            torch.cuda.synchronize()
            res.append((losses[:, 0].double().cpu(), step.opt.ctl.double().cpu(), step.flat.double().cpu(), L.a2s_debug_get(b"tallk_wgrad_launches") - n0))
            del step, m
    finally:
        hip.check(L.a2s_debug_set(b"tallk_wgrad", prev), "debug_set")
    (l0, c0, p0, n_off), (l1, c1, p1, n_on) = res
    # two layers x two directions x (weight_ih, weight_hh) + the three attention modules' key products (Backward.dK: the segment decoder and the two staves')
    assert n_off == 0 and n_on == 11, f"tall-K launches: {n_off} with the switch off, {n_on} with it on (11 expected)"
    assert torch.isfinite(l1).all() and float(c1[2]) == 1.0
    assert torch.allclose(l0, l1, rtol=2e-6, atol=0), (l0, l1)
    print(f"clip norm {float(c0[0]):.8g} / {float(c1[0]):.8g}; parameters differ by {float((p0 - p1).abs().max()) / float(p0.abs().max()):.3e} of their maximum")
    assert abs(float(c0[0]) - float(c1[0])) <= 2e-5 * float(c0[0]), (c0, c1)
    assert float((p0 - p1).abs().max()) <= 5e-6 * float(p0.abs().max())
