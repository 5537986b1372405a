"""The note decoders' weight gradients late (in Backward.finish, on the weight-gradient stream: the default) against inline (behind each call's reverse
loop on the staff's stream), nothing else toggled: the two placements of dec_bwd_plan walk the same products over the same rows on other streams.  The
case is the small one of test_gpu_step_ordering.test_group_buffers_hold_decoder_gradients_only: it splits into clip groups and some of its calls gather
sparse live (step, row) pairs.  Bounds: those tests/test_gpu_round5_paths.py applies to the same comparison (same products, other streams)."""
import random
import threading
from unittest import mock

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def test_late_weight_gradients_equal_the_inline_ones(dev):
    import models
    from piano_a2s_amd import engine_bwd, spec, synthetic, train
    from piano_a2s_amd.dec_bwd_plan import plan_note_decoder_bwd
    cfg = spec.default_cfg(max_length=(40, 24))
    batch = synthetic.make_batch(12, cfg, 78, frames=151, upper_range=(3, 12), lower_range=(2, 8), full_tail=0.0, full_rows=((3, 1, "up"), (8, 3, "lo")))
    dbatch = [t.to(dev) if torch.is_tensor(t) else t for t in batch]
    torch.manual_seed(6)
    init = models.ScoreTranscription(**cfg).state_dict()
    decoder_group, lock, res = engine_bwd.Backward.decoder_group, threading.Lock(), []

    for late in (False, True):
        plans = []

        def spy(self, gidx, gs, *grads):          # the plan of every decode call, from what the forward saved for the group
            for seg in gs["segments"]:
                for k in ("up", "lo"):
                    sv = seg["staff"][k][2]
                    act = sv.get("active") or {}
                    live = act.get("live_idx")
                    with lock:
                        plans.append(plan_note_decoder_bwd(sv["steps"], sv.get("groups", 1) * (gs["range"][1] - gs["range"][0]), act.get("live_steps"),
                                                           live.numel() if live is not None else None, self.late_wgrads))
            return decoder_group(self, gidx, gs, *grads)

        m = models.ScoreTranscription(**cfg)
        m.load_state_dict(init)
        m = m.to(dev).train()
        step = train.TrainStep(m, dropout=True, group_plan={"step_cost": 4.0})
        step.late_wgrads = late
        torch.manual_seed(1234)                   # the dropout masks
        with mock.patch.object(engine_bwd.Backward, "decoder_group", spy):
            losses = step(dbatch, 0.7, rng=random.Random(4))
        torch.cuda.synchronize()
        res.append((losses[:, 0].double().cpu(), step.flat.double().cpu(), float(step.opt.ctl[2]), len(step._last[2]), plans))
        del step, m
    (l0, p0, a0, g0, plans0), (l1, p1, a1, g1, plans1) = res
    assert g0 >= 2 and g1 >= 2, "the case must split into clip groups"
    assert {p.placement for p in plans0} == {"inline"} and {p.placement for p in plans1} == {"late"}
    for plans in (plans0, plans1):
        assert any(p.gather and not p.empty for p in plans), "no call of the case gathers its live pairs: the gather is not exercised"
    assert sorted(p[:3] for p in plans0) == sorted(p[:3] for p in plans1)
    assert torch.isfinite(l1).all() and a0 == 1.0 and a1 == 1.0
    assert torch.allclose(l0, l1, rtol=2e-6, atol=0), (l0, l1)
    assert float((p0 - p1).abs().max()) <= 5e-6 * float(p0.abs().max()), float((p0 - p1).abs().max())
