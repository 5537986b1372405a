"""bench.py --dump-outputs: the arrays dump_outputs writes for the last timed step (CPU stand-in for the step: the same attributes a
TrainStep has after a call) -- names, dtypes, the fixed row / parameter samples, run-to-run identity and the 64 MB budget."""
import importlib.util
import os
import types

import numpy as np
import torch

from piano_a2s_amd import spec, synthetic
from piano_a2s_amd.spec import PAD, VOCAB_SIZE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    s = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(s)
    s.loader.exec_module(m)
    return m


def _fake_step(cfg, B, flat, seed):
    g = torch.Generator().manual_seed(seed)
    bars, (U, L) = cfg["max_bars"], cfg["max_length"]
    logp = lambda *shape: torch.log_softmax(torch.randn(*shape, generator=g), -1)
    outs = (logp(B, bars, cfg["num_time_sig"]), logp(B, bars, cfg["num_keys"]), logp(B, bars, U, VOCAB_SIZE), logp(B, bars, L, VOCAB_SIZE))
    return types.SimpleNamespace(last_outputs=outs, objective=types.SimpleNamespace(losses=torch.rand(4, 2, generator=g)),
                                 total=torch.rand(1, generator=g), opt=types.SimpleNamespace(ctl=torch.rand(3, generator=g)), flat=flat)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_holds_the_last_step_outputs(tmp_path):
    import models
    bench = _bench()
    cfg = spec.default_cfg(freq_bins=24, conv_feature_size=32, hidden_size=32, max_length=(12, 8))
    model = models.ScoreTranscription(**cfg)
    step = _fake_step(cfg, 3, model.flatten_(), 0)
    batch = synthetic.make_batch(3, cfg, 5, frames=41, upper_range=(3, 10), lower_range=(2, 7), full_tail=0.1)
    bench.dump_outputs(str(tmp_path / "a"), step, model, batch, staff_rows=20, param_samples=500)
    bench.dump_outputs(str(tmp_path / "b"), step, model, batch, staff_rows=20, param_samples=500)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(["loss_terms", "loss_total", "clip_adadelta_ctl", "time_sig_logp", "key_logp", "upper_logp_rows", "upper_logp_rows_index",
                                "lower_logp_rows", "lower_logp_rows_index", "param_norms", "batchnorm_buffers", "params_sample", "params_sample_index"])
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), f"{k}: the sample is not fixed"
    assert np.array_equal(a["loss_terms"], step.objective.losses[:, 0].numpy()) and np.array_equal(a["clip_adadelta_ctl"], step.opt.ctl.numpy())
    assert np.array_equal(a["time_sig_logp"], step.last_outputs[0].numpy()) and np.array_equal(a["key_logp"], step.last_outputs[1].numpy())
    for name, o, tgt in (("upper", step.last_outputs[2], batch[3]), ("lower", step.last_outputs[3], batch[5])):
        idx = a[f"{name}_logp_rows_index"].astype(np.int64)
        assert idx.shape == (20, 3) and len(np.unique(idx, axis=0)) == 20
        assert (tgt.numpy()[idx[:, 0], idx[:, 1], idx[:, 2]] != PAD).all(), "only rows with a target are defined"
        assert np.array_equal(a[f"{name}_logp_rows"], o.numpy()[idx[:, 0], idx[:, 1], idx[:, 2]])
    pidx = a["params_sample_index"].astype(np.int64)
    assert len(np.unique(pidx)) == 500 and np.array_equal(a["params_sample"], step.flat.numpy()[pidx])
    want = [float(p.detach().double().norm()) for p in model.parameters()]
    assert np.allclose(a["param_norms"], want, rtol=1e-12, atol=0)
    assert a["batchnorm_buffers"].size == sum(t.numel() for t in model.buffers())


def test_dump_fits_the_budget_at_full_size(tmp_path):
    """The default sample sizes against the full model's 16.36 M parameters and enough live staff rows to fill both samples."""
    import models
    bench = _bench()
    cfg = spec.default_cfg()
    model = models.ScoreTranscription(**spec.default_cfg(freq_bins=24, conv_feature_size=32, hidden_size=32, max_length=(12, 8)))
    B = 80
    step = _fake_step(cfg, B, torch.randn(16_358_684), 1)
    batch = synthetic.make_batch(B, cfg, 7, frames=8, full_tail=0.01)
    total = bench.dump_outputs(str(tmp_path), step, model, batch)
    files = _load(tmp_path)
    assert total == sum(a.nbytes for a in files.values()) <= bench.DUMP_MAX_BYTES
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= bench.DUMP_MAX_BYTES
    assert files["upper_logp_rows"].shape == files["lower_logp_rows"].shape == (16384, VOCAB_SIZE)
