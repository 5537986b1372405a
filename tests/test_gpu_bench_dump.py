"""bench.py --dump-outputs on the MI355X: the timed path's last step written out, --steps timed steps taken."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_dumps_its_last_timed_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8",
                        "--no-cpu-baseline", "--no-secondary", "--no-inference", "--no-straggler-sim", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["steps"] == 3 and len(out["config"]["step_ms"]) == 3 and len(out["config"]["hipMalloc_segments_per_step"]) == 3
    d = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert sum(a.nbytes for a in d.values()) <= 64 * 2 ** 20 and all(a.dtype in (np.float32, np.float64) for a in d.values())
    for k in ("loss_terms", "loss_total", "clip_adadelta_ctl", "upper_logp_rows", "lower_logp_rows", "params_sample", "param_norms"):
        assert np.isfinite(d[k]).all(), k
    assert abs(float(d["loss_total"][0]) - out["config"]["final_loss"]) <= 1e-4          # (the JSON line rounds to 4 decimals)
    assert abs(float(d["loss_terms"].sum()) - float(d["loss_total"][0])) <= 1e-5 * abs(float(d["loss_total"][0]))
    assert d["clip_adadelta_ctl"][2] == 1.0, "the last timed step's update was skipped"
    assert d["time_sig_logp"].shape == (8, 5, 7) and d["key_logp"].shape == (8, 5, 14)
    assert d["upper_logp_rows"].shape[1] == d["lower_logp_rows"].shape[1] == 173
    assert np.allclose(np.exp(d["upper_logp_rows"]).sum(-1), 1.0, atol=1e-4)
