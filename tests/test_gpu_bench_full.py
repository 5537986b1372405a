"""bench.py on the MI355X: a plain run prints the headline of its timed steps and nothing that takes runs of its own; --full adds those."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "dtype_note",
            "data", "config", "roofline_step", "build"}


def _bench(*flags):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8", *flags],
                       capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only():
    out = _bench()
    assert set(out) == HEADLINE, sorted(set(out) ^ HEADLINE)
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0 and len(out["config"]["step_ms"]) == 2
    assert out["roofline_step"]["ms_per_step"] == out["ms_per_step"]


@pytest.mark.gpu
def test_full_adds_the_measurements_of_their_own():
    """(the blocks at fixed sizes -- inference, VQT, straggler simulation, CPU baseline -- left out by their switches)"""
    out = _bench("--full", "--no-cpu-baseline", "--no-inference", "--no-straggler-sim")
    extra = {"tail_off", "roofline", "roofline_phases", "roofline_linear", "roofline_attention", "loss_parity"}
    assert set(out) == HEADLINE | extra, sorted(set(out) ^ (HEADLINE | extra))
    assert out["steps"] == 2 and out["tail_off"]["value"] > 0 and out["loss_parity"]["ok"]
