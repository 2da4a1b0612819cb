"""GPU: what a plain `bench.py` run and a `--full` run put into the result line.  A plain run carries the headline figure and
nothing that needs a pass of its own; --full adds the per-kernel attribution / roofline and the CPU baseline (the legs that
--headline-only leaves out are timed by the --full benchmark run itself, not here).  Smallest configuration (c1)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config", "chain_error")
FULL_ONLY = ("roofline", "roofline_next", "step_traffic", "kernel_families_ms_per_step", "cpu_baseline", "speedup_vs_cpu_baseline")
LEGS = ("eager_ms_per_step", "train_mode_dropout", "parity_modes", "train_step_with_optimizer", "t5_body")


def _run(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK") and not k.startswith("PQ3D_BENCH_")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--config", "c1", *extra]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(env, OMP_NUM_THREADS="4"), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def _check_headline(r):
    assert all(k in r for k in HEADLINE), sorted(r)
    assert r["unit"] == "scenes/s" and r["higher_is_better"] is True and r["dtype"] == "bf16" and r["chain_error"] is False
    assert r["steps"] == 4 and r["warmup"] == 2 and r["repeats"] == 1
    assert r["value"] > 0 and abs(r["value"] - r["config"]["global_batch"] / (r["ms_per_step"] * 1e-3)) < 1e-6 * r["value"]


def test_plain_run_is_the_headline_alone():
    r = _run()
    _check_headline(r)
    assert not [k for k in FULL_ONLY + LEGS if k in r]


def test_full_run_adds_the_attribution_and_the_cpu_baseline():
    r = _run("--full", "--headline-only", "--no-live-trace", "--profile-steps", "1", "--cpu-steps", "4")
    _check_headline(r)
    assert all(k in r for k in FULL_ONLY), sorted(r)
    assert not [k for k in LEGS if k in r]                     # --headline-only
    assert r["kernel_families_ms_per_step"] and r["roofline"]["kernel"] and r["roofline"]["trace"] == "disabled"
    assert r["cpu_baseline"]["value"] > 0 and r["speedup_vs_cpu_baseline"] > 0
