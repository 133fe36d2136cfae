"""bench.py on the GPU: a plain run prints the headline line alone and spends little time outside its steps; `--full` adds the
legs beside it."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
LEGS = {"clock", "phases_ms", "roofline", "cpu_baseline", "parity", "native_abi", "throughput_mode", "throughput_sweep", "stress_mode"}


def _bench_line(*args, timeout):
    """(the one JSON line, wall seconds from start to exit) of `bench.py --gpus 1 <args>` in a fresh process"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), wall


TINY = ("--tiny", "--steps", "1", "--warmup", "1")


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_full_adds_the_legs():
    plain, _ = _bench_line(*TINY, timeout=300)
    assert CONTRACT <= set(plain) and plain["value"] > 0 and plain["steps"] == 1
    assert not LEGS & set(plain), sorted(LEGS & set(plain))
    full, _ = _bench_line(*TINY, "--full", timeout=600)
    assert CONTRACT <= set(full) and full["value"] > 0
    # (the tiny config has no native-ABI, batch-8 or 768x768 leg: those run on the SD1.5-width config only)
    assert {"clock", "phases_ms", "roofline", "cpu_baseline", "parity"} <= set(full), sorted(full)
    assert full["parity"]["ok"], full["parity"]
    assert full["roofline"]["launches_per_step"] > 0


@pytest.mark.gpu
def test_plain_run_spends_little_outside_its_steps():
    """The benchmarked configuration, plain: the whole run (imports, weights, inputs, the graph-capturing warm-up calls, exit)
    less (steps + warmup) x ms_per_step stays under 30 s.  About 3 s on an MI355X: no kernel is compiled or tuned at run time."""
    steps, warmup = 2, 1
    line, wall = _bench_line("--steps", str(steps), "--warmup", str(warmup), timeout=300)
    outside = wall - (steps + warmup) * line["ms_per_step"] * 1e-3
    assert line["value"] > 0 and not LEGS & set(line), sorted(line)
    assert outside < 30.0, (wall, line["ms_per_step"], outside)
