"""bench.py's two kinds of run: a plain run does what its headline needs (set up, warm up, time the steps, dump, print the line); --full adds the side
measurements (CPU baseline, film read-back, scaling projection, the other BASELINE configs)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_side_measurements_belong_to_full_runs():
    import bench
    ap = bench.parser()
    plain = ap.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not plain.full and bench.side_measurements(plain, 1, False) == (0, False)
    assert bench.side_measurements(ap.parse_args(["--gpus", "1", "--full"]), 1, False) == (8, True)
    # "auto" stays off away from the default workload on one GPU, also under --full
    for argv, world, in_process in ((["--full", "--config", "C3"], 1, False), (["--full", "--spp", "64"], 1, False), (["--full"], 2, False), (["--full", "--gpus", "2"], 1, True)):
        assert bench.side_measurements(ap.parse_args(argv), world, in_process) == (0, False), argv
    # "on" / "off" decide either way
    assert bench.side_measurements(ap.parse_args(["--projection", "on", "--other-configs", "on"]), 1, False) == (8, True)
    assert bench.side_measurements(ap.parse_args(["--full", "--projection", "off", "--other-configs", "off"]), 1, False) == (0, False)
    assert bench.side_measurements(ap.parse_args(["--other-configs", "on"]), 2, False) == (0, False)   # launcher form: never


def _bench_line(argv, trace_env_fn):
    env = trace_env_fn({k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--xres", "160", "--yres", "96", "--spp", "8", "--mesh-n", "48", "--steps", "2", "--warmup", "1"] + argv
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return json.loads([l for l in r.stdout.strip().split("\n") if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_full_adds_the_side_measurements(trace_mode):
    from conftest import trace_env
    if trace_mode == "exact":
        pytest.skip("which measurements a run makes does not depend on the walk: the production instance runs it")
    plain = _bench_line([], trace_env)
    assert plain["metric"].startswith("Msamples/s") and plain["unit"] == "Msamples/s" and plain["higher_is_better"] is True and plain["dtype"] == "f32"
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["steps"] == 2 and plain["warmup"] == 1
    assert plain["cpu_baseline"] is None
    assert not {"film_readback_ms", "value_with_readback", "scaling_projection", "other_configs"} & set(plain)
    full = _bench_line(["--full", "--cpu-seconds", "1", "--projection", "on"], trace_env)
    assert full["cpu_baseline"]["value"] > 0 and full["film_readback_ms"] > 0 and full["value_with_readback"] > 0
    assert full["scaling_projection"]["world"] == 8 and full["scaling_projection"]["shard_ms"] > 0
    assert "other_configs" not in full    # "auto": the default workload's side measurement only
