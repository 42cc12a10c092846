"""bench.py --dump-outputs: the film the timed path computed in its last step, written so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from parity import assert_same_film

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_writes_the_film_whole_or_a_fixed_sample_within_the_cap(tmp_path):
    import bench
    film = np.random.default_rng(1).random((1080, 1920, 4), dtype=np.float32)     # the headline's film: 33 MB, written whole
    bench.dump_outputs(str(tmp_path / "a"), film)
    assert np.array_equal(np.load(tmp_path / "a" / "film.npy"), film)
    big = np.random.default_rng(2).random((2160, 3840, 4), dtype=np.float32)     # 133 MB: a sample of its pixels, the same one every time
    big[..., 0] = np.arange(2160 * 3840, dtype=np.float32).reshape(2160, 3840)   # channel 0 = the pixel's index (exact in f32 below 2^24)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), big)
        assert os.path.getsize(tmp_path / d / "film.npy") <= bench.DUMP_MAX_BYTES
    s = np.load(tmp_path / "b" / "film.npy")
    assert s.dtype == np.float32 and s.shape[1] == 4 and s.shape[0] > 4_000_000 and np.array_equal(s, np.load(tmp_path / "c" / "film.npy"))
    idx = s[:, 0].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and np.array_equal(s, big.reshape(-1, 4)[idx])   # whole pixels of the film, in pixel order


@pytest.mark.gpu
def test_dumped_film_is_the_render_of_the_timed_steps(pkg, gpu, tmp_path, trace_mode):
    from conftest import trace_env
    if trace_mode == "exact":
        pytest.skip("the dump does not depend on the walk: the production instance runs it")
    env = trace_env({k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--xres", "160", "--yres", "96", "--spp", "8", "--mesh-n", "48", "--steps", "3", "--warmup", "0",
           "--cpu-seconds", "0", "--other-configs", "off", "--projection", "off", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    line = json.loads([l for l in r.stdout.strip().split("\n") if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path / "out")) == ["film.npy"]
    film = np.load(tmp_path / "out" / "film.npy")
    sd, rp = pkg.scenes.ganesha_scale(n=48, xres=160, yres=96, spp=8).world_end()
    ref = pkg.Scene(gpu, sd).render(rp)
    assert film.dtype == np.float32 and film.shape == ref.shape == (96, 160, 4)
    assert_same_film(film, ref)
