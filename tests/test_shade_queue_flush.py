"""The mid-loop queue flush of the three vertex kernels (kern_shade_common.h: VertexQueues::flush with reserve 256), at test size.

A block's LDS queue flushes before its loop ends only when fewer than 256 slots are left, i.e. after several rounds of one block; blocks_for gives every block
a single round until a launch exceeds CUs x blocks-per-CU x 256 vertices, so nothing smaller than a 1080p frame gets there. PT_TEST_MAX_BLOCKS=1 (render_loop.hip,
read per render call) caps the persistent grids at one block: a 64 x 48 render then makes tens of rounds per launch. A persistent kernel's result may not depend on
its grid, so each render must equal the oracle's like any other -- film at the suite's rtol, every counter -- and must have run the flush:
  * items / launches >= 4096 for the kernel under test (16 rounds of the one block), and
  * shadow rays traced >= 0.2 x the vertices shaded: with one vertex in five pushing a shadow ray, the shadow queue (capacity at most 1024) passes 768 entries
    before the last round of an average launch, so the run cannot be green without a mid-loop flush.
Both are conditions on the scene and its spp, not figures of the code under test. "Vertices shaded" = the items of every shade launch kind but shade_miss, plus
the subsurface exit points (bssrdf, bssrdf_stage_b): everything that can push a shadow ray.
The spp below were chosen on the parent commit's kernels with the hook alone (the smallest power of two that meets the first condition; figures beside each case); the
oracle's counters give the shadow share beforehand (path integrator: shadow_tests 26 016 and 24 100 at 16 spp against at most intersect_tests 100 758 and 151 945 vertices;
volpath counts its shadow rays as intersect tests, so that share is the device's own count). Each render runs in a child process of its own with the variable
set: the library reads it per call, the test process must not inherit it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT, trace_env
from parity import ORACLE_THREADS, assert_same_render

pytestmark = pytest.mark.gpu

_CHILD = r"""
import json, sys, numpy as np
sys.path.insert(0, {root!r})
from _pkg import import_pkg
pkg = import_pkg()
try:
    import torch  # noqa: F401 -- its bundled HIP runtime before the library's (conftest.gpu)
except ImportError:
    pass
lib = pkg.load_library(); lib.init(0)
lib.set_trace_exact({exact!r})
sd, rp = ({scene}).world_end()
rp.profile = 2
g = pkg.Scene(lib, sd)
film = g.render(rp)
np.savez({out!r}, film=film, counters=json.dumps(g.counters()), stats=json.dumps(g.kernel_stats()))
"""


# case -> (scene builder, an expression over `pkg` that parent and child evaluate alike; launch kind under test). On the parent's kernels under the cap:
CASES = {
    # 29 802 matte vertices in 6 launches (4 967 a launch), shadow share 0.62; QCAP 1024, 512 (plastic) and 256 (uber) in one scene
    "surface": ("pkg.scenes.material_zoo(n=16, xres=64, yres=48, spp=16)", "shade_matte"),
    # at 16 spp 17 841 exit points in 9 launches (1 982 a launch: too few), shadow share 0.38; 64 spp: four times the vertices
    "subsurface": ("pkg.scenes.subsurface_c5(n=16, xres=64, yres=48, spp=64)", "bssrdf"),
    # volpath is this scene's integrator. 16 spp: 784 medium vertices a launch (39 launches: the shells' chains); 128 spp: 245 134 in 53 launches (4 625), shadow share 0.39;
    # stage B: the self queue flushes too
    "medium": ("pkg.scenes.shell_media(xres=64, yres=48, spp=128)", "shade_medium"),
}

_ORACLE = {}   # case -> (film, counters): rendered once, shared by the two walks


def _oracle(pkg, oracle, case):
    if case not in _ORACLE:
        sd, rp = eval(CASES[case][0], {"pkg": pkg}).world_end()
        orc = oracle.scene(sd)
        _ORACLE[case] = (orc.render(rp, nthreads=ORACLE_THREADS), orc.counters())
    return _ORACLE[case]


@pytest.mark.parametrize("case", sorted(CASES))
def test_one_block_flushes_mid_loop_and_matches_the_oracle(pkg, gpu, oracle, tmp_path, trace_mode, case):
    out = str(tmp_path / "out.npz")
    code = _CHILD.format(root=ROOT, exact=trace_mode == "exact", scene=CASES[case][0], out=out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(trace_env(), PT_TEST_MAX_BLOCKS="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "PT_TEST_MAX_BLOCKS" not in os.environ
    got = np.load(out)
    stats = {s["name"]: s for s in json.loads(str(got["stats"]))}
    kind = CASES[case][1]
    shaded = sum(s["items"] for n, s in stats.items() if (n.startswith("shade_") and n != "shade_miss") or n.startswith("bssrdf"))
    shadow = (stats.get("trace:shadow") or stats["shadow"])["items"]
    per_launch = stats[kind]["items"] / stats[kind]["launches"]
    print("%s: %s items %d launches %d (%.0f a launch); vertices shaded %d, shadow rays %d (%.3f)" %
          (case, kind, stats[kind]["items"], stats[kind]["launches"], per_launch, shaded, shadow, shadow / shaded))
    assert per_launch >= 4096, (kind, stats[kind])
    assert shadow >= 0.2 * shaded, (shadow, shaded)
    ref, want = _oracle(pkg, oracle, case)
    assert_same_render(got["film"], ref, json.loads(str(got["counters"])), want)
