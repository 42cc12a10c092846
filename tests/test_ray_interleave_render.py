"""Renders through the ray queue (kernels.h: kRayKindShift): the shade kernels append every ray of a vertex -- continuation, MIS, shadow -- to ONE queue, vertex by
vertex, and the mixed traversal launch takes each ray's kind from its entry. The order in which rays are traced changes nothing: every render equals the oracle's.

Per scene -- the material zoo (every k_shade form), a subsurface scene (k_bssrdf's pushes), and under volpath a grid medium (stage B re-pushes) and media in
material-less shells (the shadow / MIS chains' re-pushes), the latter two at the sizes tests/test_volpath.py renders them:
  * the render in this process against the oracle (parity.assert_render_matches_oracle: every counter, the film, the resolved image);
  * the same render in a child process with PT_TEST_MAX_BLOCKS=1, where the one block of every launch flushes the ray queue mid-loop, against the same oracle film;
  * its per-kind ray counts (trace:extend, trace:extend_mis, trace:shadow of kernel_stats()) and per-kind records fetched and triangle tests against those of a
    PT_TRACE_SPLIT=1 child, which scatters the ray queue into one queue per kind and traces them in three launches; that child's film and counters against the oracle too."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT, trace_env
from parity import ORACLE_THREADS, assert_render_matches_oracle, assert_same_render

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

CASES = {
    "material_zoo": "pkg.scenes.material_zoo(n=16, xres=96, yres=64, spp=8)",
    "subsurface": "pkg.scenes.subsurface_c5(n=16, xres=64, yres=48, spp=8)",
    "smoke_room": "pkg.scenes.smoke_room(xres=48, yres=36, sampler='halton')",
    "shell_media": "pkg.scenes.shell_media(xres=56, yres=40, spp=8, grid=False)",
}


def _child(tmp_path, name, case, trace_mode, **env):
    out = str(tmp_path / (name + ".npz"))
    code = _CHILD.format(root=ROOT, exact=trace_mode == "exact", scene=CASES[case], out=out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(trace_env(), **env), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    return got["film"], json.loads(str(got["counters"])), {s["name"]: s for s in json.loads(str(got["stats"]))}


@pytest.mark.parametrize("case", sorted(CASES))
def test_render_through_the_ray_queue_matches_the_oracle(pkg, gpu, oracle, tmp_path, trace_mode, case):
    assert not {"PT_TEST_MAX_BLOCKS", "PT_TRACE_SPLIT"} & set(os.environ)
    sd, rp = eval(CASES[case], {"pkg": pkg}).world_end()
    film, ref, gc, oc = assert_render_matches_oracle(pkg, gpu, oracle, sd, rp, nthreads=ORACLE_THREADS)
    assert film[..., :3].sum() > 0
    film1, c1, mixed = _child(tmp_path, "one_block", case, trace_mode, PT_TEST_MAX_BLOCKS="1")
    assert_same_render(film1, ref, c1, oc)
    film3, c3, split = _child(tmp_path, "split", case, trace_mode, PT_TRACE_SPLIT="1")
    assert_same_render(film3, ref, c3, oc)
    assert "trace" in mixed and mixed["trace"]["launches"] and "trace" not in split, (sorted(mixed), sorted(split))
    for kind in ("extend", "extend_mis", "shadow"):
        # (an iteration with continuation rays only is one `extend` launch in both modes; kernel_stats() then reports the kind's work under `extend`, with the
        #  items of those launches alone, and has no `trace:extend` row -- the kind's records and triangle tests are the totals of both kinds of launch either way)
        m, s = mixed.get("trace:" + kind) or mixed.get(kind), split.get(kind)
        assert (m is None) == (s is None), (kind, sorted(mixed), sorted(split))
        if m is None:
            continue
        print(case, kind, m["items"], s["items"], m["bvh_nodes"], s["bvh_nodes"], m["triangle_tests"], s["triangle_tests"])
        assert (m["bvh_nodes"], m["triangle_tests"]) == (s["bvh_nodes"], s["triangle_tests"]), (kind, m, s)
        if "trace:" + kind in mixed:
            assert m["items"] == s["items"], (kind, m, s)
    assert any("trace:" + kind in mixed for kind in ("extend", "extend_mis", "shadow"))
