"""The oracle's orc_intersect hook and the scenes of tests/interaction_zoo.py, on the CPU alone (the device side: tests/test_interaction_probe.py).

  * orc_intersect's (prim, t, b) == orc_trace_closest on the same rays, bit for bit, counters included; a miss leaves its words zero.
  * on a one-triangle scene its p, p_error and n == orc_tri_intersect.
  * the conditions under which the device comparison compares something (hit share of the random rays, every primitive and instance hit by both query sets,
    share of clear structured quadric rays) hold on the oracle's answers.
  * the float64 checks hold on the oracle's own output, and the worst values they show stay within the tolerances interaction_zoo.py derives from them
    (measured worst x 4): the printed line is where those constants come from."""
import ctypes as C

import numpy as np
import pytest
from interaction_zoo import SCENES, F, case, check_against_float64, check_conditions, field
from oracle.oracle_binding import INTERSECT_FIELDS, INTERSECT_WORDS


@pytest.mark.parametrize("name", list(SCENES))
def test_orc_intersect_equals_trace_closest(pkg, oracle, name):
    c = case(pkg, oracle, name)
    for part, q in c["sets"].items():
        r = c["ref"][part]
        w = r["words"]; prim, t, b = r["closest"]
        assert w.shape == (len(q["o"]), INTERSECT_WORDS)
        hit = field(w, INTERSECT_FIELDS, "hit")
        assert set(np.unique(hit)) <= {0, 1}
        assert np.array_equal(np.where(hit != 0, field(w, INTERSECT_FIELDS, "prim"), 0xFFFFFFFF), prim)
        assert np.array_equal(field(w, INTERSECT_FIELDS, "t").view(np.uint32), t.view(np.uint32))
        assert np.array_equal(field(w, INTERSECT_FIELDS, "b").view(np.uint32), b.view(np.uint32))
        assert not w[hit == 0].any()                       # a miss leaves the ray's words zero
        assert r["counters"] == r["closest_counters"] and r["counters"]["intersect_tests"] == len(q["o"])


def test_orc_intersect_equals_orc_tri_intersect_on_one_triangle(pkg, oracle):
    b = pkg.host.SceneBuilder()
    b.film.update(xres=8, yres=8); b.spp = 1
    b.world_begin()
    b.trianglemesh(np.array([[-1.0, -0.5, 0.25], [1.5, -1.0, 0.0], [0.25, 1.25, -0.5]], F), np.array([0, 1, 2], np.uint32))
    sd, _ = b.world_end()
    s = oracle.scene(sd)
    rng = np.random.default_rng(3)
    n = 512
    bb = rng.dirichlet((1.0, 1.0, 1.0), n) * 1.2 - 0.1   # aim points on and a little beside the triangle
    p = bb @ sd.P.astype(np.float64)
    o = (p + rng.normal(size=(n, 3)) * 2.0).astype(F); d = (p - o.astype(np.float64)).astype(F) * F(0.5)
    tmax = np.full(n, np.inf, F)
    w = s.intersect(o, d, tmax)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    hits = 0
    for i in range(n):
        t = np.zeros(1, F); bary = np.zeros(3, F); pp = np.zeros(3, F); pe = np.zeros(3, F); nn = np.zeros(3, F)
        got = oracle.lib.orc_tri_intersect(s.h, 0, fp(o[i]), fp(d[i]), float("inf"), fp(t), fp(bary), fp(pp), fp(pe), fp(nn))
        assert got == int(w[i, 0])
        if not got: continue
        hits += 1
        row = w[i:i + 1]
        for name, want in (("t", t), ("b", bary), ("p", pp), ("p_error", pe), ("n", nn)):
            assert np.array_equal(np.atleast_1d(field(row, INTERSECT_FIELDS, name)[0]).view(np.uint32), want.view(np.uint32)), (i, name)
    s.close()
    assert 0.5 * n < hits < n


@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_meet_their_conditions_and_float64_checks_on_the_oracle(pkg, oracle, name):
    c = case(pkg, oracle, name)
    fig = check_conditions(name, c)
    print(f"\n{name}: {len(c['targets'])} (primitive, instance) pairs; random rays {fig['random'][0]}, hit {fig['random'][1]}; structured rays {fig['structured'][0]}, "
          f"hit {fig['structured'][1]}; clear share of the structured quadric rays {fig.get('clear_share', float('nan')):.3f}")
    for part, q in c["sets"].items():
        r = c["ref"][part]
        f = check_against_float64(f"{name} {part} (oracle)", c["targets"], q, r["truth"], r["words"], INTERSECT_FIELDS, hit_any=r["any"]["inf"][1])
        print(f"{name} {part}: {f['clear']} clear rays, {f['checked']} clear hits checked against float64: worst box excess {f['box']:.3e} sizes, "
              f"worst |cross(normalize(dpdu x dpdv), n)| {f['parallel']:.3e}, worst ||n| - 1| {f['unit']:.3e}, rigid-sphere normals {f['sphere_normals']}")
