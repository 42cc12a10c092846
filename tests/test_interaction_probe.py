"""The step from a hit record to a SurfaceInteraction -- fill_hit_pkt<SPH> / fill_hit<SPH> (kern_common.h), tri_fill_from / tri_fill_interaction (dev_scene.h),
sphere_fill_interaction (dev_sphere.h) and the instance branch that carries an object-space interaction to world space -- against the CPU oracle, CALL BY CALL, and
the quadrics of sphere_hit traced with rays aimed at their edges. Renders reach this stage with generic hits only: never a vertex, a zero interpolated normal,
S parallel to N, a UV determinant below 1e-8, a pole, a disk's centre, a mirrored or non-uniformly scaled instance.

tests/device_probe/interaction_probe.hip is test code beside bsdf_probe.hip / light_probe.hip (tests/probe_build.py builds them all once per session): it traces the
rays with the library's own pth::launch_trace, receives the two quads of the hit record as k_trace writes them for the render, and calls the UNMODIFIED fill functions once
per ray. Scenes, queries, the float64 model and the conditions under which a comparison compares something: tests/interaction_zoo.py; what holds of the oracle alone:
tests/test_interaction_zoo.py.

  a. every field of probe_interaction form 0 (fill_hit_pkt) == orc_intersect, bit for bit as test_device_probe.assert_same_bits has it (every NaN one pattern; signed zeros
     and infinities count), the hit flag, prim, inst, t and b included; form 1 (fill_hit) == form 0; the packet flags' material bits == prim_material.
  b. the same rays through pt_trace_closest and through pt_trace_any with t_max just short of, just past the oracle's t and infinite: assert_same_hits, counters included.
  c. the float64 checks of interaction_zoo.check_against_float64 on the DEVICE's words: they do not trust the oracle.
  d. interaction_zoo.check_conditions: hit share, every primitive and instance hit, clear share.
  e. refusals leave the output untouched.

FIELDS_LEFT_OUT names what (a) does not compare for a shape kind, each with the line of the reference that shows nothing reads it: nothing is left out."""
import ctypes as C
import os

import numpy as np
import pytest
from interaction_zoo import SCENES, F, NONE, case, check_against_float64, check_conditions, field
from parity import assert_same_hits
from probe_build import INTERACTION_WORDS, probe_library

pytestmark = pytest.mark.gpu

if os.environ.get("PT_LIB_PATH"):   # a kernel-variant library: its pt_scene layout may differ from the one the probe is compiled against
    pytest.skip("PT_LIB_PATH names a variant library; the probe reads pt_scene of the tree's own headers", allow_module_level=True)

# (shape kind, field) -> the reference line that shows nothing reads the field there. Empty: both sides write every field for every shape kind.
FIELDS_LEFT_OUT = {}
FLAGS_WORD = 44               # the packet flags (dev_scene.h: material index in bits 16-31, 0xffff = read prim_material)
MAT_SHIFT, MAT_NONE = 16, 0xFFFF


@pytest.fixture(scope="module")
def probe(pkg, gpu):
    return probe_library(pkg)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype != F: return a
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000   # every NaN is one pattern (x86 SSE sets the sign bit of an invalid operation's NaN, the GPU does not)
    return b


def assert_same_fields(dev, ref, fields, q, names, what):
    """Every field of `fields`, row by row, bit for bit; the message names the field, the ray and what it was aimed at."""
    for name in fields:
        if name in FIELDS_LEFT_OUT: continue
        d, r = _bits(field(dev, fields, name)), _bits(field(ref, fields, name))
        if np.array_equal(d, r): continue
        rows = np.unique(np.argwhere(d != r)[:, 0]); i = int(rows[0])
        aimed = sorted({names[k] for k in np.asarray(q["target"])[rows]})
        raise AssertionError(f"{what}: field {name}: {len(rows)} of {len(d)} rays differ, aimed at {aimed[:8]}; first at ray {i} ({names[q['target'][i]]}: {q['tag'][i]}): "
                             f"{np.atleast_1d(field(dev, fields, name)[i])} != {np.atleast_1d(field(ref, fields, name)[i])}")


def device_interactions(probe, scene, form, q, n=None):
    n = len(q["tmax"]) if n is None else n
    out = np.zeros((n, INTERACTION_WORDS), np.uint32)
    o, d, tmax = (np.ascontiguousarray(q[k][:n]) for k in ("o", "d", "tmax"))
    st = probe.probe_interaction(scene.h, form, n, _fp(o), _fp(d), _fp(tmax), out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert st == 0, f"probe_interaction form {form}: status {st}"
    return out


def check_material_bits(sd, words, fields, what):
    hit = field(words, fields, "hit") != 0
    mat = words[hit, FLAGS_WORD] >> MAT_SHIFT
    want = sd.prim_material[field(words, fields, "prim")[hit]]
    want = np.where((want == NONE) | (want >= MAT_NONE), MAT_NONE, want)
    assert np.array_equal(mat, want), f"{what}: the packet flags' material bits differ from prim_material for {int((mat != want).sum())} hits"
    assert not words[~hit].any(), f"{what}: a miss left words behind"


@pytest.mark.parametrize("name", list(SCENES))
def test_interactions_match_the_oracle_field_by_field(pkg, gpu, oracle, probe, name):
    c = case(pkg, oracle, name)
    fig = check_conditions(name, c)
    fields, tg, names = c["fields"], c["targets"], c["names"]
    label = {k: (names[t["prim"]] if t["inst"] == NONE else f"{names[t['inst']]} prim {t['prim']}") for k, t in enumerate(tg)}
    scene = pkg.Scene(gpu, c["sd"])
    try:
        for part, q in c["sets"].items():
            r = c["ref"][part]
            got = scene.trace_closest(q["o"], q["d"], q["tmax"])   # (b), and the scene's workspace
            assert_same_hits(got, r["closest"], scene.counters(), r["closest_counters"])
            for key, (tm, want, counters) in r["any"].items():
                assert_same_hits(scene.trace_any(q["o"], q["d"], tm), want, scene.counters(), counters)
            dev = device_interactions(probe, scene, 0, q)
            print(f"\n{name} {part}: {len(dev)} rays compared, {int((r['words'][:, 0] != 0).sum())} hit ({fig[part][1]} by the conditions' count)")
            assert_same_fields(dev, r["words"], fields, q, label, f"{name} {part}: fill_hit_pkt vs orc_intersect")
            check_material_bits(c["sd"], dev, fields, f"{name} {part}")
            dev1 = device_interactions(probe, scene, 1, q)
            assert_same_fields(dev1, dev, fields, q, label, f"{name} {part}: fill_hit vs fill_hit_pkt")
            assert np.array_equal(dev1[:, FLAGS_WORD], dev[:, FLAGS_WORD])
            hit_any = scene.trace_any(q["o"], q["d"], np.full(len(q["tmax"]), np.inf, F))
            f = check_against_float64(f"{name} {part} (device)", tg, q, r["truth"], dev, fields, hit_any=hit_any)
            print(f"{name} {part}: {f['checked']} clear hits of the device checked against float64: box {f['box']:.3e}, parallel {f['parallel']:.3e}, unit {f['unit']:.3e}")
    finally:
        scene.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_interaction_probe_with_a_ragged_last_block(pkg, gpu, oracle, probe, n):
    c = case(pkg, oracle, "tri_zoo")
    every = 15   # every fifteenth random ray: all thirty triangles, hits and misses
    q = {k: v[::every] for k, v in c["sets"]["random"].items()}; ref = c["ref"]["random"]["words"][::every]
    assert len(ref) >= 257
    scene = pkg.Scene(gpu, c["sd"])
    try:
        scene.trace_closest(q["o"][:n], q["d"][:n], q["tmax"][:n])   # the workspace
        label = {k: c["names"][t["prim"]] for k, t in enumerate(c["targets"])}
        for form in (0, 1):
            dev = device_interactions(probe, scene, form, q, n)
            print(f"\ntri_zoo form {form}: {n} rays compared, {int((ref[:n, 0] != 0).sum())} hit")
            assert_same_fields(dev, ref[:n], c["fields"], q, label, f"tri_zoo n={n} form {form}")
    finally:
        scene.close()


def test_interaction_probe_refuses_without_touching_the_output(pkg, gpu, oracle, probe):
    c = case(pkg, oracle, "quadric_zoo")
    q = c["sets"]["random"]
    o, d, tmax = (np.ascontiguousarray(q[k][:4]) for k in ("o", "d", "tmax"))
    out = np.full((4, INTERACTION_WORDS), 0xA5A5A5A5, np.uint32); op = out.ctypes.data_as(C.POINTER(C.c_uint32))
    scene = pkg.Scene(gpu, c["sd"])
    try:
        assert probe.probe_interaction(scene.h, 0, 4, _fp(o), _fp(d), _fp(tmax), op) == 4      # a scene without a workspace
        scene.trace_closest(o, d, tmax)
        assert probe.probe_interaction(None, 0, 4, _fp(o), _fp(d), _fp(tmax), op) == 1         # null pointers
        assert probe.probe_interaction(scene.h, 0, 4, None, _fp(d), _fp(tmax), op) == 1
        assert probe.probe_interaction(scene.h, 0, 4, _fp(o), None, _fp(tmax), op) == 1
        assert probe.probe_interaction(scene.h, 0, 4, _fp(o), _fp(d), None, op) == 1
        assert probe.probe_interaction(scene.h, 0, 4, _fp(o), _fp(d), _fp(tmax), None) == 1
        assert probe.probe_interaction(scene.h, 0, 0, _fp(o), _fp(d), _fp(tmax), op) == 1      # no ray
        assert probe.probe_interaction(scene.h, 0, (1 << 20) + 1, _fp(o), _fp(d), _fp(tmax), op) == 1
        for form in (2, -1, 7):
            assert probe.probe_interaction(scene.h, form, 4, _fp(o), _fp(d), _fp(tmax), op) == 2   # an unknown form
        assert (out == 0xA5A5A5A5).all()   # nothing ran
        assert probe.probe_interaction(scene.h, 0, 4, _fp(o), _fp(d), _fp(tmax), op) == 0
        assert not (out == 0xA5A5A5A5).all()
    finally:
        scene.close()
