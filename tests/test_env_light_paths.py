"""The infinite light's two sampling paths (csrc/dev_light.h), call by call and render by render against the oracle.

A constant environment (a 1 x 1 map, so a 2 x 2 importance image) is sampled from the scene's uniform block (dev_scene.h: EnvUniform): the light's transforms, the
texel and the whole Distribution2D arrive in scalar registers and the bisection of Distribution1D::sample_continuous runs over registers. Every larger map keeps the
bisection over memory; the transforms of the first infinite light come from the block in both. The register tables hold w, h <= 1, so the environments below are the
bound (1 x 1), bound + 1 on each axis (2 x 1, 1 x 2), 2 x 2, and 3 x 2 / 2 x 3 maps (resampled to 4 x 2 / 2 x 4 by the host, as MIPMap::new does). Each sits under
the rotated light transform of test_device_probe.env_light.

Call by call (the probe kernels and helpers of tests/test_device_probe.py, results as bit patterns): light_sample_li / light_pdf_li against orc_light_sample_li /
orc_light_pdf_li for that module's random and structured queries of an infinite light (the +-z poles of the light's frame, where sin(theta) == 0, are among them) plus
  * sample points u = (u_x, u_y) over every pair of: 0, the largest float below 1, every cdf entry of the marginal (u_y) and of every conditional row (u_x) and
    its two float neighbours -- the `cdf[middle] <= u` tie of the bisection. The cdf entries are computed here with the plan's formula (scene_plan.hip: dist1d);
  * directions for pdf_li on the seams of the importance image's texels (theta = pi j / 2h, phi = 2 pi i / 2w, and a step of 1e-6 to either side).
At least LIGHT_FLOOR of the random queries of every environment have a non-zero sampled pdf in the oracle (checked before anything is compared).
An all-zero importance ROW needs two neighbouring zero texel rows, so it exists on the memory path only ("2x4_zero_rows": pdf == 0 and `diff > 0` false); in a
2 x 2 importance image both rows blend the one texel, so a zero row there means a black environment, which cannot meet the floor and is left to the plan's CPU test.

Render by render (tests/parity.py: every counter and the film), 32 x 24 pixels, 4 spp, maxdepth 3, Sobol': (a) a constant environment, a triangle area light and a
point light over a floor and a small mesh -- triangle, delta and infinite lights meet in one wave and the delta bit comes from the record header; (b) the 2 x 2 map
with an area light; (c) the 3 x 2 map. Each also once with PT_TEST_MAX_BLOCKS=1 (a child process: the library reads it per render), so that a block runs several rounds."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT, trace_env
from parity import ORACLE_THREADS, assert_same_render
from test_device_probe import (F, LIGHT_FLOOR, U_TOP, _base, _floor, _unit, assert_same_bits, check_light_floor, device_light, light_queries, oracle_light,
                               oracle_pdf, probe, second_round_directions)  # noqa: F401 -- `probe` is the module fixture

pytestmark = pytest.mark.gpu


def _texels(w, h):
    """Unequal, positive texels (rows = v)."""
    i = np.arange(w * h * 3, dtype=np.float64).reshape(h, w, 3)
    return (0.2 + 0.37 * ((i * 7) % 11)).astype(F)


def _zero_rows():
    t = _texels(2, 4)
    t[1:3] = 0.0   # importance rows 3 and 4 (of 8) blend texel rows 1 and 2 only: all zero
    return t


ENVS = {"const": None, "2x1": _texels(2, 1), "1x2": _texels(1, 2), "2x2": _texels(2, 2), "3x2": _texels(3, 2), "2x3": _texels(2, 3), "2x4_zero_rows": _zero_rows()}


def _env(pkg, b, name):
    b.attribute_begin(); b.rotate(-90.0, 1.0, 0.0, 0.0); b.rotate(30.0, 0.0, 0.0, 1.0)
    if ENVS[name] is None: b.light_source("infinite", L=(0.7, 0.9, 1.1))
    else: b.light_source("infinite", texels=ENVS[name], L=(1.0, 0.9, 0.8))
    b.attribute_end()
    return b


def env_scene(pkg, name):
    return _floor(pkg, _env(pkg, _base(pkg), name))


def dist1d_cdf(func):
    """scene_plan.hip: dist1d, in float32."""
    n = len(func)
    cdf = np.zeros(n + 1, F)
    for i in range(1, n + 1):
        cdf[i] = F(cdf[i - 1] + F(F(func[i - 1]) / F(n)))
    fint = cdf[n]
    for i in range(1, n + 1):
        cdf[i] = F(F(i) / F(n)) if fint == 0 else F(cdf[i] / fint)
    return cdf, fint


def _with_neighbours(values):
    v = np.asarray(values, F)
    out = np.concatenate([v, np.nextafter(v, F(-1.0)), np.nextafter(v, F(2.0)), [F(0.0), F(U_TOP)]]).astype(F)
    return np.unique(out[(out >= 0) & (out < 1)])


def env_queries(pkg, sd, li):
    """test_device_probe.light_queries of the light, then the cdf ties and the texel seams at one reference point."""
    q = light_queries(pkg, sd, li, seed=300 + li)
    eh, ew = sd.env["texels"].shape[:2]
    imp = np.asarray(sd.env["importance"], F).reshape(2 * eh, 2 * ew)
    rows = [dist1d_cdf(r) for r in imp]
    marg, _ = dist1d_cdf([fi for _, fi in rows])
    uy = _with_neighbours(marg); ux = _with_neighbours(np.concatenate([c for c, _ in rows]))
    u = np.array([(a, b) for b in uy for a in ux], F)
    m = np.array(list(sd.lights[li].light_to_world), np.float64).reshape(4, 4)[:3, :3]
    seams = []
    for j in range(2 * eh + 1):
        for i in range(2 * ew + 1):
            for dt in (0.0, -1e-6, 1e-6):
                for dp in (0.0, -1e-6, 1e-6):
                    th, ph = np.pi * j / (2 * eh) + dt, 2 * np.pi * i / (2 * ew) + dp
                    seams.append(m @ np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)]))
    seams = np.array(seams, F)
    n = max(len(u), len(seams))
    u = np.concatenate([u, np.tile(np.array([[0.37, 0.61]], F), (n - len(u), 1))]); w = np.concatenate([seams, np.tile(seams[:1], (n - len(seams), 1))])
    p = np.tile(np.array([[0.3, 0.2, 0.1]], F), (n, 1)); nrm = np.tile(np.array([[0.0, 1.0, 0.0]], F), (n, 1))
    out = dict(q)
    out.update(p=np.concatenate([q["p"], p]), perr=np.concatenate([q["perr"], np.zeros((n, 3), F)]), n=np.concatenate([q["n"], nrm]),
               u=np.ascontiguousarray(np.concatenate([q["u"], u]), F), w=np.ascontiguousarray(np.concatenate([q["w"], w]), F), ties=len(uy) * len(ux), seams=len(seams))
    return out


_REF = {}   # environment -> (sd, li, queries, oracle results): computed once, shared by the two walks


def reference(pkg, oracle, name):
    if name not in _REF:
        sd, rp = env_scene(pkg, name).world_end()
        li = [i for i in range(sd.n_lights) if sd.lights[i].type == pkg._abi.PT_LIGHT_INFINITE][0]
        s = oracle.scene(sd)
        q = env_queries(pkg, sd, li)
        ref = oracle_light(oracle, s, li, q, q["w"])
        w2, ok = second_round_directions(ref, q["w"])
        back2 = oracle_pdf(oracle, s, li, q, w2)
        s.close()
        _REF[name] = (sd, li, q, ref, w2, ok, back2)
    return _REF[name]


@pytest.mark.parametrize("name", list(ENVS))
def test_the_oracle_alone_keeps_the_floor(pkg, oracle, name):
    """The floor, and that the structured queries reach what they are for, before any device result is looked at."""
    sd, li, q, ref, w2, ok, back2 = reference(pkg, oracle, name)
    share = check_light_floor(name, li, q, ref)
    ties = slice(len(q["p"]) - max(q["ties"], q["seams"]), len(q["p"]))
    eh, ew = sd.env["texels"].shape[:2]
    print(f"{name}: map {ew} x {eh}, {len(q['p'])} queries ({q['random']} random, {q['ties']} cdf ties, {q['seams']} seam directions), "
          f"non-zero sampled pdf: random {share:.3f}, ties {float((ref['pdf'][ties] != 0).mean()):.3f}; non-zero pdf_li of the seam directions {float((ref['back'][ties] != 0).mean()):.3f}")
    assert (ew == 1 and eh == 1) == (name == "const")
    assert (ref["pdf"][ties] != 0).any() and (ref["back"][ties] != 0).any()
    if name == "2x4_zero_rows":   # the zero rows are there: some seam directions fall into them
        assert (ref["back"][ties][: q["seams"]] == 0).any()


@pytest.mark.parametrize("name", list(ENVS))
def test_env_light_calls_match_the_oracle(pkg, gpu, oracle, probe, name):
    sd, li, q, ref, w2, ok, back2 = reference(pkg, oracle, name)
    check_light_floor(name, li, q, ref)
    scene = pkg.Scene(gpu, sd)
    try:
        dev = device_light(probe, scene, li, q, q["w"])
        for k in ("pdf", "L", "wi", "back"):
            assert_same_bits(dev[k], ref[k], f"{name}: {'pdf_li' if k == 'back' else 'sample_li ' + k} device vs oracle")
        dev2 = device_light(probe, scene, li, q, w2)
        assert_same_bits(dev2["back"], back2, f"{name}: pdf_li of the sampled directions device vs oracle")
    finally:
        scene.close()


# ---- renders
def _render_base(pkg):
    b = pkg.host.SceneBuilder()
    b.film.update(xres=32, yres=24); b.spp = 4
    b.integ.update(maxdepth=3)
    b.look_at((0.0, 2.0, 7.0), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0)); b.camera(fov=40.0)
    b.world_begin()
    return b


def _area_light(pkg, b):
    b.attribute_begin(); b.area_light_source(L=(10.0, 9.0, 8.0)); b.translate(-1.0, 3.0, 0.0)
    b.trianglemesh(np.array([[-0.8, 0.0, -0.6], [0.9, 0.0, -0.5], [0.1, 0.0, 0.9]], F), np.array([0, 2, 1], np.uint32)); b.attribute_end()
    return b


def _mesh(pkg, b):
    b.material("matte", Kd=(0.6, 0.5, 0.4))
    P, I, N = pkg.scenes.displaced_sphere(8, False)
    b.trianglemesh(P, I)
    return _floor(pkg, b)


def scene_a(pkg):
    b = _area_light(pkg, _env(pkg, _render_base(pkg), "const"))
    b.light_source("point", I=(20.0, 18.0, 15.0), from_=(1.5, 2.5, 1.0))
    return _mesh(pkg, b)


def scene_b(pkg):
    return _mesh(pkg, _area_light(pkg, _env(pkg, _render_base(pkg), "2x2")))


def scene_c(pkg):
    return _mesh(pkg, _env(pkg, _render_base(pkg), "3x2"))


RENDERS = {"a": scene_a, "b": scene_b, "c": scene_c}
_ORACLE = {}


def _oracle_render(pkg, oracle, case):
    if case not in _ORACLE:
        sd, rp = RENDERS[case](pkg).world_end()
        orc = oracle.scene(sd)
        _ORACLE[case] = (orc.render(rp, nthreads=ORACLE_THREADS), orc.counters())
    return _ORACLE[case]


@pytest.mark.parametrize("case", sorted(RENDERS))
def test_render_matches_the_oracle(pkg, gpu, oracle, case):
    sd, rp = RENDERS[case](pkg).world_end()
    kinds = sorted(int(sd.lights[i].type) for i in range(sd.n_lights))
    A = pkg._abi
    assert kinds == {"a": sorted([A.PT_LIGHT_DIFFUSE_AREA, A.PT_LIGHT_POINT, A.PT_LIGHT_INFINITE]), "b": sorted([A.PT_LIGHT_DIFFUSE_AREA, A.PT_LIGHT_INFINITE]), "c": [A.PT_LIGHT_INFINITE]}[case]
    ref, want = _oracle_render(pkg, oracle, case)
    g = pkg.Scene(gpu, sd)
    try:
        film = g.render(rp)
        assert_same_render(film, ref, g.counters(), want)
    finally:
        g.close()


_CHILD = r"""
import json, sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
from _pkg import import_pkg
pkg = import_pkg()
try:
    import torch  # noqa: F401 -- its bundled HIP runtime before the library's (conftest.gpu)
except ImportError:
    pass
import test_env_light_paths as T
lib = pkg.load_library(); lib.init(0)
lib.set_trace_exact({exact!r})
sd, rp = T.RENDERS[{case!r}](pkg).world_end()
g = pkg.Scene(lib, sd)
film = g.render(rp)
np.savez({out!r}, film=film, counters=json.dumps(g.counters()))
"""


@pytest.mark.parametrize("case", sorted(RENDERS))
def test_render_with_one_block_matches_the_oracle(pkg, gpu, oracle, tmp_path, trace_mode, case):
    out = str(tmp_path / "out.npz")
    code = _CHILD.format(root=ROOT, exact=trace_mode == "exact", case=case, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(trace_env(), PT_TEST_MAX_BLOCKS="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    ref, want = _oracle_render(pkg, oracle, case)
    assert_same_render(got["film"], ref, json.loads(str(got["counters"])), want)
