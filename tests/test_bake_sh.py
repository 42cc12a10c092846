"""The SH points' bake on the GPU (libmi355bake.so, include/mi355bake.h "SH points") against the numpy model of its contract (tests/sh_reference.py), byte for byte:
sh_w, every single light sample (light, wi, pdf, Li, E, o, d, found) and the count of shadow rays. The light samples of the model are the oracle's, its occlusion
the oracle's any-hit query. For sphere, disk, distant and infinite lights the model takes the device's shadow ray over after holding its origin bit for bit and its
direction against the model's own exact rays of a triangle light of the same scene (sh_reference.light_samples).
bake_scenes.occluded_floor holds the instances and the alpha-masked occluder: the two geometries are the open floor and that one.

Measured on the MI355X, the largest 1 - dot(normalize(d), wi) per case: the model's exact rays of triangle lights 1.11e-7 .. 1.42e-7, the device rays taken over 1.3e-8
(distant) .. 1.48e-7 (sphere 1.45e-7, disk 1.14e-7, environment map 1.08e-7, constant infinite 5.9e-8); the largest ratio of the two in one scene was 1.24 (bound: 4)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import bake_reference as M
import lightmap_reference as LM
import lightmap_scenes as LS
import sh_reference as SR
from conftest import trace_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
_CACHE = {}   # the model's results, computed once (every test runs under both walks)


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def points(n):
    """The first n of 130 points on a 13 x 10 grid low above the floor, x in -1.7 .. 0.7, y in -1.4 .. 0.4, z in 0.12 .. 0.22, in a fixed shuffled order: about a
    fifth lie under occluded_floor's box ([-1.2, -0.2] x [-0.9, 0.1], z 0.3 .. 0.8). The odd offsets keep them out of every light's plane and off every light."""
    i = np.arange(130)
    p = np.stack([-1.7 + 0.2 * (i % 13) + 0.013, -1.4 + 0.2 * (i // 13) + 0.007, 0.12 + 0.05 * ((i * 7) % 3) + 0.003], axis=1).astype(F)
    return np.ascontiguousarray(p[np.random.RandomState(11).permutation(130)][:n])


# name: (geometry, lights, n_points, row, spp, nsamples (None: n_sel), light subset, sampler)
CASES = {
    "point": ("open_floor", "point", 65, 8, 4, None, None, "sobol"),
    "spot": ("open_floor", "spot", 65, 8, 4, None, None, "halton"),
    "distant": ("open_floor", "distant", 65, 8, 4, None, None, "sobol"),
    "quad": ("open_floor", "quad", 65, 8, 4, None, None, "sobol"),
    "quad_twosided": ("open_floor", "quad_twosided", 65, 8, 4, None, None, "halton"),
    "sphere": ("open_floor", "sphere", 65, 8, 4, None, None, "sobol"),
    "disk": ("open_floor", "disk", 65, 8, 4, None, None, "sobol"),
    "infinite": ("open_floor", "infinite", 65, 8, 4, None, None, "sobol"),
    "envmap": ("open_floor", "envmap", 65, 8, 4, None, None, "halton"),
    "one_point": ("open_floor", "point_quad", 1, 8, 4, None, None, "sobol"),        # a wave of one lane; nsamples = n_sel = 3
    "all_occluded_130": ("occluded_floor", "all", 130, 16, 4, None, None, "sobol"),  # three waves, the last of two lanes; a ragged last row
    "all_occluded_63": ("occluded_floor", "all", 63, 8, 8, 1, None, "halton"),       # nsamples = 1
    "all_occluded_64": ("occluded_floor", "all", 64, 8, 4, 16, None, "sobol"),       # a whole wave; nsamples = 2 n_sel
    "subset_occluded_65": ("occluded_floor", "all", 65, 16, 4, 2, [0, 3, 5, 7], "sobol"),   # point, a quad triangle, sphere, environment map
    "two_chunks": ("open_floor", "quad", 65, 8, 4, 70, None, "halton"),             # 70 elements per sample: chunks of 64 and 6, a pass is one sample
}


def case_scene(pkg, name):
    geometry, lights = CASES[name][:2]
    return cached(("scene", geometry, lights), lambda: LS.scene(pkg, geometry, lights)[0])


def model(pkg, oracle, sc, name):
    """The model's bake of a case (cached), with the device's single samples it held the rays it took over against."""
    geometry, lights, n_points, row, spp, ns, subset, sampler = CASES[name]
    sd = case_scene(pkg, name)

    def make():
        n = len(LM.selected_lights(int(sd.desc().n_lights), subset)) if ns is None else ns
        pt, s, k = M.sample_list(np.arange(n_points), spp, n)
        dev = sc.bake_sh_rays(points(n_points), spp, pt, s, k, nsamples=n, lights=subset, sampler=sampler, row=row)
        return SR.bake(oracle, pkg, sd, points(n_points), spp, n, subset, sampler, row, device=dev)
    return cached(("model", name), make), sd


def occlusion_is_what_the_case_is_about(want):
    """At least a tenth of the contributing samples are occluded and at least a quarter arrive: on the model."""
    occluded, rays = int(np.asarray(want["occluded"], bool).sum()), want["n_rays"]
    return 10 * occluded >= rays and 4 * (rays - occluded) >= rays


@pytest.mark.parametrize("name", sorted(CASES))
def test_sh_sums_samples_and_ray_count_are_the_models(pkg, gpu, oracle, name):
    geometry, lights, n_points, row, spp, ns, subset, sampler = CASES[name]
    sc = pkg.Scene(gpu, case_scene(pkg, name))
    want, sd = model(pkg, oracle, sc, name)
    r, n = want["samples"], want["nsamples"]
    print(name, "samples", len(r["point"]), "rays", want["n_rays"], "occluded", int(want["occluded"].sum()), "deviation exact %.3g taken over %.3g" % (r["exact_dev"], r["other_dev"]))
    # the case reaches what it is about
    assert 0 < want["n_rays"] and np.abs(want["sh_w"][:, :27]).max() > 0 and np.isfinite(want["sh_w"]).all()
    if name == "spot":
        black = (r["Li"] == 0).all(axis=1)
        assert black.any() and not black.all() and not r["contributes"][black].any()   # points outside the cone
    if geometry == "occluded_floor":
        assert occlusion_is_what_the_case_is_about(want), (want["n_rays"], int(want["occluded"].sum()))
    if subset is not None:
        assert set(np.unique(r["light"])) == set(subset)
    # every single sample
    pts = points(n_points)
    dev = sc.bake_sh_rays(pts, spp, r["point"], r["s"], r["k"], nsamples=n, lights=subset, sampler=sampler, row=row)
    assert (dev["found"] == np.where(r["contributes"], 3, 1)).all()
    for key in ("light", "wi", "pdf", "Li", "E", "o", "d"):
        assert same(dev[key], r[key]), (key, np.argwhere(dev[key] != r[key])[:4])
    beyond = sc.bake_sh_rays(pts, spp, [n_points, 0], [0, 0], [0, 0], nsamples=n, lights=subset, sampler=sampler, row=row)
    assert beyond["found"][0] == 0 and beyond["found"][1] & 1 and not any(beyond[key][0].any() for key in ("wi", "Li", "E", "o", "d")) and beyond["pdf"][0] == 0
    # the bake
    got = sc.bake_sh(pts, spp, nsamples=ns, lights=subset, sampler=sampler, row=row)
    assert same(got, want["sh_w"]), np.argwhere(got != want["sh_w"])[:6]
    c = sc.counters()
    assert c["shadow_tests"] == want["n_rays"] and c["camera_rays"] == 0
    stats = {s["name"]: s for s in sc.kernel_stats()}
    assert {"bake_sh_rays", "shadow", "bake_sh_accum"} <= set(stats) and not {"bake_light_rays", "bake_rays", "bake_raster", "bake_select"} & set(stats)
    if name == "two_chunks":
        assert stats["shadow"]["launches"] == spp * 2 and stats["bake_sh_rays"]["launches"] == spp * 2
        assert sc.bake_sh_pass_size(n_points, spp, nsamples=70, row=row) == 1
    sh, reached = pkg.runtime.resolve_sh(got, spp, n)
    want_sh, want_reached = SR.resolve(want["sh_w"], spp, n)
    assert same(sh, want_sh) and same(reached, want_reached) and reached.max() <= 1


def test_ranges_pass_sizes_repeats_device_buffers_and_the_lightmap_beside_it(pkg, gpu, oracle):
    torch = pytest.importorskip("torch")
    sd, shape = cached(("scene+shape", "occluded_floor", "point_quad"), lambda: LS.scene(pkg, "occluded_floor", "point_quad"))
    sc = pkg.Scene(gpu, sd)
    pts = points(130)
    kw = dict(nsamples=3, sampler="halton", row=16)
    want = cached("ranges model", lambda: SR.bake(oracle, pkg, sd, pts, 6, 3, None, "halton", 16))   # (point and triangle lights: no ray to take over)
    assert occlusion_is_what_the_case_is_about(want)
    light_before = sc.bake_light(shape, 16, 16, 2, planes=("light_w",))["light_w"]
    whole = sc.bake_sh(pts, 6, **kw)
    assert same(whole, want["sh_w"])
    parts = sc.bake_sh(pts, 6, samples=(0, 2), **kw)
    assert not same(parts, whole)
    assert sc.bake_sh(pts, 6, samples=(2, 4), sums=parts, **kw) is parts and same(parts, whole)
    assert sc.bake_sh_pass_size(130, 6, nsamples=3, row=16) == 6 and sc.bake_sh_pass_size(130, 6, nsamples=3, row=16, spp_per_pass=1) == 1
    assert same(sc.bake_sh(pts, 6, spp_per_pass=1, **kw), whole)
    assert {s["name"]: s for s in sc.kernel_stats()}["bake_sh_rays"]["launches"] == 6
    assert same(sc.bake_sh(pts, 6, spp_per_pass=4, **kw), whole)
    twice = sc.bake_sh(pts, 6, **kw); first = twice.copy()
    sc.bake_sh(pts, 6, sums=twice, **kw)   # added to what the buffer holds
    assert same(first, whole) and not same(twice, whole) and np.allclose(twice, 2 * whole, rtol=1e-5) and (twice[:, 27] == 2 * whole[:, 27]).all()
    dev = torch.zeros((130, 28), device="cuda")
    torch.cuda.synchronize()
    assert sc.bake_sh(pts, 6, device_ptr=dev.data_ptr(), **kw) is None
    assert dev.cpu().numpy().tobytes() == whole.tobytes()
    assert same(sc.bake_light(shape, 16, 16, 2, planes=("light_w",))["light_w"], light_before)   # the mesh's lightmap, before and after


def test_sh_refusals_that_read_the_scene(pkg, gpu):
    import ctypes as C
    A = pkg._abi
    sc = pkg.Scene(gpu, cached(("scene", "open_floor", "all"), lambda: LS.scene(pkg, "open_floor", "all")[0]))
    pts = points(5)
    sums = np.zeros((5, 28), F)
    fp = lambda a: a.ctypes.data_as(A.fp)
    for n_lights, lights in ((7, None), (9, np.ones(9, np.uint8))):
        _, hp = sc.bake_sh_params(pts, 1, n_lights)
        st = gpu.bake.pt_bake_sh(sc.h, C.byref(hp), fp(pts), None if lights is None else lights.ctypes.data_as(A.u8p), n_lights, fp(sums), 0)
        assert st == A.PT_ERR_INVALID_ARG and b"the scene 8 lights" in gpu.lib.pt_last_error()
    with pytest.raises(pkg.runtime.PtError) as e:
        sc.bake_sh(pts, 1 << 20, nsamples=1 << 31, sums=sums)
    assert "Sobol" in str(e.value)
    with pytest.raises(pkg.runtime.PtError) as e:   # a row beyond the Sobol' pixel grid
        sc.bake_sh(pts, 1, nsamples=8, row=(1 << 25) + 1, sums=sums)
    assert "Sobol" in str(e.value)
    assert not sums.any()
    assert np.abs(sc.bake_sh(pts, 1)).max() > 0   # the scene bakes after the refusals


def test_bake_sh_tool_writes_what_the_resolve_predicts(pkg, gpu, tmp_path):
    scene = tmp_path / "light.pbrt"
    scene.write_text('LookAt 0 0 5  0 0 0  0 1 0\nCamera "perspective" "float fov" 30\nFilm "image" "integer xresolution" 8 "integer yresolution" 8\nWorldBegin\n'
                     'LightSource "point" "point from" [0.5 0.5 0.5] "rgb I" [5 5 9]\n'
                     'LightSource "distant" "point from" [0 1 1] "point to" [0 0 0] "rgb L" [1 0.5 0.25]\n'
                     'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [6 6 5]\n'
                     'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-1 -1 2  -1 1 2  1 1 2]\nAttributeEnd\n'
                     'Shape "sphere" "float radius" 0.5\n'
                     'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 -2 -0.6  2 -2 -0.6  2 2 -0.6  -2 2 -0.6] "float uv" [0.1 0.1 0.9 0.1 0.9 0.9 0.1 0.9]\nWorldEnd\n')
    out = tmp_path / "probes.npz"
    tool = os.path.join(ROOT, "tools", "bake_sh.py")
    r = subprocess.run([sys.executable, tool, str(scene), "--grid", "4,3,2", "--bounds=-1.8,-1.8,-0.5,1.8,1.8,1.5", "--spp", "2", "--nsamples", "4", "--lights", "1,2", "--out", str(out)],
                       capture_output=True, text=True, timeout=300, env=trace_env())
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    got = np.load(str(out))
    pts = got["points"]
    assert pts.shape == (24, 3) and pts.dtype == F and np.allclose(pts[0], (-1.35, -1.2, 0.0)) and np.allclose(pts[1] - pts[0], (0.9, 0, 0)) and np.allclose(pts[4] - pts[0], (0, 1.2, 0)) \
        and np.allclose(pts[12] - pts[0], (0, 0, 1.0))   # cell centres, x fastest
    sc = pkg.Scene(gpu, pkg.frontend.FrontScene(path=str(scene)))
    sh_w = sc.bake_sh(pts, 2, nsamples=4, lights=[1, 2])
    rays = sc.counters()["shadow_tests"]
    sh, reached = pkg.runtime.resolve_sh(sh_w, 2, 4)
    assert same(got["sh"], sh) and same(got["reached"], reached)
    assert line["points"] == 24 and line["rays"] == rays and 0 < rays <= 24 * 8 and "shadow" in line["ms"] and "bake_sh_rays" in line["ms"] and "bake_sh_accum" in line["ms"]
    assert reached.min() < 1 and reached.max() == 1 and sh[:, 0, 0].max() > sh[:, 0, 2].max() > 0   # the sphere's shadow; the distant light's colour leads
    # the default bounds are the vertices': the floor and the emissive triangle
    import importlib.util
    spec = importlib.util.spec_from_file_location("bake_sh_tool", tool); mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    assert np.allclose(mod.scene_bounds(sc), (-2, -2, -0.6, 2, 2, 2))
