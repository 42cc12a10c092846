"""The lightmap bake on the GPU (libmi355bake.so, include/mi355bake.h "Lightmap") against the numpy model of its contract (tests/lightmap_reference.py), byte for
byte: light_w, the written planes, every single light sample (light, wi, pdf, Li, E, o, d, found) and the count of shadow rays. The light samples of the model are
the oracle's, its occlusion the oracle's any-hit query. For sphere, disk, distant and infinite lights the model takes the device's shadow ray over after holding its
origin bit for bit and its direction against the model's own exact rays of a triangle light of the same scene (lightmap_reference.light_samples).

Measured on the MI355X, the largest 1 - dot(normalize(d), wi) (float64 arithmetic on the float32 values) per case: the model's exact rays of triangle lights 0.99e-7
.. 1.48e-7, the device rays taken over 1.3e-8 (distant) .. 1.34e-7 (sphere 1.27e-7, disk 1.26e-7, environment map 1.15e-7 .. 1.32e-7, constant infinite 6.2e-8):
both are the rounding of a float32 unit vector, the largest ratio of the two in one scene was 1.33 (bound: 4)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import bake_reference as M
import lightmap_reference as LM
import lightmap_scenes as LS
from conftest import trace_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
_CACHE = {}   # the model's results, computed once (every test runs under both walks)


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# name: (geometry, lights, atlas, spp, nsamples (None: n_sel), light subset, sampler)
CASES = {
    "point": ("open_floor", "point", (16, 16), 2, None, None, "sobol"),
    "spot": ("open_floor", "spot", (16, 16), 2, None, None, "sobol"),
    "distant": ("open_floor", "distant", (16, 16), 2, None, None, "sobol"),
    "quad": ("open_floor", "quad", (16, 16), 2, None, None, "sobol"),
    "quad_twosided": ("open_floor", "quad_twosided", (16, 16), 2, None, None, "halton"),
    "sphere": ("open_floor", "sphere", (16, 16), 2, None, None, "sobol"),
    "disk": ("open_floor", "disk", (16, 16), 2, None, None, "sobol"),
    "infinite": ("open_floor", "infinite", (16, 16), 2, None, None, "sobol"),
    "envmap": ("open_floor", "envmap", (16, 16), 2, None, None, "halton"),
    "all_occluded": ("occluded_floor", "all", (16, 16), 1, None, None, "sobol"),           # nsamples = n_sel = 8
    "all_occluded_24x8": ("occluded_floor", "all", (24, 8), 2, 4, None, "halton"),        # tiles hang over the atlas
    "all_normals_24x8": ("shaded_normals", "all", (24, 8), 1, 16, None, "sobol"),         # nsamples = 2 n_sel
    "mirror_one_sample": ("shaded_mirror", "point_quad", (16, 16), 3, 1, None, "sobol"),  # nsamples = 1, spp a multiple of n_sel = 3
    "subset": ("open_floor", "all", (16, 16), 2, 2, [0, 3, 5, 7], "sobol"),               # point, a quad triangle, sphere, environment map
    "two_chunks": ("open_floor", "quad", (16, 16), 2, 70, None, "halton"),                # 70 elements per sample: chunks of 64 and 6, a pass is one sample
    "emissive_target": ("emissive_floor", None, (16, 16), 1, None, None, "sobol"),        # the baked mesh's own two triangles are lights 0 and 1
}


def case_scene(pkg, name):
    geometry, lights = CASES[name][:2]
    return cached(("scene", geometry, lights), lambda: LS.emissive_floor(pkg) if geometry == "emissive_floor" else LS.scene(pkg, geometry, lights))


def device_samples(sc, select, w, h, spp, ns, lights, sampler, tx, s, k):
    return sc.bake_light_rays(select, w, h, spp, tx, s, k, nsamples=ns, lights=lights, sampler=sampler)


def model(pkg, oracle, sc, name):
    """The model's bake of a case (cached), with the device's single samples it held the rays it took over against."""
    geometry, lights, (w, h), spp, ns, subset, sampler = CASES[name]
    sd, shape = case_scene(pkg, name)
    select = sd.prim_group == shape

    def make():
        owner = M.owner_map(M.scene_triangles(sd, select)[1], M.scene_triangles(sd, select)[0], w, h)
        n = len(LM.selected_lights(int(sd.desc().n_lights), subset)) if ns is None else ns
        tx, s, k = M.sample_list(LM.owned_texels(owner), spp, n)
        dev = device_samples(sc, select, w, h, spp, n, subset, sampler, tx, s, k)
        return LM.bake(oracle, pkg, sd, select, w, h, spp, n, subset, sampler, device=dev)
    return cached(("model", name), make), sd, select


@pytest.mark.parametrize("name", sorted(CASES))
def test_lightmap_planes_samples_and_ray_count_are_the_models(pkg, gpu, oracle, name):
    geometry, lights, (w, h), spp, ns, subset, sampler = CASES[name]
    sd, shape = case_scene(pkg, name)
    sc = pkg.Scene(gpu, sd)
    want, sd, select = model(pkg, oracle, sc, name)
    r, n = want["samples"], want["nsamples"]
    print(name, "samples", len(r["texel"]), "rays", want["n_rays"], "occluded", int(want["occluded"].sum()), "deviation exact %.3g taken over %.3g" % (r["exact_dev"], r["other_dev"]))
    # the case reaches what it is about
    assert (want["owner"] != NONE).sum() > 60 and 0 < want["n_rays"] and np.abs(want["light_w"]).max() > 0
    if name == "spot":
        black = (r["Li"] == 0).all(axis=1)
        assert black.any() and not black.all() and not r["contributes"][black].any()   # texels outside the cone
    if name == "quad":
        up, _ = cached("quad_up", lambda: LS.scene(pkg, "open_floor", [lambda b: LS.quad(b, up=True)]))
        assert not pkg.Scene(gpu, up).bake_light(1, 16, 16, 1)["light_w"].any()   # one-sided and turned away: nothing; the same quad two-sided is the case quad_twosided
    if geometry == "occluded_floor":
        assert 0 < want["occluded"].sum() < want["n_rays"]
    if subset is not None:
        assert set(np.unique(r["light"])) == set(subset)
    if name == "emissive_target":
        assert {0, 1, 2} == set(np.unique(r["light"])) and r["contributes"][r["light"] == 2].all()
    # every single sample
    dev = device_samples(sc, select, w, h, spp, n, subset, sampler, r["texel"], r["s"], r["k"])
    assert (dev["found"] == np.where(r["contributes"], 3, 1)).all()
    for key in ("light", "wi", "pdf", "Li", "E", "o", "d"):
        assert same(dev[key], r[key]), (key, np.argwhere(dev[key] != r[key])[:4])
    # the bake
    got = sc.bake_light(select, w, h, spp, nsamples=ns, lights=subset, sampler=sampler)
    for key in ("owner", "position", "normal", "light_w"):
        assert same(got[key], want[key]), (key, np.argwhere(got[key] != want[key])[:4])
    c = sc.counters()
    assert c["shadow_tests"] == want["n_rays"] and c["camera_rays"] == 0
    stats = {s["name"]: s for s in sc.kernel_stats()}
    assert {"bake_select", "bake_raster", "bake_points", "bake_light_rays", "shadow", "bake_light_accum"} <= set(stats) and "bake_rays" not in stats
    if name == "two_chunks":
        assert stats["shadow"]["launches"] == spp * 2 and stats["bake_light_rays"]["launches"] == spp * 2
        assert sc.bake_light_pass_size(w, h, spp, nsamples=70) == 1
    irr, reached = pkg.runtime.resolve_lightmap(got["light_w"], spp, n)
    want_irr, want_reached = LM.resolve(want["light_w"], spp, n)
    assert same(irr, want_irr) and same(reached, want_reached) and reached.max() <= 1


def test_ranges_pass_sizes_repeats_device_buffers_and_the_ao_bake_beside_it(pkg, gpu):
    torch = pytest.importorskip("torch")
    sd, shape = cached(("scene", "occluded_floor", "point_quad"), lambda: LS.scene(pkg, "occluded_floor", "point_quad"))
    sc = pkg.Scene(gpu, sd)
    kw = dict(nsamples=3, sampler="halton", planes=("light_w",))
    ao_before = sc.bake(shape, 16, 16, 2, nsamples=5, planes=("ao_w",))["ao_w"]
    whole = sc.bake_light(shape, 16, 16, 4, **kw)["light_w"]
    assert np.abs(whole).max() > 0
    parts = sc.bake_light(shape, 16, 16, 4, samples=(0, 2), **kw)
    sc.bake_light(shape, 16, 16, 4, samples=(2, 2), sums=parts, **kw)
    assert same(parts["light_w"], whole)
    assert sc.bake_light_pass_size(16, 16, 4, nsamples=3) == 4 and sc.bake_light_pass_size(16, 16, 4, nsamples=3, spp_per_pass=1) == 1
    assert same(sc.bake_light(shape, 16, 16, 4, spp_per_pass=1, **kw)["light_w"], whole)
    assert same(sc.bake_light(shape, 16, 16, 4, spp_per_pass=3, **kw)["light_w"], whole)
    assert same(sc.bake_light(shape, 16, 16, 4, **kw)["light_w"], whole)
    twice = sc.bake_light(shape, 16, 16, 4, **kw); first = twice["light_w"].copy()
    sc.bake_light(shape, 16, 16, 4, sums=twice, **kw)   # added to what the buffer holds
    assert same(first, whole) and not same(twice["light_w"], whole) and np.allclose(twice["light_w"], 2 * whole, rtol=1e-5)
    dev = {"owner": torch.zeros((16, 16), dtype=torch.int32, device="cuda"), "position": torch.zeros((16, 16, 3), device="cuda"), "normal": torch.zeros((16, 16, 3), device="cuda"),
           "light_w": torch.zeros((16, 16, 4), device="cuda")}
    torch.cuda.synchronize()
    host = sc.bake_light(shape, 16, 16, 4, nsamples=3, sampler="halton")
    assert sc.bake_light(shape, 16, 16, 4, nsamples=3, sampler="halton", device_ptrs={k: v.data_ptr() for k, v in dev.items()}) is None
    for k, v in dev.items():
        assert v.cpu().numpy().tobytes() == host[k].tobytes(), k
    assert same(host["light_w"], whole)
    assert same(sc.bake(shape, 16, 16, 2, nsamples=5, planes=("ao_w",))["ao_w"], ao_before)   # the mesh's own AO bake, before and after


def test_light_refusals_that_read_the_scene(pkg, gpu):
    import ctypes as C
    A, K = pkg._abi, pkg._abi_bake
    sd, shape = cached(("scene", "open_floor", "all"), lambda: LS.scene(pkg, "open_floor", "all"))
    sc = pkg.Scene(gpu, sd)
    lp = sc.bake_light_params(8, 8, 1, 8)
    planes = {"light_w": np.zeros((8, 8, 4), np.float32)}
    sel = sc.bake_select(shape)
    u8 = lambda a: a.ctypes.data_as(A.u8p)
    long = np.ones(len(sel) + 1, np.uint8)
    st = gpu.bake.pt_bake_light(sc.h, C.byref(lp), u8(long), len(long), None, 8, C.byref(K.light_buffers(planes)), 0)
    assert st == A.PT_ERR_INVALID_ARG and b"primitives" in gpu.lib.pt_last_error()
    for n_lights, lights in ((7, None), (9, np.ones(9, np.uint8))):
        q = sc.bake_light_params(8, 8, 1, n_lights)
        st = gpu.bake.pt_bake_light(sc.h, C.byref(q), u8(sel), len(sel), None if lights is None else u8(lights), n_lights, C.byref(K.light_buffers(planes)), 0)
        assert st == A.PT_ERR_INVALID_ARG and b"the scene 8 lights" in gpu.lib.pt_last_error()
    with pytest.raises(pkg.runtime.PtError) as e:   # the sphere light's sphere is shape 1
        sc.bake_light(1, 8, 8, 1)
    assert f"status {A.PT_ERR_UNSUPPORTED}" in str(e.value) and "sphere or disk" in str(e.value)
    with pytest.raises(pkg.runtime.PtError) as e:
        sc.bake_light(shape, 8, 8, 1 << 20, nsamples=1 << 31)
    assert "Sobol" in str(e.value)
    assert not planes["light_w"].any()
    assert np.abs(sc.bake_light(shape, 8, 8, 1)["light_w"]).max() > 0   # the scene bakes after the refusals


def test_bake_light_tool_writes_what_the_resolve_predicts(pkg, gpu, tmp_path):
    scene = tmp_path / "light.pbrt"
    scene.write_text('LookAt 0 0 5  0 0 0  0 1 0\nCamera "perspective" "float fov" 30\nFilm "image" "integer xresolution" 8 "integer yresolution" 8\nWorldBegin\n'
                     'LightSource "point" "point from" [0.5 0.5 0.5] "rgb I" [5 5 9]\n'
                     'LightSource "distant" "point from" [0 1 1] "point to" [0 0 0] "rgb L" [1 0.5 0.25]\n'
                     'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [6 6 5]\n'
                     'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-1 -1 2  -1 1 2  1 1 2]\nAttributeEnd\n'
                     'Shape "sphere" "float radius" 0.5\n'
                     'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 -2 -0.6  2 -2 -0.6  2 2 -0.6  -2 2 -0.6] "float uv" [0.1 0.1 0.9 0.1 0.9 0.9 0.1 0.9]\nWorldEnd\n')
    out = tmp_path / "light.pfm"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bake_light.py"), str(scene), "--shape", "2", "--size", "24x16", "--spp", "2", "--nsamples", "4", "--lights", "1,2", "--dilate", "2",
                        "--out", str(out)], capture_output=True, text=True, timeout=300, env=trace_env())
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    fs = pkg.frontend.FrontScene(path=str(scene))
    sc = pkg.Scene(gpu, fs)
    planes = sc.bake_light(2, 24, 16, 2, nsamples=4, lights=[1, 2], planes=("owner", "light_w"))
    rays = sc.counters()["shadow_tests"]
    irr, reached = pkg.runtime.resolve_lightmap(planes["light_w"], 2, 4)
    irr = sc.bake_dilate(planes["owner"], irr, 2)
    got = pkg.frontend.read_image(str(out))
    assert got.shape == (16, 24, 3) and same(got, irr)
    owned = planes["owner"] != NONE
    assert line["owned_texels"] == int(owned.sum()) and line["rays"] == rays and 0 < rays <= int(owned.sum()) * 8 and "shadow" in line["ms"] and "bake_light_rays" in line["ms"]
    assert reached[owned].min() < 1 and reached[owned].max() == 1   # the sphere's shadow; open at the rim
    assert irr[owned][:, 0].max() > irr[owned][:, 2].max() > 0   # the distant light's colour leads: the point light was not selected
