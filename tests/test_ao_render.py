"""The ambient-occlusion integrator on the GPU (libmi355ao.so, include/mi355ao.h) against the CPU oracle's render loop
(orc_ao_render) and against what can be derived analytically."""
import math
import subprocess

import numpy as np
import pytest
from conftest import trace_env
from parity import assert_same_counters

pytestmark = pytest.mark.gpu
ZERO_KEYS = ("path_length_hist", "zero_radiance_paths_num", "zero_radiance_paths_den")


def ao_scene(pkg, builder, nsamples, cossample, sampler="sobol", **kw):
    b = builder(**kw)
    b.integ.update(kind="ao", nsamples=nsamples, cossample=cossample)
    b.sampler = sampler
    return b.world_end()


def render_ao(pkg, gpu, sd, rp, **set_rp):
    for k, v in set_rp.items():
        setattr(rp, k, v)
    sc = pkg.Scene(gpu, sd)
    film = sc.render(rp)
    return sc, film


def assert_film_close(film, ref, rtol=2e-6):
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = np.abs(film.astype(np.float64) - ref.astype(np.float64))
    assert (err <= rtol * np.maximum(np.abs(ref), 1e-3 * scale) + 1e-7 * scale).all(), float(err.max())


CASES = {
    "sobol_cos": dict(builder="ganesha_scale", sampler="sobol", cossample=True, kw=dict(n=12, xres=32, yres=24, spp=2)),
    "halton_cos": dict(builder="ganesha_scale", sampler="halton", cossample=True, kw=dict(n=12, xres=32, yres=24, spp=2)),
    "sobol_sphere": dict(builder="ganesha_scale", sampler="sobol", cossample=False, kw=dict(n=12, xres=32, yres=24, spp=2)),
    "normals": dict(builder="ganesha_scale", sampler="sobol", cossample=True, kw=dict(n=12, xres=32, yres=24, spp=1, with_normals=True)),
    "alpha": dict(builder="alpha_foliage", sampler="halton", cossample=False, kw=dict(xres=32, yres=24, spp=1, instanced=False)),
    "spheres": dict(builder="spheres_c1", sampler="sobol", cossample=True, kw=dict(xres=32, yres=24, spp=2)),
    "disks": dict(builder="disk_scene", sampler="halton", cossample=False, kw=dict(xres=32, yres=24, spp=2)),
    "instances": dict(builder="instanced_garden", sampler="sobol", cossample=True, kw=dict(xres=32, yres=24, spp=1, flatten=False)),
    "max_lum": dict(builder="ganesha_scale", sampler="halton", cossample=True, kw=dict(n=12, xres=32, yres=24, spp=2), max_lum=1.0),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_ao_film_and_counters_match_the_reference(pkg, gpu, oracle, case):
    c = CASES[case]
    ns = 8
    sd, rp = ao_scene(pkg, getattr(pkg.scenes, c["builder"]), ns, c["cossample"], c["sampler"], **c["kw"])
    assert rp.integrator == pkg._abi_ao.PT_INTEGRATOR_AO
    if "max_lum" in c:
        rp.max_sample_luminance = c["max_lum"]
    sc, film = render_ao(pkg, gpu, sd, rp)
    osc = oracle.scene(sd)
    want = osc.render(rp, nthreads=4)
    got, ref = sc.counters(), osc.counters()
    assert_same_counters(got, ref)
    for k in ZERO_KEYS:
        assert not np.any(got[k]), k
    if not c["cossample"] and case == "sobol_sphere":
        assert got["sanitized_negative"] > 0   # uniform sphere sampling: some sample's sum is negative
    assert_film_close(film, want)
    if "max_lum" in c:   # the clamp fires: the unclamped film is another one
        rp.max_sample_luminance = float("inf")
        assert not np.allclose(osc.render(rp, nthreads=4), want, rtol=1e-3)


def _plane_scene(pkg, kind, inside_sphere=False, nsamples=16, cossample=True, spp=2, res=16):
    b = pkg.host.SceneBuilder()
    b.film.update(xres=res, yres=res); b.spp = spp
    b.integ.update(kind="ao", nsamples=nsamples, cossample=cossample)
    if inside_sphere:
        b.look_at((0, 0, 0), (0, 0, 1), (0, 1, 0)); b.camera(fov=60.0)
        b.world_begin(); b.rotate(90.0, 1, 0, 0); b.sphere(radius=5.0)   # (the poles, where dpdu vanishes, off the view axis)
    else:
        b.look_at((0, 0, -1), (0, 0, 0), (0, 1, 0)); b.camera(fov=30.0)
        b.world_begin()
        if kind == "sphere":
            b.translate(0, 0, 1000.0); b.rotate(90.0, 1, 0, 0); b.sphere(radius=900.0)
        elif kind == "disk":
            b.translate(50.0, 0, 0); b.disk(height=0.0, radius=100.0)   # (the centre, where dpdu vanishes, off the frame)
        else:
            b.trianglemesh([(-100, -100, 0), (100, -100, 0), (100, 100, 0), (-100, 100, 0)], [0, 1, 2, 0, 2, 3])
    return b.world_end()


def test_ao_camera_inside_a_sphere_is_black(pkg, gpu):
    sd, rp = _plane_scene(pkg, "sphere", inside_sphere=True)
    sc, film = render_ao(pkg, gpu, sd, rp)
    c = sc.counters()
    n = 16 * 16 * 2
    assert np.all(film[..., :3] == 0.0) and c["camera_rays"] == n and c["intersect_tests"] == n and c["shadow_tests"] == 16 * n
    assert c["sphere_tests"] > 0 and c["film_splats"] >= n


@pytest.mark.parametrize("kind", ["quad", "sphere", "disk"])
def test_ao_open_surface_filling_the_frame_gives_pi(pkg, gpu, kind):
    sd, rp = _plane_scene(pkg, kind)
    sc, film = render_ao(pkg, gpu, sd, rp)
    rgb = sc.resolve(film)
    assert np.all(film[..., 3] > 0)
    assert np.allclose(rgb, math.pi, rtol=1e-5, atol=0), (rgb.min(), rgb.max())
    c = sc.counters(); n = 16 * 16 * 2
    assert c["camera_rays"] == n and c["intersect_tests"] == n and c["shadow_tests"] == 16 * n
    if kind != "quad":
        assert c["sphere_tests"] >= n   # every camera ray and AO ray tests the one quadric that its box admits
    assert c["sanitized_nan"] == c["sanitized_negative"] == c["sanitized_infinite"] == 0


def test_ao_instances_match_the_flattened_reference(pkg, gpu, oracle):
    ns = 4
    sd, rp = ao_scene(pkg, pkg.scenes.instanced_garden, ns, True, xres=32, yres=24, spp=1, flatten=False)
    sc, film = render_ao(pkg, gpu, sd, rp)
    sdf, rpf = ao_scene(pkg, pkg.scenes.instanced_garden, ns, True, xres=32, yres=24, spp=1, flatten=True)
    want = oracle.scene(sdf).render(rpf, nthreads=4)
    a = sc.resolve(film); b = sc.resolve(want)
    diff = np.abs(a - b)
    assert (diff.max(axis=2) > 0.05).mean() <= 0.01 and diff.mean() < 2e-3


def test_ao_pass_sizes_and_tile_ranks_agree(pkg, gpu):
    sd, rp = ao_scene(pkg, pkg.scenes.ganesha_scale, 70, True, n=12, xres=40, yres=24, spp=4)   # 70: two chunks (64 + 6) per pass
    sc = pkg.Scene(gpu, sd)
    films = []
    for spp_per_pass in (1, 2, 0):
        rp.spp_per_pass = spp_per_pass
        films.append(sc.render(rp))
    base_c = sc.counters()
    for f in films[1:]:
        assert np.allclose(f, films[0], rtol=1e-6, atol=1e-6 * float(np.abs(films[0]).max()))
    total = np.zeros_like(films[0]); summed = {}
    for rank in range(4):
        rp.tile_rank, rp.tile_world = rank, 4
        sc.render(rp, film=total)
        for k, v in sc.counters().items():
            summed[k] = np.add(summed.get(k, 0), v)
    assert np.allclose(total, films[0], rtol=1e-6, atol=1e-6 * float(np.abs(films[0]).max()))
    assert_same_counters(summed, base_c)


def test_ao_renders_leave_free_memory_unchanged(pkg, gpu):
    torch = pytest.importorskip("torch")   # (the HIP runtime libmi355pt.so runs on: the conftest's gpu fixture loads torch's first)
    sd, rp = ao_scene(pkg, pkg.scenes.ganesha_scale, 16, True, n=12, xres=32, yres=24, spp=2)
    sc = pkg.Scene(gpu, sd)
    sc.render(rp)   # (the scene's workspace: allocated once, lives with the scene)
    before = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        sc.render(rp)
    assert torch.cuda.mem_get_info(0)[0] == before


def test_ao_errors_are_returned_with_their_text(pkg, gpu):
    import ctypes as C
    A = pkg._abi
    sd, rp = ao_scene(pkg, pkg.scenes.ganesha_scale, 8, True, n=8, xres=16, yres=16, spp=1)
    sc = pkg.Scene(gpu, sd)
    film = np.zeros((16, 16, 4), np.float32)
    ao = pkg._abi_ao.PtAOParams(0, 1)
    assert gpu.ao.pt_ao_render(sc.h, C.byref(rp), C.byref(ao), film.ctypes.data_as(C.c_void_p), 0) == A.PT_ERR_INVALID_ARG
    assert b"nsamples" in gpu.lib.pt_last_error()
    assert gpu.ao.pt_ao_render(sc.h, C.byref(rp), None, film.ctypes.data_as(C.c_void_p), 0) == A.PT_ERR_INVALID_ARG
    assert b"null" in gpu.lib.pt_last_error()
    ao = pkg._abi_ao.PtAOParams(1 << 31, 1); rp.spp = 1 << 20   # 2^51 sample numbers per pixel at a 16-pixel Sobol' grid: beyond the tables
    assert gpu.ao.pt_ao_render(sc.h, C.byref(rp), C.byref(ao), film.ctypes.data_as(C.c_void_p), 0) == A.PT_ERR_INVALID_ARG
    assert b"Sobol" in gpu.lib.pt_last_error()
    s = C.c_uint32()
    assert gpu.ao.pt_ao_pass_size(sc.h, C.byref(rp), C.byref(ao), C.byref(s)) == A.PT_ERR_INVALID_ARG
    rp.sampler_type = A.PT_SAMPLER_HALTON; rp.spp = 1 << 31   # 2^62 sample numbers per pixel; the Halton stride of a 16 x 16 grid is 2^4 * 3^3 = 432: 64-bit indices reach 4.3e16 of them
    assert gpu.ao.pt_ao_render(sc.h, C.byref(rp), C.byref(ao), film.ctypes.data_as(C.c_void_p), 0) == A.PT_ERR_INVALID_ARG
    assert b"Halton" in gpu.lib.pt_last_error()
    assert gpu.ao.pt_ao_pass_size(sc.h, C.byref(rp), C.byref(ao), C.byref(s)) == A.PT_ERR_INVALID_ARG
    assert b"Halton" in gpu.lib.pt_last_error()
    assert not film.any()


def test_mi355pbrt_renders_an_ambientocclusion_scene(pkg, gpu, tmp_path):
    scene = tmp_path / "ao.pbrt"
    out = tmp_path / "ao.pfm"
    scene.write_text('LookAt 0 0 -1  0 0 0  0 1 0\nCamera "perspective" "float fov" 30\n'
                     'Film "image" "integer xresolution" 16 "integer yresolution" 16\nSampler "sobol" "integer pixelsamples" 2\n'
                     'Integrator "ambientocclusion" "integer nsamples" 8\nWorldBegin\n'
                     'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-100 -100 0 100 -100 0 100 100 0 -100 100 0]\nWorldEnd\n')
    r = subprocess.run([pkg.frontend.CLI_PATH, str(scene), "--outfile", str(out)], capture_output=True, text=True, timeout=300, env=trace_env())
    assert r.returncode == 0, r.stderr
    img = pkg.frontend.read_image(str(out))
    assert img.shape == (16, 16, 3) and np.allclose(img, math.pi, rtol=1e-5)
