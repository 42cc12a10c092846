"""Host-side pieces of the ambient-occlusion integrator (include/mi355ao.h): the CPU oracle's AO render loop on scenes with a known
answer, the .pbrt front end's "ambientocclusion" parameters against the Python scene builder, and the C header against the ctypes
mirror."""
import ctypes as C
import math

import numpy as np
import pytest
from abi_checks import assert_mirror, c99_probe, exported_names


def _builder(pkg, nsamples=16, cossample=True, spp=2, res=8):
    b = pkg.host.SceneBuilder()
    b.film.update(xres=res, yres=res); b.spp = spp
    b.integ.update(kind="ao", nsamples=nsamples, cossample=cossample)
    return b


def _sample_values(oracle, b):
    """Oracle AO render of builder `b` in which every pixel holds exactly one sample: one Halton sample per pixel at the pixel centre
    and the box filter of radius 0.5. Returns each sample's y(L) (the film's Y, weight 1) and the render's counters."""
    b.sampler = "halton"; b.sample_at_pixel_center = True
    sd, rp = b.world_end()
    assert rp.spp == 1 and list(rp.filter_radius) == [0.5, 0.5]
    osc = oracle.scene(sd)
    film = osc.render(rp)
    c = osc.counters()
    assert c["film_splats"] == c["camera_rays"] and np.all(film[..., 3] == 1.0)
    return film[..., 1], c


def test_reference_open_quad_gives_pi_per_hit_sample(pkg, oracle):
    b = _builder(pkg, spp=1, res=16)
    b.look_at((0, 0, -1), (0, 0, 0), (0, 1, 0)); b.camera(fov=30.0)
    b.world_begin()
    b.trianglemesh([(-100, -100, 0), (100, -100, 0), (100, 100, 0), (-100, 100, 0)], [0, 1, 2, 0, 2, 3])
    L, c = _sample_values(oracle, b)
    assert np.allclose(L, math.pi, rtol=1e-6, atol=0), (L.min(), L.max())
    n = L.size
    assert c["camera_rays"] == c["intersect_tests"] == n and c["shadow_tests"] == 16 * n
    assert c["sanitized_nan"] == c["sanitized_negative"] == c["sanitized_infinite"] == 0


@pytest.mark.parametrize("cossample", [True, False])
def test_reference_inside_a_closed_box_gives_zero_or_only_escaping_back_rays(pkg, oracle, cossample):
    b = _builder(pkg, nsamples=8, cossample=cossample, spp=1)
    b.look_at((0, 0, 0), (0, 0, 1), (0, 1, 0)); b.camera(fov=60.0)
    b.world_begin()
    P = [(x, y, z) for z in (-2, 2) for y in (-2, 2) for x in (-2, 2)]   # cube corners, index = 4z + 2y + x
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    b.trianglemesh(P, [i for a, c1, c2, d in faces for i in (a, c1, c2, a, c2, d)])
    L, c = _sample_values(oracle, b)
    if cossample:
        assert np.all(L == 0.0) and c["sanitized_nan"] == c["sanitized_negative"] == c["sanitized_infinite"] == 0
    else:   # the rays of the outer hemisphere start behind the wall (offset_ray_origin along -n) and escape with dot(wi, n) < 0:
        # every sample's sum is negative, and the film's sanitiser zeroes it
        assert c["sanitized_negative"] == L.size and np.all(L == 0.0)
    assert c["camera_rays"] == c["intersect_tests"] == L.size and c["shadow_tests"] == 8 * L.size


def test_oracle_ao_render_rejects_zero_nsamples_and_null_params(pkg, oracle):
    A = pkg._abi
    sd, rp = _builder(pkg).world_end()
    osc = oracle.scene(sd)
    film = np.zeros((8, 8, 4), np.float32)
    fp = film.ctypes.data_as(A.fp)
    assert oracle.lib.orc_ao_render(osc.h, C.byref(rp), C.byref(pkg._abi_ao.PtAOParams(0, 1)), fp, 1) == A.PT_ERR_INVALID_ARG
    assert oracle.lib.orc_ao_render(osc.h, C.byref(rp), None, fp, 1) == A.PT_ERR_INVALID_ARG
    assert not film.any()


AO_SCENE = """LookAt 0 0 -1  0 0 0  0 1 0
Camera "perspective" "float fov" 30
Film "image" "integer xresolution" 24 "integer yresolution" 16
Sampler "halton" "integer pixelsamples" 4
Integrator "ambientocclusion" "integer nsamples" 16 "bool cossample" "false" "integer pixelbounds" [2 20 3 12]
WorldBegin
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-100 -100 0 100 -100 0 100 100 0 -100 100 0]
WorldEnd
"""


def test_front_end_ambientocclusion_matches_the_python_builder(pkg):
    A = pkg._abi
    fs = pkg.frontend.FrontScene(text=AO_SCENE)
    rp = fs.render_params(); ao = fs.ao_params()
    assert rp.integrator == pkg._abi_ao.PT_INTEGRATOR_AO == 2
    assert (ao.nsamples, ao.cos_sample) == (16, 0)
    b = _builder(pkg, nsamples=16, cossample=False, spp=4)
    b.film.update(xres=24, yres=16); b.sampler = "halton"; b.integ["pixelbounds"] = (2, 20, 3, 12)
    b.look_at((0, 0, -1), (0, 0, 0), (0, 1, 0)); b.camera(fov=30.0)
    b.world_begin()
    b.trianglemesh([(-100, -100, 0), (100, -100, 0), (100, 100, 0), (-100, 100, 0)], [0, 1, 2, 0, 2, 3])
    sd, rp2 = b.world_end()
    ao2 = sd.ao_params()
    assert (ao2.nsamples, ao2.cos_sample) == (ao.nsamples, ao.cos_sample)
    for f in ("integrator", "spp", "sampler_type", "pixel_bounds", "sample_bounds", "cropped_pixel_bounds", "filter_radius"):
        a, c = getattr(rp, f), getattr(rp2, f)
        assert (list(a) if hasattr(a, "__len__") else a) == (list(c) if hasattr(c, "__len__") else c), f
    assert list(rp.pixel_bounds) == [2, 3, 20, 12]
    # defaults (ao.rs:138-139)
    d = pkg.frontend.FrontScene(text=AO_SCENE.replace('"integer nsamples" 16 "bool cossample" "false" ', "")).ao_params()
    assert (d.nsamples, d.cos_sample) == (64, 1)
    b = pkg.host.SceneBuilder(); b.integ["kind"] = "ao"
    d = b.world_end()[0].ao_params()
    assert (d.nsamples, d.cos_sample) == (64, 1)


def test_front_end_path_scenes_are_unchanged_and_others_refused(pkg):
    A = pkg._abi
    for name, want in (("path", A.PT_INTEGRATOR_PATH), ("volpath", A.PT_INTEGRATOR_VOLPATH)):
        fs = pkg.frontend.FrontScene(text=AO_SCENE.replace('"ambientocclusion"', f'"{name}"'))
        assert fs.render_params().integrator == want
    for bad in ("bdpt", "whitted", "directlighting"):
        with pytest.raises(ValueError, match='only "path"'):
            pkg.frontend.FrontScene(text=f'Integrator "{bad}"\n')
    with pytest.raises(ValueError, match="nsamples"):
        pkg.frontend.FrontScene(text='Integrator "ambientocclusion" "integer nsamples" 0\n')


def test_mi355ao_header_is_c99_and_matches_the_ctypes_mirror(pkg):
    A = pkg._abi_ao
    assert_mirror("mi355ao.h", {A.PtAOParams: ("nsamples", "cos_sample")})
    assert [int(v) for v in c99_probe("mi355ao.h", 'printf("%d", PT_INTEGRATOR_AO);')] == [A.PT_INTEGRATOR_AO]

def test_ao_library_exports_only_its_entry_points(pkg):
    assert exported_names(pkg.runtime.AO_LIB_PATH) == set(pkg._abi_ao.ENTRY_POINTS)
