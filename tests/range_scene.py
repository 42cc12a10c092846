"""Test infrastructure of the sample-range tests (test_sample_ranges.py, test_film_tools.py): the scene whose film tells the job's spp from a range's length, and the
sum of several calls' counters."""
import numpy as np


def noise_image(n=64, seed=11):
    """Black / white texels without any smoothness: every MIP level is another picture, so the level the trilinear filter picks -- the ray differentials' scale -- shows."""
    rng = np.random.default_rng(seed)
    return np.repeat(rng.integers(0, 2, (n, n, 1)).astype(np.float32), 3, axis=2)


def range_scene(pkg, sampler="sobol", integrator="path", xres=32, yres=24, spp=8, maxdepth=5, spp_per_pass=2):
    """One triangle area light, a matte floor with a trilinear image-map Kd at high frequency (its MIP level follows rc.inv_sqrt_spp), one glass sphere; volpath: the
    camera stands in a homogeneous fog that fills the world."""
    b = pkg.host.SceneBuilder()
    b.film.update(xres=xres, yres=yres); b.spp = spp; b.sampler = sampler
    b.integ.update(maxdepth=maxdepth, kind=integrator)
    if integrator == "volpath":
        b.make_named_medium("fog", sigma_a=(0.02, 0.02, 0.02), sigma_s=(0.10, 0.12, 0.14), g=0.3)
        b.medium_interface("", "fog")
    b.look_at((0.0, 1.8, 6.0), (0.0, 0.2, 0.0), (0.0, 1.0, 0.0)); b.camera(fov=40.0)
    b.world_begin()
    b.attribute_begin(); b.area_light_source(L=(30.0, 28.0, 24.0))
    b.trianglemesh(np.array([(-1.5, 4.0, -1.0), (1.5, 4.0, -1.0), (0.0, 4.0, 1.5)], np.float32), np.array([0, 1, 2], np.uint32)); b.attribute_end()
    b.texture("noise", "color", "imagemap", pixels=noise_image(), trilinear=True, uscale=12.0, vscale=12.0)
    b.material("matte", Kd="noise")
    P = np.array([(-8.0, -1.0, -8.0), (-8.0, -1.0, 8.0), (8.0, -1.0, 8.0), (8.0, -1.0, -8.0)], np.float32)
    b.trianglemesh(P, np.array([0, 1, 2, 0, 2, 3], np.uint32), UV=np.array([[0, 0], [0, 1], [1, 1], [1, 0]], np.float32))
    b.attribute_begin(); b.material("glass", Kr=(1.0, 1.0, 1.0), Kt=(1.0, 1.0, 1.0), eta=1.5); b.translate(0.6, 0.0, 0.5); b.sphere(radius=1.0); b.attribute_end()
    sd, rp = b.world_end()
    rp.spp_per_pass = spp_per_pass
    return sd, rp


def add_counters(total, c):
    """total += c over every counter (lists element-wise); returns total (None: a copy of c)."""
    if total is None:
        return {k: (list(v) if isinstance(v, list) else v) for k, v in c.items()}
    for k, v in c.items():
        total[k] = [a + x for a, x in zip(total[k], v)] if isinstance(v, list) else total[k] + v
    return total


def render_ranges(scene, rp, ranges, film=None, **kw):
    """The ranges (first, n) of the job rp into one film; (film, summed counters)."""
    total = None
    for first, n in ranges:
        film = scene.render(rp, film=film, samples=(first, n), **kw)
        total = add_counters(total, scene.counters())
    return film, total
