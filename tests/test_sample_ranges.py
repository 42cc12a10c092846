"""Renders of a range of sample numbers (pt_render_samples, pt_ao_render_samples, pt_multi_render_samples): the union of disjoint ranges is the whole job -- the film to
float summation order, every counter exactly -- against the CPU oracle, which renders the whole job once per case. The scene (range_scene.py) has a high-frequency
trilinear texture, so that a range which took its own length for the job's spp (the ray differentials' scale, integrator.rs:340) renders another film."""
import ctypes as C

import numpy as np
import pytest
from parity import ORACLE_THREADS, assert_same_counters, assert_same_film, assert_same_render
from range_scene import add_counters, range_scene, render_ranges

pytestmark = pytest.mark.gpu
RANGES = [(0, 3), (3, 1), (4, 4)]   # spp_per_pass = 2: a range of two passes that ends in a ragged one, a single sample, a range of whole passes


@pytest.mark.parametrize("integrator", ["path", "volpath"])
@pytest.mark.parametrize("sampler", ["sobol", "halton"])
def test_split_equals_whole(pkg, gpu, oracle, sampler, integrator):
    sd, rp = range_scene(pkg, sampler, integrator)
    assert rp.spp == 8 and rp.spp_per_pass == 2 and sd.desc().n_textures > 0
    g = pkg.Scene(gpu, sd); orc = oracle.scene(sd)
    first, c0 = render_ranges(g, rp, RANGES[:1])
    film, rest = render_ranges(g, rp, RANGES[1:], film=first.copy())
    total = add_counters(c0, rest)
    ref = orc.render(rp, nthreads=ORACLE_THREADS)
    assert_same_render(film, ref, total, orc.counters())
    # the guard: the same three samples rendered as a JOB of 3 spp (the differentials scaled by 1/sqrt(3), not 1/sqrt(8)) are another film
    rp.spp = 3
    wrong = orc.render(rp, nthreads=ORACLE_THREADS)
    close = np.isclose(wrong[..., :3], first[..., :3], rtol=2e-6, atol=1e-7)
    print("pixels channels beyond the film tolerance when the range length leaks into the differential scale:", int((~close).sum()), "of", close.size)
    assert (~close).sum() > close.size // 20


def test_ranges_times_tile_shards(pkg, gpu, oracle):
    sd, rp = range_scene(pkg)
    g = pkg.Scene(gpu, sd); orc = oracle.scene(sd)
    ref = orc.render(rp, nthreads=ORACLE_THREADS)
    film, total = None, None
    rp.tile_world = 2
    for rank in (0, 1):
        rp.tile_rank = rank
        film, c = render_ranges(g, rp, [(0, 5), (5, 3)], film=film)
        total = add_counters(total, c)
    assert_same_render(film, ref, total, orc.counters())


def test_first_touch_light_grid_lives_across_calls(pkg, gpu, oracle):
    sd, rp = pkg.scenes.emissive_field(n_lights=48, spp=4).world_end()
    rp.light_strategy = pkg._abi.PT_LS_SPATIAL_LAZY
    g = pkg.Scene(gpu, sd); orc = oracle.scene(sd)
    film, total = render_ranges(g, rp, [(0, 2), (2, 2)])   # (a lookup of a voxel nobody computed -- `missing` != 0 -- fails the call)
    stats = {s["name"]: s for s in g.kernel_stats()}
    assert stats["light_touch"]["launches"] > 0
    ref = orc.render(rp, nthreads=ORACLE_THREADS)
    assert_same_render(film, ref, total, orc.counters())


def test_ao_ranges(pkg, gpu, oracle):
    b = pkg.scenes.ganesha_scale(n=12, xres=32, yres=24, spp=4)
    b.integ.update(kind="ao", nsamples=4, cossample=True)
    sd, rp = b.world_end()
    assert rp.integrator == pkg._abi_ao.PT_INTEGRATOR_AO
    g = pkg.Scene(gpu, sd); orc = oracle.scene(sd)
    film, total = render_ranges(g, rp, [(0, 1), (1, 3)])
    ref = orc.render(rp, nthreads=4)
    assert_same_counters(total, orc.counters())
    scale = max(float(np.abs(ref).max()), 1e-30)   # (test_ao_render.assert_film_close)
    err = np.abs(film.astype(np.float64) - ref.astype(np.float64))
    assert (err <= 2e-6 * np.maximum(np.abs(ref), 1e-3 * scale) + 1e-7 * scale).all(), float(err.max())
    whole = g.render(rp)
    assert_same_counters(g.counters(), total)
    assert_same_film(film, whole)


def test_multi_ranges_equal_the_plain_render(pkg, gpu):
    sd, rp = range_scene(pkg)
    single = pkg.Scene(gpu, sd)
    ref = single.render(rp); rc = single.counters()
    multi = pkg.MultiScene(gpu, sd, [0, 0])
    film, total = render_ranges(multi, rp, [(0, 5), (5, 3)])
    assert_same_render(film, ref, total, rc)


def test_range_of_the_whole_job_is_the_whole_render(pkg, gpu):
    sd, rp = range_scene(pkg)
    g = pkg.Scene(gpu, sd)
    whole = g.render(rp); wc = g.counters()
    film = g.render(rp, samples=(0, rp.spp))
    assert_same_render(film, whole, g.counters(), wc)


@pytest.mark.parametrize("first,n", [(0, 0), (6, 3), (2 ** 32 - 1, 2)])
def test_bad_ranges_are_refused_and_leave_the_film_alone(pkg, gpu, first, n):
    A = pkg._abi
    sd, rp = range_scene(pkg)
    film = np.full((24, 32, 4), 7.0, np.float32)
    ptr = film.ctypes.data_as(C.c_void_p)
    g = pkg.Scene(gpu, sd)
    assert gpu.lib.pt_render_samples(g.h, C.byref(rp), first, n, ptr, 0) == A.PT_ERR_INVALID_ARG
    m = pkg.MultiScene(gpu, sd, [0, 0])
    assert gpu.lib.pt_multi_render_samples(m.h, C.byref(rp), first, n, ptr, 0) == A.PT_ERR_INVALID_ARG
    ao = pkg._abi_ao.PtAOParams(4, 1)
    assert gpu.ao.pt_ao_render_samples(g.h, C.byref(rp), C.byref(ao), first, n, ptr, 0) == A.PT_ERR_INVALID_ARG
    assert (film == 7.0).all()


def _all_zero(counters):
    return all(not np.any(v) for v in counters.values())


def test_a_rank_that_owns_no_tile_renders_nothing_and_reports_nothing(pkg, gpu, oracle):
    """32x16 pixels under the box filter are two 16x16 tiles: rank 3 of 4 owns none. Either integrator's call returns PT_OK (render() raises otherwise), adds nothing to the
    film and leaves zeroed counters and no launches behind -- not those of the render before it --, and the handle renders on as before."""
    AO = pkg._abi_ao
    sd, rp = range_scene(pkg, xres=32, yres=16)
    sb = rp.sample_bounds
    assert -(-(sb[2] - sb[0]) // 16) * -(-(sb[3] - sb[1]) // 16) == 2
    g = pkg.Scene(gpu, sd); orc = oracle.scene(sd)
    ref = orc.render(rp, nthreads=ORACLE_THREADS); oc = orc.counters()
    for integrator in (rp.integrator, AO.PT_INTEGRATOR_AO):
        assert_same_render(g.render(rp), ref, g.counters(), oc)   # a normal render: counters and stats to go stale
        assert sum(s["launches"] for s in g.kernel_stats()) > 0
        path = rp.integrator
        rp.tile_world, rp.tile_rank, rp.integrator = 4, 3, integrator
        film = g.render(rp, film=np.full((16, 32, 4), 7.0, np.float32), ao=AO.PtAOParams(4, 1))
        assert (film == 7.0).all()
        assert _all_zero(g.counters()), g.counters()
        assert sum(s["launches"] for s in g.kernel_stats()) == 0, g.kernel_stats()
        rp.tile_world, rp.tile_rank, rp.integrator = 1, 0, path
    assert_same_render(g.render(rp), ref, g.counters(), oc)


@pytest.mark.parametrize("samples", [None, (2, 5)])
@pytest.mark.parametrize("spp_per_pass", [0, 3])
@pytest.mark.parametrize("integrator", ["path", "ao"])
def test_pass_size_is_the_size_of_the_passes_of_the_render_that_follows(pkg, gpu, integrator, spp_per_pass, samples):
    """pt_pass_size / pt_ao_pass_size answer from the function their render takes its geometry from: what they report for the job -- capped at the length of a range -- is
    the samples per `generate` launch (one launch per pass; the last pass may be ragged, so: n over the launches, rounded up) of the render that follows."""
    AO = pkg._abi_ao
    sd, rp = range_scene(pkg, xres=32, yres=16, spp_per_pass=spp_per_pass)
    assert rp.spp == 8
    g = pkg.Scene(gpu, sd)
    if integrator == "ao":
        rp.integrator = AO.PT_INTEGRATOR_AO
        size = g.ao_pass_size(rp, AO.PtAOParams(4, 1))
    else:
        size = g.pass_size(rp)
    n = rp.spp if samples is None else samples[1]
    want = min(size, n)
    print("pass size", size, "samples of the call", n)
    assert size == spp_per_pass or (spp_per_pass == 0 and 1 <= size <= rp.spp)
    g.render(rp, ao=AO.PtAOParams(4, 1), samples=samples)
    gen = [s for s in g.kernel_stats() if s["name"] == "generate"][0]
    print("generate launches", gen["launches"], "items", gen["items"])
    assert gen["launches"] == -(-n // want) and -(-n // gen["launches"]) == want
    assert gen["items"] == 2 * 256 * n   # two tiles of 256 pixel slots, every sample of the call once
