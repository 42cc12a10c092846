"""Renders of listed tiles (pt_render_tiles): a list is the shard it names, an arbitrary list is the sum of its tiles as the CPU oracle renders them one by one, lists
and sample ranges partition a job together, and a bad list is refused before the device is touched. Base film: range_scene at 40x24 -- a 3x2 tile grid, ragged on both
axes; under a Gaussian of radius 2 the sample bounds are [-2, 42) x [-2, 26): still 3x2, offset from the film's own 16x16 grid."""
import ctypes as C

import numpy as np
import pytest
from parity import ORACLE_THREADS, assert_same_counters, assert_same_film, assert_same_render
from range_scene import add_counters, range_scene
from tile_scene import grid_of, with_filter

pytestmark = pytest.mark.gpu


def _all_zero(counters):
    return all(not np.any(v) for v in counters.values())


def test_a_shards_list_is_the_shard(pkg, gpu, oracle):
    sd, rp = range_scene(pkg, xres=40, yres=24)
    g = pkg.Scene(gpu, sd); orc = oracle.scene(sd)
    assert g.tile_grid(rp) == grid_of(rp) == (3, 2)
    tiles = [t for t in range(6) if t % 3 == 1]
    film = g.render_tiles(rp, (0, rp.spp), tiles); lc = g.counters()
    rp.tile_rank, rp.tile_world = 1, 3
    shard = g.render(rp, samples=(0, rp.spp)); sc = g.counters()
    assert lc["camera_rays"] > 0
    assert_same_render(film, shard, lc, sc)   # (box filter: weights="exact", bit for bit)
    ref = orc.render(rp, nthreads=ORACLE_THREADS)
    assert_same_render(film, ref, lc, orc.counters())
    assert (film[:, :16, 3] == 0).all() and (film[:, 16:32, 3] > 0).all()   # tile column 1 and nothing else


@pytest.mark.parametrize("integrator,sampler", [("path", "sobol"), ("volpath", "halton")])
def test_an_arbitrary_list_is_the_sum_of_its_tiles(pkg, gpu, oracle, integrator, sampler):
    """Gaussian of radius 2: the tiles' footprints overlap, so splats of neighbouring tiles meet in one pixel and their sums are taken in another order than the
    oracle's (float atomics on the device, a sum of six films here): the weights are compared at the films' relative tolerance, not bit for bit."""
    sd, rp = range_scene(pkg, sampler, integrator, xres=40, yres=24)
    with_filter(pkg, rp, "gaussian", 2.0)
    assert list(rp.sample_bounds) == [-2, -2, 42, 26] and grid_of(rp) == (3, 2)
    g = pkg.Scene(gpu, sd); orc = oracle.scene(sd)
    whole = orc.render(rp, nthreads=ORACLE_THREADS)
    alone, alone_c = [], []
    rp.tile_world = 6
    for t in range(6):
        rp.tile_rank = t
        alone.append(orc.render(rp, nthreads=ORACLE_THREADS)); alone_c.append(orc.counters())
    rp.tile_rank, rp.tile_world = 0, 1
    films = []
    for tiles in ([0, 4, 5], [1, 2, 3]):
        film = g.render_tiles(rp, (0, rp.spp), tiles); gc = g.counters()
        want, want_c = None, None
        for t in tiles:
            want = alone[t].copy() if want is None else want + alone[t]
            want_c = add_counters(want_c, alone_c[t])
        assert_same_render(film, want, gc, want_c, weights=2e-6)
        films.append(film)
    assert_same_film(films[0] + films[1], whole, weights=2e-6)


def test_lists_times_ranges(pkg, gpu):
    sd, rp = range_scene(pkg, xres=40, yres=24, spp_per_pass=3)
    assert rp.spp == 8
    g = pkg.Scene(gpu, sd)
    whole = g.render(rp); wc = g.counters()
    film, total = None, None
    for tiles in ([0, 2, 3], [1, 4, 5]):
        for first, n in ((0, 5), (5, 3)):
            film = g.render_tiles(rp, (first, n), tiles, film=film)
            total = add_counters(total, g.counters())
            gen = [s for s in g.kernel_stats() if s["name"] == "generate"][0]
            assert gen["items"] == len(tiles) * 256 * n and gen["launches"] == -(-n // 3)
    assert_same_render(film, whole, total, wc)


def test_bad_lists_are_refused_and_leave_the_film_alone(pkg, gpu, oracle):
    A = pkg._abi
    sd, rp = range_scene(pkg, xres=40, yres=24)
    g = pkg.Scene(gpu, sd); orc = oracle.scene(sd)
    ref = orc.render(rp, nthreads=ORACLE_THREADS); oc = orc.counters()
    assert_same_render(g.render(rp), ref, g.counters(), oc)   # a normal render: counters and stats to go stale
    film = np.full((24, 40, 4), 7.0, np.float32)
    ptr = film.ctypes.data_as(C.c_void_p)

    def call(tiles, n=None):
        arr = np.array([] if tiles is None else tiles, np.uint32)
        return gpu.lib.pt_render_tiles(g.h, C.byref(rp), 0, rp.spp, arr.ctypes.data_as(A.u32p) if tiles is not None else None, len(arr) if n is None else n, ptr, 0)

    for bad in ([4, 1], [1, 1, 4], [1, 6], [0, 2 ** 32 - 1]):   # descending, repeated, out of range
        assert call(bad) == A.PT_ERR_INVALID_ARG, bad
        assert (film == 7.0).all()
    assert call(None, n=2) == A.PT_ERR_INVALID_ARG and (film == 7.0).all()
    rp.tile_world = 2
    assert call([1, 4]) == A.PT_ERR_INVALID_ARG and (film == 7.0).all()
    rp.tile_world = 1
    assert gpu.lib.pt_render_tiles(g.h, C.byref(rp), 6, 3, np.array([1], np.uint32).ctypes.data_as(A.u32p), 1, ptr, 0) == A.PT_ERR_INVALID_ARG   # a bad range, as pt_render_samples
    assert (film == 7.0).all()
    # the empty list: PT_OK, the film untouched, zeroed counters and no launches -- not those of the render before it
    assert call([]) == A.PT_OK and call(None, n=0) == A.PT_OK
    assert (film == 7.0).all()
    assert _all_zero(g.counters()), g.counters()
    assert sum(s["launches"] for s in g.kernel_stats()) == 0, g.kernel_stats()
    # ... and the handle renders on as before
    assert_same_render(g.render(rp), ref, g.counters(), oc)
