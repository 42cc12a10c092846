"""pt_tiles_select (k_tiles_select) against a numpy model (tile_scene.select_model): no render, the tile errors are a torch tensor on the device. The model maps a
sample tile to the film tiles its footprint meets in float32 with the kernel's ceil / floor; the comparison is exact -- the selection is a list of integers."""
import ctypes as C

import numpy as np
import pytest
from tile_scene import footprint, grid_of, select_model, with_filter

pytestmark = pytest.mark.gpu
THRESHOLD = 0.25


@pytest.fixture(scope="module")
def any_scene(pkg, gpu):
    sd, _ = pkg.scenes.ganesha_scale(n=4, xres=16, yres=16, spp=1, env=False).world_end()
    return pkg.Scene(gpu, sd)


def params(pkg, xres, yres, kind, radius):
    b = pkg.host.SceneBuilder(); b.film.update(xres=xres, yres=yres)
    return with_filter(pkg, b.render_params(), kind, radius)


def errors(n, seed):
    """Tile errors around the threshold: below, above, exactly equal to it (not selected) and NaN (selected)."""
    rng = np.random.default_rng(seed)
    e = rng.uniform(0.0, 2.0 * THRESHOLD, n).astype(np.float32)
    k = rng.permutation(n)
    e[k[: max(1, n // 6)]] = THRESHOLD
    if seed % 2:
        e[k[-max(1, n // 16):]] = np.nan
    return e


def run(g, rp, e, candidates):
    import torch
    d = torch.from_numpy(e).to("cuda:0")
    torch.cuda.synchronize()
    a = g.select_tiles(rp, d.data_ptr(), THRESHOLD, candidates)
    b = g.select_tiles(rp, d.data_ptr(), THRESHOLD, candidates)
    assert np.array_equal(a, b)   # deterministic: two calls, one list
    assert (np.diff(a.astype(np.int64)) > 0).all()   # ascending
    return a


@pytest.mark.parametrize("kind,radius", [("box", 0.5), ("gaussian", 2.0), ("gaussian", 2.5), ("gaussian", 10.0)])
def test_small_grids_where_the_two_tile_grids_part(pkg, any_scene, kind, radius):
    g = any_scene
    rp = params(pkg, 40, 24, kind, radius)
    ntx, nty = grid_of(rp)
    if radius == 0.5:   # the box filter: a tile's footprint is the tile
        assert all(select_model(rp, np.eye(6, dtype=np.float32)[t], 0.5, None).tolist() == [t] for t in range(6))
    if radius == 2.5:   # tile edge + radius on a pixel centre: the pixels only an edge sample reaches are left out, the footprints are those of radius 2
        assert [footprint(rp, t) for t in range(6)] == [footprint(params(pkg, 40, 24, kind, 2.0), t) for t in range(6)]
    if radius == 10.0:   # a 4x3 sample grid over the 3x2 film grid: tile 2's footprint, pixels 12 .. 39, meets all three film-tile columns
        assert max((footprint(rp, t)[2] - 1) // 16 - footprint(rp, t)[0] // 16 for t in range(ntx * nty)) == 2
    n_sel = set()
    for seed in range(12):
        e = errors(6, seed)
        for cand in (None, [], [t for t in range(ntx * nty) if (seed >> (t % 3)) & 1]):
            got = run(g, rp, e, cand)
            want = select_model(rp, e, THRESHOLD, cand)
            assert np.array_equal(got, want), (seed, cand, e, got, want)
            n_sel.add(len(got))
    assert len(n_sel) > 2
    # all below (or equal): nothing; all NaN: everything
    assert len(run(g, rp, np.full(6, THRESHOLD, np.float32), None)) == 0
    assert np.array_equal(run(g, rp, np.full(6, np.nan, np.float32), None), np.arange(ntx * nty))
    names = {s["name"]: s["kernel"] for s in g.kernel_stats()}
    assert names["tiles_select"] == "k_tiles_select"


@pytest.mark.parametrize("kind,radius", [("box", 0.5), ("gaussian", 2.0)])
def test_a_1080p_grid_in_many_chunks(pkg, any_scene, kind, radius):
    g = any_scene
    rp = params(pkg, 1920, 1080, kind, radius)
    ntx, nty = grid_of(rp)
    n = ntx * nty
    assert n == (8160 if kind == "box" else 121 * 68)
    rng = np.random.default_rng(7)
    for seed, count in enumerate([0, 1, 63, 64, 257, None]):
        e = errors(120 * 68, seed)
        cand = None if count is None else np.sort(rng.choice(n, count, replace=False)).astype(np.uint32)
        got = run(g, rp, e, cand)
        want = select_model(rp, e, THRESHOLD, cand)
        print(kind, "candidates", count, "selected", len(got), "model", len(want))
        assert len(got) == len(want) and np.array_equal(got, want)
        assert count in (0, 1) or 0 < len(got) < (n if count is None else count)
    assert len(run(g, rp, np.zeros(120 * 68, np.float32), None)) == 0


def test_select_refuses_bad_arguments(pkg, gpu, any_scene):
    import torch
    A = pkg._abi
    g = any_scene
    rp = params(pkg, 40, 24, "box", 0.5)
    d = torch.zeros(6, dtype=torch.float32, device="cuda:0"); torch.cuda.synchronize()
    out = np.full(8, 99, np.uint32); n_out = C.c_uint32(99)
    call = lambda err, cand, n, o=out: gpu.lib.pt_tiles_select(g.h, C.byref(rp), C.c_void_p(err), 0.0, None if cand is None else np.array(cand, np.uint32).ctypes.data_as(A.u32p), n,
                                                               o.ctypes.data_as(A.u32p) if o is not None else None, C.byref(n_out))
    for cand in ([3, 1], [2, 2], [1, 6]):
        assert call(d.data_ptr(), cand, len(cand)) == A.PT_ERR_INVALID_ARG
    assert call(None, [1], 1) == A.PT_ERR_INVALID_ARG and call(d.data_ptr(), [1], 1, None) == A.PT_ERR_INVALID_ARG
    assert (out == 99).all() and n_out.value == 99
