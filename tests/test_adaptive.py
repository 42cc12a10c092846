"""Adaptive sampling end to end: runtime.Scene.render_adaptive and `mi355pbrt --adaptive` over pt_render_tiles / pt_film_halves_error / pt_tiles_select.
The scene (tile_scene.background_scene) is 48x32 under the box filter -- a 3x2 tile grid on which the sample grid and the film grid coincide -- whose left third sees only
the black background: the halves error of tiles 0 and 3 is exactly 0 at every check. spp = 16, step = 2: a round is 4 samples, the first check comes at 4."""
import re
import subprocess

import numpy as np
import pytest
from conftest import trace_env
from parity import assert_same_counters, assert_same_film
from tile_scene import BACKGROUND_PBRT, background_scene, tile_pixels

pytestmark = pytest.mark.gpu
STEP = 2
BACKGROUND = [0, 3]
# The threshold of the finite case: above 0, the background's error, and below the largest tile error of every check, which the tests print (background_scene:
# 0.49 at 4 samples falling to 0.35 at 16; the scene file: 0.74 to 0.42) -- so the background stops at the first check and the worst tile renders the whole job.
THRESHOLD = 0.3
FRONT_THRESHOLD = 0.3


@pytest.fixture(scope="module")
def scene(pkg, gpu):
    sd, rp = background_scene(pkg)
    assert rp.spp == 16 and list(rp.sample_bounds) == [0, 0, 48, 32]
    return pkg.Scene(gpu, sd), rp


def inner(rp, tiles):
    """The pixels of the listed tiles minus each tile's one-pixel rim: a sample whose offset inside its pixel is exactly 0 lies on the pixel's corner and, under the box
    filter of radius 0.5, also feeds the neighbouring pixel (film.rs:134-150) -- across a tile border, a neighbour that may have another sample count."""
    mask = np.zeros_like(tile_pixels(rp, []))
    for t in tiles:
        m = tile_pixels(rp, [t])
        ys, xs = np.where(m)
        m[ys.min(), :] = m[ys.max(), :] = False; m[:, xs.min()] = m[:, xs.max()] = False
        mask |= m
    return mask


def test_background_tiles_stop_at_the_first_check_and_every_tile_holds_its_own_samples(scene):
    g, rp = scene
    rounds = []
    film, per_tile = g.render_adaptive(rp, THRESHOLD, STEP, on_round=lambda done, active, worst: rounds.append((done, list(active), worst)))
    print("samples per tile\n", per_tile, "\nrounds", rounds)
    counts = per_tile.reshape(-1)
    assert per_tile.shape == (2, 3) and per_tile.dtype == np.uint32
    assert (counts[BACKGROUND] == 2 * STEP).all()
    assert (counts >= 2 * STEP).all() and counts.max() > 2 * STEP
    assert rounds[0][0] == 2 * STEP and not set(BACKGROUND) & set(rounds[0][1])
    for (_, a, _), (_, b, _) in zip(rounds, rounds[1:]):
        assert set(b) <= set(a)   # the active set only shrinks
    for n in sorted(set(counts.tolist())):
        tiles = np.where(counts == n)[0]
        mask = inner(rp, tiles)
        whole = g.render(rp, samples=(0, n))
        assert mask.sum() >= 14 * 14 * len(tiles)
        assert_same_film(film[mask], whole[mask])
    assert (film[:, :16, :3] == 0).all()


def test_a_threshold_nothing_meets_is_the_whole_render(scene):
    """The selection keeps a tile iff not (error <= threshold). The background tiles' error is exactly 0, which IS <= 0: at threshold 0 they stop at the first check like
    at any other, and every lit tile (error > 0 at every check) renders the whole job. Below 0 nothing stops: the loop is g.render(rp), film and counters."""
    g, rp = scene
    whole = g.render(rp); wc = g.counters()
    film, per_tile = g.render_adaptive(rp, -1.0, STEP)
    assert (per_tile == rp.spp).all()
    assert_same_film(film, whole)
    assert_same_counters(g.adaptive_counters, wc)
    film0, per_tile0 = g.render_adaptive(rp, 0.0, STEP)
    counts = per_tile0.reshape(-1)
    lit = [t for t in range(6) if t not in BACKGROUND]
    assert (counts[lit] == rp.spp).all() and (counts[BACKGROUND] == 2 * STEP).all()
    assert_same_film(film0[inner(rp, lit)], whole[inner(rp, lit)])


def test_a_threshold_everything_meets_stops_at_the_first_check(scene):
    g, rp = scene
    film, per_tile = g.render_adaptive(rp, float("inf"), STEP)
    assert (per_tile == 2 * STEP).all()
    assert_same_film(film, g.render(rp, samples=(0, 2 * STEP)))
    # min_samples moves the first check
    assert (g.render_adaptive(rp, float("inf"), STEP, min_samples=7)[1] == 4 * STEP).all()


def test_mi355pbrt_adaptive_is_the_python_loop(pkg, gpu, tmp_path):
    fs = pkg.frontend.FrontScene(text=BACKGROUND_PBRT)
    rp = fs.render_params()
    g = pkg.Scene(gpu, fs)
    rounds = []
    film, per_tile = g.render_adaptive(rp, FRONT_THRESHOLD, STEP, on_round=lambda done, active, worst: rounds.append((done, len(active), worst)))
    print("samples per tile\n", per_tile, "\nrounds", rounds)
    assert per_tile.min() == 2 * STEP and per_tile.max() > 2 * STEP
    scene = tmp_path / "adaptive.pbrt"; scene.write_text(BACKGROUND_PBRT)
    out = tmp_path / "adaptive.pfm"
    r = subprocess.run([pkg.frontend.CLI_PATH, str(scene), "--outfile", str(out), "--adaptive", repr(FRONT_THRESHOLD), "--adaptive-step", str(STEP)],
                       capture_output=True, text=True, timeout=120, env=trace_env())
    assert r.returncode == 0, r.stderr
    img = pkg.frontend.read_image(str(out))
    np.testing.assert_allclose(img, g.resolve(film, scale=rp.scale), rtol=2e-6, atol=1e-7)
    m = re.search(r"adaptive: (\d+) of (\d+) tile-samples, (\d+) rounds", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) == int(per_tile.sum()) and int(m.group(2)) == 6 * rp.spp and int(m.group(3)) == len(rounds)
