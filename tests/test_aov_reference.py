"""The oracle-only facts the feature-buffer tests on the GPU (test_aov.py) lean on, so that the recipe cannot rot: with a matte surface of sigma 0, maxdepth 1 and one
distant light of L = pi, a camera sample's radiance is Kd * |dot(l, n)| of its first hit -- the film IS an albedo plane when l is the normal (identity 1) and a
projection of the normal plane otherwise (identity 2). The bound is the reference's own rounding per unit of filter weight, rounded up: 1e-6."""
import numpy as np
import pytest
from aov_reference import FOURTH_LIGHT, KD_CONST, LIGHTS, UP, albedo_scene, camera_hits, film_rgb_sums, hit_fractions, normal_scene
from tile_scene import with_filter

FLOOR = 1.0e-6   # per unit of a pixel's weight sum (measured on the oracle alone: 2.4e-7 for identity 1, 8.2e-7 at most for identity 2's prediction)
FILTERS = [("box", 0.5), ("gaussian", 2.0)]


def _render(pkg, oracle, sd, rp, filt):
    with_filter(pkg, rp, *filt)
    orc = oracle.scene(sd)
    film = orc.render(rp, nthreads=4)
    c = orc.counters()
    assert c["zero_radiance_paths_num"] == 0 and c["zero_radiance_paths_den"] > 0, c   # every hit is lit: nothing shadowed, nothing black
    return film


@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: f[0])
def test_constant_kd_film_is_the_albedo_plane(pkg, oracle, filt):
    sd, rp = albedo_scene(pkg, "const")
    film = _render(pkg, oracle, sd, rp, filt)
    rgb, w = film_rgb_sums(pkg, film), film[..., 3]
    hit, miss = hit_fractions(camera_hits(pkg, oracle, oracle.scene(sd), rp))
    assert hit >= 0.30 and miss >= 0.05, (hit, miss)
    # under the box filter a pixel whose samples all hit holds Kd * w; in general a pixel holds Kd * (the hits' weight), which is at most w
    full = rgb[..., 1] > 0.999 * KD_CONST[1] * w
    assert full.sum() > full.size // 4
    err = np.abs(rgb[full] - np.array(KD_CONST, np.float32) * w[full][:, None]) / w[full][:, None]
    print("identity 1, constant Kd, %s: largest error per unit weight %.3g" % (filt[0], err.max()))
    if filt[0] == "box":   # (w = number of samples; the hit count is a whole number, so `full` is exactly "every sample hits")
        assert err.max() <= FLOOR
    # any filter, any pixel: the three channels are Kd times ONE number, the hits' weight. Taken from green (error FLOOR * w / Kd.g), it predicts a channel c to
    # FLOOR * w * (1 + Kd.c / Kd.g)
    kd = np.array(KD_CONST, np.float64)
    lit = w > 0
    hits_w = rgb[..., 1].astype(np.float64) / kd[1]
    for c in (0, 2):
        e = np.abs(rgb[..., c] - kd[c] * hits_w)[lit] / w[lit]
        assert e.max() <= FLOOR * (1.0 + kd[c] / kd[1]), (c, e.max())
    assert (hits_w[lit] <= w[lit] * (1 + 1e-6)).all()


@pytest.mark.parametrize("surface", ["bump", "mesh"])
@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: f[0])
def test_a_fourth_light_is_predicted_from_three(pkg, oracle, filt, surface):
    """film_i.r = dot(l_i, sum of w * n) per pixel: three lights determine the sum, which predicts the render under a fourth."""
    films = []
    for light in LIGHTS + (FOURTH_LIGHT,):
        sd, rp = normal_scene(pkg, surface, light)
        films.append(_render(pkg, oracle, sd, rp, filt))
    hit, miss = hit_fractions(camera_hits(pkg, oracle, oracle.scene(sd), rp))
    assert hit >= 0.30 and miss >= 0.05, (hit, miss)
    r = np.stack([film_rgb_sums(pkg, f)[..., 0] for f in films], -1).astype(np.float64)   # (H, W, 4)
    w = films[0][..., 3].astype(np.float64)
    for f in films[1:]:
        np.testing.assert_allclose(f[..., 3], films[0][..., 3], rtol=1e-6)   # (tiles merged by several threads: the order of a wide filter's additions varies)
    n_sum = r[..., :3] @ np.linalg.inv(np.array(LIGHTS)).T
    predicted = n_sum @ np.array(FOURTH_LIGHT)
    lit = w > 0
    err = np.abs(predicted[lit] - r[..., 3][lit]) / w[lit]
    print("identity 2, %s, %s: largest error of the fourth light's prediction per unit weight %.3g" % (surface, filt[0], err.max()))
    assert err.max() <= FLOOR
    # the normals are no constant: the prediction is a test of the three lights, not of a flat floor
    tilt = np.linalg.norm(n_sum[lit][:, [0, 2]], axis=1) / w[lit]
    assert tilt.max() > 0.02, tilt.max()
