"""The SH points' model (tests/sh_reference.py) against what is known in closed form, without a GPU: the model is what the device is held against bit for bit
(tests/test_bake_sh.py), so it has to be right on its own account."""
import numpy as np
import bake_reference as M
import lightmap_reference as LM
import lightmap_scenes as LS
import sh_reference as SR

F = np.float32


def basis64(w):
    """The contract's basis with its six-digit literals, in float64."""
    x, y, z = (np.asarray(w, np.float64)[..., i] for i in range(3))
    return np.stack([np.full(x.shape, 0.282095), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * x * y, 1.092548 * y * z, 0.315392 * (3.0 * z * z - 1.0), 1.092548 * x * z,
                     0.546274 * (x * x - y * y)], axis=-1)


# Points above the floor, each with every basis function well away from its zero crossings towards both test lights (a relative bound means nothing at a zero)
POINTS = np.array([[-1.1, 0.9, 0.3], [1.4, -0.5, 0.2], [0.9, 1.2, 0.9], [-0.6, -1.3, 0.5], [1.3, 1.6, 0.1]], F)


def test_a_point_light_gives_intensity_over_r_squared_times_the_basis(pkg, oracle):
    """sh[q, c] = (I_c / r^2) Y_q(w), w the unit vector to the light: to 1e-6 relative per coefficient against float64 arithmetic on the float32 inputs -- about
    ten float32 roundings (6e-8 each, half that on average) along p1 - p, its length, the division, I / r^2, the basis and the product."""
    I, at = (3.0, 2.0, 1.0), (0.3, 0.2, 1.5)
    sd, _ = LS.scene(pkg, "open_floor", [lambda b: LS.point(b, at=at, I=I)])
    got = SR.bake(oracle, pkg, sd, POINTS, 1, 1)
    assert got["n_rays"] == len(POINTS) and not got["occluded"].any()
    sh, reached = SR.resolve(got["sh_w"], 1, 1)
    pos = np.array(list(sd.lights[0].pos)[:3], F).astype(np.float64)
    v = pos[None, :] - POINTS.astype(np.float64)
    r2 = (v * v).sum(axis=1)
    Y = basis64(v / np.sqrt(r2)[:, None])
    assert (np.abs(Y) > 0.02).all()   # the points are what the docstring says
    for c in range(3):
        want = (I[c] / r2)[:, None] * Y
        assert np.abs(sh[:, :, c] / want - 1.0).max() <= 1e-6, np.abs(sh[:, :, c] / want - 1.0).max()
    assert (reached == 1).all()


def test_a_distant_light_gives_l_times_the_basis(pkg, oracle):
    frm, L = np.array([0.3, 0.5, 1.0]), (1.0, 0.9, 0.8)
    sd, _ = LS.scene(pkg, "open_floor", [lambda b: LS.distant(b, frm=tuple(frm), L=L)])
    got = SR.bake(oracle, pkg, sd, POINTS, 2, 1)
    sh, reached = SR.resolve(got["sh_w"], 2, 1)
    Y = basis64(frm / np.sqrt((frm ** 2).sum()))
    assert (np.abs(Y) > 0.02).all()
    for c in range(3):
        assert np.abs(sh[:, :, c] / (L[c] * Y)[None, :] - 1.0).max() <= 1e-6
    assert (reached == 1).all()
    # a point under the floor: its sample contributes (there is no side test), and the floor is in between
    under = SR.bake(oracle, pkg, sd, np.array([[0.1, 0.2, -0.5]], F), 1, 1)
    assert under["n_rays"] == 1 and under["occluded"].all() and not under["sh_w"].any()


def test_behind_the_box_it_is_dark(pkg, oracle):
    """bake_scenes.occluded_floor's box spans [-1.2, -0.2] x [-0.9, 0.1] at z 0.3 .. 0.8: under a point light straight above its centre a point below it gets
    nothing, one beside it everything."""
    sd, _ = LS.scene(pkg, "occluded_floor", [lambda b: LS.point(b, at=(-0.7, -0.4, 2.0))])
    pts = np.array([[-0.7, -0.4, 0.15], [0.5, -0.2, 0.15], [-0.9, -0.1, 0.2]], F)
    got = SR.bake(oracle, pkg, sd, pts, 2, 1)
    sh, reached = SR.resolve(got["sh_w"], 2, 1)
    assert got["n_rays"] == 6 and got["occluded"].sum() == 4
    assert not sh[0].any() and reached[0] == 0 and not sh[2].any() and reached[2] == 0 and not got["sh_w"][0].any()
    assert reached[1] == 1 and sh[1, 0, 0] > 0


def test_the_round_robin_gives_every_light_the_same_number_of_samples_at_every_point():
    for n_lights, lights, spp, ns in ((8, None, 2, 8), (8, None, 4, 2), (8, [1, 4, 6], 3, 1), (3, None, 2, 6), (5, [0, 2], 1, 70)):
        sel = LM.selected_lights(n_lights, lights)
        pt, s, k = M.sample_list(np.arange(3), spp, ns)
        light = LM.light_of(sel, s * ns + k, ns)
        for t in range(3):
            mine = light[pt == t]
            assert (np.bincount(mine, minlength=n_lights)[sel] == spp * ns // len(sel)).all() and (mine[:len(sel)] == sel).all()
        assert (light[pt == 0] == light[pt == 2]).all()   # the light of a sample does not depend on the point
    assert SR.default_row(1) == 1 and SR.default_row(64) == 8 and SR.default_row(65) == 9 and SR.default_row(130) == 12


def test_the_irradiance_of_one_distant_light_is_the_addition_theorems(pkg):
    """sh[q] = L Y_q(w): E(nrm) / L = 1/4 + cos g / 2 + (5/16)(3 cos^2 g - 1) / 2, cos g = dot(nrm, w) -- the order-2 fit of the clamped cosine. To 1e-5 absolute
    per unit L: the six-digit literals are off by at most 1.4e-6 relative, their products by 3e-6; float32 rounding over about 30 operations adds about 2e-6.
    This pins all nine basis functions, their constants and the three A factors."""
    rng = np.random.RandomState(12)
    unit = lambda v: v / np.sqrt((v * v).sum(axis=1))[:, None]
    w = unit(rng.normal(size=(40, 3))); nrm = unit(rng.normal(size=(40, 3)))
    e1 = unit(np.cross(w[:3], [[0.3, -0.5, 0.8]] * 3))
    w = np.concatenate([w, w[:3], w[:3], w[:3]]); nrm = np.concatenate([nrm, w[:3], e1, -w[:3]])   # facing the light, at right angles, facing away
    w32, n32 = w.astype(F), nrm.astype(F)
    L = np.array([1.0, 0.5, 2.0], F)
    sh = (SR.basis(w32)[:, :, None] * L[None, None, :]).astype(F)
    cg = (w32.astype(np.float64) * n32.astype(np.float64)).sum(axis=1)
    want = 0.25 + cg / 2 + (5.0 / 16.0) * (3 * cg * cg - 1) / 2
    for got in (SR.irradiance(sh, n32), pkg.runtime.sh_irradiance(sh, n32)):
        assert np.abs(got / L[None, :] - want[:, None]).max() <= 1e-5, np.abs(got / L[None, :] - want[:, None]).max()
    got = SR.irradiance(sh, n32)[:, 0]
    assert np.abs(got[40:43] - 17.0 / 16.0).max() <= 1e-5 and np.abs(got[43:46] - 3.0 / 32.0).max() <= 1e-5 and np.abs(got[46:49] - 1.0 / 16.0).max() <= 1e-5
    assert SR.irradiance(sh, n32).tobytes() == pkg.runtime.sh_irradiance(sh, n32).tobytes()


def test_resolve_divides_by_the_sample_counts():
    w = np.zeros((3, 28), F)
    w[0, :27] = np.arange(27) * 3.0; w[0, 27] = 4.0; w[2, 27] = 2.0
    sh, reached = SR.resolve(w, 3, 2)
    assert sh.shape == (3, 9, 3) and sh[0].reshape(-1).tolist() == list(np.arange(27.0)) and reached[0] == F(4.0) / F(6.0) and reached[2] == F(2.0) / F(6.0)
    assert not sh[1].any() and reached[1] == 0 and sh.dtype == F and reached.dtype == F
