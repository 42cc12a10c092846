"""The lightmap's model (tests/lightmap_reference.py) against what is known in closed form, without a GPU: the model is what the device is held against bit for bit
(tests/test_bake_light.py), so it has to be right on its own account."""
import numpy as np
import pytest
import lightmap_reference as LM
import lightmap_scenes as LS

F = np.float32
W = H = 16


def floor_xy():
    """World x, y (H, W) of the texel centres of bake_scenes.floor: UVs 0 .. 1 over [-2, 2]^2."""
    u = (np.arange(W) + 0.5) / W * 4.0 - 2.0
    return np.broadcast_to(u[None, :], (H, W)), np.broadcast_to(u[:, None], (H, W))


def test_a_point_light_over_the_floor_gives_the_inverse_square_cosine_law(pkg, oracle):
    """E = I h / (x^2 + y^2 + h^2)^(3/2) at offset (x, y) from the point under the light: to 1e-5 relative -- about fifteen float32 roundings (6e-8 each) along
    the interaction, the light sample, the cosine and the resolve, with a tenfold margin."""
    I, at = (3.0, 2.0, 1.0), (0.3, 0.2, 1.5)
    sd, shape = LS.scene(pkg, "open_floor", [lambda b: LS.point(b, at=at, I=I)])
    got = LM.bake(oracle, pkg, sd, sd.prim_group == shape, W, H, 1)
    assert (got["owner"] != 0xFFFFFFFF).all() and got["n_rays"] == W * H and not got["occluded"].any()
    irr, reached = LM.resolve(got["light_w"], 1, 1)
    x, y = floor_xy()
    want = at[2] / ((x - at[0]) ** 2 + (y - at[1]) ** 2 + at[2] ** 2) ** 1.5
    for c in range(3):
        assert np.abs(irr[..., c] / (I[c] * want) - 1.0).max() <= 1e-5
    assert (reached == 1).all()


def test_a_distant_light_gives_l_cos(pkg, oracle):
    frm, L = np.array([0.3, 0.5, 1.0]), (1.0, 0.9, 0.8)
    sd, shape = LS.scene(pkg, "open_floor", [lambda b: LS.distant(b, frm=tuple(frm), L=L)])
    got = LM.bake(oracle, pkg, sd, sd.prim_group == shape, W, H, 2)
    irr, _ = LM.resolve(got["light_w"], 2, 1)
    cos = frm[2] / np.sqrt((frm ** 2).sum())
    for c in range(3):
        assert np.abs(irr[..., c] / (L[c] * cos) - 1.0).max() <= 1e-5


def test_under_the_box_it_is_dark_and_a_light_below_the_floor_adds_nothing(pkg, oracle):
    """bake_scenes.occluded_floor's box spans [-1.2, -0.2] x [-0.9, 0.1] at z 0.3 .. 0.8: under a point light straight above its centre the texels below it get
    nothing, the open ones do; the fully alpha-masked triangle over half the floor occludes nothing. The same light below the floor reaches no texel: one-sided."""
    sd, shape = LS.scene(pkg, "occluded_floor", [lambda b: LS.point(b, at=(-0.7, -0.4, 2.0))])
    got = LM.bake(oracle, pkg, sd, sd.prim_group == shape, W, H, 1)
    irr, reached = LM.resolve(got["light_w"], 1, 1)
    x, y = floor_xy()
    under = (x > -1.2) & (x < -0.2) & (y > -0.9) & (y < 0.1)
    assert under.sum() >= 9 and (irr[under] == 0).all() and (reached[under] == 0).all()
    masked = (x > 0.0) & (x < 1.2) & (y > 0.5) & (y < 1.0)   # their rays to the light cross the alpha-masked triangle (at z = 0.4, a fifth of the way) and nothing else
    assert masked.sum() >= 9 and (reached[masked] == 1).all()
    assert got["n_rays"] == W * H and 0 < got["occluded"].sum() < W * H
    sd, shape = LS.scene(pkg, "open_floor", [lambda b: LS.point(b, at=(0.3, 0.2, -1.0))])
    below = LM.bake(oracle, pkg, sd, sd.prim_group == shape, W, H, 1)
    assert below["n_rays"] == 0 and not below["light_w"].any()
    irr, reached = LM.resolve(below["light_w"], 1, 1)
    assert not irr.any() and not reached.any()


def test_the_round_robin_gives_every_light_the_same_number_of_samples():
    for n_lights, lights, spp, ns in ((8, None, 2, 8), (8, None, 4, 2), (8, [1, 4, 6], 3, 1), (3, None, 2, 6), (5, [0, 2], 1, 70)):
        sel = LM.selected_lights(n_lights, lights)
        s, k = np.divmod(np.arange(spp * ns), ns)
        light = LM.light_of(sel, s * ns + k, ns)
        assert set(light) == set(sel) and (np.bincount(light, minlength=n_lights)[sel] == spp * ns // len(sel)).all()
        assert (light[:len(sel)] == sel).all()   # ascending, from the first sample number on
    assert (LM.selected_lights(4, np.array([0, 1, 1, 0], np.uint8)) == [1, 2]).all()


def test_resolve_divides_by_the_sample_counts():
    lw = np.zeros((2, 3, 4), F)
    lw[0, 0] = (3.0, 6.0, 9.0, 4.0); lw[1, 2] = (0.0, 0.0, 0.0, 2.0)
    irr, reached = LM.resolve(lw, 3, 2)
    assert irr[0, 0].tolist() == [1.0, 2.0, 3.0] and reached[0, 0] == F(4.0) / F(6.0) and reached[1, 2] == F(2.0) / F(6.0)
    assert not irr[1, 1].any() and reached[1, 1] == 0 and irr.dtype == F and reached.dtype == F
