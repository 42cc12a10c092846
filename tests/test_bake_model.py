"""The numpy model of the bake's contract (tests/bake_reference.py) against cases computed by hand. No GPU."""
import numpy as np
import bake_reference as M
import bake_scenes as S

F = np.float32
NONE = 0xFFFFFFFF


def test_a_diagonal_through_texel_centres_goes_to_the_lower_id():
    """The unit quad as triangles (0,0)(1,0)(1,1) and (0,0)(1,1)(0,1): on u = v the first has b1 = (c - c) / 1 = 0 and the second b2 = 0, both exactly, so both
    contain the centres of the diagonal and the lower-numbered primitive owns them -- whichever order the triangles come in."""
    uv = np.array([[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]], F)
    x, y = np.meshgrid(np.arange(16), np.arange(16))
    for prims in ([4, 9], [9, 4]):
        owner = M.owner_map(uv, np.array(prims, np.uint32), 16, 16)
        first_wins = prims[0] < prims[1]   # the first triangle holds u >= v, the second u <= v
        assert np.array_equal(owner == prims[0], (x >= y) if first_wins else (x > y))
        assert np.array_equal(owner == prims[1], (x < y) if first_wins else (x <= y))
        assert np.array_equal(np.diag(owner), np.full(16, min(prims), np.uint32))
        assert (owner != NONE).all()
    # a 24 x 8 atlas: the centre ((x + .5) / 24, (y + .5) / 8) is on the diagonal where x = 3 y + 1
    owner = M.owner_map(uv, np.array([0, 1], np.uint32), 24, 8)
    for yy in range(8):
        assert owner[yy, 3 * yy + 1] == 0 and owner[yy, 3 * yy] == 1 and owner[yy, 3 * yy + 2] == 0


def test_a_triangle_with_zero_determinant_owns_nothing():
    for tri in ([(0.1, 0.1), (0.5, 0.5), (0.9, 0.9)], [(0.3, 0.3), (0.3, 0.3), (0.8, 0.1)], [(0.5, 0.5)] * 3):
        owner = M.owner_map(np.array([tri], F), np.array([0], np.uint32), 16, 16)
        assert (owner == NONE).all()
    inside, b0, b1, b2 = M.barycentrics((0, 0), (1, 0), (0, 1), F(0.25), F(0.5))
    assert inside and (b0, b1, b2) == (F(0.25), F(0.25), F(0.5))
    assert not M.barycentrics((0, 0), (1, 0), (0, 1), F(0.75), F(0.5))[0]
    # outside [0, 1]: not wrapped, and a sub-texel triangle between centres owns nothing
    assert (M.owner_map(np.array([[(1.2, 1.2), (1.9, 1.2), (1.2, 1.9)]], F), np.array([0], np.uint32), 16, 16) == NONE).all()
    assert (M.owner_map(np.array([[(0.501, 0.501), (0.53, 0.501), (0.501, 0.53)]], F), np.array([0], np.uint32), 16, 16) == NONE).all()


SLIVER = [(0.3680392, 0.27809554), (0.3954056, 0.32735506), (0.48162988, 0.4825588)]   # nearly collinear: det = 5.6e-9
BEHIND_SLIVER = [(0.45, 0.5), (0.7, 0.55), (0.5, 0.7)]


def test_a_sliver_owns_nothing_outside_its_texel_box():
    """The sliver's line passes through the centre of texel (34, 37) of a 64 x 64 atlas, far beyond its far vertex: with a determinant of a few 1e-9 the barycentrics
    there round to values >= 0. The contract's texel box -- x 22 .. 31, y 17 .. 31, from the UV bounds 23.55 .. 30.82 and 17.80 .. 30.88 texels with 0.5625 + 64 * 2.4e-7
    of margin -- denies it that texel, which the triangle behind keeps."""
    uv = np.array([SLIVER, BEHIND_SLIVER], F)
    assert M.texel_box(*uv[0], 64, 64) == (22, 31, 17, 31)
    inside = M.barycentrics(*uv[0], *M.texel_centres(64, 64))[0]
    assert inside[37, 34] and inside.sum() == 2
    boxed, unboxed = M.owner_map(uv, np.array([0, 1], np.uint32), 64, 64), M.owner_map(uv, np.array([0, 1], np.uint32), 64, 64, boxed=False)
    assert unboxed[37, 34] == 0 and boxed[37, 34] == 1 and (boxed != unboxed).sum() == 1 and (boxed == 0).sum() == 1
    # no box at all: a NaN bound, an infinite one, a box wholly outside; and a box is clamped to the atlas
    assert M.texel_box((0.1, 0.1), (np.inf, 0.2), (0.3, 0.9), 16, 16) is None and M.texel_box((1.2, 1.2), (1.9, 1.2), (1.2, 1.9), 16, 16) is None
    assert M.texel_box((-0.5, -0.2), (0.3, 0.1), (0.1, 2.0), 16, 16) == (0, 5, 0, 15)
    # a well-conditioned triangle loses nothing to its box
    for tri in ([(0, 0), (1, 0), (1, 1)], [(0.1, 0.1), (0.7, 0.15), (0.3, 0.8)], [(0.0, 0.02), (1.0, 0.97), (1.0, 0.99)]):
        for w, h in ((16, 16), (24, 8), (64, 64)):
            t = np.array([tri], F)
            assert np.array_equal(M.owner_map(t, np.array([0], np.uint32), w, h), M.owner_map(t, np.array([0], np.uint32), w, h, boxed=False))


def test_dilation_of_a_3x3_pattern():
    """Two owned texels in the top row, values 2 and 6. Iteration 1: (1,0) = (2 + 6) / 2 -- summed in the order (-1,0), (1,0) --, (0,1) = 2, (1,1) = (2 + 6) / 2,
    (2,1) = 6; the bottom row has no covered neighbour yet. Iteration 2: (0,2) = ((0,1) + (1,1)) / 2 = 3, (1,2) = (2 + 4 + 6) / 3 = 4, (2,2) = (4 + 6) / 2 = 5."""
    owner = np.full((3, 3), NONE, np.uint32); owner[0, 0] = 7; owner[0, 2] = 3
    plane = np.full((3, 3), -1.0, F); plane[0, 0] = 2.0; plane[0, 2] = 6.0
    assert np.array_equal(M.dilate(owner, plane, 0), plane)
    one = M.dilate(owner, plane, 1)
    assert np.array_equal(one, np.array([[2, 4, 6], [2, 4, 6], [-1, -1, -1]], F))
    two = M.dilate(owner, plane, 2)
    assert np.array_equal(two, np.array([[2, 4, 6], [2, 4, 6], [3, 4, 5]], F))
    assert np.array_equal(M.dilate(owner, plane, 5), two)
    rgb = np.stack([plane, plane * F(0.5), plane + F(1)], axis=-1)
    got = M.dilate(owner, rgb, 2)
    assert np.array_equal(got[..., 0], two) and np.array_equal(got[..., 1], two * F(0.5)) and np.array_equal(got[2, :, 2], np.array([4, 5, 6], F))
    empty = np.full((3, 3), NONE, np.uint32)
    assert np.array_equal(M.dilate(empty, plane, 4), plane)


def test_an_unoccluded_floor_gives_ao_1_under_cosine_sampling(pkg, oracle):
    """The floor's normal is +z and its frame vectors lie in the plane, so dot(wi, n) is the sampled wi.z exactly and a ray's weight is z / ((|z| * INV_PI) * nsamples):
    three roundings off pi / nsamples, and INV_PI itself is off 1 / pi by less than one. A texel's sum has N = spp * nsamples terms: N - 1 additions, each rounding
    a partial sum no larger than the total. pt_bake_resolve divides by the product spp * PI (one rounding, PI off pi by less than one) -- one more for the
    division. Relative error of the map: at most (N - 1 + 3 + 1 + 2 + 1) * 2^-24 = (N + 6) * 2^-24, to first order."""
    sd = S.open_floor(pkg)
    spp, ns = 3, 16
    out = M.bake(oracle, pkg, sd, sd.prim_group == 0, 16, 16, spp, ns, cos_sample=True)
    assert (out["owner"] != NONE).all() and out["n_rays"] == 256 * spp * ns and not out["occluded"].any()
    ao, bent = M.resolve(out["ao_w"], spp)
    n_terms = spp * ns
    bound = (n_terms + 6) * 2.0 ** -24
    print("max |ao - 1| =", float(np.abs(ao.astype(np.float64) - 1.0).max()), "bound", bound)
    assert np.abs(ao.astype(np.float64) - 1.0).max() <= bound
    assert (bent[..., 2] > 0.9).all() and np.allclose(np.linalg.norm(bent, axis=-1), 1.0, atol=1e-6)
    assert np.array_equal(out["normal"], np.broadcast_to(np.array([0, 0, 1], F), (16, 16, 3)))
    cu, cv = M.texel_centres(16, 16)
    assert np.allclose(out["position"][..., 0], cu * 4 - 2, atol=1e-6) and np.allclose(out["position"][..., 1], cv * 4 - 2, atol=1e-6)
    assert not M.resolve(np.zeros((2, 2, 4), F), 4)[0].any()
