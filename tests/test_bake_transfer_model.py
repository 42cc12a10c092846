"""The model of the transfer bake (tests/transfer_reference.py) against cases worked out by hand, and the scenes of the GPU tests (tests/transfer_scenes.py) against
what those tests need of them. No GPU: the hits come from the oracle's closest-hit query."""
import numpy as np
import pytest
import bake_reference as M
import transfer_reference as T
import transfer_scenes as X

F = np.float32
NONE = 0xFFFFFFFF
R = float(np.sqrt(0.5))


def model(oracle, pkg, target, source, w, h, front, back, **kw):
    return T.transfer(oracle, pkg, target, source, target.prim_group == 0, w, h, front, back, **kw)


def test_a_parallel_quad_a_quarter_below(pkg, oracle):
    """The source lies 0.25 under the target: t = front + 0.25 (front = 0.25: the ray's length to the plane is 0.5, a power of two) and height = front - t, in float32
    exactly; the normal maps to (0, 0, 1)."""
    front = F(0.25)
    m = model(oracle, pkg, X.quad_target(pkg), X.plane_source(pkg, z=-0.25), 16, 16, 0.25, 0.5)
    own = m["owner"] != NONE   # (the UVs span [0.05, 0.95]: the atlas' outermost ring has no owner)
    assert own.sum() == 14 * 14 and np.array_equal(m["detail"], own)
    # height = front - t in float32 exactly, for the t the closest-hit query reports. That t is 0.5 = front + 0.25 up to the two roundings of Triangle::intersect's
    # t = t_scaled * (1 / det): 2 ulp of the binade below 0.5, 2^-24
    t = np.array([m["t"][int(k)] for k in m["rays"]["texel"]], F)
    assert (m["height"].reshape(-1)[m["rays"]["texel"]] == front - t).all() and m["height"].dtype == F and not m["height"][~own].any()
    assert np.abs(t - (front + F(0.25))).max() <= 2.0 ** -24
    assert np.abs(m["height"][own] - (front - (front + F(0.25)))).max() <= 2.0 ** -24
    assert (m["tangent_normal"][own] == np.array([0, 0, 1], F)).all() and (m["src_normal"][own] == np.array([0, 0, 1], F)).all() and not m["tangent_normal"][~own].any()
    assert np.abs(m["src_position"][own][:, 2] - F(-0.25)).max() <= 2.0 ** -24   # (b0 z0 + b1 z1 + b2 z2 with b0 + b1 + b2 = 1 up to its two roundings)
    cu, cv = M.texel_centres(16, 16)
    assert np.abs(m["src_position"][..., 0] - ((cu - 0.05) / 0.9 * 2 - 1))[own].max() < 1e-6 and np.abs(m["src_position"][..., 1] - ((cv - 0.05) / 0.9 * 2 - 1))[own].max() < 1e-6
    assert (m["rays"]["d"] == np.array([0, 0, -1], F)).all() and (m["rays"]["o"][:, 2] == front).all() and (m["rays"]["t_max"] == F(0.75)).all() and len(m["rays"]["texel"]) == 196


def test_a_source_facing_away_is_turned_toward_the_ray(pkg, oracle):
    down = X.plane_source(pkg, z=0.1, tilt=180.0)   # (its normal looks down: away from where the rays come from)
    m = model(oracle, pkg, X.quad_target(pkg), down, 8, 8, 0.25, 0.25)
    d = m["detail"]
    assert d.all() and np.abs(m["src_normal"][d] - np.array([0, 0, 1], F)).max() < 1e-6


def test_a_plane_tilted_45_degrees_about_dpdu(pkg, oracle):
    """The target's dpdu runs along x, dpdv along y. A source turned by 45 degrees about x rises with y: its normal is (0, -r, r) in both frames, the height is y."""
    m = model(oracle, pkg, X.quad_target(pkg), X.plane_source(pkg, z=0.0, tilt=45.0), 16, 16, 1.5, 1.5)
    d = m["detail"]
    assert d.sum() == 14 * 14
    assert np.abs(m["tangent_normal"][d] - np.array([0, -R, R], F)).max() < 1e-6 and np.abs(m["src_normal"][d] - np.array([0, -R, R], F)).max() < 1e-6
    y = (M.texel_centres(16, 16)[1] - 0.05) / 0.9 * 2 - 1
    assert np.abs(m["height"] - y)[d].max() < 1e-5 and np.abs(m["src_position"][..., 2] - y)[d].max() < 1e-5


def test_a_mirrored_island_flips_the_second_component(pkg, oracle):
    """Both islands lie in z = 0 under one tilted source. In the island whose v runs against y the frame's second vector is turned round (dot(tv, dpdv) < 0), so the
    tangent normal's second component has the other sign there; the first and third do not change."""
    src = X.plane_source(pkg, z=0.0, tilt=45.0)
    m = model(oracle, pkg, X.mirrored_target(pkg), src, 16, 16, 1.5, 1.5)
    left, right = np.isin(m["owner"], (0, 1)), np.isin(m["owner"], (2, 3))
    assert left.sum() > 40 and right.sum() > 40 and m["detail"][left | right].all()
    assert np.abs(m["tangent_normal"][left] - np.array([0, -R, R], F)).max() < 1e-6
    assert np.abs(m["tangent_normal"][right] - np.array([0, R, R], F)).max() < 1e-6
    assert np.abs(m["src_normal"][left | right] - np.array([0, -R, R], F)).max() < 1e-6   # (world space: the same in both)


def test_a_source_beyond_back_is_a_miss(pkg, oracle):
    m = model(oracle, pkg, X.quad_target(pkg), X.plane_source(pkg, z=-0.25), 16, 16, 0.25, 0.2)   # the ray ends at z = -0.2
    assert (m["owner"] != NONE).sum() == 196 and (m["hit_prim"] == NONE).all() and not m["detail"].any() and set(m["kinds"].values()) == {"miss"}
    for k in ("height", "src_position", "src_normal", "tangent_normal", "ao_w"):
        assert not m[k].any(), k


def test_a_degenerate_uv_target_triangle_takes_the_fallback_partials(pkg, oracle):
    """A UV sliver owns the one texel whose centre is its vertex; its dpdu and dpdv are coordinate_system's of cross(p2 - p0, p1 - p0) = (0, 0, -1), normalised: (0, -1, 0) and
    (-1, 0, 0), not the x direction its UVs suggest. The tilted source's normal (0, -r, r) therefore shows in the FIRST component; tv = cross(ns, sv) = (1, 0, 0) is turned
    round to dpdv's side."""
    sd = X.degenerate_uv_target(pkg)
    dpdu, dpdv = T.partials(sd, 0)
    assert np.array_equal(dpdu, np.array([0, -1, 0], F)) and np.array_equal(dpdv, np.array([-1, 0, 0], F))
    m = model(oracle, pkg, sd, X.plane_source(pkg, z=0.0, tilt=45.0), 5, 5, 1.5, 1.5)
    assert (m["owner"] != NONE).sum() == 1 and m["owner"][2, 2] == 0 and m["detail"][2, 2]
    assert np.abs(m["tangent_normal"][2, 2] - np.array([R, 0, R], F)).max() < 1e-6
    assert np.abs(m["src_position"][2, 2] - np.array([1, 0, 0], F)).max() < 1e-6


def test_a_normal_along_dpdu_takes_coordinate_system(pkg):
    """Step 4's own fallback: a shading normal along dpdu leaves no tangent."""
    ns = np.array([1, 0, 0], F)
    sv, tv, fell = T.tangent_frame(dict(dpdu=np.array([2, 0, 0], F)), np.array([0, 1, 0], F), ns)
    want = M.coordinate_system(ns)
    assert fell and np.array_equal(sv, want[0]) and np.array_equal(tv, want[1])


@pytest.mark.parametrize("size", [(16, 16), (24, 8)])
@pytest.mark.parametrize("back", [0.3, 0.02])
@pytest.mark.parametrize("target", ["smooth", "mirrored"])
def test_the_gpu_cases_reach_what_they_are_about(pkg, oracle, target, back, size):
    """Each grid case has detail hits on at least a quarter of the owned texels and at least one miss; the clipped range misses more; the mixed source is hit on its
    sphere and on its instance."""
    w, h = size
    tg = X.quad_target(pkg, smooth=True) if target == "smooth" else X.mirrored_target(pkg)
    counts = {}
    for normals in (False, True):
        m = model(oracle, pkg, tg, X.bump_source(pkg, normals), w, h, 0.3, back)
        owned = int((m["owner"] != NONE).sum())
        kinds = list(m["kinds"].values())
        assert owned > w * h // 2 and kinds.count("detail") * 4 >= owned and kinds.count("miss") >= 1 and kinds.count("other") == 0, (owned, kinds.count("detail"), kinds.count("miss"))
        counts[normals] = kinds.count("miss")
    if back == 0.02:
        wide = list(model(oracle, pkg, tg, X.bump_source(pkg), w, h, 0.3, 0.3)["kinds"].values()).count("miss")
        assert counts[False] > wide   # the short range clips part of the bump
    sd = X.mixed_source(pkg)
    m = model(oracle, pkg, tg, sd, w, h, 0.3, back)
    hit = m["hit_prim"][m["hit_prim"] != NONE]
    sphere = (sd.prim_shape[hit] >> np.uint32(30)) != 0
    instanced = ~T.top_level_triangles(sd)[hit] & ~sphere
    assert sphere.any() and instanced.any() and m["detail"].any()
    other = (m["hit_prim"] != NONE) & ~m["detail"]
    assert m["height"][other].all() and not m["src_position"][other].any() and not m["tangent_normal"][other].any()
