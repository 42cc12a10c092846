"""The numpy model of the ID mattes (matte_reference.py) checks itself, without a GPU: invariance under cutting the sample range into calls, the weight balance, and
hand-made 2 x 2 films with known answers -- an overflowing ninth id, a tie in resolve, an edge sample under the box filter that reaches its neighbour. test_matte.py
holds the device against this model bit for bit."""
import numpy as np
import matte_reference as M
from aov_reference import NONE, camera_hits
from tile_scene import with_filter

F = np.float32


def _tables_of(pkg, oracle, sd, rp, cuts, groups):
    orc = oracle.scene(sd)
    tables = M.empty_tables(rp)
    count = 0
    for first, n in cuts:
        h = camera_hits(pkg, oracle, orc, rp, first, n)
        surface, ids = M.sample_ids(sd, h, groups)
        count += M.add_samples(rp, h, surface, ids, tables)
    orc.close()
    return tables, count


def test_tables_do_not_depend_on_how_the_range_is_cut(pkg, oracle):
    sd, rp = M.materials_scene(pkg)
    with_filter(pkg, rp, "gaussian", 2.0)
    groups = np.arange(len(sd.prim_material), dtype=np.uint32)
    whole, n_whole = _tables_of(pkg, oracle, sd, rp, [(0, 4)], groups)
    parts, n_parts = _tables_of(pkg, oracle, sd, rp, [(0, 1), (1, 2), (3, 1)], groups)
    assert n_whole == n_parts
    for layer in whole:
        assert whole[layer].tobytes() == parts[layer].tobytes(), layer
    # the scene is worth the comparison: several ids per pixel, background, and every material
    t = whole["material"]
    assert (t["n_ids"] >= 2).mean() > 0.2 and set(np.unique(t["id"][t["n_ids"] > 0][:, 0])) >= {1, 2, 3, 4}
    # sum(w) + w_other + background == w_total, up to rounding: the background is what the misses added, measured on its own
    orc = oracle.scene(sd)
    h = camera_hits(pkg, oracle, orc, rp)
    orc.close()
    surface, ids = M.sample_ids(sd, h, groups)
    keep = ~surface
    assert keep.any()
    background = _weights_of(rp, h, keep)
    for layer, t in whole.items():
        used = np.arange(M.SLOTS)[None, None, :] < t["n_ids"][..., None]
        total = np.where(used, t["w"], 0).astype(np.float64).sum(-1) + t["w_other"] + background
        np.testing.assert_allclose(total, t["w_total"], rtol=1e-5, atol=1e-6)
        assert (t["reserved"] == 0).all() and (t["w"][~used] == 0).all() and (t["id"][~used] == 0).all()


def _weights_of(rp, h, keep):
    """Per film pixel, the float64 sum of the filter weights of the kept samples (the model's footprint and table lookup, written once more in plain numpy)."""
    cb = list(rp.cropped_pixel_bounds)
    out = np.zeros((cb[3] - cb[1], cb[2] - cb[0]))
    rx, ry = F(rp.filter_radius[0]), F(rp.filter_radius[1])
    table = np.array(list(rp.filter_table), F)
    for i in np.nonzero(keep)[0]:
        dx, dy = F(h["pfilm"][i, 0]) - F(0.5), F(h["pfilm"][i, 1]) - F(0.5)
        for y in range(max(int(np.ceil(dy - ry)), cb[1]), min(int(np.floor(dy + ry)) + 1, cb[3])):
            for x in range(max(int(np.ceil(dx - rx)), cb[0]), min(int(np.floor(dx + rx)) + 1, cb[2])):
                iy = min(int(np.floor(np.abs((F(y) - dy) * (F(1.0) / ry) * F(16.0)))), 15); ix = min(int(np.floor(np.abs((F(x) - dx) * (F(1.0) / rx) * F(16.0)))), 15)
                out[y - cb[1], x - cb[0]] += table[iy * 16 + ix]
    return out


def _hand_made(samples, groups, radius=0.5, table=None):
    rp = M.fake_rp(2, 2, radius, table)
    h = M.fake_hits(rp, samples)
    sd = type("SD", (), {"prim_material": np.zeros(len(groups), np.uint32)})
    surface, ids = M.sample_ids(sd, h, groups)
    tables = M.empty_tables(rp, ("group",))
    return tables["group"], M.add_samples(rp, h, surface, ids, tables)


def test_a_ninth_id_overflows():
    """Ten samples in the middle of pixel (0, 0) with the ids 10 .. 18 and 10 again: eight slots in first-seen order, the ninth id in w_other, the repeat found."""
    centre = lambda p: [(0.5, 0.5, p), (1.5, 0.5, NONE), (0.5, 1.5, NONE), (1.5, 1.5, NONE)]
    t, count = _hand_made([centre(p) for p in list(range(9)) + [0]], groups=np.arange(10, 19, dtype=np.uint32))
    p = t[0, 0]
    assert count == 40 and p["n_ids"] == 8 and list(p["id"]) == list(range(10, 18))
    assert list(p["w"]) == [2.0] + [1.0] * 7 and p["w_other"] == 1.0 and p["w_total"] == 10.0
    for q in ((0, 1), (1, 0), (1, 1)):   # misses only: weight, no id
        assert t[q]["n_ids"] == 0 and t[q]["w_total"] == 10.0 and t[q]["w_other"] == 0.0 and not t[q]["w"].any()
    assert np.array_equal(M.mask(t, [10])[0], F([0.2, 0.0])) and np.array_equal(M.mask(t, [18, 11, 12]), F([[0.2, 0.0], [0.0, 0.0]]))


def test_resolve_breaks_ties_by_the_lower_id():
    centre = lambda p: [(0.5, 0.5, p), (1.5, 0.5, NONE), (0.5, 1.5, NONE), (1.5, 1.5, NONE)]
    t, _ = _hand_made([centre(p) for p in (2, 0, 1, 1)], groups=np.array([7, 5, 9], np.uint32))   # first seen: 9, 7, 5; weights 1, 1, 2
    assert list(t[0, 0]["id"][:3]) == [9, 7, 5]
    ids, cov = M.resolve(t, 4)
    assert list(ids[0, 0]) == [5, 7, 9, 0] and list(cov[0, 0]) == [0.5, 0.25, 0.25, 0.0]
    assert not ids[1, 1].any() and not cov[1, 1].any()


def test_an_edge_sample_under_the_box_filter_reaches_its_neighbour():
    """pfilm.x == 1 exactly: dx = 0.5, and ceil(0.5 - 0.5) .. floor(0.5 + 0.5) is the pixels 0 AND 1 (film.rs:300-307). The sample is pixel 1's (raster order: after pixel
    0's own sample of the same number), so pixel 0 sees its own id first."""
    row = [(0.25, 0.5, 0), (1.0, 0.5, 1), (0.5, 1.5, NONE), (1.5, 1.5, NONE)]
    t, count = _hand_made([row], groups=np.array([3, 4], np.uint32))
    assert count == 5
    assert list(t[0, 0]["id"][:2]) == [3, 4] and t[0, 0]["n_ids"] == 2 and t[0, 0]["w_total"] == 2.0
    assert list(t[0, 1]["id"][:1]) == [4] and t[0, 1]["n_ids"] == 1 and t[0, 1]["w_total"] == 1.0
    # and a corner sample reaches four pixels
    t, count = _hand_made([[(1.0, 1.0, 0), (1.5, 0.5, NONE), (0.5, 1.5, NONE), (1.5, 1.5, NONE)]], groups=np.array([3], np.uint32))
    assert count == 4 + 3 and (t["n_ids"] == 1).all() and (t["id"][..., 0] == 3).all()
