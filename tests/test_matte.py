"""pt_matte_render on the GPU against the numpy model of the contract (matte_reference.py) fed by the unchanged oracle's camera hits. Every comparison of tables is on
their raw bytes -- ids, n_ids, weights, w_total, w_other --: the ids are integers, the weights the filter table's entries for bit-exact pfilm values, and the order of the
additions is part of the contract. Every case is a 32 x 24 film at 4 spp: 2 x 2 sample tiles (more under the wide filter) with the lower row half full."""
import ctypes as C

import numpy as np
import pytest
import matte_reference as M
from aov_reference import NONE, camera_hits
from tile_scene import with_filter

pytestmark = pytest.mark.gpu


def _same(got, want, what=""):
    for layer in want:
        g, w = np.ascontiguousarray(got[layer]), np.ascontiguousarray(want[layer])
        if g.tobytes() != w.tobytes():
            bad = [f for f in w.dtype.names if not np.array_equal(g[f].view(np.uint32), w[f].view(np.uint32))]
            first = np.argwhere(g.view(np.uint8).reshape(g.shape + (80,)).astype(np.int16) - w.view(np.uint8).reshape(w.shape + (80,)) != 0)[0]
            pytest.fail("%s %s: tables differ in %s, first at pixel (y, x) = %s: got %s, want %s" % (what, layer, bad, tuple(first[:2]), g[tuple(first[:2])], w[tuple(first[:2])]))


def _prim_groups(sd):
    return np.arange(len(sd.prim_material), dtype=np.uint32)   # group = primitive index


# ---- 1, 9: several materials over a ground plane, box filter --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["sobol", "halton", "lens", "orthographic"])
def test_materials_and_groups_under_the_box_filter(pkg, gpu, oracle, variant):
    hits = None
    if variant == "orthographic":   # k_generate_cam<1> feeds the same records; the oracle has no such camera: camera_model's rays, the oracle's hits
        import camera_model
        sd, rp = M.orthographic_scene(pkg); hits = camera_model.camera_hits
    else:
        sd, rp = M.materials_scene(pkg, sampler="halton" if variant == "halton" else "sobol", lensradius=0.08 if variant == "lens" else 0.0)
    groups = _prim_groups(sd)
    h, surface, ids, want, count = M.reference(pkg, oracle, ("materials", variant), sd, rp, groups=groups, hits=hits, layers=("material", "group"))
    t = want["material"]
    assert set(np.unique(t["id"][..., 0][t["n_ids"] > 0])) >= {1, 2, 3, 4} and (t["n_ids"] >= 2).mean() > 0.03   # four materials, and edges between them
    assert variant == "orthographic" or 0.05 < (~surface).mean() < 0.7
    assert (want["group"]["n_ids"] >= want["material"]["n_ids"]).all() and (want["group"]["n_ids"] > want["material"]["n_ids"]).any()
    g = pkg.Scene(gpu, sd)
    got = g.render_mattes(rp, layers=("material", "group"), groups=groups)
    assert sorted(got) == ["group", "material"] and got["material"].shape == (M.YRES, M.XRES) and got["material"].dtype == pkg._abi_aov.MATTE_DTYPE
    _same(got, want, variant)
    c = g.counters()
    assert c["camera_rays"] == len(h["prim"]) == c["intersect_tests"] and c["film_splats"] == count
    assert {"generate", "extend_camera", "matte", "matte_film"} <= {s["name"] for s in g.kernel_stats()}


# ---- 2: a wide filter and a crop window inside the full resolution -------------------------------------------------------------------------------------------------

def _gaussian_job(pkg):
    sd, rp = M.materials_scene(pkg, crop=True)
    with_filter(pkg, rp, "gaussian", 2.0)
    return sd, rp


def _gaussian_reference(pkg, oracle):
    sd, rp = _gaussian_job(pkg)
    return sd, rp, _prim_groups(sd), M.reference(pkg, oracle, "gaussian", sd, rp, groups=_prim_groups(sd))


def test_gaussian_filter_with_sample_bounds_beyond_the_film(pkg, gpu, oracle):
    sd, rp, groups, (h, surface, ids, want, count) = _gaussian_reference(pkg, oracle)
    cb, sb = list(rp.cropped_pixel_bounds), list(rp.sample_bounds)
    assert cb == [16, 12, 48, 36] and sb == [14, 10, 50, 38]   # source pixels outside the film contribute, and the sample tiles are 3 x 2
    t = want["material"]
    assert (t["w_total"] > 0).all() and (t["n_ids"] >= 2).mean() > 0.3 and 0.05 < (~surface).mean() < 0.7
    g = pkg.Scene(gpu, sd)
    got = g.render_mattes(rp, layers=M.LAYERS, groups=groups)
    _same(got, want, "gaussian")
    assert not got["instance"]["id"].any() and (got["instance"]["n_ids"] <= 1).all()   # top-level geometry only: the id 0, once
    c = g.counters()
    assert c["camera_rays"] == len(h["prim"]) and c["film_splats"] == count


# ---- 3: overflow ---------------------------------------------------------------------------------------------------------------------------------------------------------

def test_overflowing_tables(pkg, gpu, oracle):
    """The ground as 24 x 24 quads, each quad of the left half a group of its own, under the gaussian filter: a pixel gathers the samples of 5 x 5 pixels and more than
    eight groups where the quads are small on the film. The two conditions are the REFERENCE's."""
    sd, rp, groups = M.overflow_scene(pkg, 24)
    with_filter(pkg, rp, "gaussian", 2.0)
    h, surface, ids, want, count = M.reference(pkg, oracle, "overflow", sd, rp, groups=groups, layers=("group",))
    t = want["group"]
    assert (t["w_other"] > 0).mean() >= 0.05, (t["w_other"] > 0).mean()
    assert ((t["n_ids"] >= 2) & (t["w_other"] == 0)).mean() >= 0.05
    assert (t["n_ids"][t["w_other"] > 0] == 8).all()
    g = pkg.Scene(gpu, sd)
    got = g.render_mattes(rp, layers=("group",), groups=groups)
    _same(got, want, "overflow")
    assert g.counters()["film_splats"] == count
    # n_prims is the scene's, or the call is refused with the tables untouched
    kept = got["group"].copy()
    with pytest.raises(pkg.runtime.PtError, match="status %d" % pkg._abi.PT_ERR_INVALID_ARG):
        g.render_mattes(rp, groups=groups[:-1], tables=got)
    assert got["group"].tobytes() == kept.tobytes()


# ---- 4: instances ------------------------------------------------------------------------------------------------------------------------------------------------------

def test_instance_ids(pkg, gpu, oracle):
    sd, rp, object_prims = M.instance_scene(pkg)

    def instance_of(h):   # the object's instances stand far apart in x: the first at x < 0 (id 1), the second at x > 0 (id 2); everything else is top level
        x = h["o"][:, 0].astype(np.float64) + h["t"].astype(np.float64) * h["d"][:, 0]
        inside = np.isin(h["prim"], object_prims)
        assert np.abs(x[inside]).min() > 0.5
        return np.where(inside, np.where(x < 0, 1, 2), 0).astype(np.uint32)

    h, surface, ids, want, count = M.reference(pkg, oracle, "instances", sd, rp, instance_of=instance_of, layers=("material", "instance"))
    assert set(np.unique(ids[surface, 1])) == {0, 1, 2} and min((ids[surface, 1] == k).mean() for k in (0, 1, 2)) > 0.03
    g = pkg.Scene(gpu, sd)
    got = g.render_mattes(rp)   # the default layers
    assert sorted(got) == ["instance", "material"]
    _same(got, want, "instances")
    t = got["instance"]
    assert {0, 1, 2} == set(np.unique(t["id"][np.arange(8)[None, None, :] < t["n_ids"][..., None]]))


# ---- 5: a surface without a material is passed through ---------------------------------------------------------------------------------------------------------------

def test_a_shell_changes_nothing(pkg, gpu, oracle):
    sd, rp = M.shell_scene(pkg, True)
    bare, _ = M.shell_scene(pkg, False)
    orc = oracle.scene(sd); shells = camera_hits(pkg, oracle, orc, rp); orc.close()
    h, surface, ids, want, count = M.reference(pkg, oracle, "shell-bare", bare, rp, groups=bare.prim_group, layers=("material", "group"))
    crossed = shells["prim"] == 2
    assert sd.prim_material[2] == NONE and crossed.mean() > 0.05 and surface[crossed].all()   # the sphere is in the way, wholly inside the ground's silhouette
    g, gb = pkg.Scene(gpu, sd), pkg.Scene(gpu, bare)
    got = g.render_mattes(rp, layers=("material", "group"), groups=sd.prim_group)   # per-shape groups: the ground is shape 0 in both scenes
    c = g.counters()
    _same(got, want, "behind the shell")
    _same(gb.render_mattes(rp, layers=("material", "group"), groups=bare.prim_group), got, "bare")
    assert c["camera_rays"] == len(h["prim"]) and c["intersect_tests"] >= c["camera_rays"] + int(crossed.sum()) and c["film_splats"] == count
    assert {"extend", "matte"} <= {s["name"] for s in g.kernel_stats()}


# ---- 6: ranges, passes, host and device buffers, determinism ---------------------------------------------------------------------------------------------------------

def _device_tables(layers, like):
    import torch
    dev = {k: torch.zeros(like.size * 80, dtype=torch.uint8, device="cuda") for k in layers}
    torch.cuda.synchronize()   # (the library renders on its own stream)
    return dev


def _read_back(pkg, dev, like):
    return {k: v.cpu().numpy().view(pkg._abi_aov.MATTE_DTYPE).reshape(like.shape) for k, v in dev.items()}


def test_ranges_passes_and_buffers(pkg, gpu, oracle):
    sd, rp, groups, (h, surface, ids, want, count) = _gaussian_reference(pkg, oracle)
    g = pkg.Scene(gpu, sd)
    like = want["material"]
    # [0, 1) then [1, 4) into the same DEVICE buffers
    dev = _device_tables(M.LAYERS, like)
    ptrs = {k: v.data_ptr() for k, v in dev.items()}
    splats = 0
    for samples in ((0, 1), (1, 3)):
        assert g.render_mattes(rp, groups=groups, samples=samples, device_ptrs=ptrs) is None
        splats += g.counters()["film_splats"]
    _same(_read_back(pkg, dev, like), want, "[0, 1) + [1, 4) on the device")
    assert splats == count
    # ... and into the same host arrays
    parts = g.render_mattes(rp, layers=M.LAYERS, groups=groups, samples=(0, 1))
    assert g.render_mattes(rp, groups=groups, samples=(1, 3), tables=parts) is parts
    _same(parts, want, "[0, 1) + [1, 4) on the host")
    # the pass size does not show
    for spp_per_pass in (1, 3, 0):
        rp.spp_per_pass = spp_per_pass
        size = g.matte_pass_size(rp)
        assert size == spp_per_pass or (spp_per_pass == 0 and 1 <= size <= rp.spp)
        _same(g.render_mattes(rp, layers=M.LAYERS, groups=groups), want, "spp_per_pass %d" % spp_per_pass)
        launches = [s for s in g.kernel_stats() if s["name"] == "matte_film"][0]["launches"]
        assert launches == -(-rp.spp // size)
    # two identical calls, device buffers: the same bytes (and the host's)
    again = _device_tables(M.LAYERS, like)
    g.render_mattes(rp, groups=groups, device_ptrs={k: v.data_ptr() for k, v in again.items()})
    first = _read_back(pkg, again, like)
    once_more = _device_tables(M.LAYERS, like)
    g.render_mattes(rp, groups=groups, device_ptrs={k: v.data_ptr() for k, v in once_more.items()})
    _same(_read_back(pkg, once_more, like), first, "second identical call")
    _same(first, want, "device buffers")
    # a layer that is not wanted is not touched
    only = _device_tables(M.LAYERS, like)
    g.render_mattes(rp, device_ptrs={"instance": only["instance"].data_ptr()})
    back = _read_back(pkg, only, like)
    _same({"instance": back["instance"]}, {"instance": want["instance"]}, "one layer")
    assert not back["material"].view(np.uint8).any() and not back["group"].view(np.uint8).any()


# ---- 7: masks ----------------------------------------------------------------------------------------------------------------------------------------------------------

def test_masks(pkg, gpu, oracle):
    import torch
    sd, rp, groups, (h, surface, ids, want, count) = _gaussian_reference(pkg, oracle)
    g = pkg.Scene(gpu, sd)
    table = np.array(want["material"])
    dev = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    present = sorted(set(int(v) for v in np.unique(table["id"][np.arange(8)[None, None, :] < table["n_ids"][..., None]])))
    assert len(present) >= 4
    for wanted in ([present[1]], present[1:3] + [present[-1]], [987654], list(range(5000, 9096))):   # one id, several, an absent one, 4096 absent ones
        expect = M.mask(table, wanted)
        host = g.matte_mask(table, wanted)
        assert host.shape == table.shape and host.tobytes() == expect.tobytes(), wanted[:4]
        from_device = g.matte_mask(dev.data_ptr(), wanted, n_pixels=table.size)
        assert from_device.tobytes() == expect.tobytes()
        out = torch.full((table.size,), 7.0, dtype=torch.float32, device="cuda"); torch.cuda.synchronize()
        assert g.matte_mask(dev.data_ptr(), wanted, n_pixels=table.size, mask_ptr=out.data_ptr()) is None
        assert out.cpu().numpy().tobytes() == expect.tobytes()
        assert (expect == 0).all() == (wanted[0] >= 5000 or wanted == [987654])
    one = M.mask(table, [present[1]])
    assert 0.02 < (one > 0).mean() < 0.9 and one.max() <= 1.0 and ((one > 0) & (one < 1)).any()   # a matte with soft edges
    assert "matte_mask" in {s["name"] for s in g.kernel_stats()}
    with pytest.raises(pkg.runtime.PtError):
        g.matte_mask(table, list(range(4097)))


# ---- 8: counters, and the refusal of tile shards -----------------------------------------------------------------------------------------------------------------------

def test_counters_and_tile_shards(pkg, gpu, oracle):
    sd, rp = M.materials_scene(pkg)
    groups = _prim_groups(sd)
    h, surface, ids, want, count = M.reference(pkg, oracle, ("materials", "sobol"), sd, rp, groups=groups, layers=("material", "group"))
    g = pkg.Scene(gpu, sd)
    got = g.render_mattes(rp, layers=("material",))
    c = g.counters()
    assert c["camera_rays"] == len(h["prim"]) == M.XRES * M.YRES * M.SPP and c["intersect_tests"] == c["camera_rays"]
    assert c["film_splats"] == count                                      # once per (sample, pixel), with one layer ...
    g.render_mattes(rp, layers=M.LAYERS, groups=groups)
    assert g.counters()["film_splats"] == count                           # ... and with three
    assert c["shadow_tests"] == 0 and c["zero_radiance_paths_den"] == 0 and not any(c["path_length_hist"])
    rp.tile_world = 2
    kept = got["material"].copy()
    for rank in (0, 1):
        rp.tile_rank = rank
        st = gpu.aov.pt_matte_render(g.h, C.byref(rp), C.byref(pkg._abi_aov.matte_buffers(got)), 0)
        assert st == pkg._abi.PT_ERR_UNSUPPORTED and b"tile_world" in gpu.lib.pt_last_error()
    assert got["material"].tobytes() == kept.tobytes()
