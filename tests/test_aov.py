"""pt_aov_render on the GPU against the unchanged oracle (aov_reference.py has the three identities and test_aov_reference.py the oracle-only facts they rest on):
albedo against an oracle render, normals against three, depth / hit identity / the albedo table against the oracle's first hits; then what the call promises about
sample ranges, tile shards, NULL planes, device buffers, surfaces without a material, and its counters.

Tolerance of GPU sums against identities 1 and 2: 3e-6 x the pixel's weight sum -- the project's film tolerance (parity.assert_same_film: rtol 2e-6) plus the
reference's own floor (test_aov_reference.py: 1e-6). Identity 3 under the box filter: assert_same_film's rtol and atol, weight sums bit for bit."""
import ctypes as C

import numpy as np
import pytest
from aov_reference import LIGHTS, NONE, albedo_scene, camera_hits, film_rgb_sums, first_hit_reference, hit_fractions, normal_scene
from parity import ORACLE_THREADS, assert_same_film
from tile_scene import with_filter

pytestmark = pytest.mark.gpu
TOL = 3.0e-6
# Identity 3, samples on triangles with vertex normals. This bound is this file's own choice, not the issue's: the issue's recipe for identity 3 names face normals and
# spheres only, and a float64 normalize(sum of b_i N_i) cannot be held to assert_same_film's atol of 1e-7 (the device's value carries the roundings of the interpolation
# and of three float32 normalisations). 8 ulps of a unit vector's component (2^-23 each) per unit of weight, rounded up; measured 7.2e-7. Identity 2 is what holds
# smooth normals against the oracle itself.
SMOOTH_TOL = 1.0e-6
FILTERS = [("box", 0.5), ("gaussian", 2.0)]
_ORACLE_FILMS = {}   # oracle renders, computed once and shared by the two walks of a test


def _oracle_film(oracle, key, sd, rp):
    if key not in _ORACLE_FILMS:
        orc = oracle.scene(sd)
        film = orc.render(rp, nthreads=ORACLE_THREADS)
        _ORACLE_FILMS[key] = (film, orc.counters())
        orc.close()
    return _ORACLE_FILMS[key]


def _honest(pkg, oracle, key, sd, rp):
    """The cap that keeps a scene honest: at least 30 % of its camera samples hit and at least 5 % miss (the oracle's first hits; under the box filter's bounds)."""
    if ("cap", key) not in _ORACLE_FILMS:
        box = with_filter(pkg, _copy(rp), "box", 0.5)
        orc = oracle.scene(sd)
        _ORACLE_FILMS[("cap", key)] = camera_hits(pkg, oracle, orc, box)
        orc.close()
    h = _ORACLE_FILMS[("cap", key)]
    hit, miss = hit_fractions(h)
    assert hit >= 0.30 and miss >= 0.05, (key, hit, miss)
    return h


def _copy(rp):
    out = type(rp)()
    C.memmove(C.byref(out), C.byref(rp), C.sizeof(rp))
    return out


def _same_weights(got, want, filt):
    if filt[0] == "box": assert np.array_equal(got, want), "weights differ"
    else: np.testing.assert_allclose(got, want, rtol=TOL, atol=0)   # (a wide filter's splats are float atomics: their order varies)


def _all_hit_around(h, rp, reach):
    """Per pixel of the cropped film: every camera sample of every pixel within `reach` pixels hits."""
    sb, cb = rp.sample_bounds, rp.cropped_pixel_bounds
    ok = (h["prim"] != NONE).reshape(sb[3] - sb[1], sb[2] - sb[0], -1).all(axis=2)
    out = np.zeros((cb[3] - cb[1], cb[2] - cb[0]), bool)
    for y in range(cb[1], cb[3]):
        for x in range(cb[0], cb[2]):
            out[y - cb[1], x - cb[0]] = ok[max(y - reach - sb[1], 0):y + reach + 1 - sb[1], max(x - reach - sb[0], 0):x + reach + 1 - sb[0]].all()
    return out


# ---- identity 1: the albedo plane is the oracle's film of a matte surface lit along its normal ---------------------------------------------------------------------

@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: f[0])
@pytest.mark.parametrize("kd", ["const", "checker", "ewa", "trilinear", "ewa-lens"])
def test_albedo_against_an_oracle_render(pkg, gpu, oracle, kd, filt):
    sd, rp = albedo_scene(pkg, kd.split("-")[0], lensradius=0.08 if kd.endswith("lens") else 0.0)
    with_filter(pkg, rp, *filt)
    _honest(pkg, oracle, ("albedo", kd), sd, rp)
    film, oc = _oracle_film(oracle, ("albedo", kd, filt[0]), sd, rp)
    assert oc["zero_radiance_paths_num"] == 0
    g = pkg.Scene(gpu, sd)
    got = g.render_aov(rp, planes=("albedo",))["albedo"]
    w = film[..., 3]
    _same_weights(got[..., 3], w, filt)
    lit = w > 0
    err = np.abs(got[..., :3].astype(np.float64) - film_rgb_sums(pkg, film))[lit] / w[lit][:, None]
    print("identity 1, Kd %s, %s: largest error per unit weight %.3g" % (kd, filt[0], err.max()))
    assert err.max() <= TOL
    if kd != "const":   # the texture is there: the plane is no constant times the weight
        mean = got[..., :3][lit] / w[lit][:, None]
        assert mean.std(axis=0).max() > 0.05
    assert g.counters()["camera_rays"] == oc["camera_rays"] and g.counters()["film_splats"] == oc["film_splats"]


# ---- identity 2: the normal plane projects onto three oracle renders -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: f[0])
@pytest.mark.parametrize("surface", ["bump", "mesh"])
def test_normals_against_three_oracle_renders(pkg, gpu, oracle, surface, filt):
    films = []
    for i, light in enumerate(LIGHTS):
        sd, rp = normal_scene(pkg, surface, light)
        with_filter(pkg, rp, *filt)
        film, oc = _oracle_film(oracle, ("normal", surface, filt[0], i), sd, rp)
        assert oc["zero_radiance_paths_num"] == 0
        films.append(film)
    h = _honest(pkg, oracle, ("normal", surface), sd, rp)
    g = pkg.Scene(gpu, sd)
    got = g.render_aov(rp, planes=("albedo", "normal"))
    w = films[0][..., 3]
    _same_weights(got["albedo"][..., 3], w, filt)
    assert (got["normal"][..., 3] <= got["albedo"][..., 3] * (1 + TOL)).all()
    lit = w > 0
    worst = 0.0
    for light, film in zip(LIGHTS, films):
        want = film_rgb_sums(pkg, film)[..., 0]
        have = got["normal"][..., :3].astype(np.float64) @ np.array(light)
        worst = max(worst, float((np.abs(have - want)[lit] / w[lit]).max()))
    print("identity 2, %s, %s: largest error per unit weight %.3g" % (surface, filt[0], worst))
    assert worst <= TOL
    # on pixels no miss reaches, the normal plane's weight is the film's
    full = _all_hit_around(h, with_filter(pkg, _copy(rp), "box", 0.5), 1 if filt[0] == "box" else 3)
    assert full.sum() > full.size // 8
    _same_weights(got["normal"][..., 3][full], w[full], filt)
    tilt = np.linalg.norm(got["normal"][..., [0, 2]][lit], axis=1) / w[lit]
    assert tilt.max() > 0.02   # (no flat floor)


# ---- identity 3: depth, normals, hit identity and the albedo table against the oracle's first hits (box filter) ----------------------------------------------------

def _first_hit_scene(pkg, name):
    S = pkg.scenes
    if name == "spheres_c1": return S.spheres_c1(xres=64, yres=64, spp=4)
    if name == "spheres_c1-halton":
        b = S.spheres_c1(xres=64, yres=64, spp=4); b.sampler = "halton"; return b
    if name == "spheres_c1-lens":
        b = S.spheres_c1(xres=64, yres=64, spp=4); b.cam.update(lensradius=0.1, focaldistance=5.5); return b
    if name == "material_zoo": return S.material_zoo(n=8, spp=4)
    if name == "instanced_garden": return S.instanced_garden(spp=4)
    if name == "alpha_foliage": return S.alpha_foliage(spp=4)
    if name == "disk_scene": return S.disk_scene(spp=4)
    if name == "mix_materials": return S.mix_materials(spp=4)
    if name == "disney_spheres": return S.disney_spheres(spp=4)
    if name == "translucent_panels": return S.translucent_panels(spp=4)
    if name == "subsurface_c5": return S.subsurface_c5(n=8, spp=4)
    raise KeyError(name)


FIRST_HIT_SCENES = ["spheres_c1", "spheres_c1-halton", "spheres_c1-lens", "material_zoo", "instanced_garden", "alpha_foliage", "disk_scene",
                    "mix_materials", "disney_spheres", "translucent_panels", "subsurface_c5"]   # (the last four: the rest of the albedo table, mix included)


# The material types (PtMaterial.type; a mix as the pair of its materials' types) the oracle's first hits must find in a scene: together every row of the albedo table
MATTE, MIRROR, GLASS, PLASTIC, METAL, UBER, SUBSTRATE, SUBSURFACE, TRANSLUCENT, MIX, DISNEY = range(11)
MATERIALS_HIT = {"spheres_c1": {MATTE, MIRROR, GLASS, PLASTIC}, "material_zoo": {MATTE, MIRROR, GLASS, PLASTIC, METAL, UBER, SUBSTRATE}, "instanced_garden": {MATTE, PLASTIC},
                 "alpha_foliage": {MATTE}, "disk_scene": {MATTE, UBER}, "mix_materials": {MATTE, MIX, (MATTE, MIRROR), (PLASTIC, GLASS), (METAL, TRANSLUCENT), (TRANSLUCENT, MATTE)},
                 "disney_spheres": {DISNEY}, "translucent_panels": {MATTE, TRANSLUCENT}, "subsurface_c5": {MATTE, SUBSURFACE}}


def _materials_hit(pkg, sd, h):
    A = pkg._abi
    assert [A.PT_MAT_MATTE, A.PT_MAT_MIRROR, A.PT_MAT_GLASS, A.PT_MAT_PLASTIC, A.PT_MAT_METAL, A.PT_MAT_UBER, A.PT_MAT_SUBSTRATE, A.PT_MAT_SUBSURFACE, A.PT_MAT_TRANSLUCENT,
            A.PT_MAT_MIX, A.PT_MAT_DISNEY] == list(range(11))
    found = set()
    for mi in np.unique(sd.prim_material[h["prim"][h["prim"] != NONE]]):
        m = sd.materials[int(mi)]
        found.add(int(m.type))
        if m.type == A.PT_MAT_MIX: found.add((int(sd.materials[m.mix[0]].type), int(sd.materials[m.mix[1]].type)))
    return found


def test_the_first_hit_scenes_cover_the_albedo_table():
    assert set().union(*[{t for t in v if isinstance(t, int)} for v in MATERIALS_HIT.values()]) == set(range(11))


@pytest.mark.parametrize("name", FIRST_HIT_SCENES)
def test_first_hits_against_the_oracle(pkg, gpu, oracle, name):
    sd, rp = _first_hit_scene(pkg, name).world_end()
    h, ref, textured, smooth = first_hit_reference(pkg, oracle, name, sd, rp)
    hit, miss = hit_fractions(h)
    assert hit >= 0.30 and miss >= 0.05, (hit, miss)
    # what the comparisons below are made of: the scene's materials are hit, and the masks leave most of the surface pixels in
    assert _materials_hit(pkg, sd, h) >= MATERIALS_HIT[name.split("-")[0]], _materials_hit(pkg, sd, h)
    surface = ref["normal"][..., 3] > 0
    assert (surface & ~textured).sum() >= 0.3 * surface.sum() and (surface & ~smooth).sum() >= 0.5 * surface.sum()
    g = pkg.Scene(gpu, sd)
    got = g.render_aov(rp)
    for plane in ("albedo", "normal", "depth"):
        assert np.array_equal(got[plane][..., -1], ref[plane][..., -1]), plane + ": weights differ"
    scale = lambda a, b_: float(np.abs(a.astype(np.float64) - b_).max())
    print("identity 3, %s: largest absolute error of the sums: depth %.3g (of %.3g), normal %.3g (where a smooth-shaded sample reaches: %.3g), albedo %.3g" %
          (name, scale(got["depth"][..., 0], ref["depth"][..., 0]), ref["depth"][..., 0].max(), scale(got["normal"][..., :3][~smooth], ref["normal"][..., :3][~smooth]),
           scale(got["normal"][..., :3][smooth], ref["normal"][..., :3][smooth]) if smooth.any() else 0.0,
           scale(got["albedo"][..., :3][~textured], ref["albedo"][..., :3][~textured])))
    np.testing.assert_allclose(got["depth"][..., 0], ref["depth"][..., 0], rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(got["albedo"][..., :3][~textured], ref["albedo"][..., :3][~textured], rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(got["normal"][..., :3][~smooth], ref["normal"][..., :3][~smooth], rtol=2e-6, atol=1e-7)
    # A triangle with vertex normals is outside identity 3's recipe (face normals, spheres): its reference here is normalize(sum of b_i N_i) in float64, from which the
    # shading normal differs by the roundings of three float32 normalisations and of the interpolation -- well inside SMOOTH_TOL per unit of weight
    if smooth.any():
        err = np.abs(got["normal"][..., :3].astype(np.float64) - ref["normal"][..., :3])[smooth].max(axis=-1) / ref["albedo"][..., 3][smooth]
        assert err.max() <= SMOOTH_TOL, err.max()
    c = g.counters()
    n_samples = len(h["prim"])
    assert c["camera_rays"] == n_samples and c["intersect_tests"] == n_samples   # (no surface without a material: no continuation)
    assert c["film_splats"] == int(ref["albedo"][..., 3].sum())                 # (box filter: every splat adds a weight of 1 to the albedo plane)
    assert c["shadow_tests"] == 0 and c["zero_radiance_paths_den"] == 0 and not any(c["path_length_hist"])


def test_camera_rays_equal_the_oracle_render(pkg, gpu, oracle):
    sd, rp = _first_hit_scene(pkg, "spheres_c1").world_end()
    _, oc = _oracle_film(oracle, "spheres_c1", sd, rp)
    g = pkg.Scene(gpu, sd)
    g.render_aov(rp, planes=("depth",))
    c = g.counters()
    assert c["camera_rays"] == oc["camera_rays"] and c["film_splats"] == oc["film_splats"] and c["intersect_tests"] == c["camera_rays"]


# ---- what the call promises ------------------------------------------------------------------------------------------------------------------------------------------

def _range_scene(pkg, filt, bump=True):
    """The EWA-textured ground of identity 1, by default under normal_scene's bump map as well, 8 spp in passes of 2: ranges that begin and end inside passes."""
    sd, rp = albedo_scene(pkg, "ewa", bump=bump, spp=8)
    mat = sd.materials[sd.prim_material[0]]
    assert (mat.tex[pkg._abi.PT_MP_BUMP] >= 0) == bump and mat.tex[pkg._abi.PT_MP_KD] >= 0
    with_filter(pkg, rp, *filt)
    rp.spp_per_pass = 2
    return sd, rp


def _split_and_whole(g, rp):
    whole = g.render_aov(rp)
    wc = g.counters()
    parts = g.render_aov(rp, samples=(0, 3))
    c0 = g.counters()
    assert g.render_aov(rp, samples=(3, 5), sums=parts) is parts
    c1 = g.counters()
    for k in ("camera_rays", "intersect_tests", "film_splats"):
        assert c0[k] + c1[k] == wc[k], k
    return parts, whole


@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: f[0])
def test_split_ranges_equal_the_whole(pkg, gpu, oracle, filt):
    """Box filter: bit for bit, on textured albedo AND bumped normals. Gaussian: assert_same_film on the scene without the bump map, whose sums are of one sign like a
    film's. With the bump map the normal plane's x and z are sums of BOTH signs that nearly cancel, added by float atomics in an order that varies: an absolute 1e-7 is
    not theirs to keep (measured on an MI355X: 3 of 2304 elements off by up to 3.1e-7, pixel weights about 6); that plane is held to TOL per unit of weight, the bound of
    every other sum here, and the bumped scene's other planes to assert_same_film."""
    sd, rp = _range_scene(pkg, filt)
    _honest(pkg, oracle, ("albedo", "ewa", 8), sd, rp)
    g = pkg.Scene(gpu, sd)
    parts, whole = _split_and_whole(g, rp)
    lit = whole["normal"][..., 3] > 0
    assert (np.linalg.norm(whole["normal"][..., [0, 2]][lit], axis=1) / whole["normal"][..., 3][lit]).max() > 0.02   # (the bump map is in the normal plane)
    for plane in whole:
        if filt[0] == "box": assert np.array_equal(parts[plane], whole[plane]), plane   # bit for bit: one chain of additions per pixel, in sample order
        elif plane != "normal": assert_same_film(_as_film(parts[plane]), _as_film(whole[plane]), weights=TOL)
    if filt[0] != "box":
        np.testing.assert_allclose(parts["normal"][..., 3], whole["normal"][..., 3], rtol=TOL, atol=0)
        err = np.abs(parts["normal"][..., :3].astype(np.float64) - whole["normal"][..., :3]).max(axis=-1)[lit] / whole["normal"][..., 3][lit]
        print("split ranges, gaussian, bumped normal plane: largest difference per unit weight %.3g" % err.max())
        assert err.max() <= TOL
        flat_sd, flat_rp = _range_scene(pkg, filt, bump=False)
        flat_parts, flat_whole = _split_and_whole(pkg.Scene(gpu, flat_sd), flat_rp)
        for plane in flat_whole:
            assert_same_film(_as_film(flat_parts[plane]), _as_film(flat_whole[plane]), weights=TOL)
    # the guard: the same three samples as a JOB of 3 spp (the differentials scaled by 1 / sqrt(3), not 1 / sqrt(8)) are another albedo plane
    first = g.render_aov(rp, samples=(0, 3), planes=("albedo",))["albedo"]
    rp.spp = 3
    wrong = g.render_aov(rp, planes=("albedo",))["albedo"]
    assert (~np.isclose(wrong[..., :3], first[..., :3], rtol=2e-6, atol=1e-7)).sum() > first[..., :3].size // 20


def _as_film(plane):
    """A plane's sums as (H, W, 4) with the weight last: what assert_same_film compares."""
    if plane.shape[-1] == 4: return plane
    return np.concatenate([plane[..., :1], np.zeros(plane.shape[:2] + (2,), np.float32), plane[..., 1:]], -1)


def test_tile_shards_add_up_to_the_whole(pkg, gpu):
    sd, rp = _first_hit_scene(pkg, "spheres_c1").world_end()
    g = pkg.Scene(gpu, sd)
    whole = g.render_aov(rp)
    wc = g.counters()
    rp.tile_world = 2
    total, rays = None, 0
    for rank in (0, 1):
        rp.tile_rank = rank
        part = g.render_aov(rp)
        rays += g.counters()["camera_rays"]
        total = part if total is None else {k: total[k] + part[k] for k in part}
    assert rays == wc["camera_rays"]
    for plane in whole:   # (a sample on a tile's edge reaches the neighbour tile's pixel by an atomic: the order of that pixel's additions varies)
        assert_same_film(_as_film(total[plane]), _as_film(whole[plane]))
    # a rank that owns no tile adds nothing and reports nothing
    rp.tile_world, rp.tile_rank = 64, 63
    kept = {k: v.copy() for k, v in whole.items()}
    g.render_aov(rp, sums=whole)
    assert all(np.array_equal(whole[k], kept[k]) for k in whole) and g.counters()["camera_rays"] == 0


def test_null_planes_and_device_buffers(pkg, gpu):
    import torch
    sd, rp = _first_hit_scene(pkg, "spheres_c1").world_end()
    g = pkg.Scene(gpu, sd)
    host = g.render_aov(rp)
    h, w = host["depth"].shape[:2]
    # the host side of "ADDED to": the same render into host arrays that hold 7s -- a pixel's chain of additions starts from the 7 on either side
    sevens = g.render_aov(rp, sums={k: np.full(v.shape, 7.0, np.float32) for k, v in host.items()})
    assert all((np.abs((sevens[k] - 7.0) - host[k]) <= 4e-6 * (1 + np.abs(host[k]))).all() and not np.array_equal(sevens[k], host[k]) for k in host)   # (it IS 7 + the sums)
    for wanted in (("normal",), ("albedo", "depth"), ("albedo", "normal", "depth")):
        dev = {k: torch.full((h, w, c), 7.0, dtype=torch.float32, device="cuda") for k, c in pkg._abi_aov.CHANNELS.items()}
        torch.cuda.synchronize()   # (the library renders on its own stream)
        assert g.render_aov(rp, device_ptrs={k: dev[k].data_ptr() for k in wanted}) is None
        splats = g.counters()["film_splats"]
        for k in dev:
            out = dev[k].cpu().numpy()
            if k in wanted: assert_same_film(_as_film(out), _as_film(sevens[k]))   # device output == host output (weights bit for bit, sums within the film tolerance)
            else: assert (out == 7.0).all(), k + " was not asked for"
        only = g.render_aov(rp, planes=wanted)
        assert sorted(only) == sorted(wanted)
        for k in wanted:
            assert_same_film(_as_film(only[k]), _as_film(host[k]))
        assert g.counters()["film_splats"] == splats   # once per sample and pixel, whatever the planes
    assert splats == int(host["albedo"][..., 3].sum())


def _without_shells(pkg, sd):
    """`sd` without its primitives that carry no material (medium-interface shells), area lights re-pointed."""
    keep = sd.prim_material != NONE
    assert sd.top_refs is None and keep.any() and not keep.all()
    new_index = np.cumsum(keep) - 1
    for k in range(sd.n_lights):
        if sd.lights[k].prim != NONE:
            assert keep[sd.lights[k].prim]
            sd.lights[k].prim = int(new_index[sd.lights[k].prim])
    for name in ("prim_shape", "prim_material", "prim_light", "prim_med_in", "prim_med_out"):
        if getattr(sd, name) is not None:
            setattr(sd, name, np.ascontiguousarray(getattr(sd, name)[keep]))
    return sd


@pytest.mark.parametrize("grid,lift", [(False, 0.0), (True, 0.05), (True, 0.0)], ids=["sphere-shell", "sphere-and-lifted-box-shells", "sphere-and-box-shells"])
def test_surfaces_without_a_material_are_passed_through(pkg, gpu, oracle, grid, lift):
    """shell_media: a sphere shell (and, grid: a box shell of twelve triangles) stands between the camera and much of the scene. The planes are those of the scene without
    the shells; the depth is the sum of the segments, each begun at an offset origin -- a few ulps of the scene's scale apart (measured on an MI355X: 1.3e-6 relative).
    The box shell's bottom face lies IN the floor's plane: a ray inside the box meets both at one t, and where the closest hit of that tie is the shell, the ray spawned
    behind it starts below the floor and leaves the scene, as the path integrator's does (path.rs:124-129). Pixels such a sample may reach are compared by their
    weights alone -- and with the box lifted off the floor by 0.05 (scenes.shell_media: box_lift) there is no tie: every pixel is held to the tolerance."""
    sd, rp = pkg.scenes.shell_media(spp=4, grid=grid, box_lift=lift).world_end()
    bare, _ = pkg.scenes.shell_media(spp=4, grid=grid, box_lift=lift).world_end()
    bare = _without_shells(pkg, bare)
    h = _honest(pkg, oracle, ("shell_media-bare", grid, lift), bare, rp)
    shells = camera_hits(pkg, oracle, oracle.scene(sd), rp)
    first = np.minimum(shells["prim"], len(sd.prim_material) - 1)
    crossed = (shells["prim"] != NONE) & (sd.prim_material[first] == NONE)
    assert crossed.mean() > 0.05, crossed.mean()   # (the shells are in the way of many camera rays)
    # samples that reach the floor under the box shell (scenes.shell_media: x in [0.6, 2.6], z in [-1, 1], y = 0)
    p = h["o"].astype(np.float64) + h["t"].astype(np.float64)[:, None] * h["d"]
    in_floor = grid and lift == 0.0
    under = (h["prim"] != NONE) & (np.abs(p[:, 1]) < 1e-4) & (p[:, 0] > 0.6 - 1e-3) & (p[:, 0] < 2.6 + 1e-3) & (np.abs(p[:, 2]) < 1.0 + 1e-3) & in_floor
    assert under.any() == in_floor
    tie = np.zeros(rp.cropped_pixel_bounds[3::-1][:2], bool)
    for (x, y) in h["pix"][under]:
        tie[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = True
    # the exclusion cannot grow unnoticed: a small part of the frame, and most of the samples that cross a shell lie outside it
    assert tie.mean() < 0.08, tie.mean()
    crossed_px = tie[shells["pix"][crossed][:, 1], shells["pix"][crossed][:, 0]]
    assert (~crossed_px).mean() > 0.7, (~crossed_px).mean()
    g, gb = pkg.Scene(gpu, sd), pkg.Scene(gpu, bare)
    got, want = g.render_aov(rp), gb.render_aov(rp)
    c, cb = g.counters(), gb.counters()
    assert c["camera_rays"] == cb["camera_rays"] == cb["intersect_tests"] == len(h["prim"])
    assert c["intersect_tests"] >= c["camera_rays"] + int(crossed.sum())   # every crossing is one more Scene::intersect (a ray may cross twice and more)
    assert c["film_splats"] == cb["film_splats"]
    assert np.array_equal(got["albedo"][..., 3], want["albedo"][..., 3])
    for plane in ("normal", "depth"):
        assert np.array_equal(got[plane][..., -1][~tie], want[plane][..., -1][~tie]), plane + ": weights differ"
        assert (got[plane][..., -1] <= want[plane][..., -1]).all()
    w = want["albedo"][..., 3]
    for plane in ("albedo", "normal"):
        err = (np.abs(got[plane][..., :3].astype(np.float64) - want[plane][..., :3]).max(axis=-1) / w)[~tie]
        print("pass-through, %s: largest error per unit weight %.3g" % (plane, err.max()))
        assert err.max() <= TOL
    d, dw = got["depth"][..., 0].astype(np.float64), want["depth"][..., 0].astype(np.float64)
    m = ~tie & (dw > 0)
    rel = np.abs(d - dw)[m] / dw[m]
    print("pass-through, depth: largest relative difference %.3g" % rel.max())
    assert rel.max() <= 1e-4 and (d[~tie & (dw == 0)] == 0).all() and (np.abs(d - dw)[m] > 0).any()   # (the segments' sum is no copy of the single segment)


@pytest.mark.parametrize("filt", FILTERS, ids=lambda f: f[0])
def test_a_textured_surface_behind_a_shell_keeps_the_camera_differentials(pkg, gpu, oracle, filt):
    """The trilinear-filtered ground of identity 1 with a material-less sphere in front of its middle: the planes are the ones without the sphere -- the albedo is still
    the oracle's film of the bare scene (identity 1: the texture filtered with the camera ray's differentials), where the path integrator would point-sample it.
    The bound. Behind the shell the hit point is the bare scene's to a few ulps of the scene's scale only (the segments start at offset origins: the depth test above
    measures 1.3e-6 relative), and the albedo follows the texture's slope there: TOL + G * S, with S = 16 ulps (2^-23 each) of the largest depth and G the image's
    largest step between neighbouring texels over a texel's size on the ground (bilinear interpolation is no steeper; coarser MIP levels are flatter). The trilinear
    lookup, because it is continuous in the lookup position; EWA's weight table and texel loop bounds are step functions of it."""
    kd = "trilinear"
    sd, rp = albedo_scene(pkg, kd, shell=True)
    bare, _ = albedo_scene(pkg, kd)
    with_filter(pkg, rp, *filt)
    _honest(pkg, oracle, ("albedo", kd), bare, rp)
    box = with_filter(pkg, _copy(rp), "box", 0.5)
    shells = camera_hits(pkg, oracle, oracle.scene(sd), box)
    crossed = (shells["prim"] != NONE) & (sd.prim_material[np.minimum(shells["prim"], len(sd.prim_material) - 1)] == NONE)
    assert 0.1 < crossed.mean() < 0.5, crossed.mean()
    film, _ = _oracle_film(oracle, ("albedo", kd, filt[0]), bare, rp)
    g = pkg.Scene(gpu, sd)
    got = g.render_aov(rp)
    assert g.counters()["intersect_tests"] >= g.counters()["camera_rays"] + 2 * int(crossed.sum()) - int(0.05 * crossed.sum())   # (in and out of the sphere; a grazing ray may lose a crossing)
    w = film[..., 3]
    _same_weights(got["albedo"][..., 3], w, filt)
    lit = w > 0
    want = pkg.Scene(gpu, bare).render_aov(rp)
    image = pkg.scenes.test_image(16, 16, seed=4).astype(np.float64)
    step = max(np.abs(np.diff(image, axis=0)).max(), np.abs(np.diff(image, axis=1)).max(), np.abs(image[0] - image[-1]).max(), np.abs(image[:, 0] - image[:, -1]).max())
    G = step * 16 * 0.45                                  # (planar mapping: 0.45 of the image per unit of length, 16 texels across it)
    S = 16 * 2.0 ** -23 * float(shells["t"][shells["prim"] != NONE].max() * 2)   # (twice the first hit's t bounds the whole way's in this scene)
    bound = TOL + G * S
    err = np.abs(got["albedo"][..., :3].astype(np.float64) - film_rgb_sums(pkg, film))[lit] / w[lit][:, None]
    print("textured behind a shell, %s: largest albedo error per unit weight against the oracle's film of the bare scene %.3g (bound %.3g)" % (filt[0], err.max(), bound))
    assert err.max() <= bound
    _same_weights(got["normal"][..., 3], want["normal"][..., 3], filt)
    assert (np.abs(got["normal"][..., :3] - want["normal"][..., :3]).max(axis=-1)[lit] / w[lit]).max() <= TOL
    d, dw = got["depth"][..., 0].astype(np.float64), want["depth"][..., 0].astype(np.float64)
    assert (np.abs(d - dw)[dw > 0] / dw[dw > 0]).max() <= 1e-4
    # the guard: without differentials (what a spawned ray has) the texture is point-sampled -- another plane by far more than the bound. The device's own word for it:
    # the same scene as a job of 10 000 spp scales the differentials to a hundredth
    sharp = _copy(rp); sharp.spp = 10000
    point = pkg.Scene(gpu, bare).render_aov(sharp, samples=(0, rp.spp), planes=("albedo",))["albedo"]
    far = np.abs(point[..., :3].astype(np.float64) - got["albedo"][..., :3]).max(axis=-1)[lit] / w[lit]
    print("   point-sampled instead: median difference per unit weight %.3g" % np.median(far))
    assert (far > 10 * bound).mean() > 0.2


def test_pass_size_is_the_size_of_the_passes(pkg, gpu):
    sd, rp = _range_scene(pkg, FILTERS[0])
    g = pkg.Scene(gpu, sd)
    for spp_per_pass, samples in ((3, None), (0, None), (3, (2, 5))):
        rp.spp_per_pass = spp_per_pass
        size = g.aov_pass_size(rp)
        assert size == spp_per_pass or (spp_per_pass == 0 and 1 <= size <= rp.spp)
        n = rp.spp if samples is None else samples[1]
        g.render_aov(rp, samples=samples, planes=("depth",))
        gen = [s for s in g.kernel_stats() if s["name"] == "generate"][0]
        assert gen["launches"] == -(-n // min(size, n)), (gen, size, n)
        assert {"extend_camera", "aov", "film"} <= {s["name"] for s in g.kernel_stats()}
