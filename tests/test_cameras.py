"""The orthographic and the environment camera on the GPU. There is no oracle for them: the device is held against the numpy model of camera_model.py (proved against
the oracle's perspective camera in test_cameras_host.py) and, through the model's rays, against the unchanged oracle's traversal (orc_trace_closest).

Every job is 32 x 24 pixels x 4 samples under a box filter, a crop window that starts at (16, 4) of a 64 x 32 frame: a film that is not square (x / y swaps), a window
that does not start at 0 (pixel-versus-film offsets) and, for the environment camera, angles that must come from the full resolution, not from the window.

What the tests do not claim: radiance after the first vertex under the new cameras is not compared with a reference -- that code is untouched and the existing suite
holds it against the oracle."""
import ctypes as C

import numpy as np
import pytest

import camera_model as cm
from aov_reference import GROUND_I, GROUND_P, GROUND_UV, NONE, UP, _light, box_sums, film_rgb_sums, sample_values
from model_math import concentric_sample_disk
from parity import assert_same_film, assert_same_render

pytestmark = pytest.mark.gpu
F = np.float32
TOL = 3.0e-6   # tests/test_aov.py, identities 1 and 2: per unit of a pixel's weight sum
_CACHE = {}    # references, computed once and shared by the two walks of a test


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _fp(pkg, a):
    return a.ctypes.data_as(pkg._abi.fp)


def device_rays(pkg, gpu, rp, cs):
    N = len(cs)
    o = np.zeros((N, 3), F); d = np.zeros((N, 3), F)
    gpu.check(gpu.lib.pt_camera_rays(C.byref(rp), N, _fp(pkg, cs), _fp(pkg, o), _fp(pkg, d)), "pt_camera_rays")
    return o, d


def device_differentials(pkg, gpu, rp, cs):
    N = len(cs)
    out = np.full((N, 12), np.nan, F); has = np.full(N, 7, np.uint8)
    gpu.check(gpu.lib.pt_camera_ray_differentials(C.byref(rp), N, _fp(pkg, cs), _fp(pkg, out), has.ctypes.data_as(C.POINTER(C.c_uint8))), "pt_camera_ray_differentials")
    return out, has


CASES = [("orthographic", False), ("orthographic", True), ("environment", False)]
CASE_IDS = ["orthographic", "orthographic-lens", "environment"]


def _samples(pkg, oracle, kind, lens, sampler):
    key = ("cs", kind, lens, sampler)
    if key not in _CACHE:
        rp = cm.job(pkg, kind, sampler=sampler, lens=lens).render_params()
        _, cs = cm.camera_samples(pkg, oracle, rp)
        cs = np.ascontiguousarray(np.concatenate([cs, cm.film_corners(rp)]), F)
        _CACHE[key] = (rp, cs, cm.rays(oracle, rp, cs), cm.differentials(oracle, rp, cs))
    return _CACHE[key]


# ---- 6. rays ----------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sampler", ["sobol", "halton"])
@pytest.mark.parametrize("kind,lens", CASES, ids=CASE_IDS)
def test_camera_rays_equal_the_model_bit_for_bit(pkg, gpu, oracle, kind, lens, sampler):
    """Every sample of the job and pfilm at the four corners of the full resolution (the environment camera's theta = 0 and theta = pi)."""
    rp, cs, (mo, md), _ = _samples(pkg, oracle, kind, lens, sampler)
    assert len(cs) == 32 * 24 * 4 + 4
    o, d = device_rays(pkg, gpu, rp, cs)
    assert np.array_equal(_bits(o), _bits(mo)), int((_bits(o) != _bits(mo)).any(axis=1).sum())
    assert np.array_equal(_bits(d), _bits(md)), int((_bits(d) != _bits(md)).any(axis=1).sum())
    if kind == "orthographic" and not lens:
        assert (_bits(d) == _bits(d[0])).all() and abs(float(np.linalg.norm(d[0])) - 1.0) > 1e-3   # one direction, not normalised after the scaled camera_to_world
    if kind == "environment":
        # one origin, moved along each direction by its error bound (transform_ray); theta = 0: sin is 0 and both upper corners are the camera's +y axis exactly; theta = pi: sin is nearly 0, the lower corners nearly its -y axis
        assert np.ptp(o, axis=0).max() < 4e-6 and np.array_equal(_bits(d[-4]), _bits(d[-3])) and np.abs(d[-2:] + d[-4]).max() < 1e-6 and np.abs(d[-4]).max() > 0.5


# ---- 7. differentials -------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sampler", ["sobol", "halton"])
@pytest.mark.parametrize("kind,lens", CASES, ids=CASE_IDS)
def test_camera_ray_differentials_equal_the_model_bit_for_bit(pkg, gpu, oracle, kind, lens, sampler):
    rp, cs, _, (mout, mhas) = _samples(pkg, oracle, kind, lens, sampler)
    out, has = device_differentials(pkg, gpu, rp, cs)
    assert np.array_equal(has, mhas)
    assert np.array_equal(_bits(out), _bits(mout)), int((_bits(out) != _bits(mout)).any(axis=1).sum())
    if kind == "environment":
        assert not has.any() and not out.any()   # no generate_ray_differential of its own, and the trait's default leaves rd.diff None
    elif lens:   # orthographic.rs:130,135: the 0.1 and the reused d.z show -- a "corrected" build would be caught
        fixed, _ = cm.differentials(oracle, rp, cs, corrected=True)
        assert (np.abs(mout[:, 9:] - fixed[:, 9:]).max(axis=1) > 1e-3).all() and np.array_equal(mout[:, :9], fixed[:, :9])


def _parent_perspective_differentials(oracle, rp, cs, o, d):
    """camera_ray_differentials as the commit before the cameras wrote it (kern_shade_common.h then; perspective.rs:143-176, transform.rs:565-575, ray.rs:34-41), sample by
    sample in float32 scalars -- a second transcription, independent of camera_model.differentials."""
    m, c2w = [F(v) for v in rp.raster_to_camera], [F(v) for v in rp.camera_to_world]

    def point(t, p):
        x, y, z = p
        q = [x * t[0] + y * t[1] + z * t[2] + t[3], x * t[4] + y * t[5] + z * t[6] + t[7], x * t[8] + y * t[9] + z * t[10] + t[11]]
        w = x * t[12] + y * t[13] + z * t[14] + t[15]
        if w == F(1.0): return q
        inv = F(1.0) / w
        return [q[0] * inv, q[1] * inv, q[2] * inv]
    vector = lambda t, v: [v[0] * t[0] + v[1] * t[1] + v[2] * t[2], v[0] * t[4] + v[1] * t[5] + v[2] * t[6], v[0] * t[8] + v[1] * t[9] + v[2] * t[10]]
    add = lambda a, b: [a[0] + b[0], a[1] + b[1], a[2] + b[2]]
    sub = lambda a, b: [a[0] - b[0], a[1] - b[1], a[2] - b[2]]
    mul = lambda a, s: [a[0] * s, a[1] * s, a[2] * s]

    def normalize(a):
        inv = F(1.0) / np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
        return mul(a, inv)
    zero = [F(0.0)] * 3
    p2t = point(m, zero)
    dxc, dyc = sub(point(m, [F(1.0), F(0.0), F(0.0)]), p2t), sub(point(m, [F(0.0), F(1.0), F(0.0)]), p2t)
    sc = F(1.0) / np.sqrt(F(rp.spp))
    lens_r, focal = F(rp.lens_radius), F(rp.focal_distance)
    dsk = concentric_sample_disk(oracle, cs[:, 3:5]) if lens_r > 0 else None
    out = np.zeros((len(cs), 12), F)
    for i in range(len(cs)):
        pc = point(m, [cs[i, 0], cs[i, 1], F(0.0)])
        if lens_r > 0:
            pl = [dsk[i, 0] * lens_r, dsk[i, 1] * lens_r, F(0.0)]
            dx = normalize(add(pc, dxc)); rx_o, rx_d = pl, normalize(sub(add(zero, mul(dx, focal / dx[2])), pl))
            dy = normalize(add(pc, dyc)); ry_o, ry_d = pl, normalize(sub(add(zero, mul(dy, focal / dy[2])), pl))
        else:
            rx_o = ry_o = zero
            rx_d, ry_d = normalize(add(pc, dxc)), normalize(add(pc, dyc))
        ro, rd = list(o[i]), list(d[i])
        parts = []
        for aux_o, aux_d in ((rx_o, rx_d), (ry_o, ry_d)):
            parts += add(ro, mul(sub(point(c2w, aux_o), ro), sc)) + add(rd, mul(sub(vector(c2w, aux_d), rd), sc))
        out[i] = parts
    return out


@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "lens"])
def test_perspective_differentials_are_what_they_were(pkg, gpu, oracle, lens):
    """The code that moved: the device equals the model, and the model what the parent commit's formulae give."""
    rp = cm.job(pkg, "perspective", lens=lens).render_params()
    _, cs = cm.camera_samples(pkg, oracle, rp)
    cs = np.ascontiguousarray(cs[::7], F)   # (the scalar transcription is slow: every seventh sample, all four sample numbers among them)
    mout, mhas = cm.differentials(oracle, rp, cs)
    mo, md = cm.rays(oracle, rp, cs)
    assert mhas.all() and np.array_equal(_bits(mout), _bits(_parent_perspective_differentials(oracle, rp, cs, mo, md)))
    out, has = device_differentials(pkg, gpu, rp, cs)
    assert has.all() and np.array_equal(_bits(out), _bits(mout))
    o, d = device_rays(pkg, gpu, rp, cs)
    assert np.array_equal(_bits(o), _bits(mo)) and np.array_equal(_bits(d), _bits(md))


# ---- 8. / 9. the render uses those rays: an emissive patchwork at maxdepth 0, and its feature buffers ------------------------------------------------------------------

def _le(i):
    """Distinct per primitive, small dyadic rationals: sums of a pixel's samples are exact."""
    return (0.25 * (1 + i % 4), 0.5 * (1 + (i // 4) % 4), 0.25 * (1 + i // 16))


def _emitters(b, triangles):
    for i, tri in enumerate(triangles):
        b.attribute_begin(); b.area_light_source(L=_le(i))
        b.trianglemesh(np.array(tri, F), np.array([0, 1, 2], np.uint32)); b.attribute_end()


def patchwork(pkg, kind, lens, sampler="sobol"):
    """Orthographic: a ground of 4 x 4 one-sided emissive quads (32 triangles, facing up) and one raised emissive triangle that hides part of it and shows its BACK
    (facing down), all in front of the camera. Environment: a closed box around the camera, each of its 12 triangles its own emitter, facing inwards."""
    b = cm.job(pkg, kind, sampler=sampler, lens=lens, view="oblique" if kind == "orthographic" else "shifted")
    b.integ.update(maxdepth=0)
    b.material("matte", Kd=(0.5, 0.5, 0.5))
    tris = []
    if kind == "orthographic":
        g = np.linspace(-3.0, 3.0, 5)
        for j in range(4):
            for i in range(4):
                p00, p10, p11, p01 = (g[i], 0.0, g[j]), (g[i + 1], 0.0, g[j]), (g[i + 1], 0.0, g[j + 1]), (g[i], 0.0, g[j + 1])
                tris += [(p00, p01, p11), (p00, p11, p10)]   # (n = cross(p0 - p2, p1 - p2) is +y)
        tris.append(((-1.0, 1.0, -0.5), (1.5, 1.0, 0.0), (0.0, 1.0, 1.5)))   # wound the other way: its normal is -y, the camera above sees no emission
    else:
        c = np.array([[x, y, z] for x in (-2.0, 3.0) for y in (-1.0, 2.5) for z in (3.0, 8.5)])   # around the camera at (-.5, 1, 6)
        quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
        centre = c.mean(axis=0)
        for q in quads:
            for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3])):
                p = [c[k] for k in t]
                n = np.cross(p[0] - p[2], p[1] - p[2])
                if np.dot(n, centre - p[0]) < 0: p = [p[0], p[2], p[1]]   # face the inside
                tris.append(tuple(tuple(float(v) for v in x) for x in p))
    _emitters(b, tris)
    return b.world_end() + (np.array(tris, F),)


def _patchwork_reference(pkg, oracle, kind, lens, sampler="sobol"):
    key = ("patch", kind, lens, sampler)
    if key not in _CACHE:
        sd, rp, tris = patchwork(pkg, kind, lens, sampler)
        orc = oracle.scene(sd)
        h = cm.camera_hits(pkg, oracle, orc, rp)
        orc.close()
        hit = h["prim"] != NONE
        prim = np.where(hit, h["prim"], 0).astype(np.int64)
        P = tris[prim]
        n = np.cross((P[:, 0] - P[:, 2]).astype(np.float64), (P[:, 1] - P[:, 2]).astype(np.float64))   # triangle.rs:283; DiffuseAreaLight::l emits where dot(n, w) > 0
        front = hit & (np.einsum("ni,ni->n", n, -h["d"].astype(np.float64)) > 0)
        le = np.array([_le(i) for i in range(len(tris))], F)[prim]
        L = np.where(front[:, None], le, F(0.0)).astype(F)
        sums = box_sums(rp, h, np.ones(len(hit), bool), L, np.zeros((len(hit), 3), F))["albedo"]   # (rgb sums and the weight of EVERY sample: misses splat black)
        r, g, b_ = sums[..., 0], sums[..., 1], sums[..., 2]
        film = np.stack([F(0.412453) * r + F(0.357580) * g + F(0.180423) * b_, F(0.212671) * r + F(0.715160) * g + F(0.072169) * b_,
                         F(0.019334) * r + F(0.119193) * g + F(0.950227) * b_, sums[..., 3]], -1).astype(F)   # Film::merge_film_tile: the RGB sums to XYZ (spectrum.rs:472-482)
        _CACHE[key] = (sd, rp, h, hit, front, film)
    return _CACHE[key]


@pytest.mark.parametrize("kind,lens", CASES, ids=CASE_IDS)
def test_the_render_uses_the_model_rays(pkg, gpu, oracle, kind, lens):
    """maxdepth 0: path.rs adds the first hit's emission and stops. Per pixel the sum over its samples of Le[prim] of the oracle's hit of the model's ray -- 0 where
    the ray misses or meets a back face --, weight = the sample count. No sample is left out: the rays are bit-equal and the project's hits are the oracle's."""
    sd, rp, h, hit, front, want = _patchwork_reference(pkg, oracle, kind, lens)
    n = 32 * 24 * 4
    assert len(hit) == n and front.sum() > 0.3 * n
    if kind == "orthographic":
        assert (~hit).sum() > 0.02 * n and (hit & ~front).sum() > 0.01 * n and len(np.unique(h["prim"][hit])) >= 20   # misses, the raised triangle's back, most quads
    else:
        assert hit.all() and front.all() and len(np.unique(h["prim"])) >= 8                                           # a closed box seen from inside (the window spans half the azimuth)
    g = pkg.Scene(gpu, sd)
    film = g.render(rp)
    print("%s lens=%s: largest |film - expected| %.3g of %.3g" % (kind, lens, np.abs(film[..., :3] - want[..., :3]).max(), want[..., :3].max()))
    assert_same_film(film, want, resolved=(g.resolve, g.resolve, 1e-4))   # parity.py's defaults for a device film against an oracle film
    c = g.counters()
    assert c["camera_rays"] == n and c["intersect_tests"] == n
    assert c["film_splats"] == int(want[..., 3].sum())


@pytest.mark.parametrize("kind,lens", CASES, ids=CASE_IDS)
def test_feature_buffers_under_the_new_cameras(pkg, gpu, oracle, kind, lens):
    """pt_aov_render on the same scenes: depth, normal and albedo sums from the model's hits with aov_reference's helpers, tolerances of test_aov.py's identity 3."""
    sd, rp, h, _, _, _ = _patchwork_reference(pkg, oracle, kind, lens)
    key = ("aov", kind, lens)
    if key not in _CACHE:
        shit, albedo, normal, smooth = sample_values(pkg, oracle, sd, h)
        assert not smooth.any() and not np.isnan(albedo).any()
        _CACHE[key] = box_sums(rp, h, shit, albedo, normal)
    ref = _CACHE[key]
    g = pkg.Scene(gpu, sd)
    got = g.render_aov(rp)
    for plane in ("albedo", "normal", "depth"):
        assert np.array_equal(got[plane][..., -1], ref[plane][..., -1]), plane + ": weights differ"
        np.testing.assert_allclose(got[plane][..., :-1], ref[plane][..., :-1], rtol=2e-6, atol=1e-7)
    assert ref["depth"][..., 0].max() > 1.0 and np.abs(ref["albedo"][..., :3] - 0.5 * ref["normal"][..., 3:]).max() < 1e-6   # Kd = 0.5 on every sample that hits
    assert g.counters()["camera_rays"] == 32 * 24 * 4


# ---- 10. / 11. texture filtering at the first hit ------------------------------------------------------------------------------------------------------------------------

# The ground of aov_reference (y = 0, 6 x 6) carries a trilinear 16 x 16 image map through a planar mapping, lit as identity 1 of aov_reference: matte, sigma 0, one distant
# light of L = pi along the normal, maxdepth 1 -- a hitting sample's radiance is Kd.
#
# Orthographic, straight down from y = 5 (LookAt up = -z: camera x is world -x, camera y world -z), screen window [-4, 4] x [-1, 1] over the full 64 x 32 frame:
#   dx_camera = 8 / 64 = 2^-3 along x, dy_camera = 2 / 32 = 2^-4 along y -- pixels are not square;
#   dpdx = dx_camera in world space * 1 / sqrt(4) = 2^-4 along x, dpdy = 2^-5 along z (interaction.rs:262-342 on a plane the rays meet at a right angle);
#   planar mapping v1 = (2, 0, 0), v2 = (0, 0, 1/2): |dudx| = 2 * 2^-4 = 2^-3, |dvdy| = 2^-5 / 2 = 2^-6, dvdx = dudy = 0 -- only dx sets the width, and a build
#   that gave dx the y pixel's size would get |dudx| = 2^-4, |dvdy| = 2^-5: another width;
#   width = max(|dudx|, |dvdx|, |dudy|, |dvdy|) = 2^-3 of the texture: k = 3. (MIPMap::lookup2, mipmap.rs:225-233, hands the maximum itself to lookup(); the
#   issue that asked for this test writes the width as twice the maximum, as pbrt-v3's C++ has it. The reference this project follows has no factor 2, the device
#   is held to it by the oracle's trilinear renders (test_aov.py identity 1, test_gpu_parity.py), and so the arithmetic here follows mipmap.rs.)
# MIPMap::lookup (mipmap.rs:202-223): level = n_levels - 1 + log2(width) = 4 - 3 = 1 of the 16 x 16 map's five levels (16, 8, 4, 2, 1) -- an interior level, delta = 0:
# lerp(0, triangle(1), triangle(2)) = triangle(1). A missing 1 / sqrt(spp) gives level 2. The device's dpdx carries the roundings of the plane intersection; log2 of a
# width of 2^-3 (1 +- 1e-6) moves the level by 1.5e-6, so the blend takes 1.5e-6 of the neighbouring level -- of texels in [0, 1], below the comparison's 3e-6.
#
# Environment: the camera's rays carry no differentials, so every first hit is filtered with width 0: level = 4 + log2(1e-8) < 0 -> triangle(0). A build that gave this
# camera the trait's default differentials (rays through pfilm + 1) would filter with widths of a pixel's footprint and land on levels 1 to 3.
TEX_V1, TEX_V2, TEX_DELTA = (2.0, 0.0, 0.0), (0.0, 0.0, 0.5), (0.13, 0.31)


def filter_scene(pkg, kind):
    if kind == "orthographic":
        b = cm.job(pkg, kind, view="down", screenwindow=(-4.0, 4.0, -1.0, 1.0))
    else:
        b = cm.job(pkg, kind, view="none")
        b.cam.update(c2w=pkg.host.Transform.translate((0.2, 0.6, -0.4)) * pkg.host.Transform.rotate(25.0, (1.0, 0.2, 0.0)))   # above the ground, tilted
    b.integ.update(maxdepth=1, kind="path")
    _light(b, UP)
    b.texture("kd", "color", "imagemap", pixels=pkg.scenes.test_image(16, 16, seed=4), trilinear=True, mapping="planar", v1=TEX_V1, v2=TEX_V2, udelta=TEX_DELTA[0], vdelta=TEX_DELTA[1])
    b.material("matte", Kd="kd", sigma=0.0)
    b.trianglemesh(GROUND_P, GROUND_I, UV=GROUND_UV)
    levels = b.images[-1]["levels"]
    return b.world_end() + (levels,)


def _filter_reference(pkg, oracle, kind, level):
    key = ("filter", kind)
    if key not in _CACHE:
        sd, rp, levels = filter_scene(pkg, kind)
        assert [l.shape[0] for l in levels] == [16, 8, 4, 2, 1]
        orc = oracle.scene(sd)
        h = cm.camera_hits(pkg, oracle, orc, rp)
        orc.close()
        hit = h["prim"] != NONE
        tri = GROUND_P[GROUND_I.reshape(2, 3)][np.where(hit, h["prim"], 0)]
        b = h["b"]
        p = (tri[:, 0] * b[:, 0:1] + tri[:, 1] * b[:, 1:2] + tri[:, 2] * b[:, 2:3]).astype(F)   # triangle.rs:265: the hit point from the barycentrics
        v1, v2 = np.array(TEX_V1, F), np.array(TEX_V2, F)
        u = (F(TEX_DELTA[0]) + (p[:, 0] * v1[0] + p[:, 1] * v1[1] + p[:, 2] * v1[2])).astype(F)   # PlanarMapping2D::map (texture.rs:136-152)
        v = (F(TEX_DELTA[1]) + (p[:, 0] * v2[0] + p[:, 1] * v2[1] + p[:, 2] * v2[2])).astype(F)
        kd = np.zeros((len(hit), 3), F)
        for i in np.nonzero(hit)[0]:
            kd[i] = pkg.host._triangle(levels[level], u[i:i + 1], v[i:i + 1])[0, 0]
        other = np.zeros((len(hit), 3), F)   # what a neighbouring level would give: the test tells the levels apart
        for i in np.nonzero(hit)[0]:
            other[i] = pkg.host._triangle(levels[level + 1], u[i:i + 1], v[i:i + 1])[0, 0]
        sums = box_sums(rp, h, np.ones(len(hit), bool), kd, np.zeros((len(hit), 3), F))["albedo"]
        wrong = box_sums(rp, h, np.ones(len(hit), bool), other, np.zeros((len(hit), 3), F))["albedo"]
        _CACHE[key] = (sd, rp, hit, sums, wrong)
    return _CACHE[key]


@pytest.mark.parametrize("kind,level", [("orthographic", 1), ("environment", 0)], ids=["orthographic", "environment"])
def test_texture_filtering_at_the_first_hit(pkg, gpu, oracle, kind, level):
    sd, rp, hit, want, wrong = _filter_reference(pkg, oracle, kind, level)
    assert 0.3 * len(hit) < hit.sum() and (kind == "orthographic" or hit.sum() < 0.9 * len(hit))   # (the environment camera also looks up, past the ground)
    w = want[..., 3]
    assert (np.abs(want[..., :3] - wrong[..., :3]).max(axis=-1) / w > 100 * TOL).mean() > 0.25   # the next level is another picture
    g = pkg.Scene(gpu, sd)
    film = g.render(rp)                                      # k_shade's caller of camera_ray_differentials: radiance = Kd
    assert np.array_equal(film[..., 3], w)
    err = np.abs(film_rgb_sums(pkg, film).astype(np.float64) - want[..., :3]).max(axis=-1) / w
    albedo = g.render_aov(rp, planes=("albedo",))["albedo"]   # the feature kernel's caller: the albedo plane = Kd
    assert np.array_equal(albedo[..., 3], w)
    err_aov = np.abs(albedo[..., :3].astype(np.float64) - want[..., :3]).max(axis=-1) / w
    print("first-hit filtering, %s: largest error per unit weight: film %.3g, albedo plane %.3g (level %d; against level %d: %.3g)" %
          (kind, err.max(), err_aov.max(), level, level + 1, (np.abs(film_rgb_sums(pkg, film) - wrong[..., :3]).max(axis=-1) / w).max()))
    assert err.max() <= TOL and err_aov.max() <= TOL


# ---- 12. the drivers inherit it -------------------------------------------------------------------------------------------------------------------------------------------

def _textured(pkg, kind, integrator="path"):
    b = pkg.scenes.textured(xres=32, yres=24, spp=4)
    if kind == "orthographic": b.cam.update(kind=kind, screenwindow=(-4.0, 4.0, -3.0, 3.0), focaldistance=1e30, shutteropen=0.0, shutterclose=0.0)
    else: b.cam.update(kind=kind, focaldistance=1e30, shutteropen=1.0, shutterclose=1.0)
    if integrator == "ao": b.integ.update(kind="ao", nsamples=4, cossample=True)
    return b.world_end()


@pytest.mark.parametrize("kind", ["orthographic", "environment"])
def test_every_driver_renders_under_the_new_cameras(pkg, gpu, kind):
    A = pkg._abi
    sd, rp = _textured(pkg, kind)
    assert rp.camera_type == {"orthographic": 1, "environment": 2}[kind]
    g = pkg.Scene(gpu, sd)
    whole = g.render(rp); c = g.counters()
    n = 32 * 24 * 4
    assert c["camera_rays"] == n and sum(c["path_length_hist"]) == n and np.isfinite(whole).all() and whole[..., :3].max() > 0
    assert (whole[..., 3] > 0).all()
    again = g.render(rp)
    assert_same_render(again, whole, g.counters(), c)                              # two renders of one job
    parts = g.render(rp, samples=(0, 2)); g.render(rp, film=parts, samples=(2, 2))
    assert_same_film(parts, whole)                                                 # sample ranges add up
    ntx, nty = g.tile_grid(rp)
    tiles = g.render_tiles(rp, (0, rp.spp), np.arange(ntx * nty, dtype=np.uint32))
    assert_same_film(tiles, whole); assert g.counters()["camera_rays"] == n        # a list of all tiles is the whole render
    multi = pkg.MultiScene(gpu, sd, [0, 0])
    assert_same_render(multi.render(rp), whole, multi.counters(), c)               # two replicas on one device
    rgb, film = g.render_denoised(rp)
    assert np.isfinite(rgb).all() and rgb.max() > 0 and np.isfinite(film).all()
    assert_same_film(film, whole)
    sd_ao, rp_ao = _textured(pkg, kind, "ao")
    assert rp_ao.integrator == pkg._abi_ao.PT_INTEGRATOR_AO and rp_ao.camera_type == rp.camera_type
    ao = pkg.Scene(gpu, sd_ao)
    f = ao.render(rp_ao)
    assert np.isfinite(f).all() and f[..., :3].max() > 0 and ao.counters()["camera_rays"] == n


# ---- 13. error statuses ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_an_unknown_camera_type_is_an_invalid_argument_everywhere(pkg, gpu):
    A, AOV = pkg._abi, pkg._abi_aov
    sd, rp = _textured(pkg, "orthographic")
    sd_ao, rp_ao = _textured(pkg, "orthographic", "ao")
    g, ao = pkg.Scene(gpu, sd), pkg.Scene(gpu, sd_ao)
    multi = pkg.MultiScene(gpu, sd, [0, 0])
    good = g.render(rp)
    rp.camera_type = 3; rp_ao.camera_type = 3
    film = np.zeros_like(good)
    sums = {k: np.zeros(film.shape[:2] + (AOV.CHANNELS[k],), F) for k in AOV.PLANES}
    cs = np.zeros((4, 5), F); o = np.zeros((4, 3), F); d = np.zeros((4, 3), F); out = np.zeros((4, 12), F); has = np.zeros(4, np.uint8)
    calls = {
        "pt_render": lambda: gpu.lib.pt_render(g.h, C.byref(rp), film.ctypes.data_as(C.c_void_p), 0),
        "pt_render_samples": lambda: gpu.lib.pt_render_samples(g.h, C.byref(rp), 0, 2, film.ctypes.data_as(C.c_void_p), 0),
        "pt_ao_render": lambda: gpu.ao.pt_ao_render(ao.h, C.byref(rp_ao), C.byref(ao.ao_params()), film.ctypes.data_as(C.c_void_p), 0),
        "pt_aov_render": lambda: gpu.aov.pt_aov_render(g.h, C.byref(rp), C.byref(AOV.buffers(sums)), 0),
        "pt_camera_rays": lambda: gpu.lib.pt_camera_rays(C.byref(rp), 4, _fp(pkg, cs), _fp(pkg, o), _fp(pkg, d)),
        "pt_camera_ray_differentials": lambda: gpu.lib.pt_camera_ray_differentials(C.byref(rp), 4, _fp(pkg, cs), _fp(pkg, out), has.ctypes.data_as(C.POINTER(C.c_uint8))),
        "pt_multi_render": lambda: gpu.lib.pt_multi_render(multi.h, C.byref(rp), film.ctypes.data_as(C.c_void_p), 0),
    }
    for name, call in calls.items():
        st = call()
        msg = gpu.lib.pt_last_error().decode(errors="replace")
        assert st == A.PT_ERR_INVALID_ARG and "camera_type 3" in msg, (name, st, msg)
    assert not film.any() and not any(v.any() for v in sums.values())
    rp.camera_type = 1
    assert_same_film(g.render(rp), good)        # the scenes stay usable
    assert_same_film(multi.render(rp), good)


# ---- 14. kernel symbols ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_the_new_cameras_run_their_own_generate_kernel_and_nothing_else_changes(pkg, gpu):
    """(A perspective render's "generate": "k_generate" is pinned by test_kernel_symbols.py.)"""
    maps = {}
    for kind in ("perspective", "orthographic", "environment"):
        b = pkg.scenes.textured(xres=32, yres=24, spp=4)
        if kind != "perspective": b.cam.update(kind=kind, screenwindow=(-4.0, 4.0, -3.0, 3.0))
        sd, rp = b.world_end()
        g = pkg.Scene(gpu, sd)
        g.render(rp)
        maps[kind] = {s["name"]: s["kernel"] for s in g.kernel_stats() if s["launches"] > 0}
    print(maps)
    assert maps["perspective"]["generate"] == "k_generate"
    assert maps["orthographic"]["generate"] == "k_generate_cam<1>" and maps["environment"]["generate"] == "k_generate_cam<2>"
    rest = lambda m: {k: v for k, v in m.items() if k != "generate"}
    assert rest(maps["orthographic"]) == rest(maps["perspective"]) and rest(maps["environment"]) == rest(maps["perspective"])
