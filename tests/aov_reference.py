"""Test infrastructure of the feature-buffer tests (test_aov_reference.py, test_aov.py, test_aov_frontend.py): the scenes of the three reference identities that hold
pt_aov_render against the unchanged oracle, and the numpy side of the third.

1. Albedo against an oracle render: matte, sigma 0, maxdepth 1, one distant light of L = pi along the normal of planar geometry -- every hitting sample's radiance is Kd.
2. Normals against three oracle renders: the same with Kd = 1 and a light l_i a few degrees off the vertical -- a sample's radiance is dot(l_i, n).
3. Depth, normals and hit identity against the oracle's first hits: orc_sobol_samples / orc_halton_samples -> orc_camera_rays -> orc_trace_closest give prim, t and the
   barycentrics of every camera sample; numpy forms the sums under the box filter (FilmTile::add_sample's footprint, a pixel's own samples in sample order)."""
import ctypes as C
import math

import numpy as np
import camera_model
from model_math import F, NONE, cross, dm_map, dm_sin, dot, normalize, transform_ray, xf_normal_inv

XRES, YRES, SPP = 32, 24, 4
_norm = lambda v: tuple(float(x) for x in np.asarray(v, np.float64) / np.linalg.norm(v))
LIGHTS = (_norm((0.3, 1.0, 0.1)), _norm((-0.2, 1.0, 0.25)), _norm((0.05, 1.0, -0.3)))
FOURTH_LIGHT = _norm((0.1, 1.0, 0.2))
UP = (0.0, 1.0, 0.0)
KD_CONST = (0.7, 0.45, 0.2)


def _builder(pkg, sampler="sobol", lensradius=0.0, xres=XRES, yres=YRES, spp=SPP):
    b = pkg.host.SceneBuilder()
    b.film.update(xres=xres, yres=yres); b.spp = spp; b.sampler = sampler
    b.integ.update(maxdepth=1, kind="path")
    b.look_at((0.3, 2.5, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)); b.camera(fov=40.0, lensradius=lensradius, focaldistance=6.5)
    b.world_begin()
    return b


def _light(b, direction):
    b.light_source("distant", L=(math.pi, math.pi, math.pi), from_=direction, to=(0.0, 0.0, 0.0))


GROUND_P = np.array([(-3.0, 0.0, -3.0), (-3.0, 0.0, 3.0), (3.0, 0.0, 3.0), (3.0, 0.0, -3.0)], F)
GROUND_I = np.array([0, 1, 2, 0, 2, 3], np.uint32)
GROUND_UV = np.array([[0, 0], [0, 1], [1, 1], [1, 0]], F)


def albedo_scene(pkg, kd="const", bump=False, shell=False, **kw):
    """Identity 1. kd: "const", or a texture through the planar mapping of the ground's plane -- "checker" (closed-form antialiasing), "ewa", "trilinear" (image maps).
    bump: normal_scene's bump map on the ground as well (the matte BSDF then sees another normal: no identity, a scene for the planes' own promises).
    shell: a sphere without a material (a medium-interface shell, api.rs:597) stands over the middle of the ground, in the way of about a fifth of the camera rays."""
    scenes = pkg.scenes
    b = _builder(pkg, **kw)
    _light(b, UP)
    plane = dict(mapping="planar", v1=(0.45, 0.0, 0.0), v2=(0.0, 0.0, 0.45), udelta=0.13, vdelta=0.31)
    if kd == "const":
        b.material("matte", Kd=KD_CONST, sigma=0.0)
    else:
        if kd == "checker":
            b.texture("kd", "color", "checkerboard", aamode="closedform", tex1=(0.85, 0.8, 0.7), tex2=(0.1, 0.15, 0.3), **plane)
        else:
            b.texture("kd", "color", "imagemap", pixels=scenes.test_image(16, 16, seed=4), trilinear=(kd == "trilinear"), **plane)
        b.material("matte", Kd="kd", sigma=0.0)
    if bump:
        b.texture("bump", "float", "imagemap", pixels=scenes.test_image(16, 16, seed=6), scale=0.08, uscale=6.0, vscale=6.0)
        b.material("matte", Kd=KD_CONST if kd == "const" else "kd", sigma=0.0, bumpmap="bump")
    b.trianglemesh(GROUND_P, GROUND_I, UV=GROUND_UV)
    if shell:
        b.attribute_begin(); b.material("none"); b.translate(0.2, 1.3, 0.6); b.sphere(radius=1.2); b.attribute_end()
    return b.world_end()


def undulating_mesh(n=12, amplitude=0.08):
    """The 6 x 6 ground as n x n quads with y = amplitude * sin(1.7 x) * cos(1.3 z) and the surface's analytic vertex normals."""
    g = np.linspace(-3.0, 3.0, n + 1)
    x, z = np.meshgrid(g, g, indexing="xy")
    x, z = x.ravel(), z.ravel()
    y = amplitude * np.sin(1.7 * x) * np.cos(1.3 * z)
    dydx = amplitude * 1.7 * np.cos(1.7 * x) * np.cos(1.3 * z); dydz = -amplitude * 1.3 * np.sin(1.7 * x) * np.sin(1.3 * z)
    N = np.stack([-dydx, np.ones_like(x), -dydz], 1); N /= np.linalg.norm(N, axis=1, keepdims=True)
    i0 = (np.arange(n)[None, :] + (n + 1) * np.arange(n)[:, None]).ravel()
    idx = np.concatenate([np.stack([i0, i0 + n + 1, i0 + n + 2], 1), np.stack([i0, i0 + n + 2, i0 + 1], 1)])   # (+y faces)
    return np.stack([x, y, z], 1).astype(F), idx.astype(np.uint32), N.astype(F)


def normal_scene(pkg, surface, light, **kw):
    """Identity 2. surface: "bump" (the ground quad under a float image-map bump: scale 0.08, uscale = vscale = 6) or "mesh" (undulating_mesh)."""
    scenes = pkg.scenes
    b = _builder(pkg, **kw)
    _light(b, light)
    if surface == "bump":
        b.texture("bump", "float", "imagemap", pixels=scenes.test_image(16, 16, seed=6), scale=0.08, uscale=6.0, vscale=6.0)
        b.material("matte", Kd=(1.0, 1.0, 1.0), sigma=0.0, bumpmap="bump")
        b.trianglemesh(GROUND_P, GROUND_I, UV=GROUND_UV)
    else:
        b.material("matte", Kd=(1.0, 1.0, 1.0), sigma=0.0)
        P, I, N = undulating_mesh()
        b.trianglemesh(P, I, N=N)
    return b.world_end()


def film_rgb_sums(pkg, film):
    """xyz_to_rgb of a film's XYZ sums, per pixel (float32, spectrum.rs:484-492)."""
    x, y, z = (film[..., k].astype(F) for k in range(3))
    return np.stack([F(3.240479) * x - F(1.537150) * y - F(0.498535) * z, F(-0.969256) * x + F(1.875991) * y + F(0.041556) * z,
                     F(0.055648) * x - F(0.204043) * y + F(1.057311) * z], -1).astype(F)


# ---- identity 3: the oracle's first hits -> numpy sums ------------------------------------------------------------------------------------------------------------

def oracle_rays(oracle, rp, cs):
    """orc_camera_rays: the oracle's own (perspective) camera for the camera samples cs (N, 5)."""
    fp = oracle.A.fp
    o = np.zeros((len(cs), 3), F); d = np.zeros((len(cs), 3), F)
    assert oracle.lib.orc_camera_rays(C.byref(rp), len(cs), cs.ctypes.data_as(fp), o.ctypes.data_as(fp), d.ctypes.data_as(fp)) == 0
    return o, d


def camera_hits(pkg, oracle, orc, rp, first=0, n=None):
    """camera_model.camera_hits in the oracle's words throughout: its samplers' camera samples, its camera's rays, its first hits."""
    return camera_model.camera_hits(pkg, oracle, orc, rp, first, n, oracle_rays)


def hit_fractions(h):
    hit = h["prim"] != NONE
    return float(hit.mean()), float((~hit).mean())


def _m4(a):
    return np.array(list(a), np.float64).reshape(4, 4)


def _point(m, p):
    q = p @ m[:3, :3].T + m[:3, 3]
    return q


def _normal(m_inv, n):   # Transform::transform_normal: the inverse's transpose
    return n @ m_inv[:3, :3]


def leaf_albedo(pkg, sd, mi):
    """The albedo table of include/mi355aov.h for material `mi` with constant parameters (float64; None when a parameter it reads is textured)."""
    A = pkg._abi
    m = sd.materials[mi]
    v = lambda a: np.maximum(np.array(list(a), np.float64), 0.0)
    tex = lambda *slots: any(m.tex[s] >= 0 for s in slots)
    if m.type == A.PT_MAT_MIX:
        if tex(A.PT_MP_KD): return None
        a1, a2 = leaf_albedo(pkg, sd, m.mix[0]), leaf_albedo(pkg, sd, m.mix[1])
        if a1 is None or a2 is None: return None
        s1 = v(m.kd)
        return s1 * a1 + np.maximum(1.0 - s1, 0.0) * a2
    if m.type in (A.PT_MAT_MIRROR, A.PT_MAT_GLASS, A.PT_MAT_SUBSURFACE):
        return None if tex(A.PT_MP_KR) else v(m.kr)
    if m.type == A.PT_MAT_METAL:   # fr_conductor(1, 1, eta, k) (reflection.rs:54-76) at cos = 1
        if tex(A.PT_MP_ETA_RGB, A.PT_MP_K_RGB): return None
        eta, k = np.array(list(m.eta_rgb), np.float64), np.array(list(m.k_rgb), np.float64)
        t0 = eta * eta - k * k
        a2b2 = np.sqrt(t0 * t0 + 4.0 * eta * eta * k * k)
        t1 = a2b2 + 1.0; a = np.sqrt(0.5 * (a2b2 + t0)); t2 = 2.0 * a
        rs = (t1 - t2) / (t1 + t2)
        return np.maximum(0.5 * (rs + rs), 0.0)   # (sin = 0: rp = rs)
    if m.type == A.PT_MAT_UBER:
        return None if tex(A.PT_MP_OPACITY, A.PT_MP_KD) else v(m.opacity) * v(m.kd)
    return None if tex(A.PT_MP_KD) else v(m.kd)


def sample_values(pkg, oracle, sd, h):
    """Per camera sample of camera_hits: hit (bool), albedo (N, 3; NaN where the material's parameters are textured), the shading normal facing the camera (N, 3) and
    smooth (bool). The normal of a flat triangle, a sphere or a disk is formed in the device's own float32 arithmetic (tests/model_math.py), through the instance the hit lies in --
    the one of the primitive's object that maps the hit point back onto the primitive. A triangle with vertex normals (smooth) gets normalize(sum of b_i N_i) in
    float64: its shading normal is that direction renormalised three times over (triangle.rs:300-345), which identity 2 holds against the oracle."""
    A = pkg._abi
    N = len(h["prim"])
    hit = h["prim"] != NONE
    albedo = np.zeros((N, 3)); normal = np.zeros((N, 3)); smooth_all = np.zeros(N, bool)
    rows = np.nonzero(hit)[0]
    prim = h["prim"][rows].astype(np.int64)
    t32, o32, d32 = h["t"][rows], h["o"][rows], h["d"][rows]
    t, b, o, d = t32.astype(np.float64), h["b"][rows].astype(np.float64), o32.astype(np.float64), d32.astype(np.float64)
    mat = sd.prim_material[prim]
    assert (mat != NONE).all(), "identity 3 is for scenes whose primitives all carry a material"
    for mi in np.unique(mat):
        a = leaf_albedo(pkg, sd, int(mi))
        albedo[rows[mat == mi]] = np.nan if a is None else a
    pw = o + t[:, None] * d
    sh = sd.prim_shape[prim].astype(np.int64); tri = (sh >> 30) == A.PT_SHAPE_TRIANGLE; index = sh & 0x3FFFFFFF
    n = len(rows)
    q = np.zeros((n, 3))   # a triangle hit's point in its object's space
    vid = sd.idx[index[tri]].astype(np.int64) if tri.any() else np.zeros((0, 3), np.int64)
    if tri.any():
        P = sd.P.astype(np.float64)
        q[tri] = b[tri][:, :1] * P[vid[:, 0]] + b[tri][:, 1:2] * P[vid[:, 1]] + b[tri][:, 2:] * P[vid[:, 2]]
    quadrics = {int(k): (sd.spheres[int(k)], _m4(sd.spheres[int(k)].world_to_object)) for k in np.unique(index[~tri])}

    def residual(sel, i2w, w2i):   # how far the instance (i2w, w2i) leaves the hits `sel` from their primitives
        r = np.zeros(int(sel.sum()))
        ts = tri[sel]
        r[ts] = np.linalg.norm(_point(i2w, q[sel][ts]) - pw[sel][ts], axis=1)
        for k, (S, w2o) in quadrics.items():
            m = (~ts) & (index[sel] == k)
            if m.any():
                ql = _point(w2o, _point(w2i, pw[sel][m]))
                r[m] = np.abs(ql[:, 2] - S.z_min) if S.kind == A.PT_QUADRIC_DISK else np.abs(np.linalg.norm(ql, axis=1) - S.radius)
        return r

    eye = np.eye(4, dtype=F).ravel()
    w2i = np.tile(eye, (n, 1)); through = np.zeros(n, bool)   # per hit: the instance's world_to_instance (float32, row major); an instance that is no identity
    if sd.top_refs is not None:
        owner = np.full(len(sd.prim_shape), -1)
        for k in range(sd.n_objects):
            owner[sd.objects[k].first_prim:sd.objects[k].first_prim + sd.objects[k].n_prims] = k
        for k in np.unique(owner[prim]):
            if k < 0: continue
            sel = owner[prim] == k
            cands = [I for I in list(sd.instances)[:sd.n_instances] if I.object == k]
            res = np.stack([residual(sel, _m4(I.instance_to_world), _m4(I.world_to_instance)) for I in cands])
            assert (res.min(axis=0) < 1e-3).all()
            best = res.argmin(axis=0)
            w2i[sel] = np.stack([np.array(list(I.world_to_instance), F) for I in cands])[best]
            through[sel] = np.array([not np.array_equal(np.array(list(I.instance_to_world), F), eye) for I in cands])[best]
    lo, ld = transform_ray(w2i, o32, d32)   # TransformedPrimitive::intersect (primitive.rs:58-80)
    lo, ld = np.where(through[:, None], lo, o32), np.where(through[:, None], ld, d32)
    n32 = np.zeros((n, 3), F)
    if tri.any():
        P32 = sd.P
        n32[tri] = normalize(cross(P32[vid[:, 0]] - P32[vid[:, 2]], P32[vid[:, 1]] - P32[vid[:, 2]]))   # triangle.rs:283
    for k, (S, _) in quadrics.items():
        m = (~tri) & (index == k)
        w2o = np.array(list(S.world_to_object), F)
        so, sdir = transform_ray(w2o, lo[m], ld[m])
        ph = (so + sdir * t32[m][:, None]).astype(F)
        r, phi_max = F(S.radius), F(S.phi_max)
        if S.kind == A.PT_QUADRIC_DISK:   # disk.rs:78-96
            r_hit = np.sqrt(ph[:, 0] * ph[:, 0] + ph[:, 1] * ph[:, 1])
            dpdu = np.stack([-phi_max * ph[:, 1], phi_max * ph[:, 0], np.zeros_like(r_hit)], 1)
            flat = np.stack([ph[:, 0], ph[:, 1], np.zeros_like(r_hit)], 1)
            dpdv = (flat * (F(S.inner_radius) - r)).astype(F) * (F(1.0) / r_hit)[:, None]
        else:   # sphere.rs:130-176: near the poles many ulps from the radial direction (:160-176 form it from sin(acos(z / r))) -- the reference's normal all the same
            ph = (ph * (r / np.sqrt(dot(ph, ph)))[:, None]).astype(F)
            ph[:, 0] = np.where((ph[:, 0] == 0) & (ph[:, 1] == 0), F(1e-5) * r, ph[:, 0])
            theta = dm_map(oracle.lib.orc_dm_acos, np.clip(ph[:, 2] / r, F(-1.0), F(1.0)))
            inv = F(1.0) / np.sqrt(ph[:, 0] * ph[:, 0] + ph[:, 1] * ph[:, 1])
            cos_phi, sin_phi = ph[:, 0] * inv, ph[:, 1] * inv
            dpdu = np.stack([-phi_max * ph[:, 1], phi_max * ph[:, 0], np.zeros_like(inv)], 1)
            dpdv = np.stack([ph[:, 2] * cos_phi, ph[:, 2] * sin_phi, -r * dm_sin(oracle, theta)], 1) * (F(S.theta_max) - F(S.theta_min))
        nq = normalize(cross(dpdu.astype(F), dpdv.astype(F)))
        n32[m] = normalize(xf_normal_inv(w2o, nq))
    n32 = np.where(through[:, None], normalize(xf_normal_inv(w2i, n32)), n32)   # transform_surface_interaction (transform.rs:607-636)
    n32 = np.where((dot(n32, -d32) < 0)[:, None], -n32, n32)
    nw = n32.astype(np.float64)
    if tri.any() and sd.N is not None:
        smooth = np.zeros(n, bool)
        smooth[tri] = (sd.tri_flags[index[tri]] & A.PT_TRI_HAS_N) != 0
        if smooth.any():
            Nv, bs, vs = sd.N.astype(np.float64), b[smooth], sd.idx[index[smooth]].astype(np.int64)
            ns = bs[:, :1] * Nv[vs[:, 0]] + bs[:, 1:2] * Nv[vs[:, 1]] + bs[:, 2:] * Nv[vs[:, 2]]
            ns = np.einsum("nj,nji->ni", ns, w2i[smooth].astype(np.float64).reshape(-1, 4, 4)[:, :3, :3])   # Transform::transform_normal: the inverse's transpose
            ns /= np.linalg.norm(ns, axis=1, keepdims=True)
            nw[smooth] = np.where((np.einsum("ni,ni->n", ns, -d[smooth]) < 0.0)[:, None], -ns, ns)
            smooth_all[rows[smooth]] = True
    normal[rows] = nw
    return hit, albedo, normal, smooth_all


def box_sums(rp, h, hit, albedo, normal):
    """FilmTile::add_sample (film.rs:292-331) of every sample of camera_hits in float32 under the box filter: {"albedo": (H, W, 4), "normal": (H, W, 4),
    "depth": (H, W, 2)}. A pixel's own samples are added first, in sample order (as the device's pixel threads add them); the splats that a sample on a pixel's edge
    sends to a neighbour follow."""
    cb, sb = rp.cropped_pixel_bounds, rp.sample_bounds
    assert list(rp.filter_radius) == [0.5, 0.5] and list(sb) == list(cb)
    W, H, n = cb[2] - cb[0], cb[3] - cb[1], h["n"]
    rx, ry = F(rp.filter_radius[0]), F(rp.filter_radius[1])
    table = np.array(list(rp.filter_table), F)
    val = np.zeros((len(hit), 10), F)
    val[:, :3] = np.where(hit[:, None], albedo, 0.0); val[:, 3] = 1.0
    val[:, 4:7] = normal; val[:, 7] = hit; val[:, 8] = np.where(hit, h["t"], 0.0); val[:, 9] = hit
    dx, dy = (h["pfilm"][:, 0] - F(0.5)).astype(F), (h["pfilm"][:, 1] - F(0.5)).astype(F)
    weight = lambda x, y, i: table[np.minimum(np.floor(np.abs((y.astype(F) - dy[i]) * (F(1.0) / ry) * F(16.0))), 15).astype(np.int64) * 16 +
                                   np.minimum(np.floor(np.abs((x.astype(F) - dx[i]) * (F(1.0) / rx) * F(16.0))), 15).astype(np.int64)]
    every = np.arange(len(hit))
    own = (val * weight(h["pix"][:, 0], h["pix"][:, 1], every)[:, None]).astype(F).reshape(H * W, n, 10)
    out = np.zeros((H * W, 10), F)
    for s in range(n):
        out += own[:, s]
    out = out.reshape(H, W, 10)
    x0 = np.maximum(np.ceil(dx - rx), cb[0]).astype(np.int64); x1 = np.minimum(np.floor(dx + rx) + 1, cb[2]).astype(np.int64)
    y0 = np.maximum(np.ceil(dy - ry), cb[1]).astype(np.int64); y1 = np.minimum(np.floor(dy + ry) + 1, cb[3]).astype(np.int64)
    for i in np.nonzero((x1 - x0 > 1) | (y1 - y0 > 1))[0]:
        px, py = h["pix"][i]
        for y in range(y0[i], y1[i]):
            for x in range(x0[i], x1[i]):
                if x != px or y != py:
                    out[y - cb[1], x - cb[0]] += (val[i] * weight(np.int64(x), np.int64(y), i)).astype(F)
    return {"albedo": out[..., :4].copy(), "normal": out[..., 4:8].copy(), "depth": out[..., 8:].copy()}


_CACHE = {}


def first_hit_reference(pkg, oracle, key, sd, rp):
    """(camera_hits, box_sums, pixels a textured-albedo sample may reach, pixels a smooth-normal sample may reach) of a scene under the box filter, computed once per
    `key` and left unchanged."""
    if key not in _CACHE:
        orc = oracle.scene(sd)
        h = camera_hits(pkg, oracle, orc, rp)
        hit, albedo, normal, smooth = sample_values(pkg, oracle, sd, h)
        textured = np.isnan(albedo).any(axis=1)
        sums = box_sums(rp, h, hit, np.nan_to_num(albedo), normal)
        cb = rp.cropped_pixel_bounds

        def reach(samples):   # (a sample's own pixel and, from an edge, its neighbours)
            mask = np.zeros((cb[3] - cb[1], cb[2] - cb[0]), bool)
            for (x, y) in h["pix"][samples]:
                mask[max(y - 1 - cb[1], 0):y + 2 - cb[1], max(x - 1 - cb[0], 0):x + 2 - cb[0]] = True
            return mask
        orc.close()
        _CACHE[key] = (h, sums, reach(textured), reach(smooth))
    return _CACHE[key]
