"""A float32 numpy model of the lightmap's contract (include/mi355bake.h "Lightmap") on the model of the atlas bake (tests/bake_reference.py: owner, interaction,
offset_ray_origin, array_samples). Light samples come from the oracle's Light::sample_li (orc_light_sample_li: wi, pdf, Li), occlusion from its any-hit query
(orc_trace_any) with t_max = 1 - 1e-4. The oracle's hook does not hand out the far end p1 of the visibility segment, so the model rebuilds it:
  * point and spot lights: p1 = the light's position, no error bound, no normal;
  * triangle lights: Triangle::sample restated (uniform_sample_triangle, the point, its gamma(6) error bound, the normal), with the model's own
    wi = normalize(p1 - p) held bit for bit against the oracle's wi;
and from it the whole shadow ray, Interaction::spawn_ray_to. For the lights whose p1 it cannot restate bit for bit -- sphere and disk lights (the transforms'
error bounds), distant and infinite lights (the world radius is the top-level accelerator's) -- it takes the ray the device built (pt_bake_light_rays) and holds it:
the origin bit for bit against offset_ray_origin(p, p_error, n, wi), the direction within 4 x the largest deviation 1 - dot(normalize(d), wi) its own exact
rays show for the triangle lights of the same scene; that ray then goes to the oracle's any-hit query."""
import ctypes as C

import numpy as np
import bake_reference as M

F = M.F
T_MAX = F(1.0) - F(0.0001)


def vdot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def vnormalize(a):
    with np.errstate(all="ignore"):
        return (a * (F(1) / np.sqrt(vdot(a, a)))[..., None]).astype(F)


def selected_lights(n_lights, lights):
    """The selected lights in ascending order: `lights` None (all), a list of indices, or a per-light mask."""
    if lights is None:
        return np.arange(n_lights, dtype=np.int64)
    lights = np.asarray(lights)
    if lights.dtype in (np.bool_, np.uint8):
        return np.nonzero(lights)[0].astype(np.int64)
    return np.unique(lights.astype(np.int64))


def light_of(sel, spp_numbers, nsamples):
    """The light of sample numbers j = s * nsamples + k: sel[j mod n_sel] (contract step 2)."""
    return sel[np.asarray(spp_numbers, dtype=np.int64) % len(sel)]


def light_class(pkg, sd, li):
    """"position" (point, spot), "triangle", or "other": how the model comes by p1."""
    A = pkg._abi
    L = sd.lights[li]
    if L.type in (A.PT_LIGHT_POINT, A.PT_LIGHT_SPOT):
        return "position"
    if L.type == A.PT_LIGHT_DIFFUSE_AREA and (int(sd.prim_shape[L.prim]) >> 30) == A.PT_SHAPE_TRIANGLE:
        return "triangle"
    return "other"


def triangle_sample(sd, prim, u):
    """Triangle::sample (triangle.rs:556-584) for the array values u (m, 2): (p (m, 3), p_error (m, 3), n (m, 3))."""
    tri = int(sd.prim_shape[prim] & np.uint32(0x3fffffff))
    fl = int(sd.tri_flags[tri])
    i0, i1, i2 = (int(i) for i in sd.idx[tri])
    p0, p1, p2 = M.v3(sd.P[i0]), M.v3(sd.P[i1]), M.v3(sd.P[i2])
    with np.errstate(all="ignore"):
        su0 = np.sqrt(u[:, 0].astype(F))
        b0 = F(1) - su0
        b1 = u[:, 1].astype(F) * su0
        b2 = F(1) - b0 - b1
        a0, a1, a2 = p0[None, :] * b0[:, None], p1[None, :] * b1[:, None], p2[None, :] * b2[:, None]
        p = (a0 + a1 + a2).astype(F)
        perr = ((np.abs(a0) + np.abs(a1) + np.abs(a2)) * M.gamma(6)).astype(F)
        n = M.normalize(M.cross(p1 - p0, p2 - p0))
        flip = bool(fl & M.TRI_REVERSE) != bool(fl & M.TRI_SWAPS)
        if not (fl & M.TRI_HAS_N) and flip:
            n = -n
        n = np.broadcast_to(n[None, :], p.shape).astype(F)
        if fl & M.TRI_HAS_N:
            ns = M.v3(sd.N[i0])[None, :] * b0[:, None] + M.v3(sd.N[i1])[None, :] * b1[:, None] + M.v3(sd.N[i2])[None, :] * b2[:, None]
            n = np.where((vdot(n, ns) < 0)[:, None], -n, n).astype(F)
    return p, perr, n


def spawn_ray_to(p, perr, n, p1, p1err, p1n):
    """Interaction::spawn_ray_to (interaction.rs:45-52), rows of (m, 3) arrays: (o, d)."""
    with np.errstate(all="ignore"):
        o = M.offset_ray_origin(p, perr, n, (p1 - p).astype(F))
        t = M.offset_ray_origin(p1, p1err, p1n, (o - p1).astype(F))
        return o, (t - o).astype(F)


def sample_list(owner, spp, nsamples, samples=None):
    """(texel, s, k) of every light sample of the owned texels, ordered by texel, then (s, k): arrays of int64."""
    height, width = owner.shape
    first, count = (0, spp) if samples is None else samples
    texels = np.nonzero(owner.reshape(-1) != M.NONE)[0].astype(np.int64)
    per = count * nsamples
    tx = np.repeat(texels, per)
    s = np.tile(np.repeat(np.arange(first, first + count, dtype=np.int64), nsamples), len(texels))
    k = np.tile(np.arange(nsamples, dtype=np.int64), len(texels) * count)
    return tx, s, k


def deviation(d, wi):
    """1 - dot(normalize(d), wi), in float64 from the float32 values."""
    d, wi = d.astype(np.float64), wi.astype(np.float64)
    with np.errstate(all="ignore"):
        return 1.0 - vdot(d / np.sqrt(vdot(d, d))[..., None], wi)


def rough_world_radius(sd):
    """The radius of the bounding sphere of the meshes' vertices: NOT the device's (the accelerator's bounds); for model-only runs, see light_samples."""
    P = np.asarray(sd.P, F).reshape(-1, 3)
    lo, hi = P.min(axis=0), P.max(axis=0)
    return F(np.sqrt(((hi - (lo + hi) * F(0.5)) ** 2).sum(dtype=F)))


def light_samples(oracle, pkg, sd, owner, spp, nsamples, lights=None, sampler="sobol", samples=None, orc_scene=None, device=None):
    """Contract steps 2 to 5 for every light sample of the owned texels: dict(texel, s, k, light, wi, pdf, Li, E, o, d, contributes) over the samples in
    sample_list's order, and exact_dev / other_dev: the largest direction deviation of the model's exact rays of triangle lights / of the device's rays taken over.
    `device`: what Scene.bake_light_rays returns for sample_list's samples; needed (and held) for the lights whose p1 the model cannot restate. Without it --
    a model-only run -- such a light's ray goes from the exact origin along wi, 2 x rough_world_radius long: good for occlusion queries in scenes whose
    occluders are far from that ray's end, and never compared with the device."""
    A = pkg._abi
    height, width = owner.shape
    n_lights = int(sd.desc().n_lights)
    sel = selected_lights(n_lights, lights)
    n_sel = len(sel)
    assert n_sel > 0 and (spp * nsamples) % n_sel == 0
    tx, s, k = sample_list(owner, spp, nsamples, samples)
    m = len(tx)
    z3 = lambda: np.zeros((m, 3), F)
    out = dict(texel=tx, s=s, k=k, light=light_of(sel, s * nsamples + k, nsamples).astype(np.uint32), wi=z3(), pdf=np.zeros(m, F), Li=z3(), E=z3(), o=z3(), d=z3(),
               contributes=np.zeros(m, bool), exact_dev=0.0, other_dev=0.0)
    if m == 0:
        return out
    orc_scene = orc_scene or oracle.scene(sd)
    u = M.array_samples(oracle, pkg, sampler, width, height, tx % width, tx // width, s * nsamples + k)
    sis = M.texel_interactions(sd, owner)
    p, perr, n, ns = z3(), z3(), z3(), z3()
    fp = lambda a: a.ctypes.data_as(A.fp)
    # Light::sample_li per (texel, light): the oracle's hook takes one reference point and many samples
    for t in np.unique(tx):
        rows = np.nonzero(tx == t)[0]
        si = sis[int(t)]
        with np.errstate(all="ignore"):
            p[rows], perr[rows], n[rows], ns[rows] = si["p"], si["p_error"], si["n"], M.normalize(si["sh_n"])
        for li in np.unique(out["light"][rows]):
            r = rows[out["light"][rows] == li]
            uu = np.ascontiguousarray(u[r], dtype=F)
            wi, pdf, L = np.zeros((len(r), 3), F), np.zeros(len(r), F), np.zeros((len(r), 3), F)
            ref = [np.ascontiguousarray(si[key], dtype=F) for key in ("p", "p_error", "n")]
            st = oracle.lib.orc_light_sample_li(orc_scene.h, int(li), fp(ref[0]), fp(ref[1]), fp(ref[2]), len(r), fp(uu), fp(wi), fp(pdf), fp(L))
            assert st == 0, st
            out["wi"][r], out["pdf"][r], out["Li"][r] = wi, pdf, L
    # contribution (step 4)
    scale = F(n_sel) / F(nsamples)
    with np.errstate(all="ignore"):
        c = vdot(out["wi"], ns)
        black = (out["Li"] == 0).all(axis=1)
        ok = (out["pdf"] > 0) & ~black & (c > 0) & (vdot(out["wi"], n) > 0)
        w = ((c * scale) / out["pdf"]).astype(F)
        out["E"][ok] = (out["Li"] * w[:, None]).astype(F)[ok]
    out["contributes"] = ok
    # the shadow ray (step 5)
    others = np.zeros(m, bool)
    for li in np.unique(out["light"]):
        r = np.nonzero((out["light"] == li) & ok)[0]
        if len(r) == 0:
            continue
        cls = light_class(pkg, sd, int(li))
        if cls == "position":
            L = sd.lights[int(li)]
            p1 = np.broadcast_to(np.array([L.pos[0], L.pos[1], L.pos[2]], F)[None, :], (len(r), 3)).astype(F)
            p1err, p1n = np.zeros((len(r), 3), F), np.zeros((len(r), 3), F)
        elif cls == "triangle":
            p1, p1err, p1n = triangle_sample(sd, int(sd.lights[int(li)].prim), u[r])
            mine = vnormalize((p1 - p[r]).astype(F))
            assert mine.tobytes() == out["wi"][r].tobytes(), ("Triangle::sample restated: wi differs from the oracle's", int(li))
        else:
            others[r] = True
            continue
        out["o"][r], out["d"][r] = spawn_ray_to(p[r], perr[r], n[r], p1, p1err, p1n)
        if cls == "triangle":
            out["exact_dev"] = max(out["exact_dev"], float(np.abs(deviation(out["d"][r], out["wi"][r])).max()))
    r = np.nonzero(others)[0]
    if len(r):
        want_o = M.offset_ray_origin(p[r], perr[r], n[r], out["wi"][r])
        if device is None:
            out["o"][r] = want_o
            out["d"][r] = (out["wi"][r] * (F(2) * rough_world_radius(sd))).astype(F)
        else:
            assert (np.asarray(device["found"])[r] == 3).all()
            assert device["o"][r].tobytes() == want_o.tobytes(), "a device ray taken over: its origin is not offset_ray_origin(p, p_error, n, wi)"
            out["other_dev"] = float(np.abs(deviation(device["d"][r], out["wi"][r])).max())
            assert out["exact_dev"] > 0, "the scene has no triangle light whose exact rays set the yardstick"
            assert out["other_dev"] <= 4.0 * out["exact_dev"], (out["other_dev"], out["exact_dev"])
            out["o"][r], out["d"][r] = device["o"][r], device["d"][r]
    return out


def accumulate(light_w, r, occluded, nsamples):
    """light_w (H, W, 4) += (E, 1) of the unoccluded contributing samples, per texel in ascending (s, k) order. Returns light_w (modified in place)."""
    flat = light_w.reshape(-1, 4)
    arrived = r["contributes"].copy()
    arrived[r["contributes"]] = ~np.asarray(occluded, bool)
    order = r["s"] * nsamples + r["k"]
    for j in np.unique(order):   # one (s, k) at a time: every texel has at most one sample of it
        m = (order == j) & arrived
        t = r["texel"][m]
        flat[t, 0:3] = flat[t, 0:3] + r["E"][m]
        flat[t, 3] = flat[t, 3] + F(1)
    return light_w


def bake(oracle, pkg, sd, select, width, height, spp, nsamples=None, lights=None, sampler="sobol", samples=None, light_w=None, orc_scene=None, device=None):
    """The model's lightmap bake: dict(owner, position, normal, light_w, n_rays, samples, occluded). `device`: see light_samples."""
    prims, uv_tris = M.scene_triangles(sd, select)
    owner = M.owner_map(uv_tris, prims, width, height)
    pos, nrm = M.planes(sd, owner)
    n_sel = len(selected_lights(int(sd.desc().n_lights), lights))
    nsamples = n_sel if nsamples is None else nsamples
    orc_scene = orc_scene or oracle.scene(sd)
    r = light_samples(oracle, pkg, sd, owner, spp, nsamples, lights, sampler, samples, orc_scene, device)
    ok = r["contributes"]
    n_rays = int(ok.sum())
    occ = orc_scene.trace_any(r["o"][ok], r["d"][ok], np.full(n_rays, T_MAX, F)) if n_rays else np.zeros(0, np.uint8)
    light_w = np.zeros((height, width, 4), F) if light_w is None else light_w
    accumulate(light_w, r, occ, nsamples)
    return dict(owner=owner, position=pos, normal=nrm, light_w=light_w, n_rays=n_rays, samples=r, occluded=occ, nsamples=nsamples)


def resolve(light_w, spp, nsamples):
    """(irradiance (H, W, 3), reached (H, W)): pt_bake_light_resolve."""
    light_w = np.asarray(light_w, F)
    any_ = (light_w != 0).any(axis=-1)
    with np.errstate(all="ignore"):
        irr = np.where(any_[..., None], light_w[..., 0:3] / F(spp), F(0)).astype(F)
        reached = np.where(any_, light_w[..., 3] / (F(spp) * F(nsamples)), F(0)).astype(F)
    return irr, reached
