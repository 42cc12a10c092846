"""A float32 numpy model of the lightmap's contract (include/mi355bake.h "Lightmap") on the model of the atlas bake (tests/bake_reference.py: owner, interaction,
array_samples, sample_list, accumulate) in the float32 arithmetic of tests/model_math.py. Light samples come from the oracle's Light::sample_li (orc_light_sample_li: wi, pdf, Li), occlusion from its any-hit query
(orc_trace_any) with t_max = 1 - 1e-4. The oracle's hook does not hand out the far end p1 of the visibility segment, so the model rebuilds it:
  * point and spot lights: p1 = the light's position, no error bound, no normal;
  * triangle lights: Triangle::sample restated (uniform_sample_triangle, the point, its gamma(6) error bound, the normal), with the model's own
    wi = normalize(p1 - p) held bit for bit against the oracle's wi;
and from it the whole shadow ray, Interaction::spawn_ray_to. For the lights whose p1 it cannot restate bit for bit -- sphere and disk lights (the transforms'
error bounds), distant and infinite lights (the world radius is the top-level accelerator's) -- it takes the ray the device built (pt_bake_light_rays) and holds it:
the origin bit for bit against offset_ray_origin(p, p_error, n, wi), the direction within 4 x the largest deviation 1 - dot(normalize(d), wi) its own exact
rays show for the triangle lights of the same scene; that ray then goes to the oracle's any-hit query.

The SH points (tests/sh_reference.py) sample the lights the same way from a reference point without a surface: sample_lights is the one body of both."""
import numpy as np
import bake_reference as M
from model_math import F, NONE, cross, dot, gamma, normalize, offset_ray_origin, spawn_ray_to

T_MAX = F(1.0) - F(0.0001)


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
        perr = ((np.abs(a0) + np.abs(a1) + np.abs(a2)) * gamma(6)).astype(F)
        n = normalize(cross(p1 - p0, p2 - p0))
        flip = bool(fl & M.TRI_REVERSE) != bool(fl & M.TRI_SWAPS)
        if not (fl & M.TRI_HAS_N) and flip:
            n = -n
        n = np.broadcast_to(n[None, :], p.shape).astype(F)
        if fl & M.TRI_HAS_N:
            ns = M.v3(sd.N[i0])[None, :] * b0[:, None] + M.v3(sd.N[i1])[None, :] * b1[:, None] + M.v3(sd.N[i2])[None, :] * b2[:, None]
            n = np.where((dot(n, ns) < 0)[:, None], -n, n).astype(F)
    return p, perr, n


def deviation(d, wi):
    """1 - dot(normalize(d), wi), in float64 from the float32 values."""
    d, wi = d.astype(np.float64), wi.astype(np.float64)
    with np.errstate(all="ignore"):
        return 1.0 - dot(d / np.sqrt(dot(d, d))[..., None], wi)


def rough_world_radius(sd):
    """The radius of the bounding sphere of the meshes' vertices: NOT the device's (the accelerator's bounds); for model-only runs, see light_samples."""
    P = np.asarray(sd.P, F).reshape(-1, 3)
    lo, hi = P.min(axis=0), P.max(axis=0)
    return F(np.sqrt(((hi - (lo + hi) * F(0.5)) ** 2).sum(dtype=F)))


def sample_lights(oracle, pkg, sd, key, item, s, k, u, p, perr, n, ns, sel, nsamples, orc_scene, device):
    """Light sampling, contribution and shadow ray (contract steps 2 to 5) of the samples (item, s, k) with array values u (m, 2), each from the reference point
    {p, perr, n} (m, 3) of its item: dict(<key>=item, s, k, light, wi, pdf, Li, E, o, d, contributes) over the samples, and exact_dev / other_dev: the largest direction
    deviation of the model's exact rays of triangle lights / of the device's rays taken over. ns (m, 3): the shading normals of a surface, whose cosine weighs the
    sample and whose sides (ns and n) it must be in front of; None: a point without a surface -- no cosine, no side test. `device`: see light_samples."""
    A = pkg._abi
    m = len(item)
    z3 = lambda: np.zeros((m, 3), F)
    out = {key: item}
    out.update(s=s, k=k, light=light_of(sel, s * nsamples + k, nsamples).astype(np.uint32), wi=z3(), pdf=np.zeros(m, F), Li=z3(), E=z3(), o=z3(), d=z3(),
               contributes=np.zeros(m, bool), exact_dev=0.0, other_dev=0.0)
    if m == 0:
        return out
    fp = lambda a: a.ctypes.data_as(A.fp)
    # Light::sample_li per (item, light): the oracle's hook takes one reference point and many samples
    for t in np.unique(item):
        rows = np.nonzero(item == t)[0]
        ref = [np.ascontiguousarray(a[rows[0]], dtype=F) for a in (p, perr, n)]
        for li in np.unique(out["light"][rows]):
            r = rows[out["light"][rows] == li]
            uu = np.ascontiguousarray(u[r], dtype=F)
            wi, pdf, L = np.zeros((len(r), 3), F), np.zeros(len(r), F), np.zeros((len(r), 3), F)
            st = oracle.lib.orc_light_sample_li(orc_scene.h, int(li), fp(ref[0]), fp(ref[1]), fp(ref[2]), len(r), fp(uu), fp(wi), fp(pdf), fp(L))
            assert st == 0, st
            out["wi"][r], out["pdf"][r], out["Li"][r] = wi, pdf, L
    # contribution (step 4)
    scale = F(len(sel)) / F(nsamples)
    with np.errstate(all="ignore"):
        ok = (out["pdf"] > 0) & ~(out["Li"] == 0).all(axis=1)
        if ns is None:
            w = (scale / out["pdf"]).astype(F)
        else:
            c = dot(out["wi"], ns)
            ok = ok & (c > 0) & (dot(out["wi"], n) > 0)
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
            mine = normalize((p1 - p[r]).astype(F))
            assert mine.tobytes() == out["wi"][r].tobytes(), ("Triangle::sample restated: wi differs from the oracle's", int(li))
        else:
            others[r] = True
            continue
        out["o"][r], out["d"][r] = spawn_ray_to(p[r], perr[r], n[r], p1, p1err, p1n)
        if ns is None:
            assert out["o"][r].tobytes() == (p[r] + F(0)).astype(F).tobytes()   # n = 0: the ray starts at the point
        if cls == "triangle":
            out["exact_dev"] = max(out["exact_dev"], float(np.abs(deviation(out["d"][r], out["wi"][r])).max()))
    r = np.nonzero(others)[0]
    if len(r):
        want_o = offset_ray_origin(p[r], perr[r], n[r], out["wi"][r])   # (p + 0 for a point without a surface)
        if device is None:
            out["o"][r] = want_o
            out["d"][r] = (out["wi"][r] * (F(2) * rough_world_radius(sd))).astype(F)
        else:
            assert (np.asarray(device["found"])[r] == 3).all()
            assert device["o"][r].tobytes() == want_o.tobytes(), "a device ray taken over: its origin is not " + ("the point" if ns is None else "offset_ray_origin(p, p_error, n, wi)")
            out["other_dev"] = float(np.abs(deviation(device["d"][r], out["wi"][r])).max())
            assert out["exact_dev"] > 0, "the scene has no triangle light whose exact rays set the yardstick"
            assert out["other_dev"] <= 4.0 * out["exact_dev"], (out["other_dev"], out["exact_dev"])
            out["o"][r], out["d"][r] = device["o"][r], device["d"][r]
    return out


def light_samples(oracle, pkg, sd, owner, spp, nsamples, lights=None, sampler="sobol", samples=None, orc_scene=None, device=None):
    """Contract steps 2 to 5 for every light sample of the owned texels: what sample_lights returns, `texel` its items, in the order of
    bake_reference.sample_list(owned_texels(owner), ..). `device`: what Scene.bake_light_rays returns for those samples; needed (and held) for the lights whose p1
    the model cannot restate. Without it -- a model-only run -- such a light's ray goes from the exact origin along wi, 2 x rough_world_radius long: good for
    occlusion queries in scenes whose occluders are far from that ray's end, and never compared with the device."""
    height, width = owner.shape
    sel = selected_lights(int(sd.desc().n_lights), lights)
    assert len(sel) > 0 and (spp * nsamples) % len(sel) == 0
    tx, s, k = M.sample_list(owned_texels(owner), spp, nsamples, samples)
    m = len(tx)
    p, perr, n, ns = (np.zeros((m, 3), F) for _ in range(4))
    sis = M.texel_interactions(sd, owner) if m else {}
    for t in np.unique(tx):
        rows, si = tx == t, sis[int(t)]
        with np.errstate(all="ignore"):
            p[rows], perr[rows], n[rows], ns[rows] = si["p"], si["p_error"], si["n"], normalize(si["sh_n"])
    u = M.array_samples(oracle, pkg, sampler, width, height, tx % width, tx // width, s * nsamples + k) if m else np.zeros((0, 2), F)
    return sample_lights(oracle, pkg, sd, "texel", tx, s, k, u, p, perr, n, ns, sel, nsamples, orc_scene or oracle.scene(sd), device)


def owned_texels(owner):
    """The numbers y * width + x of the owned texels of an owner map, ascending."""
    return np.nonzero(owner.reshape(-1) != NONE)[0].astype(np.int64)


def arrived(r, occluded):
    """Per sample: it contributes and its shadow ray (`occluded` runs over the contributing samples) is free."""
    out = r["contributes"].copy()
    out[r["contributes"]] = ~np.asarray(occluded, bool)
    return out


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
    # light_w (H, W, 4) += (E, 1) of the unoccluded contributing samples
    M.accumulate(light_w.reshape(-1, 4), r["texel"], r, nsamples, np.concatenate([r["E"], np.ones((len(ok), 1), F)], axis=1), arrived(r, occ))
    return dict(owner=owner, position=pos, normal=nrm, light_w=light_w, n_rays=n_rays, samples=r, occluded=occ, nsamples=nsamples)


def resolve(sums, spp, nsamples):
    """(sums / spp, count / (spp * nsamples)) of rows (.., c + 1) of c sums and a count, zeros where a row holds nothing: pt_bake_light_resolve's
    (irradiance (H, W, 3), reached (H, W)) of light_w (H, W, 4)."""
    sums = np.asarray(sums, F)
    any_ = (sums != 0).any(axis=-1)
    with np.errstate(all="ignore"):
        mean = np.where(any_[..., None], sums[..., :-1] / F(spp), F(0)).astype(F)
        reached = np.where(any_, sums[..., -1] / (F(spp) * F(nsamples)), F(0)).astype(F)
    return mean, reached
