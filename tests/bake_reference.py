"""A float32 numpy model of the texture-space bake's contract (include/mi355bake.h): ownership, the surface point, the AO rays, the sums and the dilation,
every operation in the header's order, in the float32 arithmetic of tests/model_math.py (which also lends the oracle's dm_sincosf and the samplers' array values);
the occlusion of the model's rays is the oracle's (orc_trace_any)."""
import numpy as np
from model_math import F, INV_4PI, INV_PI, NONE, PI, concentric_sample_disk, coordinate_system, cross, dm_cos, dm_sin, dot, gamma, normalize, offset_ray_origin, sampler_values

TRI_REVERSE, TRI_SWAPS, TRI_HAS_N, TRI_HAS_S, TRI_HAS_UV = 1, 2, 4, 8, 16
NEIGHBOURS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]   # (dx, dy): the dilation's order of summation


# ---- ownership ----
def texel_centres(width, height):
    """(u (H, W), v (H, W)) in float32: u = (x + 0.5) / width, v = (y + 0.5) / height."""
    u = (np.arange(width, dtype=F) + F(0.5)) / F(width)
    v = (np.arange(height, dtype=F) + F(0.5)) / F(height)
    return np.broadcast_to(u[None, :], (height, width)), np.broadcast_to(v[:, None], (height, width))


def barycentrics(uv0, uv1, uv2, cu, cv):
    """(inside, b0, b1, b2) of the centres (cu, cv) in the UV triangle: arrays like cu."""
    uv0, uv1, uv2 = (np.asarray(a, F) for a in (uv0, uv1, uv2))
    e0x, e0y, e1x, e1y = uv1[0] - uv0[0], uv1[1] - uv0[1], uv2[0] - uv0[0], uv2[1] - uv0[1]
    dx, dy = cu - uv0[0], cv - uv0[1]
    det = e0x * e1y - e0y * e1x
    if det == 0 or det != det:
        z = np.zeros(np.shape(cu), F)
        return np.zeros(np.shape(cu), bool), z, z, z
    with np.errstate(all="ignore"):
        b1 = (dx * e1y - dy * e1x) / det
        b2 = (e0x * dy - e0y * dx) / det
        b0 = F(1) - b1 - b2
    return (b0 >= 0) & (b1 >= 0) & (b2 >= 0), b0, b1, b2


def texel_box(uv0, uv1, uv2, width, height):
    """The texel box of a triangle (mi355bake.h "Ownership"): (x0, x1, y0, y1) inclusive, or None when the triangle has none. float32, in the header's order."""
    uv = np.array([uv0, uv1, uv2], F)
    with np.errstate(all="ignore"):
        fmin3 = lambda a, b, c: np.fmin(a, np.fmin(b, c))   # fminf / fmaxf: a NaN operand loses
        fmax3 = lambda a, b, c: np.fmax(a, np.fmax(b, c))
        ulo, uhi = fmin3(*uv[:, 0]) * F(width), fmax3(*uv[:, 0]) * F(width)
        vlo, vhi = fmin3(*uv[:, 1]) * F(height), fmax3(*uv[:, 1]) * F(height)
        if not (ulo <= uhi and vlo <= vhi and all(abs(v) < F(1e30) for v in (ulo, uhi, vlo, vhi))):
            return None
        mx, my = F(0.5625) + F(width) * F(2.4e-7), F(0.5625) + F(height) * F(2.4e-7)
        fx0, fx1 = np.fmax(np.floor(ulo - mx), F(0)), np.fmin(np.ceil(uhi - F(1) + mx), F(width - 1))
        fy0, fy1 = np.fmax(np.floor(vlo - my), F(0)), np.fmin(np.ceil(vhi - F(1) + my), F(height - 1))
    if not (fx0 <= fx1 and fy0 <= fy1):
        return None
    return int(fx0), min(int(fx1), width - 1), int(fy0), min(int(fy1), height - 1)


def owner_map(uv_tris, prims, width, height, boxed=True):
    """uv_tris: (n, 3, 2) float32 vertex UVs of the selected triangles, prims: their primitive numbers. The lowest-numbered primitive that contains a centre of its
    texel box owns it. `boxed` False: the barycentrics alone, over the whole atlas -- NOT the contract; what the box denies a sliver is the difference."""
    cu, cv = texel_centres(width, height)
    owner = np.full((height, width), NONE, np.uint32)
    for k in np.argsort(np.asarray(prims), kind="stable")[::-1]:   # descending: the lowest number is written last
        inside, _, _, _ = barycentrics(uv_tris[k][0], uv_tris[k][1], uv_tris[k][2], cu, cv)
        if boxed:
            box = texel_box(uv_tris[k][0], uv_tris[k][1], uv_tris[k][2], width, height)
            in_box = np.zeros((height, width), bool)
            if box is not None:
                in_box[box[2]:box[3] + 1, box[0]:box[1] + 1] = True
            inside = inside & in_box
        owner[inside] = np.uint32(prims[k])
    return owner


def scene_triangles(sd, select):
    """(prims, uv_tris) of the selected primitives of a host.SceneData: `select` is a per-primitive mask."""
    prims = np.nonzero(np.asarray(select))[0].astype(np.uint32)
    tris = sd.prim_shape[prims] & np.uint32(0x3fffffff)
    return prims, sd.UV[sd.idx[tris]].astype(F)


# ---- the surface point: Triangle::intersect's interaction for given barycentrics (dev_scene.h: tri_partials, tri_fill_from) ----
def v3(a):
    return np.asarray(a, F).reshape(3)


def interaction(sd, prim, b0, b1, b2):
    """dict(p, p_error, n, dpdu, sh_n) of primitive `prim` of a host.SceneData at the barycentrics (float32 scalars)."""
    tri = int(sd.prim_shape[prim] & np.uint32(0x3fffffff))
    fl = int(sd.tri_flags[tri])
    i0, i1, i2 = (int(i) for i in sd.idx[tri])
    p0, p1, p2 = v3(sd.P[i0]), v3(sd.P[i1]), v3(sd.P[i2])
    uv = [sd.UV[i].astype(F) for i in (i0, i1, i2)]
    b0, b1, b2 = F(b0), F(b1), F(b2)
    with np.errstate(all="ignore"):
        duv02, duv12 = uv[0] - uv[2], uv[1] - uv[2]
        dp02, dp12 = p0 - p2, p1 - p2
        det = duv02[0] * duv12[1] - duv02[1] * duv12[0]
        degenerate = abs(det) < F(1.0e-8)
        dpdu, dpdv = np.zeros(3, F), np.zeros(3, F)
        if not degenerate:
            inv = F(1) / det
            dpdu = (dp02 * duv12[1] - dp12 * duv02[1]) * inv
            dpdv = (dp02 * (-duv12[0]) + dp12 * duv02[0]) * inv
        c = cross(dpdu, dpdv)
        if degenerate or dot(c, c) == 0:
            ng = cross(p2 - p0, p1 - p0)
            if dot(ng, ng) != 0:
                dpdu, dpdv = coordinate_system(normalize(ng))
        perr = np.array([abs(b0 * p0[k]) + abs(b1 * p1[k]) + abs(b2 * p2[k]) for k in range(3)], F) * gamma(7)
        p = p0 * b0 + p1 * b1 + p2 * b2
        flip = bool(fl & TRI_REVERSE) != bool(fl & TRI_SWAPS)
        nn = normalize(cross(dp02, dp12))
        n = -nn if flip else nn
        sh_n = n.copy()
        if fl & (TRI_HAS_N | TRI_HAS_S):
            ns = n
            if fl & TRI_HAS_N:
                ns = v3(sd.N[i0]) * b0 + v3(sd.N[i1]) * b1 + v3(sd.N[i2]) * b2
                ns = normalize(ns) if dot(ns, ns) > 0 else n
            ss = normalize(dpdu)
            if fl & TRI_HAS_S:
                ss = v3(sd.S[i0]) * b0 + v3(sd.S[i1]) * b1 + v3(sd.S[i2]) * b2
                ss = normalize(ss) if dot(ss, ss) > 0 else normalize(dpdu)
            ts = cross(ss, ns)
            if dot(ts, ts) > 0:
                ts = normalize(ts); ss = cross(ts, ns)
            else:
                ss, ts = coordinate_system(ns)
            if fl & TRI_REVERSE:
                ts = -ts
            sh_n = normalize(cross(ss, ts))
            if flip:
                sh_n = -sh_n
            if dot(n, sh_n) < 0:
                n = -n
    return dict(p=p, p_error=perr, n=n, dpdu=dpdu, sh_n=sh_n)


def texel_interactions(sd, owner):
    """{texel index: interaction} of every owned texel of an owner map (H, W)."""
    height, width = owner.shape
    cu, cv = texel_centres(width, height)
    out = {}
    for y, x in zip(*np.nonzero(owner != NONE)):
        prim = int(owner[y, x])
        tri = int(sd.prim_shape[prim] & np.uint32(0x3fffffff))
        uv = sd.UV[sd.idx[tri]].astype(F)
        _, b0, b1, b2 = barycentrics(uv[0], uv[1], uv[2], cu[y, x], cv[y, x])
        out[int(y) * width + int(x)] = interaction(sd, prim, b0, b1, b2)
    return out


def planes(sd, owner):
    """(position (H, W, 3), normal (H, W, 3)) of an owner map: p and the normalised shading normal, zeros where no primitive owns the texel."""
    height, width = owner.shape
    pos = np.zeros((height * width, 3), F); nrm = np.zeros((height * width, 3), F)
    for t, si in texel_interactions(sd, owner).items():
        pos[t] = si["p"]; nrm[t] = normalize(si["sh_n"])
    return pos.reshape(height, width, 3), nrm.reshape(height, width, 3)


# ---- the AO rays ----
def array_samples(oracle, pkg, sampler, width, height, px, py, numbers):
    """The 2-D array values (m, 2) of sample numbers `numbers` of pixels (px, py): dimensions 5 and 6 of a sampler for sample bounds [0, width) x [0, height)."""
    return sampler_values(oracle, pkg, sampler, (0, 0, width, height), np.stack([px, py], axis=1), numbers, 7)[:, 5:7].copy()


def directions(oracle, u, cos_sample):
    """(wi (m, 3), pdf (m,)) of the array values u (m, 2): cosine_sample_hemisphere or uniform_sample_sphere (side/ao_rays.h: ao_ray)."""
    ux, uy = u[:, 0].astype(F), u[:, 1].astype(F)
    with np.errstate(all="ignore"):
        if cos_sample:
            dsk = concentric_sample_disk(oracle, u)
            dx, dy = dsk[:, 0], dsk[:, 1]
            z = np.sqrt(np.maximum(F(0), F(1) - dx * dx - dy * dy)).astype(F)
            return np.stack([dx, dy, z], axis=1).astype(F), (np.abs(z) * INV_PI).astype(F)
        z = F(1) - F(2) * ux
        r = np.sqrt(np.maximum(F(1) - z * z, F(0))).astype(F)
        phi = (F(2) * PI) * uy
        s, c = dm_sin(oracle, phi), dm_cos(oracle, phi)
        return np.stack([r * c, r * s, z], axis=1).astype(F), np.full(len(ux), INV_4PI, F)


def sample_list(items, spp, nsamples, samples=None):
    """(item, s, k) of every sample of the items (texels, points: ascending numbers), for sample numbers `samples` = (first, n) of the job (default: all spp), ordered
    by item, then (s, k): arrays of int64."""
    first, count = (0, spp) if samples is None else samples
    items = np.asarray(items, dtype=np.int64)
    return (np.repeat(items, count * nsamples), np.tile(np.repeat(np.arange(first, first + count, dtype=np.int64), nsamples), len(items)),
            np.tile(np.arange(nsamples, dtype=np.int64), len(items) * count))


def rays(oracle, pkg, sd, owner, spp, nsamples, cos_sample, sampler, samples=None):
    """The AO rays of the owned texels of an owner map, for sample numbers `samples` = (first, n) of the job (default: all spp): dict(texel, s, k, o, d, w) of
    arrays over the rays, ordered by texel, then (s, k)."""
    height, width = owner.shape
    sis = texel_interactions(sd, owner)
    texels = np.array(sorted(sis), dtype=np.int64)
    tx, s, k = sample_list(texels, spp, nsamples, samples)
    if len(tx) == 0:
        z3 = np.zeros((0, 3), F)
        return dict(texel=tx, s=s, k=k, o=z3, d=z3, w=np.zeros(0, F))
    per = len(tx) // len(texels)
    u = array_samples(oracle, pkg, sampler, width, height, tx % width, tx // width, s * nsamples + k)
    wi, pdf = directions(oracle, u, cos_sample)
    with np.errstate(all="ignore"):
        frames = {t: (si["n"], normalize(si["dpdu"])) for t, si in sis.items()}
        n = np.repeat(np.array([frames[t][0] for t in texels], F), per, axis=0)
        sv = np.repeat(np.array([frames[t][1] for t in texels], F), per, axis=0)
        tv = np.repeat(np.array([cross(frames[t][0], frames[t][1]) for t in texels], F), per, axis=0)
        p = np.repeat(np.array([sis[t]["p"] for t in texels], F), per, axis=0)
        perr = np.repeat(np.array([sis[t]["p_error"] for t in texels], F), per, axis=0)
        wo = (sv * wi[:, 0:1] + tv * wi[:, 1:2] + n * wi[:, 2:3]).astype(F)
        o = offset_ray_origin(p, perr, n, wo)
        w = (dot(wo, n) / (pdf * F(nsamples))).astype(F)
    return dict(texel=tx, s=s, k=k, o=o, d=wo, w=w)


def accumulate(sums, item, r, nsamples, rows, take):
    """sums (n, c) += rows (m, c) of the samples `take` (m,) of r = dict(s, k, ..), per item (m,) in ascending (s, k) order. Returns sums (modified in place)."""
    order = r["s"] * nsamples + r["k"]
    for j in np.unique(order):   # one (s, k) at a time: every item has at most one sample of it
        m = (order == j) & take
        t = item[m]
        sums[t] = (sums[t] + rows[m]).astype(F)
    return sums


def add_ao_rays(ao_w, r, occluded, nsamples):
    """ao_w (H, W, 4) += the unoccluded rays' direction and weight, per texel in ascending (s, k) order. Returns ao_w (modified in place)."""
    accumulate(ao_w.reshape(-1, 4), r["texel"], r, nsamples, np.concatenate([r["d"], r["w"][:, None]], axis=1), ~np.asarray(occluded, bool))
    return ao_w


def bake(oracle, pkg, sd, select, width, height, spp, nsamples, cos_sample=True, max_distance=float("inf"), sampler="sobol", samples=None, ao_w=None, orc_scene=None):
    """The model's bake: dict(owner, position, normal, ao_w, n_rays). Occlusion: the oracle's any-hit query over the model's rays."""
    prims, uv_tris = scene_triangles(sd, select)
    owner = owner_map(uv_tris, prims, width, height)
    pos, nrm = planes(sd, owner)
    r = rays(oracle, pkg, sd, owner, spp, nsamples, cos_sample, sampler, samples)
    orc_scene = orc_scene or oracle.scene(sd)
    occ = orc_scene.trace_any(r["o"], r["d"], np.full(len(r["w"]), max_distance, F)) if len(r["w"]) else np.zeros(0, np.uint8)
    ao_w = np.zeros((height, width, 4), F) if ao_w is None else ao_w
    add_ao_rays(ao_w, r, occ, nsamples)
    return dict(owner=owner, position=pos, normal=nrm, ao_w=ao_w, n_rays=len(r["w"]), rays=r, occluded=occ)


def resolve(ao_w, spp):
    """(ao (H, W), bent (H, W, 3)): pt_bake_resolve."""
    x, y, z, w = (ao_w[..., k].astype(F) for k in range(4))
    any_ = (x != 0) | (y != 0) | (z != 0) | (w != 0)
    with np.errstate(all="ignore"):
        ao = np.where(any_, w / (F(spp) * PI), F(0)).astype(F)
        ln = np.sqrt(x * x + y * y + z * z).astype(F)
        ok = any_ & (ln > 0)
        inv = np.where(ok, F(1) / ln, F(0)).astype(F)
        bent = np.where(ok[..., None], np.stack([x * inv, y * inv, z * inv], axis=-1), F(0)).astype(F)
    return ao, bent


# ---- dilation ----
def dilate(owner, plane, iterations):
    """pt_bake_dilate: a dilated copy of `plane` ((H, W) or (H, W, channels))."""
    height, width = owner.shape
    out = np.array(plane, dtype=F).reshape(height, width, -1)
    covered = owner != NONE
    for _ in range(iterations):
        nxt, ncov = out.copy(), covered.copy()
        for y in range(height):
            for x in range(width):
                if covered[y, x]:
                    continue
                acc = np.zeros(out.shape[2], F); n = 0
                for dx, dy in NEIGHBOURS:
                    qx, qy = x + dx, y + dy
                    if 0 <= qx < width and 0 <= qy < height and covered[qy, qx]:
                        acc = acc + out[qy, qx]; n += 1
                if n:
                    nxt[y, x] = acc / F(n); ncov[y, x] = True
        out, covered = nxt, ncov
    return out.reshape(np.shape(plane))
