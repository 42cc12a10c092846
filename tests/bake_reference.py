"""A float32 numpy model of the texture-space bake's contract (include/mi355bake.h): ownership, the surface point, the AO rays, the sums and the dilation,
every operation in the header's order. numpy's float32 +, -, *, / and sqrt round as the device's do (no fusing on either side); what numpy has no twin of comes
from the oracle's probes: dm_sincosf (orc_dm_sin / orc_dm_cos), the samplers' array values (orc_sobol_samples / orc_halton_samples), and the occlusion of the
model's rays (orc_trace_any)."""
import numpy as np

F = np.float32
NONE = np.uint32(0xFFFFFFFF)
PI, PI_OVER_2, PI_OVER_4, INV_PI, INV_4PI = F(3.14159265358979323846), F(1.57079632679489661923), F(0.78539816339744830961), F(0.31830988618379067154), F(0.07957747154594766788)
MACH_EPS = F(5.9604644775390625e-08)
TRI_REVERSE, TRI_SWAPS, TRI_HAS_N, TRI_HAS_S, TRI_HAS_UV = 1, 2, 4, 8, 16
NEIGHBOURS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]   # (dx, dy): the dilation's order of summation


def gamma(n):
    return (F(n) * MACH_EPS) / (F(1) - F(n) * MACH_EPS)


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


def cross(a, b):   # vector.rs:339-352: f64 products, one rounding
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]).astype(F)


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def normalize(a):
    with np.errstate(all="ignore"):
        return a * (F(1) / np.sqrt(dot(a, a)))


def coordinate_system(v1):
    if abs(v1[0]) > abs(v1[1]):
        v2 = np.array([-v1[2], F(0), v1[0]], F) * (F(1) / np.sqrt(v1[0] * v1[0] + v1[2] * v1[2]))
    else:
        v2 = np.array([F(0), v1[2], -v1[1]], F) * (F(1) / np.sqrt(v1[1] * v1[1] + v1[2] * v1[2]))
    return v2, cross(v1, v2)


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
def next_up(v):
    v = np.where(v == 0, F(0), v).astype(F)   # -0 -> +0
    bits = v.view(np.uint32)
    out = np.where(v >= 0, bits + np.uint32(1), bits - np.uint32(1)).astype(np.uint32).view(F)
    return np.where(np.isposinf(v), v, out)


def next_down(v):
    v = np.where(v == 0, F(-0.0), v).astype(F)
    bits = v.view(np.uint32)
    out = np.where(v > 0, bits - np.uint32(1), bits + np.uint32(1)).astype(np.uint32).view(F)
    return np.where(np.isneginf(v), v, out)


def offset_ray_origin(p, perr, n, w):
    """dev_math.h: offset_ray_origin, rows of (m, 3) arrays."""
    d = np.abs(n[:, 0]) * perr[:, 0] + np.abs(n[:, 1]) * perr[:, 1] + np.abs(n[:, 2]) * perr[:, 2]
    offset = n * d[:, None]
    neg = (w[:, 0] * n[:, 0] + w[:, 1] * n[:, 1] + w[:, 2] * n[:, 2]) < 0
    offset = np.where(neg[:, None], -offset, offset)
    po = (p + offset).astype(F)
    return np.where(offset > 0, next_up(po), np.where(offset < 0, next_down(po), po)).astype(F)


def array_samples(oracle, pkg, sampler, width, height, px, py, numbers):
    """The 2-D array values (m, 2) of sample numbers `numbers` of pixels (px, py): dimensions 5 and 6 of a sampler for sample bounds [0, width) x [0, height)."""
    import ctypes as C
    A = pkg._abi
    m = len(numbers)
    sb = (C.c_int32 * 4)(0, 0, width, height)
    xy = np.ascontiguousarray(np.stack([px, py], axis=1), dtype=np.int32)
    num = np.ascontiguousarray(numbers, dtype=np.uint32)
    out = np.zeros((m, 7), F)
    args = (m, xy.ctypes.data_as(A.i32p), num.ctypes.data_as(A.u32p), 7, out.ctypes.data_as(A.fp), None)
    st = oracle.lib.orc_sobol_samples(sb, *args) if sampler == "sobol" else oracle.lib.orc_halton_samples(sb, 0, *args)
    assert st == 0, st
    return out[:, 5:7].copy()


def directions(oracle, u, cos_sample):
    """(wi (m, 3), pdf (m,)) of the array values u (m, 2): cosine_sample_hemisphere or uniform_sample_sphere (side/ao_rays.h: ao_ray)."""
    sin = np.frompyfunc(lambda x: oracle.lib.orc_dm_sin(float(x)), 1, 1)
    cos = np.frompyfunc(lambda x: oracle.lib.orc_dm_cos(float(x)), 1, 1)
    ux, uy = u[:, 0].astype(F), u[:, 1].astype(F)
    with np.errstate(all="ignore"):
        if cos_sample:
            ox, oy = ux * F(2) - F(1), uy * F(2) - F(1)
            first = np.abs(ox) > np.abs(oy)
            r = np.where(first, ox, oy).astype(F)
            theta = np.where(first, PI_OVER_4 * (oy / ox), PI_OVER_2 - PI_OVER_4 * (ox / oy)).astype(F)
            theta = np.where((ox == 0) & (oy == 0), F(0), theta).astype(F)
            s, c = sin(theta).astype(F), cos(theta).astype(F)
            dx, dy = c * r, s * r
            zero = (ox == 0) & (oy == 0)
            dx, dy = np.where(zero, F(0), dx).astype(F), np.where(zero, F(0), dy).astype(F)
            z = np.sqrt(np.maximum(F(0), F(1) - dx * dx - dy * dy)).astype(F)
            return np.stack([dx, dy, z], axis=1).astype(F), (np.abs(z) * INV_PI).astype(F)
        z = F(1) - F(2) * ux
        r = np.sqrt(np.maximum(F(1) - z * z, F(0))).astype(F)
        phi = (F(2) * PI) * uy
        s, c = sin(phi).astype(F), cos(phi).astype(F)
        return np.stack([r * c, r * s, z], axis=1).astype(F), np.full(len(ux), INV_4PI, F)


def rays(oracle, pkg, sd, owner, spp, nsamples, cos_sample, sampler, samples=None):
    """The AO rays of the owned texels of an owner map, for sample numbers `samples` = (first, n) of the job (default: all spp): dict(texel, s, k, o, d, w) of
    arrays over the rays, ordered by texel, then (s, k)."""
    height, width = owner.shape
    first, count = (0, spp) if samples is None else samples
    sis = texel_interactions(sd, owner)
    texels = np.array(sorted(sis), dtype=np.int64)
    per = count * nsamples
    tx = np.repeat(texels, per)
    s = np.tile(np.repeat(np.arange(first, first + count, dtype=np.int64), nsamples), len(texels))
    k = np.tile(np.arange(nsamples, dtype=np.int64), len(texels) * count)
    if len(tx) == 0:
        z3 = np.zeros((0, 3), F)
        return dict(texel=tx, s=s, k=k, o=z3, d=z3, w=np.zeros(0, F))
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
        w = ((wo[:, 0] * n[:, 0] + wo[:, 1] * n[:, 1] + wo[:, 2] * n[:, 2]) / (pdf * F(nsamples))).astype(F)
    return dict(texel=tx, s=s, k=k, o=o, d=wo, w=w)


def accumulate(ao_w, r, occluded, nsamples):
    """ao_w (H, W, 4) += the unoccluded rays' direction and weight, per texel in ascending (s, k) order. Returns ao_w (modified in place)."""
    flat = ao_w.reshape(-1, 4)
    order = r["s"] * nsamples + r["k"]
    free = ~np.asarray(occluded, bool)
    for j in np.unique(order):   # one (s, k) at a time: every texel has at most one ray of it
        m = (order == j) & free
        t = r["texel"][m]
        flat[t, 0:3] = flat[t, 0:3] + r["d"][m]
        flat[t, 3] = flat[t, 3] + r["w"][m]
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
    accumulate(ao_w, r, occ, nsamples)
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
