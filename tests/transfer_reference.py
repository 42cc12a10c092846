"""A float32 numpy model of the transfer bake's contract (include/mi355bake.h "Transfer"): the projection ray of every owned texel of the target, the source hit
classified, height, position, world- and tangent-space normal, and the AO at the hit -- every operation in the header's order. It builds on bake_reference (owner
map, Triangle::intersect's interaction, array values, directions, sample_list, add_ao_rays) and on model_math's float32 arithmetic; the hits and the occlusion
come from the oracle's closest-hit and any-hit queries over the SOURCE scene."""
import types

import numpy as np
import bake_reference as M
from model_math import F, NONE, coordinate_system, cross, dot, normalize, offset_ray_origin


def partials(sd, prim):
    """(dpdu, dpdv) of Triangle::intersect (triangle.rs:236-265; dev_scene.h: tri_partials) for a triangle WITH UVs: bake_reference.interaction hands out dpdu alone,
    so the formula it uses stands here once more."""
    tri = int(sd.prim_shape[prim] & np.uint32(0x3fffffff))
    i0, i1, i2 = (int(i) for i in sd.idx[tri])
    p0, p1, p2 = M.v3(sd.P[i0]), M.v3(sd.P[i1]), M.v3(sd.P[i2])
    uv = [sd.UV[i].astype(F) for i in (i0, i1, i2)]
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
    return dpdu, dpdv


def source_interaction(sd, prim, b0, b1, b2):
    """bake_reference.interaction for a triangle of any mesh: one without UVs has (0, 0), (1, 0), (1, 1) at its corners (triangle.rs:109-115)."""
    tri = int(sd.prim_shape[prim] & np.uint32(0x3fffffff))
    if int(sd.tri_flags[tri]) & M.TRI_HAS_UV:
        return M.interaction(sd, prim, b0, b1, b2)
    i0, i1, i2 = (int(i) for i in sd.idx[tri])
    uv = {i0: np.array([0, 0], F), i1: np.array([1, 0], F), i2: np.array([1, 1], F)}
    view = types.SimpleNamespace(prim_shape=sd.prim_shape, tri_flags=sd.tri_flags, idx=sd.idx, P=sd.P, N=sd.N, S=sd.S, UV=uv)
    return M.interaction(view, prim, b0, b1, b2)


def top_level_triangles(sd):
    """Per primitive: a triangle that belongs to no instanced object (a detail hit's primitive)."""
    ok = (sd.prim_shape >> np.uint32(30)) == 0
    for k in range(sd.n_objects):
        ok[sd.objects[k].first_prim:sd.objects[k].first_prim + sd.objects[k].n_prims] = False
    return ok


def tangent_frame(si, dpdv, ns):
    """(sv, tv) of a target texel (step 4)."""
    with np.errstate(all="ignore"):
        sv = si["dpdu"] - ns * dot(ns, si["dpdu"])
        if dot(sv, sv) > 0:
            sv = normalize(sv)
            tv = cross(ns, sv)
            if dot(tv, dpdv) < 0:
                tv = -tv
            return sv, tv, False
        sv, tv = coordinate_system(ns)
        return sv, tv, True


def projection(sd_t, owner, front, back):
    """The projection rays of the owned texels (steps 1 and 2): dict(texel (m,), o, d (m, 3), t_max (m,), si: the target interactions, ns (m, 3))."""
    height, width = owner.shape
    sis = M.texel_interactions(sd_t, owner)
    texels = np.array(sorted(sis), dtype=np.int64)
    with np.errstate(all="ignore"):
        ns = np.array([normalize(sis[t]["sh_n"]) for t in texels], F).reshape(-1, 3)
        p = np.array([sis[t]["p"] for t in texels], F).reshape(-1, 3)
        o = (p + ns * F(front)).astype(F)
    return dict(texel=texels, o=o, d=(-ns).astype(F), t_max=np.full(len(texels), F(front) + F(back), F), si=[sis[t] for t in texels], ns=ns)


def ao_rays(oracle, pkg, hits, width, height, spp, nsamples, cos_sample, sampler, samples=None):
    """The AO rays of the detail hits (step 5), ordered by texel, then (s, k): dict(texel, s, k, o, d, w). hits: [(texel, hs, ns)]."""
    tx, s, k = M.sample_list([h[0] for h in hits], spp, nsamples, samples)
    if len(tx) == 0:
        z3 = np.zeros((0, 3), F)
        return dict(texel=tx, s=s, k=k, o=z3, d=z3, w=np.zeros(0, F))
    per = len(tx) // len(hits)
    u = M.array_samples(oracle, pkg, sampler, width, height, tx % width, tx // width, s * nsamples + k)
    wi, pdf = M.directions(oracle, u, cos_sample)
    with np.errstate(all="ignore"):
        rep = lambda rows: np.repeat(np.array(rows, F).reshape(-1, 3), per, axis=0)
        ng = rep([hs["n"] for _, hs, _ in hits])                                                       # hs.n: the origin's offset and t
        n = rep([(-hs["n"] if dot(hs["n"], ns) < 0 else hs["n"]) for _, hs, ns in hits])             # face_forward(hs.n, -d), -d = ns
        sv = rep([normalize(hs["dpdu"]) for _, hs, _ in hits])
        tv = rep([cross(hs["n"], normalize(hs["dpdu"])) for _, hs, _ in hits])
        p, perr = rep([hs["p"] for _, hs, _ in hits]), rep([hs["p_error"] for _, hs, _ in hits])
        wo = (sv * wi[:, 0:1] + tv * wi[:, 1:2] + n * wi[:, 2:3]).astype(F)
        o = offset_ray_origin(p, perr, ng, wo)
        w = (dot(wo, n) / (pdf * F(nsamples))).astype(F)
    return dict(texel=tx, s=s, k=k, o=o, d=wo, w=w)


def transfer(oracle, pkg, sd_t, sd_s, select, width, height, front, back, spp=1, nsamples=0, cos_sample=True, max_distance=float("inf"), sampler="sobol", samples=None, ao_w=None,
             orc_source=None):
    """The model's transfer bake: dict of the seven planes plus rays (the projection rays), t (their hits' t, by texel), detail ((H, W) bool), kinds (per owned texel
    "miss" / "detail" / "other"), fallback (texels whose tangent frame is coordinate_system's), ao_rays, occluded, n_rays. nsamples = 0: no AO."""
    prims, uv_tris = M.scene_triangles(sd_t, select)
    owner = M.owner_map(uv_tris, prims, width, height)
    pr = projection(sd_t, owner, front, back)
    orc_source = orc_source or oracle.scene(sd_s)
    m = len(pr["texel"])
    hp, ht, hb = orc_source.trace_closest(pr["o"], pr["d"], pr["t_max"]) if m else (np.zeros(0, np.uint32), np.zeros(0, F), np.zeros((0, 3), F))
    top = top_level_triangles(sd_s)
    n_tex = width * height
    hit_prim = np.full(n_tex, NONE, np.uint32); hgt = np.zeros(n_tex, F)
    pos, nrm, tn = np.zeros((n_tex, 3), F), np.zeros((n_tex, 3), F), np.zeros((n_tex, 3), F)
    detail = np.zeros(n_tex, bool); kinds = {}; fallback = []; hits = []; t_of = {}
    for j, texel in enumerate(int(t) for t in pr["texel"]):
        if hp[j] == NONE:
            kinds[texel] = "miss"
            continue
        hit_prim[texel] = hp[j]; hgt[texel] = F(front) - F(ht[j]); t_of[texel] = F(ht[j])
        if not top[hp[j]]:
            kinds[texel] = "other"
            continue
        kinds[texel] = "detail"; detail[texel] = True
        si, ns = pr["si"][j], pr["ns"][j]
        hs = source_interaction(sd_s, int(hp[j]), hb[j, 0], hb[j, 1], hb[j, 2])
        with np.errstate(all="ignore"):
            nh = normalize(hs["sh_n"])
            if dot(nh, -ns) > 0:
                nh = -nh
            sv, tv, fell = tangent_frame(si, partials(sd_t, int(owner.reshape(-1)[texel]))[1], ns)
            pos[texel] = hs["p"]; nrm[texel] = nh; tn[texel] = np.array([dot(nh, sv), dot(nh, tv), dot(nh, ns)], F)
        if fell:
            fallback.append(texel)
        hits.append((texel, hs, ns))
    out = dict(owner=owner, hit_prim=hit_prim.reshape(height, width), height=hgt.reshape(height, width), src_position=pos.reshape(height, width, 3),
               src_normal=nrm.reshape(height, width, 3), tangent_normal=tn.reshape(height, width, 3), rays=pr, t=t_of, detail=detail.reshape(height, width), kinds=kinds,
               fallback=fallback, n_rays=0)
    ao_w = np.zeros((height, width, 4), F) if ao_w is None else ao_w
    if nsamples:
        r = ao_rays(oracle, pkg, hits, width, height, spp, nsamples, cos_sample, sampler, samples)
        occ = orc_source.trace_any(r["o"], r["d"], np.full(len(r["w"]), max_distance, F)) if len(r["w"]) else np.zeros(0, np.uint8)
        M.add_ao_rays(ao_w, r, occ, nsamples)
        out.update(ao_rays=r, occluded=occ, n_rays=len(r["w"]))
    out["ao_w"] = ao_w
    return out
