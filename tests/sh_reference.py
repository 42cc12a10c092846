"""A float32 numpy model of the SH points' contract (include/mi355bake.h "SH points") on the model of the lightmap (tests/lightmap_reference.py, whose helpers it
uses). Light samples come from the oracle's Light::sample_li (orc_light_sample_li) with p_error = n = 0 -- a reference point without surface --, occlusion from its
any-hit query (orc_trace_any) with t_max = 1 - 1e-4. As there, the oracle's hook does not hand out the far end p1 of the visibility segment:
  * point and spot lights: p1 = the light's position; the shadow ray is (p, p1 - p);
  * triangle lights: Triangle::sample restated, the model's own wi held bit for bit against the oracle's, the whole ray by spawn_ray_to;
  * sphere, disk, distant and infinite lights: the device's ray (pt_bake_sh_rays) is taken over after two checks -- its origin is p bit for bit (with n = 0
    offset_ray_origin adds nothing), its direction deviates from wi by at most 4 x what the model's exact rays of a triangle light of the same scene show
    (lightmap_reference.py's yardstick, margin and reason).
The sums: 28 per point, E.c * Y_q(wi) at 3 q + c and the count at 27, in ascending (s, k)."""
import numpy as np
import bake_reference as M
import lightmap_reference as LM

F = M.F
T_MAX = LM.T_MAX
A_BAND = (F(3.141593), F(2.094395), F(0.785398))   # Ramamoorthi and Hanrahan's cosine-lobe factors of orders 0, 1, 2
A_Q = np.array([A_BAND[0]] + [A_BAND[1]] * 3 + [A_BAND[2]] * 5, F)


def basis(w):
    """Y_0 .. Y_8 (m, 9) at the rows (x, y, z) of w (m, 3): contract step 6, float32, unfused."""
    w = np.asarray(w, F).reshape(-1, 3)
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    with np.errstate(all="ignore"):
        Y = [np.full(len(w), F(0.282095), F), F(0.488603) * y, F(0.488603) * z, F(0.488603) * x, F(1.092548) * (x * y), F(1.092548) * (y * z),
             F(0.315392) * ((F(3.0) * (z * z)) - F(1.0)), F(1.092548) * (x * z), F(0.546274) * ((x * x) - (y * y))]
    return np.stack(Y, axis=1).astype(F)


def default_row(n):
    """ceil(sqrt(n))."""
    r = max(1, int(np.floor(np.sqrt(n))))
    while r * r < n:
        r += 1
    return r


def sample_list(n_points, spp, nsamples, samples=None):
    """(point, s, k) of every light sample, ordered by point, then (s, k): arrays of int64."""
    first, count = (0, spp) if samples is None else samples
    per = count * nsamples
    pt = np.repeat(np.arange(n_points, dtype=np.int64), per)
    s = np.tile(np.repeat(np.arange(first, first + count, dtype=np.int64), nsamples), n_points)
    k = np.tile(np.arange(nsamples, dtype=np.int64), n_points * count)
    return pt, s, k


def light_samples(oracle, pkg, sd, points, spp, nsamples, lights=None, sampler="sobol", row=None, samples=None, orc_scene=None, device=None):
    """Contract steps 1 to 5 for every light sample of the points: dict(point, s, k, light, wi, pdf, Li, E, o, d, contributes) in sample_list's order, and
    exact_dev / other_dev as lightmap_reference.light_samples. `device`: what Scene.bake_sh_rays returns for sample_list's samples; needed (and held) for the lights
    whose p1 the model cannot restate. Without it such a light's ray goes from p along wi, 2 x rough_world_radius long, and is never compared with the device."""
    A = pkg._abi
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n_points = len(points)
    row = default_row(n_points) if row is None else row
    rows = (n_points + row - 1) // row
    sel = LM.selected_lights(int(sd.desc().n_lights), lights)
    n_sel = len(sel)
    assert n_sel > 0 and (spp * nsamples) % n_sel == 0 and np.isfinite(points).all()
    pt, s, k = sample_list(n_points, spp, nsamples, samples)
    m = len(pt)
    z3 = lambda: np.zeros((m, 3), F)
    out = dict(point=pt, s=s, k=k, light=LM.light_of(sel, s * nsamples + k, nsamples).astype(np.uint32), wi=z3(), pdf=np.zeros(m, F), Li=z3(), E=z3(), o=z3(), d=z3(),
               contributes=np.zeros(m, bool), exact_dev=0.0, other_dev=0.0)
    orc_scene = orc_scene or oracle.scene(sd)
    u = M.array_samples(oracle, pkg, sampler, row, rows, pt % row, pt // row, s * nsamples + k)
    p = points[pt]
    fp = lambda a: a.ctypes.data_as(A.fp)
    zero = np.zeros(3, F)
    for t in range(n_points):   # Light::sample_li per (point, light): the oracle's hook takes one reference point and many samples
        rows_t = np.nonzero(pt == t)[0]
        ref = np.ascontiguousarray(points[t])
        for li in np.unique(out["light"][rows_t]):
            r = rows_t[out["light"][rows_t] == li]
            uu = np.ascontiguousarray(u[r], dtype=F)
            wi, pdf, L = np.zeros((len(r), 3), F), np.zeros(len(r), F), np.zeros((len(r), 3), F)
            st = oracle.lib.orc_light_sample_li(orc_scene.h, int(li), fp(ref), fp(zero), fp(zero), len(r), fp(uu), fp(wi), fp(pdf), fp(L))
            assert st == 0, st
            out["wi"][r], out["pdf"][r], out["Li"][r] = wi, pdf, L
    # contribution (step 4): no cosine, no side test
    scale = F(n_sel) / F(nsamples)
    with np.errstate(all="ignore"):
        ok = (out["pdf"] > 0) & ~(out["Li"] == 0).all(axis=1)
        w = (scale / out["pdf"]).astype(F)
        out["E"][ok] = (out["Li"] * w[:, None]).astype(F)[ok]
    out["contributes"] = ok
    # the shadow ray (step 5) from ref = {p, 0, 0}
    others = np.zeros(m, bool)
    for li in np.unique(out["light"]):
        r = np.nonzero((out["light"] == li) & ok)[0]
        if len(r) == 0:
            continue
        cls = LM.light_class(pkg, sd, int(li))
        z = np.zeros((len(r), 3), F)
        if cls == "position":
            L = sd.lights[int(li)]
            p1 = np.broadcast_to(np.array([L.pos[0], L.pos[1], L.pos[2]], F)[None, :], (len(r), 3)).astype(F)
            p1err, p1n = z, z
        elif cls == "triangle":
            p1, p1err, p1n = LM.triangle_sample(sd, int(sd.lights[int(li)].prim), u[r])
            mine = LM.vnormalize((p1 - p[r]).astype(F))
            assert mine.tobytes() == out["wi"][r].tobytes(), ("Triangle::sample restated: wi differs from the oracle's", int(li))
        else:
            others[r] = True
            continue
        out["o"][r], out["d"][r] = LM.spawn_ray_to(p[r], z, z, p1, p1err, p1n)
        assert out["o"][r].tobytes() == (p[r] + F(0)).astype(F).tobytes()   # n = 0: the ray starts at the point
        if cls == "triangle":
            out["exact_dev"] = max(out["exact_dev"], float(np.abs(LM.deviation(out["d"][r], out["wi"][r])).max()))
    r = np.nonzero(others)[0]
    if len(r):
        want_o = (p[r] + F(0)).astype(F)
        if device is None:
            out["o"][r] = want_o
            out["d"][r] = (out["wi"][r] * (F(2) * LM.rough_world_radius(sd))).astype(F)
        else:
            assert (np.asarray(device["found"])[r] == 3).all()
            assert device["o"][r].tobytes() == want_o.tobytes(), "a device ray taken over: its origin is not the point"
            out["other_dev"] = float(np.abs(LM.deviation(device["d"][r], out["wi"][r])).max())
            assert out["exact_dev"] > 0, "the scene has no triangle light whose exact rays set the yardstick"
            assert out["other_dev"] <= 4.0 * out["exact_dev"], (out["other_dev"], out["exact_dev"])
            out["o"][r], out["d"][r] = device["o"][r], device["d"][r]
    return out


def accumulate(sh_w, r, occluded, nsamples):
    """sh_w (n, 28) += (E.c * Y_q(wi), 1) of the unoccluded contributing samples, per point in ascending (s, k) order. Returns sh_w (modified in place)."""
    arrived = r["contributes"].copy()
    arrived[r["contributes"]] = ~np.asarray(occluded, bool)
    order = r["s"] * nsamples + r["k"]
    with np.errstate(all="ignore"):
        Y = basis(r["wi"])
        add = (r["E"][:, None, :] * Y[:, :, None]).astype(F).reshape(-1, 27)   # [sample][3 q + c]
        for j in np.unique(order):   # one (s, k) at a time: every point has at most one sample of it
            m = (order == j) & arrived
            t = r["point"][m]
            sh_w[t, 0:27] = (sh_w[t, 0:27] + add[m]).astype(F)
            sh_w[t, 27] = sh_w[t, 27] + F(1)
    return sh_w


def bake(oracle, pkg, sd, points, spp, nsamples=None, lights=None, sampler="sobol", row=None, samples=None, sh_w=None, orc_scene=None, device=None):
    """The model's bake: dict(sh_w (n, 28), n_rays, samples, occluded, nsamples). `device`: see light_samples."""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n_sel = len(LM.selected_lights(int(sd.desc().n_lights), lights))
    nsamples = n_sel if nsamples is None else nsamples
    orc_scene = orc_scene or oracle.scene(sd)
    r = light_samples(oracle, pkg, sd, points, spp, nsamples, lights, sampler, row, samples, orc_scene, device)
    ok = r["contributes"]
    n_rays = int(ok.sum())
    occ = orc_scene.trace_any(r["o"][ok], r["d"][ok], np.full(n_rays, T_MAX, F)) if n_rays else np.zeros(0, np.uint8)
    sh_w = np.zeros((len(points), 28), F) if sh_w is None else sh_w
    accumulate(sh_w, r, occ, nsamples)
    return dict(sh_w=sh_w, n_rays=n_rays, samples=r, occluded=np.asarray(occ), nsamples=nsamples)


def resolve(sh_w, spp, nsamples):
    """(sh (n, 9, 3), reached (n,)): pt_bake_sh_resolve."""
    sh_w = np.asarray(sh_w, F).reshape(-1, 28)
    any_ = (sh_w != 0).any(axis=-1)
    with np.errstate(all="ignore"):
        sh = np.where(any_[:, None], sh_w[:, 0:27] / F(spp), F(0)).astype(F).reshape(-1, 9, 3)
        reached = np.where(any_, sh_w[:, 27] / (F(spp) * F(nsamples)), F(0)).astype(F)
    return sh, reached


def irradiance(sh, normals):
    """E (n, 3) of the coefficients sh (n, 9, 3) under the unit normals (n, 3): pt_bake_sh_irradiance -- the sum over q ascending, from 0, of (A_q * sh[q, c]) * Y_q."""
    sh = np.asarray(sh, F).reshape(-1, 9, 3)
    Y = basis(normals)
    e = np.zeros((len(sh), 3), F)
    with np.errstate(all="ignore"):
        for q in range(9):
            e = (e + ((A_Q[q] * sh[:, q, :]).astype(F) * Y[:, q, None]).astype(F)).astype(F)
    return e
