"""Vertex- and edge-aimed rays through the render path (the mixed k_trace<2, MODE, false, Q> launch), not only through pt_trace_closest.

With the Halton sampler and `sample_at_pixel_center`, every camera sample of pixel (x, y) is the ray through (x + 0.5, y + 0.5); oracle.orc_camera_rays
gives those rays bit for bit as the device makes them (test_gpu_parity.test_camera_rays_bit_exact). So a scene can put mesh vertices, and the midpoints of
shared edges, exactly on the rays the render will shoot:

  grid     a height field whose vertex (i, j) lies on the ray of pixel (i, j) at a jittered distance (valence 6: interior vertices are closed fans)
  fan{k}   independent closed fans, apex on the ray of every aimed pixel, the k rim vertices on the rays through a k-gon of 0.35 pixels round the
           pixel centre, at the apex's distance jittered by +-2 %; the apex is the first, second or third vertex of its triangles in turn. These are the
           rays on which the reference's t_max is not monotone: Triangle::intersect tests `tscaled < t_max * det`, then rounds t = tscaled * (1 / det)
           ABOVE that t_max, and `r.t_max = thit` raises it (the round-6 walk bug, csrc/kern_trace.h `t_slack`). test_fan_scenes_raise_t_max_on_the_oracle
           keeps that property asserted.
  edges    triangle pairs whose shared edge has its midpoint on the ray

Each adversary comes in four geometry variants, one per k_trace MODE (render_loop.hip launch_trace): 0 triangles only, 1 plus a sphere in view, 2 alpha
masks (half the fans are two coincident layers with complementary checkerboard alpha; shadowalpha on the occluder), 3 the aimed mesh as two object
instances (identity, and a half-size object under Scale 2 2 2: powers of two keep world <-> object space exact). A point light outside the frustum sits
behind an occluder grid whose vertices lie on the segments from the aimed points to the light (the NEE any-hit lanes pass within ulps of its shared
vertices). The point light is pure red and the environment is (0, 1, 1); every surface has Kd = (0.7, 0.6, 0.4), so whatever a surface reflects of the
environment has green / blue = 1.5^n >= 1.5 (n bounces), and a pixel that shows the environment (green = blue) where it should show a surface is
recognisable without the oracle.
"""
import ctypes as C
import time

import numpy as np
import pytest

from parity import assert_same_hits, assert_same_render

W, H = 128, 96              # film; the aimed pixels are those with x < AIM_X (the sphere of variant 1 sits to their right)
AIM_X = 96
KD = (0.7, 0.6, 0.4)        # green / blue = 1.5: the environment light a surface reflects has green / blue >= 1.5, the environment itself 1
ENV = (0.0, 1.0, 1.0)
LIGHT_FROM = (0.0, 8.0, 0.0)   # (the reference's point light lands at (x, y, x): x = 0 keeps it where it is written)
OCC_FRAC = 0.85             # the occluder lies 85 % of the way from the aimed points to the light
ULP23 = 2.0 ** -23
KINDS = ("grid", "fan6", "fan16", "fan48", "edges")
GEOMETRIES = (0, 1, 2, 3)
TREES = ("sah1", "sah4", "hlbvh")
FAN_STRIDE = {6: 1, 16: 1, 48: 2}   # every n-th pixel along x and y is aimed at (fan48 at full density: 0.44 M triangles)
RIM_PX = 0.35                # fan rims: vertices on the camera rays through a k-gon of this radius (in pixels) round the pixel centre ...
RIM_JIT = 0.02               # ... at the apex's distance times 1 +- RIM_JIT
T_BOUND = 8 * ULP23         # |t - t_aimed| / t_aimed on every aimed ray (measured worst cases: test output)


def _builder(pkg, geometry, tree):
    b = pkg.host.SceneBuilder()
    b.film.update(xres=W, yres=H)
    b.sampler = "halton"; b.sample_at_pixel_center = True; b.spp = 2
    b.integ["maxdepth"] = 3
    if tree == "hlbvh":
        b.split_method = "hlbvh"
    else:
        b.max_node_prims = int(tree[3:])
    b.look_at((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0))   # the camera at the origin: every primary ray starts at (0, 0, 0) exactly
    b.camera(fov=40.0)
    b.world_begin()
    return b


def pixel_rays(oracle, pkg, rp, pix, offset=0.5):
    """The render's camera ray of each pixel (x, y) in `pix` (n, 2), as the oracle (bit-identical to the device) makes it; `offset` (a number or (n, 2)):
    the film position inside the pixel (0.5: the centre, where every sample of the render lies)."""
    A = pkg._abi
    n = len(pix)
    cs = np.zeros((n, 5), np.float32)
    cs[:, :2] = pix + np.asarray(offset, np.float32); cs[:, 2:4] = 0.5
    o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32)
    assert oracle.lib.orc_camera_rays(C.byref(rp), n, cs.ctypes.data_as(A.fp), o.ctypes.data_as(A.fp), d.ctypes.data_as(A.fp)) == 0
    return o, d


def _frame(d):
    """Two unit vectors perpendicular to each d (float64)."""
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    a = np.where(np.abs(d[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    u = np.cross(d, a); u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u, np.cross(d, u)


class Adversary:
    """The aimed structures of one kind as float32 triangles; per aimed ray: its pixel, the float64 aimed point and the triangles that must contain it."""

    def __init__(self, kind, o, d, ij, rng, rays_at=None, ij_pix=None):
        o64, d64 = o.astype(np.float64), d.astype(np.float64)
        n = len(o)
        t = 4.0 + 0.5 * rng.random(n)
        if kind == "grid":
            # ij is the full lattice; vertex (i, j) on ray (i, j); two triangles per cell, every interior vertex has valence 6
            ni, nj = ij[:, 0].max() + 1, ij[:, 1].max() + 1
            P = (o64 + t[:, None] * d64).astype(np.float32)
            vid = np.arange(n).reshape(nj, ni)
            a, b, c, e = vid[:-1, :-1].ravel(), vid[:-1, 1:].ravel(), vid[1:, 1:].ravel(), vid[1:, :-1].ravel()
            idx = np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, e], 1)])
            interior = ((ij[:, 0] > 0) & (ij[:, 0] < ni - 1) & (ij[:, 1] > 0) & (ij[:, 1] < nj - 1))
            self.ray = np.nonzero(interior)[0]
            self.point = P[self.ray].astype(np.float64)
            inc = [[] for _ in range(n)]
            for tri, (p0, p1, p2) in enumerate(idx):
                inc[p0].append(tri); inc[p1].append(tri); inc[p2].append(tri)
            self.tris = [inc[v] for v in self.ray]
            self.owner = np.concatenate([np.arange(len(a))] * 2)   # the grid's structures: its cells (two triangles each)
        elif kind.startswith("fan"):
            k = int(kind[3:])
            apex = (o64 + t[:, None] * d64).astype(np.float32)
            # the rim vertex m of fan f on the camera ray through film position centre + RIM_PX (cos, sin)(phi_m), at the apex's distance jittered
            phi = 2 * np.pi * (np.arange(k) + 0.5 * rng.random((n, k))) / k
            ro, rd = rays_at(np.repeat(ij_pix, k, axis=0), 0.5 + RIM_PX * np.stack([np.cos(phi), np.sin(phi)], -1).reshape(-1, 2))
            tr = (t[:, None] * (1 + RIM_JIT * (2 * rng.random((n, k)) - 1))).reshape(-1, 1)
            rim = (ro.astype(np.float64) + tr * rd.astype(np.float64)).astype(np.float32).reshape(n, k, 3)
            P = np.concatenate([apex[:, None, :], rim], axis=1).reshape(-1, 3)       # k + 1 vertices per fan, apex first
            base = (k + 1) * np.arange(n)[:, None]
            i = np.arange(k)[None, :]
            idx = np.stack([np.broadcast_to(base, (n, k)), base + 1 + i, base + 1 + (i + 1) % k], axis=-1).reshape(-1, 3)
            rot = np.arange(n * k) % 3                         # the apex as the first, second and third vertex in turn (orientation kept)
            idx = np.take_along_axis(idx, (np.arange(3)[None, :] + rot[:, None]) % 3, axis=1)
            self.ray = np.arange(n)
            self.point = apex.astype(np.float64)
            self.tris = [list(range(f * k, (f + 1) * k)) for f in range(n)]
            self.owner = np.repeat(np.arange(n), k)
        elif kind == "edges":
            u, v = _frame(d64)
            mid = o64 + t[:, None] * d64
            e = 1e-3 * t
            jit = 0.002 * (2 * rng.random((n, 2)) - 1)
            dn = d64 / np.linalg.norm(d64, axis=1, keepdims=True)
            e0 = (mid + e[:, None] * u).astype(np.float32); e1 = (mid - e[:, None] * u).astype(np.float32)
            a0 = (mid + e[:, None] * v + jit[:, :1] * dn).astype(np.float32); a1 = (mid - e[:, None] * v + jit[:, 1:] * dn).astype(np.float32)
            P = np.stack([e0, e1, a0, a1], axis=1).reshape(-1, 3)
            base = 4 * np.arange(n)[:, None]
            idx = np.concatenate([base + [0, 1, 2], base + [1, 0, 3]], axis=1).reshape(-1, 3)
            self.ray = np.arange(n)
            self.point = (e0.astype(np.float64) + e1.astype(np.float64)) / 2     # the midpoint of the float32 edge
            self.tris = [[2 * f, 2 * f + 1] for f in range(n)]
            self.owner = np.repeat(np.arange(n), 2)
        else:
            raise ValueError(kind)
        self.P, self.idx = P, idx.astype(np.uint32)


def build_scene(pkg, oracle, kind, geometry, tree, seed=7):
    """(SceneData, PtRenderParams, info) of one instance. info: per aimed ray its pixel, origin, direction, float64 aimed point, and the prim ids of the
    triangles that contain that point (the ones of them that are opaque, under alpha); the occluder's prim ids; the kernel MODE the variant pins."""
    rng = np.random.default_rng(seed + 1000 * GEOMETRIES.index(geometry) + 100 * KINDS.index(kind))
    b = _builder(pkg, geometry, tree)
    rp0 = b.render_params()
    stride = FAN_STRIDE[int(kind[3:])] if kind.startswith("fan") else 1
    if kind == "grid":
        xs, ys = np.arange(0, AIM_X), np.arange(0, H)
    else:
        xs, ys = np.arange(stride // 2, AIM_X, stride), np.arange(stride // 2, H, stride)
    gx, gy = np.meshgrid(xs, ys)
    pix = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.int32)
    lattice = np.stack([np.meshgrid(np.arange(len(xs)), np.arange(len(ys)))[k].ravel() for k in (0, 1)], 1)
    o, d = pixel_rays(oracle, pkg, rp0, pix)
    adv = Adversary(kind, o, d, lattice, rng, lambda p, off: pixel_rays(oracle, pkg, rp0, p, off), pix)

    b.material("matte", Kd=KD)
    b.light_source("infinite", L=ENV)
    b.light_source("point", I=(40.0, 0.0, 0.0), from_=LIGHT_FROM)
    L = np.array(b.lights[-1].pos[:], np.float64)

    P, idx, owner = adv.P, adv.idx, adv.owner
    n_struct = owner.max() + 1
    opaque = np.ones(len(idx), bool)
    first = {}
    if geometry == 2:
        # half the structures (every second one) as two coincident layers with complementary checkerboard alpha: per triangle u = 0.25 (check 0 ->
        # alpha 1) or 1.25 (check 1 -> alpha 0), constant over the triangle; the union of the opaque triangles is the closed structure again
        b.texture("checks", "float", "checkerboard", tex1=1.0, tex2=0.0)
        masked = (owner % 2) == 1
        plain = ~masked
        keep_tri = np.nonzero(plain)[0]
        pv = P[idx[keep_tri]].reshape(-1, 3)
        first["plain"] = (b.trianglemesh(pv, np.arange(len(pv)).reshape(-1, 3)), keep_tri)
        mt = np.nonzero(masked)[0]
        cut = [((np.arange(len(idx)) % 2) == layer)[mt] for layer in (0, 1)]
        mv = np.concatenate([P[idx[mt]].reshape(-1, 3)] * 2)
        uv = np.zeros((len(mv), 2), np.float32)
        uv[:, 0] = np.repeat(np.where(np.concatenate(cut), 1.25, 0.25), 3); uv[:, 1] = 0.25
        first["masked"] = (b.trianglemesh(mv, np.arange(len(mv)).reshape(-1, 3), UV=uv, alpha="checks"), np.concatenate([mt, mt]), ~np.concatenate(cut))
    elif geometry == 3:
        half = owner < (n_struct + 1) // 2
        for name, sel, s in (("near", half, 1.0), ("half", ~half, 0.5)):
            tri = np.nonzero(sel)[0]
            b.object_begin(name)
            first[name] = (b.trianglemesh(P[idx[tri]].reshape(-1, 3) * np.float32(s), np.arange(3 * len(tri)).reshape(-1, 3)), tri)
            b.object_end()
        b.object_instance("near")
        b.attribute_begin(); b.scale(2.0, 2.0, 2.0); b.object_instance("half"); b.attribute_end()
    else:
        first["plain"] = (b.trianglemesh(P, idx), np.arange(len(idx)))
    if geometry == 1:
        b.attribute_begin(); b.translate(1.9, 0.0, 5.0); b.sphere(radius=0.25); b.attribute_end()   # right of the aimed pixels, in view

    # occluder: vertex (i, j) on the segment from aimed point (i, j) to the light; per-triangle UVs so that variant 2 cuts every second triangle
    ni, nj = lattice[:, 0].max() + 1, lattice[:, 1].max() + 1
    apt = np.zeros((len(lattice), 3))
    apt[adv.ray] = adv.point
    if kind == "grid":
        apt = adv.P.astype(np.float64)                     # (the border vertices too: the occluder covers the whole grid)
    ov = (apt + OCC_FRAC * (L - apt)).astype(np.float32)
    vid = np.arange(ni * nj).reshape(nj, ni)
    a, bb, c, e = vid[:-1, :-1].ravel(), vid[:-1, 1:].ravel(), vid[1:, 1:].ravel(), vid[1:, :-1].ravel()
    oidx = np.concatenate([np.stack([a, bb, c], 1), np.stack([a, c, e], 1)])
    if geometry == 2:
        b.texture("ochecks", "float", "checkerboard", tex1=1.0, tex2=0.0)
        ouv = np.zeros((3 * len(oidx), 2), np.float32)
        ouv[:, 0] = np.repeat(np.where(np.arange(len(oidx)) % 2 == 1, 1.25, 0.25), 3); ouv[:, 1] = 0.25
        occ_first = b.trianglemesh(ov[oidx].reshape(-1, 3), np.arange(3 * len(oidx)).reshape(-1, 3), UV=ouv, shadowalpha="ochecks")
    else:
        occ_first = b.trianglemesh(ov, oidx)
    sd, rp = b.world_end()

    # prim ids of the triangles that contain each aimed point (opaque ones only, under alpha)
    mesh_prims = [dict() for _ in range(len(idx))]   # local triangle -> [(prim, opaque)]
    for key, val in first.items():
        f0, tri = val[0], val[1]
        op = val[2] if len(val) > 2 else np.ones(len(tri), bool)
        for j, (tt, oo) in enumerate(zip(tri, op)):
            mesh_prims[tt][f0 + j] = bool(oo)
    want = [sorted(p for tt in tris for p, oo in mesh_prims[tt].items() if oo) for tris in adv.tris]
    info = dict(kind=kind, geometry=geometry, tree=tree, pix=pix[adv.ray], o=o[adv.ray], d=d[adv.ray], point=adv.point, want=want,
                occluder=(occ_first, occ_first + len(oidx)), n_tris=len(idx), instanced=geometry == 3, mode=geometry)
    return sd, rp, info


def all_pixel_rays(oracle, pkg, rp):
    gx, gy = np.meshgrid(np.arange(W), np.arange(H))
    pix = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.int32)
    return pix, pixel_rays(oracle, pkg, rp, pix)


def check_aimed_hits(info, prim, t, inst_prims=None):
    """Independent of the oracle, in float64: every aimed ray hits, the triangle it hits contains the aimed vertex (or edge), and t is within T_BOUND of the
    ray parameter of the aimed point, relative to it. Returns the worst relative error in units of 2^-23."""
    want = info["want"]
    missing = [i for i in range(len(want)) if int(prim[i]) not in want[i]]
    assert not missing, (len(missing), [(tuple(info["pix"][i]), int(prim[i]), want[i][:6]) for i in missing[:5]])
    d = info["d"].astype(np.float64); o = info["o"].astype(np.float64)
    ta = ((info["point"] - o) * d).sum(1) / (d * d).sum(1)
    rel = np.abs(t.astype(np.float64) - ta) / ta
    worst = float(rel.max())
    assert worst <= T_BOUND, (worst / ULP23, tuple(info["pix"][int(rel.argmax())]))
    return worst / ULP23, ta


def any_hit_tmax(ta):
    """t_max just short of / just past each aimed point: 2^-10 of its distance (far beyond the few ulps of the hit, far inside the structure's depth)."""
    return (ta * (1 - 2.0 ** -10)).astype(np.float32), (ta * (1 + 2.0 ** -10)).astype(np.float32)


def env_signature(rgb):
    return (np.abs(rgb[..., 0]) < 1e-3) & (np.abs(rgb[..., 1] - ENV[1]) < 1e-3) & (np.abs(rgb[..., 2] - ENV[2]) < 1e-3)


def check_film(info, rgb, occ_hits):
    """No aimed pixel shows the environment; the pixels beyond every structure do (the signature is right); no pixel-centre ray hits the occluder."""
    assert occ_hits == 0
    sig = env_signature(rgb)
    px = info["pix"]
    assert not sig[px[:, 1], px[:, 0]].any(), int(sig[px[:, 1], px[:, 0]].sum())
    assert sig[:, AIM_X + 2:W - 1].mean() > 0.5      # the strip right of the aimed pixels (the sphere covers part of it in variant 1)
    g, bl = rgb[px[:, 1], px[:, 0], 1], rgb[px[:, 1], px[:, 0], 2]
    lit = bl > 1e-3
    assert (g[lit] >= 1.49 * bl[lit]).all() and lit.mean() > 0.5   # what the aimed pixels show of the environment came off a surface


# -------------------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the adversary is real on the oracle (t_max raises), and the oracle's own hits pass the float64 checks

@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("kind", ["fan6", "fan16", "fan48"])
def test_fan_scenes_raise_t_max_on_the_oracle(pkg, oracle, kind, tree):
    sd, rp, info = build_scene(pkg, oracle, kind, 0, tree)
    orc = oracle.scene(sd)
    oracle.lib.orc_reset_tmax_raises()
    tmax = np.full(len(info["o"]), np.inf, np.float32)
    op, ot, ob = orc.trace_closest(info["o"], info["d"], tmax)
    raises = oracle.lib.orc_tmax_raises()
    worst, ta = check_aimed_hits(info, op, ot)
    lo, hi = any_hit_tmax(ta)
    assert not orc.trace_any(info["o"], info["d"], lo).any() and orc.trace_any(info["o"], info["d"], hi).all()
    oracle.lib.orc_reset_tmax_raises()
    film = orc.render(rp, nthreads=8)
    render_raises = oracle.lib.orc_tmax_raises()
    pix, (ao, adir) = all_pixel_rays(oracle, pkg, rp)
    ap, _, _ = orc.trace_closest(ao, adir, np.full(len(ao), np.inf, np.float32))
    check_film(info, orc.resolve(film), int(((ap >= info["occluder"][0]) & (ap < info["occluder"][1])).sum()))
    print(f"{kind} {tree}: {len(op)} aimed rays, {info['n_tris']} aimed triangles, t_max raises {raises} (trace) / {render_raises} (render), worst |dt|/t {worst:.2f} 2^-23")
    assert raises >= 100 and render_raises >= 100


@pytest.mark.parametrize("kind", ["grid", "edges"])
def test_grid_and_edge_scenes_hold_on_the_oracle(pkg, oracle, kind):
    """The same float64 checks on the oracle's hits for the other two adversaries (watertightness and tie order; they need not raise t_max)."""
    sd, rp, info = build_scene(pkg, oracle, kind, 0, "sah4")
    orc = oracle.scene(sd)
    op, ot, _ = orc.trace_closest(info["o"], info["d"], np.full(len(info["o"]), np.inf, np.float32))
    worst, ta = check_aimed_hits(info, op, ot)
    lo, hi = any_hit_tmax(ta)
    assert not orc.trace_any(info["o"], info["d"], lo).any() and orc.trace_any(info["o"], info["d"], hi).all()
    print(f"{kind}: {len(op)} aimed rays, worst |dt|/t {worst:.2f} 2^-23")


# -------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU: the render (k_trace<2, MODE, false, Q>) and pt_trace_closest / pt_trace_any on the same scenes, against the oracle and the float64 checks.
# Every kind under all three trees with triangles only, and every kind under each of the other three variants with one tree each (that variant's
# kernel does not change with the tree): 30 instances, about 230 000 aimed primary rays per walk.

INSTANCES = ([(k, 0, t) for k in KINDS for t in TREES] + [(k, 1, "sah1") for k in KINDS] + [(k, 2, "sah4") for k in KINDS] + [(k, 3, "hlbvh") for k in KINDS])
_ORACLE_RUNS = {}   # the oracle's side of an instance does not depend on the walk: made once, used by both


def _oracle_run(pkg, oracle, kind, geometry, tree):
    key = (kind, geometry, tree)
    if key not in _ORACLE_RUNS:
        sd, rp, info = build_scene(pkg, oracle, kind, geometry, tree)
        orc = oracle.scene(sd)
        inf = np.full(len(info["o"]), np.inf, np.float32)
        oracle.lib.orc_reset_tmax_raises()
        tr = orc.trace_closest(info["o"], info["d"], inf); tr_counters = orc.counters()
        raises = oracle.lib.orc_tmax_raises()
        check_aimed_hits(info, tr[0], tr[1])
        ta = ((info["point"] - info["o"].astype(np.float64)) * info["d"]).sum(1) / (info["d"].astype(np.float64) ** 2).sum(1)
        lo, hi = any_hit_tmax(ta)
        film = orc.render(rp, nthreads=8)
        counters = orc.counters()   # (every call sets the scene's counters anew)
        any_lo = orc.trace_any(info["o"], info["d"], lo); lo_counters = orc.counters()
        any_hi = orc.trace_any(info["o"], info["d"], hi); hi_counters = orc.counters()
        _ORACLE_RUNS[key] = dict(sd=sd, rp=rp, info=info, trace=tr, trace_counters=tr_counters, lo=lo, hi=hi, any_lo=any_lo, any_hi=any_hi,
                                 lo_counters=lo_counters, hi_counters=hi_counters, film=film, counters=counters, raises=raises)
        orc.close()
    return _ORACLE_RUNS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,geometry,tree", INSTANCES, ids=[f"{k}-m{g}-{t}" for k, g, t in INSTANCES])
def test_vertex_aimed_render_matches_oracle(pkg, gpu, oracle, kind, geometry, tree):
    t0 = time.perf_counter()
    R = _oracle_run(pkg, oracle, kind, geometry, tree)
    info = R["info"]
    g = pkg.Scene(gpu, R["sd"])
    film = g.render(R["rp"])
    assert_same_render(film, R["film"], g.counters(), R["counters"])
    # the trace launch of the render is the mixed kernel of the MODE this variant was built for
    traces = {k["kernel"] for k in g.kernel_stats() if k["kernel"].startswith("k_trace<")}
    assert any(k.startswith(f"k_trace<2, {info['mode']}, false, ") for k in traces), traces
    assert not any(k.startswith("k_trace<2, ") and not k.startswith(f"k_trace<2, {info['mode']}, ") for k in traces), traces
    # the film, independent of the oracle: no aimed pixel shows the environment, no pixel-centre ray reaches the occluder
    pix, (ao, adir) = all_pixel_rays(oracle, pkg, R["rp"])
    ap, _, _ = g.trace_closest(ao, adir, np.full(len(ao), np.inf, np.float32))
    check_film(info, g.resolve(film), int(((ap >= info["occluder"][0]) & (ap < info["occluder"][1])).sum()))
    # pt_trace_closest on the aimed rays: the float64 checks, and the oracle's (prim, t, b) bit for bit
    inf = np.full(len(info["o"]), np.inf, np.float32)
    gh = g.trace_closest(info["o"], info["d"], inf)
    worst, _ = check_aimed_hits(info, gh[0], gh[1])
    assert_same_hits(gh, R["trace"], g.counters(), R["trace_counters"])
    # pt_trace_any just short of / just past the aimed point
    lo = g.trace_any(info["o"], info["d"], R["lo"]); assert_same_hits(lo, R["any_lo"], g.counters(), R["lo_counters"])
    hi = g.trace_any(info["o"], info["d"], R["hi"]); assert_same_hits(hi, R["any_hi"], g.counters(), R["hi_counters"])
    assert not lo.any() and hi.all()
    g.close()
    print(f"\n{kind} m{geometry} {tree}: {len(gh[0])} aimed rays, oracle t_max raises {R['raises']} (trace), worst |dt|/t {worst:.2f} 2^-23, {time.perf_counter() - t0:.2f} s")
