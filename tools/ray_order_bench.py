#!/usr/bin/env python3
"""Prices ONE thing on the GPU: which rays sit next to each other in the traversal's queue. A shaded vertex emits up to three rays from one point (continuation, MIS,
shadow); the mixed launch reads them as three segments, millions of entries apart. This tool traces the same ray set through trace_closest in two arrangements:
 (A) segments:    [all first cosine rays | all second cosine rays | all rays towards the light quad]   (what the queues hold today)
 (B) interleaved: origin 0's three rays, origin 1's three rays, ...                                      (what one tagged queue, filled vertex by vertex, would hold)
for two kinds of origins of the headline (C2) scene:
 camera:    the camera rays' hit points, in tile order of their pixels (neighbouring lanes = neighbouring pixels),
 scattered: the hit points of ONE cosine bounce ray per camera hit, kept in the order of their parent camera pixels (what a queue looks like a bounce further down).
A and B alternate in one session; per case the best of REPS launches, their median and every time are printed as one JSON line (ms, records per ray, Mrays/s). The last line
blends the two origin kinds by the scene's own per-depth vertex counts (path_length_hist of a small render of the same scene) into the predicted change of the mixed
launches' time. tools/study/ray_order_model.py is the CPU model of the same experiment.
Environment: MESH_N (1466), MIN_RAYS (16 200 000 per case), REPS (4), TRACE_MS (the step's `trace` class in ms, for the blend; 130.1 = profiles/r6/NOTES.md section 13)."""
import ctypes as C, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _pkg import import_pkg
pkg = import_pkg(); A = pkg._abi
n_mesh = int(os.environ.get("MESH_N", "1466")); min_rays = int(os.environ.get("MIN_RAYS", "16200000")); reps = int(os.environ.get("REPS", "4"))
trace_ms = float(os.environ.get("TRACE_MS", "130.1"))
XR, YR = 1920, 1080
lib = pkg.load_library(); lib.init(0)
b = pkg.scenes.ganesha_scale(n=n_mesh, xres=XR, yres=YR, spp=4)
sd, rp = b.world_end()
scene = pkg.Scene(lib, sd)
rng = np.random.default_rng(0)
say = lambda **kw: print(json.dumps(kw), flush=True)

# ---- per-depth vertex counts of the scene itself: a path that ends after b bounces had a vertex at every depth 1 .. b
scene.render(rp)
hist = np.asarray(scene.counters()["path_length_hist"], np.float64)
verts = np.array([hist[k:].sum() for k in range(1, 16)])           # verts[k - 1]: vertices at depth k (k = 1: the camera ray's hit)
frac_scattered = float(verts[1:].sum() / verts.sum())
say(path_length_hist=[int(x) for x in hist[:8]], vertices_per_depth=[int(x) for x in verts[:6]], scattered_fraction=round(frac_scattered, 4))

# ---- origins
xs, ys = np.meshgrid(np.arange(XR), np.arange(YR))
tile = (ys // 16) * (XR // 16) + xs // 16
order = np.lexsort((xs.ravel() % 16, ys.ravel() % 16, tile.ravel()))
px = np.stack([xs.ravel()[order], ys.ravel()[order]], axis=1).astype(np.float32)     # pixels in tile order
Pv = np.asarray(sd.P, np.float32).reshape(-1, 3); Iv = np.asarray(sd.idx, np.uint32).reshape(-1, 3)
shape = np.asarray(sd.prim_shape, np.uint32)
assert (shape >> 30 == 0).all(), "triangles only"

def camera_rays(spp):
    """`spp` rays per pixel, pixels in tile order, the samples of a pixel adjacent"""
    n = spp * len(px)
    cs = np.concatenate([np.repeat(px, spp, axis=0) + rng.random((n, 2), dtype=np.float32), rng.random((n, 3), dtype=np.float32)], axis=1).astype(np.float32)
    o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32)
    assert lib.lib.pt_camera_rays(C.byref(rp), n, cs.ctypes.data_as(A.fp), o.ctypes.data_as(A.fp), d.ctypes.data_as(A.fp)) == 0
    return o, d

def hit_points(o, d):
    """(origins a hair off the surface, geometric normals facing the incoming ray, which rays hit) of a closest-hit launch"""
    prim, t, _ = scene.trace_closest(o, d, np.full(len(o), np.inf, np.float32))
    hit = prim != 0xFFFFFFFF
    tri = Iv[shape[prim[hit]] & 0x3fffffff]
    p0, p1, p2 = Pv[tri[:, 0]], Pv[tri[:, 1]], Pv[tri[:, 2]]
    ng = np.cross(p1 - p0, p2 - p0); ng /= np.maximum(np.linalg.norm(ng, axis=1, keepdims=True), 1e-30)
    ng = np.where((ng * d[hit]).sum(axis=1, keepdims=True) > 0, -ng, ng).astype(np.float32)
    p = o[hit] + d[hit] * t[hit][:, None]
    return (p + 1e-3 * ng).astype(np.float32), ng, hit

def cosine_dirs(nrm):
    u = rng.random((len(nrm), 2)); r = np.sqrt(u[:, 0]); phi = 2 * np.pi * u[:, 1]
    l = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1 - u[:, 0])], axis=1)
    a = np.where(np.abs(nrm[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    t = np.cross(nrm, a); t /= np.linalg.norm(t, axis=1, keepdims=True); bt = np.cross(nrm, t)
    return (t * l[:, :1] + bt * l[:, 1:2] + nrm * l[:, 2:3]).astype(np.float32)

def origins(spp):
    o, d = camera_rays(spp)
    p_cam, n_cam, hit = hit_points(o, d)
    sample = (np.arange(len(o)) % spp)[hit]                     # which of its pixel's samples a camera hit is
    p_sc, n_sc, _ = hit_points(p_cam, cosine_dirs(n_cam))       # one cosine bounce per camera hit; the ones that hit something, in their parents' order
    return p_cam, n_cam, sample, p_sc, n_sc

# Most bounce rays off the ground leave the scene, so the scattered origins decide how many camera rays per pixel are needed.
yield_1 = len(origins(1)[3])
spp = int(np.ceil(1.02 * min_rays / 3 / yield_1))
p_cam, n_cam, sample, p_sc, n_sc = origins(spp)
m = min(len(p_sc), (min_rays + 2) // 3)                         # origins per case, the same for both kinds
k = 1 + int(np.searchsorted(np.cumsum(np.bincount(sample, minlength=spp)), m))     # the camera kind: the first k samples of every pixel, so the whole image and not its top
assert k <= spp
keep = sample < k
p_sc, n_sc, p_cam, n_cam = p_sc[:m], n_sc[:m], p_cam[keep][:m], n_cam[keep][:m]
say(camera_rays_per_pixel=spp, bounce_hits_per_camera_ray_per_pixel=yield_1, camera_samples_kept=k, origins_per_case=m, rays_per_case=3 * m)

def three_rays(p, nrm):
    """per origin: two cosine directions (tmax inf) and one ray to a point of the light quad (y = 4, |x|, |z| <= 1; tmax just short of it); arrays of shape (origins, 3 kinds, ...)"""
    lp = np.stack([rng.random(len(p)) * 2 - 1, np.full(len(p), 4.0), rng.random(len(p)) * 2 - 1], axis=1).astype(np.float32)
    D = np.stack([cosine_dirs(nrm), cosine_dirs(nrm), lp - p], axis=1).astype(np.float32)
    O = np.repeat(p[:, None, :], 3, axis=1)
    T = np.tile(np.array([np.inf, np.inf, 0.9999], np.float32), (len(p), 1))
    return O, D, T

def arrange(rays, interleaved):
    O, D, T = rays
    if not interleaved: O, D, T = O.transpose(1, 0, 2), D.transpose(1, 0, 2), T.T
    return np.ascontiguousarray(O).reshape(-1, 3), np.ascontiguousarray(D).reshape(-1, 3), np.ascontiguousarray(T).reshape(-1)

# ---- the four cases
res = {}
for kind, (p, nrm) in (("camera", (p_cam, n_cam)), ("scattered", (p_sc, n_sc))):
    rays = three_rays(p, nrm)
    arr = {"A_segments": arrange(rays, False), "B_interleaved": arrange(rays, True)}
    times = {a: [] for a in arr}; cnt = {}
    for _ in range(reps):                                       # A, B, A, B, ...
        for a, (ro, rd, rt) in arr.items():
            scene.trace_closest(ro, rd, rt)
            times[a].append(scene.kernel_stats()[0]["total_ms"]); cnt[a] = scene.counters()
    for a in arr:
        ms = min(times[a]); res[kind, a] = ms
        say(origins=kind, order=a, rays=3 * m, ms=round(ms, 3), ms_median=round(float(np.median(times[a])), 3), ms_all=[round(x, 3) for x in times[a]],
            records_per_ray=round(cnt[a]["bvh_nodes_visited"] / (3 * m), 2), tris_per_ray=round(cnt[a]["triangle_tests"] / (3 * m), 2), mrays_s=round(3 * m / ms / 1e3, 1))
    assert all(cnt["A_segments"][c] == cnt["B_interleaved"][c] for c in ("bvh_nodes_visited", "triangle_tests")), "the two arrangements are the same rays"

# ---- the blend. A scattered origin's rays cost more than a camera origin's, so each kind's share of the vertices is weighted by its arrangement-A time per ray.
r_cam = res["camera", "B_interleaved"] / res["camera", "A_segments"]; r_sc = res["scattered", "B_interleaved"] / res["scattered", "A_segments"]
w_sc = frac_scattered * res["scattered", "A_segments"]; w_cam = (1 - frac_scattered) * res["camera", "A_segments"]
blend = (w_sc * r_sc + w_cam * r_cam) / (w_sc + w_cam)
say(ratio_B_over_A_camera=round(r_cam, 4), ratio_B_over_A_scattered=round(r_sc, 4), scattered_fraction=round(frac_scattered, 4), blended_ratio=round(blend, 4),
    trace_ms=trace_ms, predicted_trace_saving_ms=round(trace_ms * (1 - blend), 2))
