"""CPU model of the ray queue's order (no GPU): how many DISTINCT records and packets a wave of 64 consecutive queue entries asks for when a vertex's three rays
(two cosine bounce rays, one ray towards the light quad) are queued as three segments (one per kind: the order until the ray queue) or interleaved per vertex.
The walk is the production walk of wide_study.cpp (reference tree, two levels per record, reference order) with a log of every fetch; waves run in lock step.
Origins: the camera hits of a window of pixels in tile-major order (neighbouring lanes = neighbouring pixels), and the same points shuffled (what a queue looks
like a bounce further down). tools/ray_order_bench.py is the same experiment on the GPU.
usage: python tools/study/ray_order_model.py [mesh_n=733] [window=320]"""
import ctypes as C, os, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from _pkg import import_pkg
pkg = import_pkg(); A = pkg._abi
from oracle.oracle_binding import Oracle
out = os.path.join(tempfile.mkdtemp(prefix="ray_order_model_"), "libmodel.so")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, os.path.join(ROOT, "tools", "study", "ray_order_model.cpp")])
L = C.CDLL(out)
mesh_n = int(sys.argv[1]) if len(sys.argv) > 1 else 733
win = int(sys.argv[2]) if len(sys.argv) > 2 else 320
XR, YR = 1920, 1080
t0 = time.time()
b = pkg.scenes.ganesha_scale(n=mesh_n, xres=XR, yres=YR, spp=1)
sd, rp = b.world_end()
orc = Oracle(A, pkg.runtime.TABLES_PATH); sc = orc.scene(sd)
nodes, ordered = sc.bvh()
print(f"scene: {len(sd.idx)} triangles, {len(nodes)} reference nodes, built in {time.time() - t0:.1f} s")
Pv = np.ascontiguousarray(sd.P, np.float32); Iv = np.ascontiguousarray(sd.idx, np.uint32)
shape = np.asarray(sd.prim_shape, np.uint32)
assert (shape >> 30 == 0).all()
idx_by_prim = np.ascontiguousarray(Iv.reshape(-1, 3)[shape & 0x3fffffff], np.uint32)      # the model indexes triangles by primitive
L.model_set(nodes, ordered.ctypes.data_as(A.u32p), Pv.ctypes.data_as(A.fp), idx_by_prim.ctypes.data_as(A.u32p))
L.model_log.restype = C.c_uint64; L.model_groups.restype = C.c_double
ray_t = np.dtype([("o", np.float32, 3), ("d", np.float32, 3), ("tmax", np.float32), ("any", np.uint32)])
rng = np.random.default_rng(1)

# camera rays of a window around the image centre, one per pixel, in tile-major order (16 x 16 tiles)
x0, y0 = (XR - win) // 2, (YR - win) // 2
xs, ys = np.meshgrid(np.arange(x0, x0 + win), np.arange(y0, y0 + win))
order = np.lexsort((xs.ravel() % 16, ys.ravel() % 16, xs.ravel() // 16, ys.ravel() // 16))
n_cam = win * win
cs = np.concatenate([np.stack([xs.ravel()[order], ys.ravel()[order]], axis=1) + rng.random((n_cam, 2)), rng.random((n_cam, 3))], axis=1).astype(np.float32)
o = np.zeros((n_cam, 3), np.float32); d = np.zeros((n_cam, 3), np.float32)
assert orc.lib.orc_camera_rays(C.byref(rp), n_cam, cs.ctypes.data_as(A.fp), o.ctypes.data_as(A.fp), d.ctypes.data_as(A.fp)) == 0
cam = np.zeros(n_cam, ray_t); cam["o"] = o; cam["d"] = d; cam["tmax"] = np.inf
th = np.zeros(n_cam, np.float32); L.model_closest(cam.ctypes.data_as(C.c_void_p), n_cam, th.ctypes.data_as(A.fp))
hit = np.isfinite(th)
ph = o[hit] + d[hit] * th[hit][:, None]
nrm = np.where((ph[:, 1] < -1.15)[:, None], np.array([0, 1, 0], np.float32), ph / np.linalg.norm(ph, axis=1, keepdims=True)).astype(np.float32)   # the ground / the displaced sphere
ph = (ph + nrm * 1e-3).astype(np.float32)
m = len(ph)

def cosine_dirs(n):
    u = rng.random((len(n), 2)); r = np.sqrt(u[:, 0]); phi = 2 * np.pi * u[:, 1]
    l = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1 - u[:, 0])], axis=1)
    a = np.where(np.abs(n[:, :1]) > 0.9, np.array([[0, 1, 0]]), np.array([[1, 0, 0]]))
    t = np.cross(n, a); t /= np.linalg.norm(t, axis=1, keepdims=True); bt = np.cross(n, t)
    return (t * l[:, :1] + bt * l[:, 1:2] + n * l[:, 2:3]).astype(np.float32)

# ray 3 i + k: origin i, kind k (two cosine bounce rays, one towards the light quad: any hit, tmax just short of the light)
rays = np.zeros((m, 3), ray_t)
rays["o"] = ph[:, None, :]
rays["d"][:, 0] = cosine_dirs(nrm); rays["d"][:, 1] = cosine_dirs(nrm)
lp = np.stack([rng.random(m) * 2 - 1, np.full(m, 4.0), rng.random(m) * 2 - 1], axis=1).astype(np.float32)
rays["d"][:, 2] = lp - ph
rays["tmax"][:, :2] = np.inf; rays["tmax"][:, 2] = 0.9999; rays["any"][:, 2] = 1
rays = np.ascontiguousarray(rays.reshape(-1))
fetches = L.model_log(rays.ctypes.data_as(C.c_void_p), len(rays))
print(f"{m} origins of {n_cam} camera rays, {len(rays)} rays, {fetches / len(rays):.2f} fetches per ray (records + packets)")
print(f"per origin: the three rays' distinct fetches are {L.model_groups(len(rays), 3):.3f} of their summed fetches")

def waves(origin_order, interleaved):
    q = (3 * origin_order[:, None] + np.arange(3)).astype(np.uint32)
    q = np.ascontiguousarray(q.reshape(-1) if interleaved else q.T.reshape(-1))
    res = (C.c_double * 3)(); L.model_waves(q.ctypes.data_as(A.u32p), len(q), 64, res)
    return res[1] / res[0], res[2] / res[0]

print("| origins | order | distinct lines / lane fetch, per wave-step | ... per wave |\n|---|---|---|---|")
for name, oo in (("camera hit points, tile order", np.arange(m)), ("the same points shuffled", rng.permutation(m))):
    a, bb = waves(oo, False), waves(oo, True)
    print(f"| {name} | three segments | {a[0]:.3f} | {a[1]:.3f} |")
    print(f"| {name} | interleaved per vertex | {bb[0]:.3f} (x{bb[0] / a[0]:.2f}) | {bb[1]:.3f} (x{bb[1] / a[1]:.2f}) |")
