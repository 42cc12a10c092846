"""Test-side reference of the ambient-occlusion integrator (integrators/ao.rs:63-110 in SamplerIntegrator::render,
integrator.rs:263-403), assembled from the CPU oracle's existing exports: Sobol' / Halton samples of dimensions 0-6, camera rays,
closest-hit and any-hit traversal, the single-triangle interaction (p, pError, n), offset_ray_origin and the deterministic sin / cos.
numpy float32 restates what the oracle does not export: the triangle's dpdu in triangle.rs's operation order, the AO frame and
directions, and the film deposit. Non-instanced triangle scenes (alpha masks included)."""
import ctypes as C
import numpy as np

F = np.float32
INV_PI = F(0.31830988618379067154)
INV4_PI = F(0.07957747154594766788)
PI = F(3.14159265358979323846)
PI_OVER_2, PI_OVER_4 = F(1.57079632679489661923), F(0.78539816339744830961)
COUNTER_KEYS = ("camera_rays", "intersect_tests", "shadow_tests", "bvh_nodes_visited", "triangle_tests", "sphere_tests")


def _cross(a, b):   # vector.rs:339-352: f64 products, one rounding
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(F)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(v):   # v * (1 / length)
    ln = np.sqrt(_dot(v, v)).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F(1) / ln).astype(F)
    return (v * inv[..., None]).astype(F)


def _coordinate_system(v1):   # vector.rs:551-559, first vector
    x, y, z = v1
    if abs(x) > abs(y):
        return (np.array([-z, F(0), x], F) * (F(1) / np.sqrt(F(x * x + z * z)))).astype(F)
    return (np.array([F(0), z, -y], F) * (F(1) / np.sqrt(F(y * y + z * z)))).astype(F)


def tri_dpdu(sd, tri):
    """Triangle::intersect's dpdu (triangle.rs:244-264), degenerate-uv fallback included."""
    i = sd.idx[tri]
    p0, p1, p2 = (sd.P[k].astype(F) for k in i)
    if sd.UV is not None and int(sd.tri_flags[tri]) & 16:   # PT_TRI_HAS_UV: this mesh has "uv" (other meshes' rows of sd.UV are zeros)
        uv = [sd.UV[k].astype(F) for k in i]
    else:
        uv = [np.array([0, 0], F), np.array([1, 0], F), np.array([1, 1], F)]
    duv02, duv12 = uv[0] - uv[2], uv[1] - uv[2]
    dp02, dp12 = p0 - p2, p1 - p2
    det = F(duv02[0] * duv12[1]) - F(duv02[1] * duv12[0])
    degenerate = abs(det) < F(1e-8)
    dpdu = dpdv = np.zeros(3, F)
    if not degenerate:
        invdet = F(1) / det
        dpdu = ((dp02 * duv12[1] - dp12 * duv02[1]) * invdet).astype(F)
        dpdv = ((dp02 * -duv12[0] + dp12 * duv02[0]) * invdet).astype(F)
    c = _cross(dpdu, dpdv)
    if degenerate or _dot(c, c) == 0:
        ng = _cross(p2 - p0, p1 - p0)
        dpdu = _coordinate_system(_normalize(ng))
    return dpdu


def _concentric(orc, u):   # sampling.rs:162-186 with the oracle's sin / cos
    ox, oy = F(u[0] * F(2) - F(1)), F(u[1] * F(2) - F(1))
    if ox == 0 and oy == 0:
        return F(0), F(0)
    if abs(ox) > abs(oy):
        r, theta = ox, F(PI_OVER_4 * F(oy / ox))
    else:
        r, theta = oy, F(PI_OVER_2 - F(PI_OVER_4 * F(ox / oy)))
    return F(F(orc.lib.orc_dm_cos(theta)) * r), F(F(orc.lib.orc_dm_sin(theta)) * r)


def _direction(orc, u, cos_sample):
    if cos_sample:   # cosine_sample_hemisphere + cosine_hemisphere_pdf
        x, y = _concentric(orc, u)
        z = np.sqrt(max(F(0), F(F(F(1) - F(x * x)) - F(y * y)))).astype(F)
        return np.array([x, y, z], F), F(abs(z) * INV_PI)
    z = F(F(1) - F(F(2) * u[0]))   # uniform_sample_sphere + uniform_sphere_pdf
    r = np.sqrt(max(F(F(1) - F(z * z)), F(0))).astype(F)
    phi = F(F(F(2) * PI) * u[1])
    return np.array([F(r * F(orc.lib.orc_dm_cos(phi))), F(r * F(orc.lib.orc_dm_sin(phi))), z], F), INV4_PI


class AOReference:
    def __init__(self, orc, A, sd, rp, nsamples=64, cos_sample=True):
        self.orc, self.A, self.sd, self.rp = orc, A, sd, rp
        self.ns, self.cos = int(nsamples), bool(cos_sample)
        self.osc = orc.scene(sd)
        self.counters = {k: 0 for k in COUNTER_KEYS + ("film_splats", "sanitized_nan", "sanitized_negative", "sanitized_infinite")}
        L = orc.lib
        L.orc_dm_sin.restype = C.c_float; L.orc_dm_sin.argtypes = [C.c_float]
        L.orc_dm_cos.restype = C.c_float; L.orc_dm_cos.argtypes = [C.c_float]

    def _count(self, kind):
        c = self.osc.counters()
        for k in ("bvh_nodes_visited", "triangle_tests", "sphere_tests"):
            self.counters[k] += c[k]
        self.counters[kind] += c[kind]

    def samples(self, pix, nums):
        """Dimensions 0-6 of sample numbers `nums` of pixels `pix` (n x 2)."""
        A, rp = self.A, self.rp
        pix = np.ascontiguousarray(pix, np.int32); nums = np.ascontiguousarray(nums, np.uint32)
        n = len(nums); out = np.zeros((n, 7), F); sb = (C.c_int32 * 4)(*rp.sample_bounds)
        if rp.sampler_type == A.PT_SAMPLER_HALTON:
            self.orc.lib.orc_halton_samples(sb, rp.sample_at_pixel_center, n, pix.ctypes.data_as(A.i32p), nums.ctypes.data_as(A.u32p), 7, out.ctypes.data_as(A.fp), None)
        else:
            self.orc.lib.orc_sobol_samples(sb, n, pix.ctypes.data_as(A.i32p), nums.ctypes.data_as(A.u32p), 7, out.ctypes.data_as(A.fp), None)
        return out

    def li(self, pix, s):
        """L of sample s of every pixel in `pix`, and its pfilm."""
        A, orc, rp = self.A, self.orc, self.rp
        n = len(pix)
        cs = self.samples(pix, np.full(n, s))
        pfilm = pix.astype(F) + cs[:, :2]
        cam = np.ascontiguousarray(np.concatenate([pfilm, cs[:, 2:5]], 1), F)
        o = np.zeros((n, 3), F); d = np.zeros((n, 3), F)
        orc.lib.orc_camera_rays(C.byref(rp), n, cam.ctypes.data_as(A.fp), o.ctypes.data_as(A.fp), d.ctypes.data_as(A.fp))
        self.counters["camera_rays"] += n
        prim, t, b = self.osc.trace_closest(o, d, np.full(n, np.inf, F))
        self._count("intersect_tests")
        L = np.zeros(n, F)
        fp = lambda a: a.ctypes.data_as(A.fp)
        for i in np.nonzero(prim != A.PT_NONE)[0]:
            tri = int(self.sd.prim_shape[prim[i]]) & 0x3fffffff
            tt, bb, p, perr, nn = (np.zeros(1, F), np.zeros(3, F), np.zeros(3, F), np.zeros(3, F), np.zeros(3, F))
            ok = orc.lib.orc_tri_intersect(self.osc.h, tri, fp(o[i].copy()), fp(d[i].copy()), C.c_float(np.inf), fp(tt), fp(bb), fp(p), fp(perr), fp(nn))
            assert ok
            n_ff = -nn if _dot(nn, -d[i]) < 0 else nn
            sv = _normalize(tri_dpdu(self.sd, tri))
            tv = _cross(nn, sv)
            u = self.samples(np.repeat(pix[i:i + 1], self.ns, 0), s * self.ns + np.arange(self.ns))[:, 5:7]
            ro = np.zeros((self.ns, 3), F); rd = np.zeros((self.ns, 3), F); w = np.zeros(self.ns, F)
            for k in range(self.ns):
                wi, pdf = _direction(orc, u[k], self.cos)
                wo = ((sv * wi[0] + tv * wi[1]).astype(F) + (n_ff * wi[2]).astype(F)).astype(F)
                orc.lib.orc_offset_ray_origin(fp(p), fp(perr), fp(nn), fp(wo), fp(ro[k]))
                rd[k] = wo
                w[k] = F(_dot(wo, n_ff) / F(pdf * F(self.ns)))
            occ = self.osc.trace_any(ro, rd, np.full(self.ns, np.inf, F))
            self._count("shadow_tests")
            acc = F(0)
            for k in range(self.ns):
                if not occ[k]:
                    acc = F(acc + w[k])
            L[i] = acc
        return L, pfilm

    def render(self):
        """RGB sums + weight of the cropped film (H, W, 4), converted to XYZ as Film::merge_film_tile does."""
        rp = self.rp
        cb, sb, pb = list(rp.cropped_pixel_bounds), list(rp.sample_bounds), list(rp.pixel_bounds)
        W, H = cb[2] - cb[0], cb[3] - cb[1]
        film = np.zeros((H, W, 4), F)
        ys, xs = np.mgrid[pb[1]:pb[3], pb[0]:pb[2]]
        pix = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.int32)
        table = np.array(list(rp.filter_table), F)
        rx, ry = F(rp.filter_radius[0]), F(rp.filter_radius[1])
        # the 16 x 16 tile of each pixel, its footprint bounds (film.rs:125-140)
        tx0 = sb[0] + ((pix[:, 0] - sb[0]) // 16) * 16; ty0 = sb[1] + ((pix[:, 1] - sb[1]) // 16) * 16
        tx1 = np.minimum(tx0 + 16, sb[2]); ty1 = np.minimum(ty0 + 16, sb[3])
        tb0 = np.maximum(np.ceil((tx0.astype(F) - F(0.5)) - rx).astype(np.int64), cb[0]); tb1 = np.maximum(np.ceil((ty0.astype(F) - F(0.5)) - ry).astype(np.int64), cb[1])
        tb2 = np.minimum(np.floor((tx1.astype(F) - F(0.5)) + rx).astype(np.int64) + 1, cb[2]); tb3 = np.minimum(np.floor((ty1.astype(F) - F(0.5)) + ry).astype(np.int64) + 1, cb[3])
        for s in range(rp.spp):
            L, pfilm = self.li(pix, s)
            y = ((F(0.212671) * L + F(0.715160) * L) + F(0.072169) * L).astype(F)
            nan, neg, inf = np.isnan(L), y < F(-1e-5), np.isinf(y)
            self.counters["sanitized_nan"] += int(nan.sum()); self.counters["sanitized_negative"] += int((neg & ~nan).sum())
            self.counters["sanitized_infinite"] += int((inf & ~nan & ~neg).sum())
            L = np.where(nan | neg | inf, F(0), L).astype(F)
            dx, dy = pfilm[:, 0] - F(0.5), pfilm[:, 1] - F(0.5)
            p0x = np.maximum(np.ceil(dx - rx).astype(np.int64), tb0); p0y = np.maximum(np.ceil(dy - ry).astype(np.int64), tb1)
            p1x = np.minimum(np.floor(dx + rx).astype(np.int64) + 1, tb2); p1y = np.minimum(np.floor(dy + ry).astype(np.int64) + 1, tb3)
            for oy in range(int((p1y - p0y).max(initial=0))):
                for ox in range(int((p1x - p0x).max(initial=0))):
                    X, Y = p0x + ox, p0y + oy
                    m = (X < p1x) & (Y < p1y)
                    fx = np.abs((X.astype(F) - dx) * (F(1) / rx) * F(16)); fy = np.abs((Y.astype(F) - dy) * (F(1) / ry) * F(16))
                    fw = table[np.minimum(np.floor(fy).astype(np.int64), 15) * 16 + np.minimum(np.floor(fx).astype(np.int64), 15)]
                    c = (L * fw).astype(F)
                    for i in np.nonzero(m)[0]:
                        cell = film[Y[i] - cb[1], X[i] - cb[0]]
                        cell[:3] += c[i]; cell[3] += fw[i]
                    self.counters["film_splats"] += int(m.sum())
        xyz = np.zeros_like(film)
        r, g, b = film[..., 0], film[..., 1], film[..., 2]
        xyz[..., 0] = (F(0.412453) * r + F(0.357580) * g) + F(0.180423) * b
        xyz[..., 1] = (F(0.212671) * r + F(0.715160) * g) + F(0.072169) * b
        xyz[..., 2] = (F(0.019334) * r + F(0.119193) * g) + F(0.950227) * b
        xyz[..., 3] = film[..., 3]
        return xyz

