"""float32 arithmetic as the device and the oracle write it (dev_math.h / ref_math.h), for the numpy models of the tests: products and sums left to right with
nothing fused (numpy's float32 +, -, *, / and sqrt round as the device's do: it is built with -ffp-contract=off and correctly rounded division and square root),
cross products through double with one rounding, a vector divided by its length multiplied by the reciprocal (vector.rs:481-495). What numpy has no twin of comes
from the oracle: dm_sincosf (orc_dm_sin / orc_dm_cos, element by element) and the samplers' values (orc_sobol_samples / orc_halton_samples).

Vectors are the trailing axis of 3 of an array of any shape; a transform is 16 numbers, row major, or one such row per vector."""
import ctypes as C

import numpy as np

F = np.float32
NONE = np.uint32(0xFFFFFFFF)
PI, PI_OVER_2, PI_OVER_4, INV_PI, INV_4PI = F(3.14159265358979323846), F(1.57079632679489661923), F(0.78539816339744830961), F(0.31830988618379067154), F(0.07957747154594766788)
MACH_EPS = F(5.9604644775390625e-08)


def gamma(n):
    return (F(n) * MACH_EPS) / (F(1) - F(n) * MACH_EPS)


# ---- vectors ----
def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def normalize(a):
    with np.errstate(all="ignore"):
        return a * (F(1) / np.sqrt(dot(a, a)))[..., None]


def cross(a, b):   # vector.rs:339-352: f64 products, one rounding
    a, b = a.astype(np.float64), b.astype(np.float64)
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(F)


def coordinate_system(v1):
    """(v2, v3) of one vector (3,)."""
    if abs(v1[0]) > abs(v1[1]):
        v2 = np.array([-v1[2], F(0), v1[0]], F) * (F(1) / np.sqrt(v1[0] * v1[0] + v1[2] * v1[2]))
    else:
        v2 = np.array([F(0), v1[2], -v1[1]], F) * (F(1) / np.sqrt(v1[1] * v1[1] + v1[2] * v1[2]))
    return v2, cross(v1, v2)


# ---- transforms ----
def _rows(m, v):
    m = np.asarray(m, F)
    return v[:, 0], v[:, 1], v[:, 2], lambda k: m[..., k]


def xf_point(m, p):
    """Transform::transform_point (transform.rs:413-432) with the divide by w where w != 1 (an affine transform's w is 1 exactly). p: (N, 3) float32."""
    x, y, z, M = _rows(m, p)
    q = np.stack([x * M(0) + y * M(1) + z * M(2) + M(3), x * M(4) + y * M(5) + z * M(6) + M(7), x * M(8) + y * M(9) + z * M(10) + M(11)], 1).astype(F)
    wp = x * M(12) + y * M(13) + z * M(14) + M(15)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (F(1.0) / wp).astype(F)
        return np.where((wp == F(1.0))[:, None], q, (q * inv[:, None]).astype(F)).astype(F)


def xf_point_err(m, p):
    """transform_point_with_error (transform.rs:434-459): the point and its absolute error bound."""
    x, y, z, M = _rows(m, p)
    err = np.stack([np.abs(x * M(0)) + np.abs(y * M(1)) + np.abs(z * M(2)) + np.abs(M(3)), np.abs(x * M(4)) + np.abs(y * M(5)) + np.abs(z * M(6)) + np.abs(M(7)),
                    np.abs(x * M(8)) + np.abs(y * M(9)) + np.abs(z * M(10)) + np.abs(M(11))], 1).astype(F) * gamma(3)
    return xf_point(m, p), err.astype(F)


def xf_vector(m, v):
    x, y, z, M = _rows(m, v)
    return np.stack([x * M(0) + y * M(1) + z * M(2), x * M(4) + y * M(5) + z * M(6), x * M(8) + y * M(9) + z * M(10)], 1).astype(F)


def xf_normal_inv(minv, n):   # Transform::transform_normal: the inverse's transpose
    x, y, z, M = _rows(minv, n)
    return np.stack([x * M(0) + y * M(4) + z * M(8), x * M(1) + y * M(5) + z * M(9), x * M(2) + y * M(6) + z * M(10)], 1).astype(F)


def transform_ray(m, o, d):
    """Transform::transform_ray (transform.rs:543-577): the origin moved along the direction by its error bound; the direction as it comes out."""
    ow, oerr = xf_point_err(m, o)
    dw = xf_vector(m, d)
    l2 = dot(dw, dw)
    with np.errstate(divide="ignore", invalid="ignore"):
        dt = (dot(np.abs(dw), oerr) / l2).astype(F)
    ow = np.where((l2 > 0)[:, None], (ow + dw * dt[:, None]).astype(F), ow)
    return ow.astype(F), dw


# ---- ray origins off a surface ----
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
    offset = np.where((dot(w, n) < 0)[:, None], -offset, offset)
    po = (p + offset).astype(F)
    return np.where(offset > 0, next_up(po), np.where(offset < 0, next_down(po), po)).astype(F)


def spawn_ray_to(p, perr, n, p1, p1err, p1n):
    """Interaction::spawn_ray_to (interaction.rs:45-52), rows of (m, 3) arrays: (o, d)."""
    with np.errstate(all="ignore"):
        o = offset_ray_origin(p, perr, n, (p1 - p).astype(F))
        t = offset_ray_origin(p1, p1err, p1n, (o - p1).astype(F))
        return o, (t - o).astype(F)


# ---- what the oracle lends ----
def dm_map(fn, x):
    """One of the oracle's device-math functions (orc_dm_sin, orc_dm_cos, orc_dm_acos), element by element."""
    return np.array([fn(float(v)) for v in x], F)


def dm_sin(oracle, x):
    return dm_map(oracle.lib.orc_dm_sin, x)


def dm_cos(oracle, x):
    return dm_map(oracle.lib.orc_dm_cos, x)


def concentric_sample_disk(oracle, u):
    """sampling.rs:153-176. u: (N, 2)."""
    ox, oy = (u[:, 0] * F(2.0) - F(1.0)).astype(F), (u[:, 1] * F(2.0) - F(1.0)).astype(F)
    wide = np.abs(ox) > np.abs(oy)
    with np.errstate(divide="ignore", invalid="ignore"):
        theta = np.where(wide, PI_OVER_4 * (oy / ox), PI_OVER_2 - PI_OVER_4 * (ox / oy)).astype(F)
    r = np.where(wide, ox, oy).astype(F)
    zero = (ox == 0) & (oy == 0)
    theta = np.where(zero, F(0.0), theta).astype(F)
    s, c = dm_sin(oracle, theta), dm_cos(oracle, theta)
    return np.where(zero[:, None], F(0.0), np.stack([c * r, s * r], 1)).astype(F)


def sampler_values(oracle, pkg, sampler, sample_bounds, pixels, numbers, n_dims, at_pixel_centre=0):
    """The first n_dims values (N, n_dims) of sample numbers `numbers` of the pixels (N, 2) under a sampler ("sobol" / "halton", or PT_SAMPLER_*) made for
    `sample_bounds`: orc_sobol_samples / orc_halton_samples."""
    A = pkg._abi
    xy = np.ascontiguousarray(pixels, dtype=np.int32)
    num = np.ascontiguousarray(numbers, dtype=np.uint32)
    out = np.zeros((len(num), n_dims), F)
    sb = (C.c_int32 * 4)(*sample_bounds)
    args = (len(num), xy.ctypes.data_as(A.i32p), num.ctypes.data_as(A.u32p), n_dims, out.ctypes.data_as(A.fp), None)
    if sampler in ("halton", A.PT_SAMPLER_HALTON):
        st = oracle.lib.orc_halton_samples(sb, at_pixel_centre, *args)
    else:
        st = oracle.lib.orc_sobol_samples(sb, *args)
    assert st == 0, st
    return out
