"""The numpy model of the denoiser (include/mi355dn.h): the a-trous filter of pt_denoise, operation by operation. `dtype` = np.float32 runs every
operation in float32 in the device's order (dn_kernels.h) -- the device differs from it by its expf alone; np.float64 runs the same operations on the same float32
constants and inputs exactly enough to serve as the yardstick. Also here: the inputs of a test -- half films from the unchanged oracle, sums from aov_reference -- and
synthetic ones."""
import numpy as np

F = np.float32
DEFAULTS = dict(iterations=5, sigma_l=4.0, sigma_z=1.0, sigma_n=0.25, albedo_floor=0.01, scale=1.0)
TAPS = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)
BIN = (0.25, 0.5, 0.25)
XYZ2RGB = ((3.240479, -1.537150, -0.498535), (-0.969256, 1.875991, 0.041556), (0.055648, -0.204043, 1.057311))
LUM = (0.212671, 0.715160, 0.072169)


def _c(T, v):
    return T(F(v))   # a constant of the device's code: the float32 value, in the model's type


def resolve(xyzw, scale, T):
    """film_resolve_pixel (dev_math.h): rgb = max(0, xyz_to_rgb(xyz) / w) * scale; not divided and not clamped where w is 0."""
    x, y, z, w = (xyzw[..., k] for k in range(4))
    rgb = np.stack([(_c(T, r[0]) * x + _c(T, r[1]) * y) + _c(T, r[2]) * z for r in XYZ2RGB], -1)
    lit = w != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = T(1) / w
        rgb = np.where(lit[..., None], np.fmax(rgb * inv[..., None], T(0)), rgb)
    return rgb * _c(T, scale)


def lum(rgb, T):
    return (_c(T, LUM[0]) * rgb[..., 0] + _c(T, LUM[1]) * rgb[..., 1]) + _c(T, LUM[2]) * rgb[..., 2]


def _shift(a, dx, dy, fill=0):
    """b[y, x] = a[y + dy, x + dx], `fill` outside."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dx) < w and abs(dy) < h:
        b[yd, xd] = a[ys, xs]
    return b


def prepare(film_a, film_b, sums, albedo_floor, T):
    """The filter's first step: dict of d (H, W, 3), v, m (H, W, 3), n (H, W, 3), z, fw, valid, hit, and c = the film A + B resolved at scale 1."""
    a, b = film_a.astype(T), film_b.astype(T)
    aw, nw, dw = (sums[k].astype(T) for k in ("albedo", "normal", "depth"))
    ab = a + b   # summed per channel first
    ra, rb, c = resolve(a, 1.0, T), resolve(b, 1.0, T), resolve(ab, 1.0, T)
    valid = (a[..., 3] != 0) & (b[..., 3] != 0)
    hit = nw[..., 3] > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        has = aw[..., 3] != 0
        alb = np.where(has[..., None], aw[..., :3] / aw[..., 3:4], T(0))
        cov = np.where(has, np.fmin(nw[..., 3] / aw[..., 3], T(1)), T(0))
        length = np.sqrt((nw[..., 0] * nw[..., 0] + nw[..., 1] * nw[..., 1]) + nw[..., 2] * nw[..., 2])
        n = np.where((length != 0)[..., None], nw[..., :3] / length[..., None], T(0))
        z = np.where(hit, dw[..., 0] / dw[..., 1], T(0))
        m = np.fmax(alb + (T(1) - cov)[..., None], _c(T, albedo_floor))
        d = c / m
        dl = lum(ra / m, T) - lum(rb / m, T)
    v = np.where(valid, T(0.25) * (dl * dl), T(0))

    def slope(dx, dy):
        fwd, bwd = hit & _shift(hit, dx, dy, False), hit & _shift(hit, -dx, -dy, False)
        return np.where(fwd, np.abs(_shift(z, dx, dy) - z), np.where(bwd, np.abs(z - _shift(z, -dx, -dy)), T(0)))
    fw = slope(1, 0) + slope(0, 1)
    return dict(d=d.astype(T), v=v.astype(T), m=m.astype(T), n=n.astype(T), z=z.astype(T), fw=fw.astype(T), valid=valid, hit=hit, c=c, ab=ab)


def level(g, d, v, s, sigma_l, sigma_z, sigma_n, T):
    """One a-trous level of stride s over the valid pixels: (d', v'); invalid pixels keep theirs."""
    valid, hit, n, z, fw = g["valid"], g["hit"], g["n"], g["z"], g["fw"]
    vs, vw = np.zeros_like(v), np.zeros_like(v)
    for j in (-1, 0, 1):          # rows outer
        for i in (-1, 0, 1):
            ok = _shift(valid, i, j, False)   # the pixel's neighbours at every level, whatever the stride of the taps
            wk = T(BIN[j + 1] * BIN[i + 1])
            vs = np.where(ok, vs + wk * _shift(v, i, j), vs)
            vw = np.where(ok, vw + wk, vw)
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.sqrt(np.fmax(T(0), vs / vw))
    den_l = _c(T, sigma_l) * sd + _c(T, 1.0e-6)
    lum_p = lum(d, T)
    sn2 = _c(T, sigma_n) * _c(T, sigma_n)
    sw, sv = np.zeros_like(v), np.zeros_like(v)
    sc = np.zeros_like(d)
    for j in range(-2, 3):
        for i in range(-2, 3):
            dx, dy = s * i, s * j
            ok = valid & _shift(valid, dx, dy, False) & (_shift(hit, dx, dy, False) == hit)
            nq, zq, dq, vq = _shift(n, dx, dy), _shift(z, dx, dy), _shift(d, dx, dy), _shift(v, dx, dy)
            r = T(F(s) * np.sqrt(F(i * i + j * j)))
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                dot = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                e_n = np.where(hit, np.fmax(T(0), T(2) - T(2) * dot) / sn2, T(0))
                e_z = np.where(hit, np.abs(z - zq) / ((_c(T, sigma_z) * fw) * r + _c(T, 1.0e-4)), T(0))
                e_l = np.abs(lum_p - lum(dq, T)) / den_l
                w = T(TAPS[j + 2] * TAPS[i + 2]) * np.exp(-((e_n + e_z) + e_l))
                w = np.where(ok, w, T(0)).astype(T)
                sw = np.where(ok, sw + w, sw)
                sc = np.where(ok[..., None], sc + w[..., None] * dq, sc)
                sv = np.where(ok, sv + (w * w) * vq, sv)
    with np.errstate(divide="ignore", invalid="ignore"):
        d2 = np.where(valid[..., None], sc / sw[..., None], d)
        v2 = np.where(valid, sv / (sw * sw), v)
    return d2.astype(T), v2.astype(T)


def denoise_reference(film_a, film_b, sums, dtype=np.float32, **params):
    """pt_denoise of host arrays: film_a, film_b (H, W, 4), sums = {"albedo": (H, W, 4), "normal": (H, W, 4), "depth": (H, W, 2)}; params as PtDenoiseParams' fields
    (DEFAULTS where not given). Returns (H, W, 3) in `dtype`."""
    T = np.float32 if dtype in (np.float32, "float32") else np.float64
    p = dict(DEFAULTS); p.update(params)
    g = prepare(film_a, film_b, sums, p["albedo_floor"], T)
    d, v = g["d"], g["v"]
    for i in range(int(p["iterations"])):
        d, v = level(g, d, v, 1 << i, p["sigma_l"], p["sigma_z"], p["sigma_n"], T)
    out = np.fmax(T(0), d * g["m"]) * _c(T, p["scale"])
    plain = resolve(g["ab"], p["scale"], T)
    return np.where(g["valid"][..., None], out, plain).astype(T)


def params_struct(pkg, **params):
    """The PtDenoiseParams of the same keyword arguments."""
    p = dict(DEFAULTS); p.update(params)
    return pkg._abi_dn.PtDenoiseParams(int(p["iterations"]), *[float(p[k]) for k in ("sigma_l", "sigma_z", "sigma_n", "albedo_floor", "scale")])


def rel_mse(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2)))


def deviation(x, ref):
    """max |x - ref| / max(|ref|, 1e-3): the measure of the device's tolerance (test_denoise.py) and of the float32 model's floor (test_denoise_model.py)."""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(x - ref) / np.maximum(np.abs(ref), 1e-3)))


_CACHE = {}


def oracle_inputs(pkg, oracle, key, sd, rp):
    """(A, B, sums, yardstick) of an UNTEXTURED scene under the box filter from the unchanged oracle, computed once per `key` and left unchanged:
    A = render(spp = n / 2), B = render(spp = n) - A with the weights rounded -- sample k of a pixel depends on the pixel and k alone, and spp only scales texture
    differentials --, the sums of aov_reference.first_hit_reference, and the oracle's 1024-spp image."""
    if key not in _CACHE:
        from aov_reference import first_hit_reference
        n = rp.spp
        orc = oracle.scene(sd)
        try:
            rp.spp = n // 2
            a = orc.render(rp, nthreads=4).copy()
            rp.spp = n
            whole = orc.render(rp, nthreads=4)
            b = (whole - a).astype(F)
            b[..., 3] = np.rint(b[..., 3])
            rp.spp = 1024
            ref = orc.resolve(orc.render(rp, nthreads=4))
        finally:
            rp.spp = n
            orc.close()
        sums = first_hit_reference(pkg, oracle, ("denoise",) + tuple(key), sd, rp)[1]
        for arr in (a, b, ref, *sums.values()):
            arr.setflags(write=False)
        _CACHE[key] = (a, b, sums, ref)
    return _CACHE[key]


def synthetic_inputs(w, h, seed=0, guides="steps", invalid=0.0):
    """Half films and sums made by hand, 4 'samples' per half and pixel: a smooth image times an albedo pattern plus noise that differs between the halves.
    guides: "steps" -- a normal step at x = w / 2 and a depth step at y = h / 2, every pixel a hit; "boundary" -- hits left of a slanted line, misses right of it, the
    pixels ON the line partially covered; "miss" -- no hit at all. invalid: the fraction of pixels whose A.w or B.w is 0."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    spp = 4.0
    base = 0.4 + 0.3 * np.sin(xx / 7.0)[..., None] * np.array([1.0, 0.8, 0.6]) + 0.2 * (yy / max(h - 1, 1))[..., None]
    albedo = np.where((((xx // 5) + (yy // 4)) % 2)[..., None] > 0, np.array([0.8, 0.6, 0.3]), np.array([0.2, 0.5, 0.7]))
    if guides == "miss":
        cov = np.zeros((h, w))
    elif guides == "boundary":
        cov = np.clip(0.55 * w + 0.2 * yy - xx, 0.0, 1.0)
        cov = np.where((cov > 0) & (cov < 1), np.round(cov * spp * 2) / (spp * 2), cov)
        cov[h // 2, :] = np.where(cov[h // 2, :] > 0, 0.5, 0.0)   # a row of partially covered pixels
    else:
        cov = np.ones((h, w))
    normal = np.where((xx < w / 2)[..., None], np.array([0.0, 0.6, 0.8]), np.array([0.6, 0.0, 0.8]))
    depth = 4.0 + 0.05 * xx + 0.03 * yy + np.where(yy < h / 2, 0.0, 3.0)
    wsum = 2 * spp
    sums = {"albedo": np.concatenate([albedo * cov[..., None] * wsum, np.full((h, w, 1), wsum)], -1),
            "normal": np.concatenate([normal * (cov * wsum)[..., None], (cov * wsum)[..., None]], -1),
            "depth": np.stack([depth * cov * wsum, cov * wsum], -1)}
    m = albedo * cov[..., None] + (1.0 - cov)[..., None]
    rgb2xyz = np.linalg.inv(np.array(XYZ2RGB))
    halves = []
    for _ in range(2):
        rgb = base * m * np.exp(0.35 * rng.standard_normal((h, w, 1))) * (1.0 + 0.1 * rng.standard_normal((h, w, 3)))
        halves.append(np.concatenate([np.maximum(rgb, 0.0) @ rgb2xyz.T * spp, np.full((h, w, 1), spp)], -1))
    if invalid > 0:
        hole = rng.random((h, w))
        halves[0][hole < invalid / 2] = 0.0            # nothing at all in A
        halves[1][..., 3][(hole >= invalid / 2) & (hole < invalid)] = 0.0   # B without weight, its sums left: resolved undivided
    a, b = (x.astype(F) for x in halves)
    return a, b, {k: x.astype(F) for k, x in sums.items()}
