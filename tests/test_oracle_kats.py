"""Pins the CPU oracle against the reference's own known-answer / property tests
(/root/reference/tests/*.rs, restated here).  CPU only."""
import ctypes as C
import math
import numpy as np
import pytest


def _rev32(a):
    return int("{:032b}".format(a)[::-1], 2)


def test_sobol_dim0_is_bit_reversal(oracle):
    # tests/sampling.rs:99-106
    for i in range(8192):
        assert oracle.lib.orc_sobol_sample_float(i, 0, 0) == np.float32(_rev32(i)) * np.float32(2.3283064365386963e-10)


def test_radical_inverse_base2(oracle):
    # tests/sampling.rs:16-21
    for a in range(1024):
        assert oracle.lib.orc_radical_inverse(0, a) == np.float32(_rev32(a)) * np.float32(2.3283064365386963e-10)


def test_radical_inverse_other_bases(oracle):
    # lowdiscrepancy.rs:399-414 against an exact rational evaluation
    for bi, base in ((1, 3), (2, 5), (3, 7), (4, 11)):
        for n in (0, 1, 2, 7, 26, 127, 1151):
            digits = []; m = n
            while m:
                digits.append(m % base); m //= base
            exact = sum(d * float(base) ** -(k + 1) for k, d in enumerate(digits))
            assert abs(oracle.lib.orc_radical_inverse(bi, n) - exact) < 1e-6


def test_find_interval(oracle, pkg):
    # tests/find_interval.rs:7-22
    A = pkg._abi
    a = np.arange(10, dtype=np.float32)
    fi = lambda x: oracle.lib.orc_find_interval(len(a), a.ctypes.data_as(A.fp), x)
    assert fi(-1.0) == 0
    assert fi(100.0) == len(a) - 2
    for i in range(len(a) - 1):
        assert fi(float(i)) == i
        assert fi(i + 0.5) == i
        if i > 0:
            assert fi(i - 0.5) == i - 1


def test_next_float_up_down(oracle, pkg):
    # tests/fp.rs:24-43 with the RNG::default() stream
    A = pkg._abi
    up, down = oracle.lib.orc_next_float_up, oracle.lib.orc_next_float_down
    assert up(-0.0) > 0.0 and down(0.0) < 0.0
    assert up(math.inf) == math.inf and down(math.inf) < math.inf
    assert down(-math.inf) == -math.inf and up(-math.inf) > -math.inf
    n = 100000
    bits = np.zeros(n, np.uint32)
    oracle.lib.orc_rng_u32_stream(0, 1, n, bits.ctypes.data_as(A.u32p), None)
    f = bits.view(np.float32)
    ok = ~np.isnan(f) & ~np.isinf(f)
    f = f[ok]
    exp_up = np.nextafter(f, np.float32(np.inf)); exp_dn = np.nextafter(f, np.float32(-np.inf))
    for k in range(0, len(f), 37):  # subsample for speed; every element is checked vectorised below
        assert up(float(f[k])) == exp_up[k] and down(float(f[k])) == exp_dn[k]


def test_pcg32_known_stream(oracle, pkg):
    # core/rng.rs:25-76: PCG32 reference implementation values for RNG::default() (pcg32 demo vector state/stream)
    A = pkg._abi
    out = np.zeros(6, np.uint32)
    oracle.lib.orc_rng_u32_stream(0, 1, 6, out.ctypes.data_as(A.u32p), None)
    # independent Python restatement of rng.rs
    state, inc = 0x853c49e6748fea9b, 0xda3e39cb94b95bdb
    exp = []
    for _ in range(6):
        old = state
        state = (old * 0x5851f42d4c957f2d + inc) & (2**64 - 1)
        xs = (((old >> 18) ^ old) >> 27) & 0xffffffff
        rot = old >> 59
        exp.append(((xs >> rot) | (xs << ((-rot) & 31))) & 0xffffffff)
    assert list(out) == exp


def test_distribution1d_discrete(oracle, pkg):
    # tests/sampling.rs:202-257
    A = pkg._abi
    func = np.array([0.0, 1.0, 0.0, 3.0], dtype=np.float32)
    fp = func.ctypes.data_as(A.fp)
    dp = lambda i: oracle.lib.orc_dist1d_discrete_pdf(fp, 4, i)
    assert (dp(0), dp(1), dp(2), dp(3)) == (0.0, 0.25, 0.0, 0.75)

    def sd(u):
        pdf, ur = C.c_float(), C.c_float()
        i = oracle.lib.orc_dist1d_sample_discrete(fp, 4, u, C.byref(pdf), C.byref(ur))
        return i, pdf.value, ur.value
    assert sd(0.0)[:2] == (1, 0.25)
    assert sd(0.125) == (1, 0.25, 0.5)
    assert sd(0.24999)[:2] == (1, 0.25)
    assert sd(0.250001)[:2] == (3, 0.75)
    assert sd(0.625) == (3, 0.75, 0.5)
    assert sd(float(np.float32(1) - np.float32(2**-24)))[:2] == (3, 0.75)
    assert sd(1.0)[:2] == (3, 0.75)
    u = np.float32(0.25); umax = np.float32(0.25)
    for _ in range(20):
        u = np.nextafter(u, np.float32(-np.inf)); umax = np.nextafter(umax, np.float32(np.inf))
    while u < umax:
        if sd(float(u))[0] == 3:
            break
        assert sd(float(u))[0] == 1
        u = np.nextafter(u, np.float32(np.inf))
    assert u < umax
    while u <= umax:
        assert sd(float(u))[0] == 3
        u = np.nextafter(u, np.float32(np.inf))


def _one_triangle_scene(pkg, oracle, p):
    b = pkg.host.SceneBuilder()
    b.trianglemesh(np.array(p, dtype=np.float32), np.array([[0, 1, 2]], dtype=np.uint32))
    sd, _ = b.world_end()
    return oracle.scene(sd)


def test_triangle_badcase(oracle, pkg):
    # tests/shapes.rs:586-607: must return false
    A = pkg._abi
    s = _one_triangle_scene(pkg, oracle, [(-1113.45459, -79.049614, -56.2431908), (-1113.45459, -87.0922699, -56.2431908),
                                          (-1113.45459, -79.2090149, -56.2431908)])
    o = np.array([-1081.47925, 99.9999542, 87.7701111], np.float32); d = np.array([-32.1072998, -183.355865, -144.607635], np.float32)
    buf = [np.zeros(3, np.float32) for _ in range(4)]; t = C.c_float()
    hit = oracle.lib.orc_tri_intersect(s.h, 0, o.ctypes.data_as(A.fp), d.ctypes.data_as(A.fp), 0.9999, C.byref(t),
                                       *[x.ctypes.data_as(A.fp) for x in buf])
    assert hit == 0


def test_triangle_reintersect_property(oracle):
    # tests/shapes.rs:173-224 with the same seeds RNG::new(0..999) and the reference's 10 000 spawned ray pairs per triangle
    n = C.c_int()
    failures = oracle.lib.orc_test_triangle_reintersect(1000, 10000, C.byref(n))
    assert n.value > 100
    assert failures == 0


def test_bounds_union_with_empty(oracle, pkg):
    # tests/bounds.rs:22-35 through the BVH builder: the root of a 2-triangle scene is the union of both bounds
    b = pkg.host.SceneBuilder()
    b.trianglemesh(np.array([(-10, -10, 5), (0, 20, 10), (-5, 0, 7), (-15, 10, 30), (-15, 10, 30.5), (-14, 10, 30)], np.float32),
                   np.array([[0, 1, 2], [3, 4, 5]], np.uint32))
    sd, _ = b.world_end()
    nodes, _ = oracle.scene(sd).bvh()
    assert tuple(nodes[0].bmin) == (-15.0, -10.0, 5.0) and tuple(nodes[0].bmax) == (0.0, 20.0, 30.5)


def test_deterministic_math_against_libm(oracle):
    """The oracle and the kernels share one double-precision scheme for sin/cos/acos/atan2/ln. It must agree
    with the correctly rounded value to within 1 ulp everywhere and bit-exactly almost everywhere."""
    rng = np.random.default_rng(7)
    L = oracle.lib
    def check(fn, ref, xs, max_mismatch_frac):
        got = np.array([fn(float(x)) for x in xs], dtype=np.float32)
        exp = ref(xs.astype(np.float64)).astype(np.float32)
        ulp = np.abs(got.view(np.int32).astype(np.int64) - exp.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, ulp.max()
        assert (ulp != 0).mean() <= max_mismatch_frac
    xs = (rng.random(20000) * 8 - 2).astype(np.float32)
    check(L.orc_dm_sin, np.sin, xs, 1e-3)
    check(L.orc_dm_cos, np.cos, xs, 1e-3)
    check(L.orc_dm_acos, np.arccos, (rng.random(20000) * 2 - 1).astype(np.float32), 1e-3)
    check(L.orc_dm_log, np.log, (10 ** (rng.random(20000) * 6 - 4)).astype(np.float32), 1e-3)
    y = (rng.random(20000) * 2 - 1).astype(np.float32); x = (rng.random(20000) * 2 - 1).astype(np.float32)
    got = np.array([L.orc_dm_atan2(float(a), float(b)) for a, b in zip(y, x)], dtype=np.float32)
    exp = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32)
    ulp = np.abs(got.view(np.int32).astype(np.int64) - exp.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1 and (ulp != 0).mean() <= 1e-3
    assert L.orc_dm_atan2(0.0, -1.0) == np.float32(np.pi) and L.orc_dm_atan2(-0.0, -1.0) == -np.float32(np.pi)
    assert L.orc_dm_acos(1.0) == 0.0 and L.orc_dm_acos(-1.0) == np.float32(np.pi)


def test_furnace_closed_form(oracle, pkg):
    """Analytic check independent of any implementation: inside a closed box whose every face is a
    two-sided diffuse emitter Le with Lambertian albedo rho, E[L] = Le * sum_{k=0..maxdepth} rho^k for every pixel."""
    Le, rho, depth = 0.5, 0.6, 4
    b = pkg.host.SceneBuilder()
    b.film.update(xres=16, yres=16); b.spp = 256
    b.integ.update(maxdepth=depth, rrthreshold=0.0)  # rr_threshold 0 disables roulette (path.rs:209)
    b.look_at((0.1, 0.2, 0.0), (0.3, 0.1, 1.0), (0.0, 1.0, 0.0)); b.camera(fov=70.0)
    b.world_begin()
    b.material("matte", Kd=(rho, rho, rho))
    b.area_light_source(L=(Le, Le, Le), twosided=True)
    c = [(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)]
    faces = [(0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (3, 2, 6, 7), (0, 3, 7, 4), (1, 2, 6, 5)]
    idx = []
    for f in faces:
        idx += [(f[0], f[1], f[2]), (f[0], f[2], f[3])]
    b.trianglemesh(np.array(c, np.float32), np.array(idx, np.uint32))
    sd, rp = b.world_end()
    s = oracle.scene(sd)
    rgb = s.resolve(s.render(rp, nthreads=4))
    expected = Le * sum(rho ** k for k in range(depth + 1))
    assert abs(rgb.mean() - expected) < 0.01 * expected
    assert np.abs(rgb.mean(axis=2) - expected).max() < 0.15 * expected  # 256-spp Monte Carlo noise per pixel


def test_sphere_reintersect_property(oracle):
    # tests/shapes.rs:472-487 (full) and :538-565 (partial), seeds RNG::new(0..99); 2 000 ray pairs per sphere here
    f = oracle.lib.orc_test_sphere_reintersect
    for partial in (0, 1):
        n = C.c_int()
        failures = f(100, 2000, partial, C.byref(n))
        assert n.value > 20
        assert failures == 0, (partial, failures)


def test_spheres_scene_renders(oracle, pkg):
    sd, rp = pkg.scenes.spheres_c1(xres=48, yres=48, spp=8).world_end()
    s = oracle.scene(sd)
    rgb = s.resolve(s.render(rp, nthreads=4))
    c = s.counters()
    assert c["sphere_tests"] > 0 and np.isfinite(rgb).all() and rgb.mean() > 0.01


def test_instancing_equals_flattened_geometry(oracle, pkg):
    """TransformedPrimitive (primitive.rs:58-88): rendering ObjectInstances must agree with the same geometry emitted
    explicitly, up to the float differences of the object-space round trip (a few divergent paths)."""
    imgs = []
    for flatten in (False, True):
        sd, rp = pkg.scenes.instanced_garden(xres=64, yres=48, spp=16, flatten=flatten).world_end()
        s = oracle.scene(sd)
        imgs.append(s.resolve(s.render(rp, nthreads=4)))
    d = np.abs(imgs[0] - imgs[1])
    assert d.mean() < 5e-3 and (d.max(axis=2) > 0.1).mean() < 0.03


# ---- BSSRDF (row a23): no golden vectors exist in the reference for core/bssrdf.rs / core/interpolation.rs, so the
# restatement is pinned through the mathematical properties those functions must have ("parity unpinned" otherwise).
def _bss_table(pkg):
    import importlib
    B = importlib.import_module("pbrt_rust_amd.bssrdf")
    A = pkg._abi
    t = B.compute_beam_diffusion_bssrdf(0.0, 1.33)
    e = A.PtBSSRDFTable()
    e.n_rho, e.n_radius = t.n_rho, t.n_radius
    for name in ("rho_samples", "radius_samples", "profile", "rhoeff", "profile_cdf"):
        setattr(e, name, getattr(t, name).ctypes.data_as(A.fp))
    return B, t, e


def test_bssrdf_table_properties(pkg):
    B, t, _ = _bss_table(pkg)
    assert t.rho_samples[0] == 0.0 and abs(t.rho_samples[-1] - 1.0) < 1e-6 and np.all(np.diff(t.rho_samples) > 0)
    assert t.radius_samples[0] == 0.0 and np.all(np.diff(t.radius_samples) > 0)
    assert np.isfinite(t.profile).all() and (t.profile >= 0).all()
    assert np.all(np.diff(t.rhoeff) > 0) and t.rhoeff[0] == 0.0 and 0.9 < t.rhoeff[-1] < 1.3   # effective albedo grows with rho
    cdf = t.profile_cdf.reshape(t.n_rho, t.n_radius)
    assert np.all(np.diff(cdf[1:], axis=1) >= 0) and np.allclose(cdf[:, -1], t.rhoeff)
    # subsurface_from_diffuse inverts rhoeff(rho) (bssrdf.rs:190-202)
    sa, ss = B.subsurface_from_diffuse(t, [0.2, 0.5, 0.8], [1.0, 2.0, 0.5])
    rho = ss / (sa + ss)
    got = np.interp(rho, t.rho_samples, t.rhoeff)
    assert np.allclose(got, [0.2, 0.5, 0.8], atol=5e-3)
    assert np.allclose(1.0 / (sa + ss), [1.0, 2.0, 0.5], rtol=1e-5)


def test_catmull_rom_weights_partition_of_unity(oracle, pkg):
    import ctypes as C
    A = pkg._abi
    nodes = np.array([0.0, 0.1, 0.25, 0.5, 1.0, 2.0, 4.5], dtype=np.float32)
    vals = (3.0 * nodes - 1.0).astype(np.float32)   # cubic Hermite splines reproduce linear functions exactly
    for x in np.linspace(0.0, 4.49, 97, dtype=np.float32):
        off = C.c_int(0); w = np.zeros(4, dtype=np.float32)
        assert oracle.lib.orc_catmull_rom_weights(len(nodes), nodes.ctypes.data_as(A.fp), float(x), C.byref(off), w.ctypes.data_as(A.fp)) == 1
        assert abs(w.sum() - 1.0) < 1e-5
        acc = sum(float(w[i]) * float(vals[off.value + i]) for i in range(4) if w[i] != 0.0)
        assert abs(acc - (3.0 * float(x) - 1.0)) < 1e-4
    off = C.c_int(0); w = np.zeros(4, dtype=np.float32)
    assert oracle.lib.orc_catmull_rom_weights(len(nodes), nodes.ctypes.data_as(A.fp), 4.5, C.byref(off), w.ctypes.data_as(A.fp)) == 0   # x == last node: out
    assert oracle.lib.orc_catmull_rom_weights(len(nodes), nodes.ctypes.data_as(A.fp), -0.1, C.byref(off), w.ctypes.data_as(A.fp)) == 0


def test_bssrdf_radial_pdf_normalised_and_sampling_inverts_it(oracle, pkg):
    """pdf_sr is a density over the plane: int pdf_sr(r) 2 pi r dr == 1 (within the table's radius range), and
    sample_sr(u) is the inverse of that CDF (bssrdf.rs:492-541, interpolation.rs:133-226)."""
    A = pkg._abi
    _, t, e = _bss_table(pkg)
    import ctypes as C
    siga = np.array([0.05, 0.4, 2.0], dtype=np.float32); sigs = np.array([1.5, 1.0, 3.0], dtype=np.float32)
    r = np.concatenate([[0.0], np.geomspace(1e-5, 250.0, 20000)]).astype(np.float32)
    sr = np.zeros((len(r), 3), dtype=np.float32); pdf = np.zeros((len(r), 3), dtype=np.float32)
    oracle.lib.orc_bssrdf_sr(C.byref(e), siga.ctypes.data_as(A.fp), sigs.ctypes.data_as(A.fp), 1.33, len(r), r.ctypes.data_as(A.fp),
                             sr.ctypes.data_as(A.fp), pdf.ctypes.data_as(A.fp))
    assert np.isfinite(sr).all() and (sr >= 0).all() and (pdf >= 0).all()
    rd = r.astype(np.float64)
    for ch in range(3):
        f = pdf[:, ch].astype(np.float64) * 2.0 * np.pi * rd
        cdf = np.concatenate([[0.0], np.cumsum(0.5 * (f[1:] + f[:-1]) * np.diff(rd))])
        assert abs(cdf[-1] - 1.0) < 0.02, (ch, cdf[-1])
        u = np.linspace(0.02, 0.98, 49, dtype=np.float32); out = np.zeros_like(u)
        oracle.lib.orc_bssrdf_sample_sr(C.byref(e), siga.ctypes.data_as(A.fp), sigs.ctypes.data_as(A.fp), 1.33, ch, len(u), u.ctypes.data_as(A.fp), out.ctypes.data_as(A.fp))
        assert np.all(np.diff(out) > 0)
        assert np.abs(np.interp(out, rd, cdf) - u).max() < 0.02
    # Sr == pdf_sr * rho_eff: the ratio is independent of r for a channel
    for ch in range(3):
        m = pdf[100:15000, ch] > 1e-12
        ratio = sr[100:15000, ch][m] / pdf[100:15000, ch][m]
        assert m.sum() > 1000 and ratio.std() / ratio.mean() < 1e-4


def test_bssrdf_sw_is_normalised(oracle):
    """sw (bssrdf.rs:324-328) integrates to ~1 over the cosine-weighted hemisphere by construction of c."""
    mu = (np.arange(4000) + 0.5) / 4000.0
    for eta in (1.2, 1.33, 1.5):
        vals = np.array([oracle.lib.orc_bssrdf_sw(eta, float(m)) for m in mu])
        assert abs((vals * mu * 2.0 * np.pi).mean() - 1.0) < 0.02


def test_subsurface_scene_renders(oracle, pkg):
    sd, rp = pkg.scenes.subsurface_c5(xres=48, yres=32, spp=8).world_end()
    s = oracle.scene(sd)
    rgb = s.resolve(s.render(rp, nthreads=4))
    assert np.isfinite(rgb).all() and rgb.mean() > 0.05
    # subsurface objects are not black where the camera sees them (light re-emerges through the adapter lobe)
    assert rgb[12:24, 8:40].mean() > 0.05


def test_image_environment_map(oracle, pkg):
    """InfiniteAreaLight with an image map (infinite.rs:62-81,118-177): the importance image is the level-0 bilinear lookup
    (scalar restatement below), and a furnace-like scene lit only by the map converges to the map's cosine-weighted mean."""
    import math
    from pbrt_rust_amd import host as H
    F = np.float32
    tex = pkg.scenes.sky_env(8, 4)
    img = H._env_importance(tex)
    h, w, _ = tex.shape
    yw = np.array([0.212671, 0.715160, 0.072169], dtype=F)
    for (v, u) in [(0, 0), (3, 5), (7, 15), (4, 8)]:
        s = F(F((F(u) + F(.5)) / F(2 * w)) * F(w) - F(.5)); t = F(F((F(v) + F(.5)) / F(2 * h)) * F(h) - F(.5))
        s0, t0 = math.floor(s), math.floor(t); ds, dt = F(s - F(s0)), F(t - F(t0))
        tx = lambda a, b: tex[b % h, a % w]
        rgb = tx(s0, t0) * F(F(1 - ds) * F(1 - dt)) + tx(s0, t0 + 1) * F(F(1 - ds) * dt)
        rgb = (rgb.astype(F) + tx(s0 + 1, t0) * F(ds * F(1 - dt))).astype(F); rgb = (rgb + tx(s0 + 1, t0 + 1) * F(ds * dt)).astype(F)
        y = F(F(yw[0] * rgb[0] + yw[1] * rgb[1]) + yw[2] * rgb[2])
        assert img[v, u] == F(y * F(math.sin(F(math.pi) * (F(v) + F(.5)) / F(2 * h))))
    with pytest.raises(ValueError):
        H._env_importance(np.ones((3, 5, 3), dtype=F))
    # a camera looking at the sky only: every pixel is the (bilinear) map value in its direction
    b = pkg.host.SceneBuilder()
    b.film.update(xres=32, yres=16); b.spp = 4
    b.look_at((0, 0, 0), (0, 1, 0.2), (0, 0, 1)); b.camera(fov=60.0)
    b.world_begin()
    b.light_source("infinite", texels=tex, L=(1.0, 1.0, 1.0))
    b.material("matte", Kd=(0.5, 0.5, 0.5))
    P, I = pkg.scenes.quad((-1, -5, -1), (1, -5, -1), (1, -5, 1), (-1, -5, 1))   # behind the camera
    b.trianglemesh(P, I)
    sd, rp = b.world_end()
    s = oracle.scene(sd)
    rgb = s.resolve(s.render(rp, nthreads=2))
    assert np.isfinite(rgb).all() and rgb.min() > 0.2 and rgb.max() <= tex.max() * 1.0001
    assert rgb.max() > 5.0   # the sun patch is in view


def _light_probe(oracle, pkg, s, li, p, n_s=4096, seed=3):
    import ctypes as C
    A = pkg._abi
    fp = lambda a: a.ctypes.data_as(A.fp)
    rng = np.random.default_rng(seed)
    p = np.asarray(p, dtype=np.float32); perr = np.zeros(3, np.float32); nrm = np.array([0, 1, 0], np.float32)
    u = rng.random((n_s, 2), dtype=np.float32)
    wi = np.zeros((n_s, 3), np.float32); pdf = np.zeros(n_s, np.float32); L = np.zeros((n_s, 3), np.float32)
    oracle.lib.orc_light_sample_li(s.h, li, fp(p), fp(perr), fp(nrm), n_s, fp(u), fp(wi), fp(pdf), fp(L))
    back = np.zeros(n_s, np.float32)
    oracle.lib.orc_light_pdf_li(s.h, li, fp(p), fp(perr), fp(nrm), n_s, fp(wi), fp(back))
    # uniform directions for the normalisation integral
    z = 1 - 2 * rng.random(200000); ph = 2 * np.pi * rng.random(200000); r = np.sqrt(1 - z * z)
    w = np.stack([r * np.cos(ph), r * np.sin(ph), z], axis=1).astype(np.float32)
    dens = np.zeros(len(w), np.float32)
    oracle.lib.orc_light_pdf_li(s.h, li, fp(p), fp(perr), fp(nrm), len(w), fp(w), fp(dens))
    return wi, pdf, L, back, float(np.abs(dens).mean() * 4 * np.pi)


def test_sphere_area_light_sampling_properties(oracle, pkg):
    """Sphere::sample_interaction / pdf_wi (sphere.rs:313-395): sampled directions carry the density pdf_li reports, pdf_li
    integrates to 1 over the sphere of directions (cone branch and inside branch), and the cone branch reproduces the
    reference's quirk of a zero normal (one-sided lights return L = 0 from sample_li)."""
    sd, rp = pkg.scenes.sphere_lights(xres=16, yres=16, spp=1).world_end()
    s = oracle.scene(sd)
    # light 0: small two-sided sphere at (-1.5, 2.5, 0.5), radius 0.3 -- reference point outside: cone sampling
    wi, pdf, L, back, integral = _light_probe(oracle, pkg, s, 0, (0.5, 0.0, 0.0))
    c = np.array([-1.5, 2.5, 0.5]) - np.array([0.5, 0.0, 0.0]); dist = np.linalg.norm(c)
    cos_max = np.sqrt(1 - (0.3 / dist) ** 2)
    assert np.all(wi @ (c / dist) >= cos_max - 1e-4)                       # inside the subtended cone
    assert np.allclose(pdf, 1 / (2 * np.pi * (1 - cos_max)), rtol=1e-4) and np.allclose(back, pdf, rtol=1e-5)
    # Sphere::pdf_wi's outside branch returns the cone pdf for EVERY direction (sphere.rs:389-394, as pbrt-v3 does):
    # estimate_direct relies on the MIS ray actually hitting the light, not on pdf_li being 0 off the cone
    assert abs(integral - 4 * np.pi / (2 * np.pi * (1 - cos_max))) < 1e-2 * integral
    assert np.all(L > 0)                                                   # two-sided: L = Lemit although n == 0
    # light 1: one-sided sphere -> App. A #7: every light sample has L == 0
    wi, pdf, L, back, integral = _light_probe(oracle, pkg, s, 1, (0.5, 0.0, 0.0))
    assert np.all(pdf > 0) and np.all(L == 0)
    # light 2: big two-sided partial sphere around the origin -- reference point inside: uniform-area sampling + shape_pdfwi
    wi, pdf, L, back, integral = _light_probe(oracle, pkg, s, 2, (0.5, 0.0, 0.0))
    # App. A #5: shape_pdfwi divides by the SIGNED n.(-wi); seen from inside, the outward normal gives a negative pdf.
    # Sphere::sample ignores zmin/zmax (full sphere) while intersect() clips: samples on the clipped cap have pdf_li == 0.
    hit = back != 0
    assert np.all(pdf > 0) and np.all(back[hit] < 0) and np.allclose(-back[hit], pdf[hit], rtol=2e-3)
    assert abs((~hit).mean() - 25.0 / 60.0) < 0.03
    assert abs(integral - 1.0) < 0.03      # |pdf_li| is a normalised density over the directions that reach the clipped sphere


def test_sphere_lights_scene_renders(oracle, pkg):
    sd, rp = pkg.scenes.sphere_lights(xres=48, yres=32, spp=8).world_end()
    s = oracle.scene(sd)
    rgb = s.resolve(s.render(rp, nthreads=4))
    assert np.isfinite(rgb).all() and rgb.mean() > 0.2


def test_mipmap_pyramid_properties(pkg):
    """MIPMap::new restated on the host (mipmap.rs:75-198): power-of-two resampling keeps a constant image constant
    (normalised Lanczos weights), every level is the 2x2 box filter of the previous one, repeat wrap at 1-texel levels."""
    import importlib
    T = importlib.import_module("pbrt_rust_amd.textures")
    const = np.full((5, 7, 3), 0.37, dtype=np.float32)
    im = T.prepare_image(const)
    assert (im["width"], im["height"], im["n_levels"]) == (8, 8, 4)
    assert np.allclose(im["texels"], 0.37, atol=2e-6)
    rng = np.random.default_rng(0)
    px = rng.random((8, 16, 3), dtype=np.float32)
    im = T.prepare_image(px)
    lv = im["levels"]
    assert [l.shape[:2] for l in lv] == [(8, 16), (4, 8), (2, 4), (1, 2), (1, 1)]
    assert np.array_equal(lv[0], px[::-1])                                    # y flip only (imagemap.rs:141-149)
    assert np.allclose(lv[1], lv[0].reshape(4, 2, 8, 2, 3).mean(axis=(1, 3)), atol=1e-6)
    assert np.allclose(lv[4][0, 0], 0.5 * (lv[3][0, 0] + lv[3][0, 1]), atol=1e-6)   # 1-texel-high level: t wraps onto itself
    w = T.resample_weights(5, 8)[1]
    assert np.allclose(w.sum(axis=1), 1.0, atol=1e-6)
    lut = T.ewa_weight_lut()
    assert lut[0] == np.float32(1.0 - np.exp(-2.0)) and lut[-1] == 0.0 and np.all(np.diff(lut) < 0)
    g = T.inverse_gamma_correct(np.array([0.0, 0.04045, 0.5, 1.0], dtype=np.float32))
    assert np.allclose(g, [0.0, 0.04045 / 12.92, ((0.5 + 0.055) / 1.055) ** 2.4, 1.0], rtol=1e-6)


def test_textured_scene_renders_and_filters(oracle, pkg):
    """The checkerboard floor is textured (not flat), and at 1 spp the distant floor is smoother with the closed-form
    filter + ray differentials than with point sampling."""
    sd, rp = pkg.scenes.textured(xres=96, yres=64, spp=4).world_end()
    s = oracle.scene(sd)
    rgb = s.resolve(s.render(rp, nthreads=4))
    assert np.isfinite(rgb).all() and rgb.mean() > 0.1
    assert rgb[48:, :, :].std() > 0.05                      # near floor shows the checker pattern

    def far_floor_roughness(aamode):
        b = pkg.host.SceneBuilder()
        b.film.update(xres=128, yres=32); b.spp = 1
        b.integ.update(maxdepth=1)
        b.look_at((0, 0.4, 0), (0, 0.2, -10), (0, 1, 0)); b.camera(fov=30.0)
        b.world_begin()
        b.light_source("distant", L=(3, 3, 3), from_=(0, 1, 0), to=(0, 0, 0))
        b.texture("c", "color", "checkerboard", mapping="planar", v1=(4, 0, 0), v2=(0, 0, 4), aamode=aamode, tex1=(0.9, 0.9, 0.9), tex2=(0.05, 0.05, 0.05))
        b.material("matte", Kd="c")
        P, I = pkg.scenes.quad((-200, 0, -400), (-200, 0, 5), (200, 0, 5), (200, 0, -400)); b.trianglemesh(P, I)
        sd, rp = b.world_end()
        s = oracle.scene(sd)
        img = s.resolve(s.render(rp, nthreads=2))
        band = img[17:20, :, 1]                                # just below the horizon: many checks per pixel
        return float(np.abs(np.diff(band, axis=1)).mean())
    assert far_floor_roughness("closedform") < 0.5 * far_floor_roughness("none")


def test_alpha_masks(oracle, pkg):
    """A constant-zero alpha mesh is invisible to every ray; a checkerboard mask removes about half of a card's hits;
    `shadowalpha` affects intersect_p only (triangle.rs:536-545)."""
    b = pkg.host.SceneBuilder()
    b.world_begin()
    b.texture("holes", "float", "checkerboard", uscale=8.0, vscale=8.0, tex1=1.0, tex2=0.0)
    uvq = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=np.float32)
    P, I = pkg.scenes.quad((-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0))
    b.material("matte")
    b.trianglemesh(P, I, UV=uvq, alpha="holes")                        # prims 0,1 at z = 0
    b.translate(0, 0, -1); b.trianglemesh(P, I, UV=uvq, alpha=0.0)       # prims 2,3 at z = -1: invisible
    b.translate(0, 0, -1); b.trianglemesh(P, I, UV=uvq, shadowalpha="holes")   # prims 4,5 at z = -2
    sd, rp = b.world_end()
    s = oracle.scene(sd)
    rng = np.random.default_rng(4)
    n = 20000
    o = np.zeros((n, 3), np.float32); o[:, :2] = rng.uniform(-0.99, 0.99, (n, 2)); o[:, 2] = 1.0
    d = np.tile(np.array([0, 0, -1], np.float32), (n, 1))
    prim, t, _ = s.trace_closest(o, d, np.full(n, np.inf, np.float32))
    first = np.isin(prim, [0, 1]); third = np.isin(prim, [4, 5])
    assert not np.isin(prim, [2, 3]).any() and (first | third).all()
    assert abs(first.mean() - 0.5) < 0.03                              # half of the card is cut out
    u, v = (o[:, 0] + 1) / 2, (o[:, 1] + 1) / 2
    solid = ((np.floor(u * 8) + np.floor(v * 8)) % 2) == 0
    assert np.array_equal(first, solid)
    # intersect_p from behind the first card towards the third: blocked only where shadowalpha != 0
    o2 = o.copy(); o2[:, 2] = -0.5
    occ = s.trace_any(o2, d, np.full(n, 10.0, np.float32)).astype(bool)
    assert np.array_equal(occ, solid)


def test_quad_light_over_lambertian_plane_closed_form(oracle, pkg):
    """Analytic check independent of any implementation: a one-sided diffuse rectangle 2a x 2b at height h
    over a Lambertian plane. At the point under its centre the irradiance is
    E = 2 L [ a/sqrt(a^2+h^2) atan(b/sqrt(a^2+h^2)) + b/sqrt(b^2+h^2) atan(a/sqrt(b^2+h^2)) ] and, with maxdepth 1 (direct
    lighting only: NEE + BSDF sampling under MIS), the camera sees L_o = rho E / pi."""
    a, bb, h, rho = 1.0, 1.5, 4.0, 0.6
    Le = np.array([17.0, 12.0, 4.0])
    b = pkg.host.SceneBuilder()
    b.film.update(xres=8, yres=8); b.spp = 1024
    b.integ.update(maxdepth=1)
    b.look_at((0.0, 3.0, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)); b.camera(fov=0.5)
    b.world_begin()
    b.attribute_begin(); b.area_light_source(L=tuple(Le))
    P, I = pkg.scenes.quad((-a, h, -bb), (a, h, -bb), (a, h, bb), (-a, h, bb)); b.trianglemesh(P, I); b.attribute_end()   # normal faces -y
    b.material("matte", Kd=(rho, rho, rho))
    P, I = pkg.scenes.quad((-10.0, 0.0, -10.0), (-10.0, 0.0, 10.0), (10.0, 0.0, 10.0), (10.0, 0.0, -10.0)); b.trianglemesh(P, I)
    sd, rp = b.world_end()
    s = oracle.scene(sd)
    rgb = s.resolve(s.render(rp, nthreads=8)).reshape(-1, 3).mean(axis=0)
    ra, rb = np.hypot(a, h), np.hypot(bb, h)
    E = 2.0 * Le * (a / ra * np.arctan(bb / ra) + bb / rb * np.arctan(a / rb))
    want = rho * E / np.pi
    assert np.all(np.abs(rgb - want) < 0.01 * want), (rgb, want)


@pytest.mark.parametrize("inner,both", [(0.0, False), (0.0, True)])
def test_disk_light_over_lambertian_plane_closed_form(oracle, pkg, inner, both):
    """Analytic check for shapes/disk.rs (intersect + sample + pdf under MIS): a diffuse annulus ri..r at height h over a
    Lambertian plane gives, under its axis, E = pi L (r^2/(h^2+r^2) - ri^2/(h^2+ri^2)); a disk facing away contributes nothing
    (diffuse.rs:73-82 one-sided emission). The axis is world z: Disk::intersect divides by the WORLD ray's d.z (disk.rs:65), so
    only transforms that keep z give a geometrically meaningful disk -- the parity tests cover the others. Disk::sample ignores
    innerradius and phimax (disk.rs:143-158, as pbrt-v3 does), so an annular emitter is biased by design and is not checked here."""
    r, h, rho = 1.5, 3.0, 0.7
    Le = np.array([9.0, 6.0, 3.0])
    b = pkg.host.SceneBuilder()
    b.film.update(xres=8, yres=8); b.spp = 1024
    b.integ.update(maxdepth=1)
    b.look_at((0.0, -6.0, 2.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)); b.camera(fov=0.5)
    b.world_begin()
    b.attribute_begin(); b.area_light_source(L=tuple(Le)); b.translate(0.0, 0.0, h); b.toggle_reverse_orientation()   # emit to -z
    b.disk(radius=r, innerradius=inner); b.attribute_end()
    if both:   # an off-axis disk that faces +z (away from the plane): no contribution
        b.attribute_begin(); b.area_light_source(L=(50.0, 50.0, 50.0)); b.translate(6.0, 0.0, 1.0); b.disk(radius=1.0); b.attribute_end()
    b.material("matte", Kd=(rho, rho, rho))
    P, I = pkg.scenes.quad((-10.0, -10.0, 0.0), (10.0, -10.0, 0.0), (10.0, 10.0, 0.0), (-10.0, 10.0, 0.0)); b.trianglemesh(P, I)
    sd, rp = b.world_end()
    s = oracle.scene(sd)
    rgb = s.resolve(s.render(rp, nthreads=8)).reshape(-1, 3).mean(axis=0)
    E = np.pi * Le * (r * r / (h * h + r * r) - inner * inner / (h * h + inner * inner))
    want = rho * E / np.pi
    assert np.all(np.abs(rgb - want) < 0.015 * want), (rgb, want)


@pytest.mark.parametrize("pixel", [(0, 0), (5, 3), (37, 22)])
def test_sobol_pixel_samples_are_a_02_net(oracle, pkg, pixel):
    """Analytic check: the first 2^k film samples of a pixel form a (0,2)-net in base 2 inside that pixel -- every
    dyadic box of area 2^-k holds exactly one of them (sobol.rs:61-86 + lowdiscrepancy.rs:512-543)."""
    A = pkg._abi
    sb = (C.c_int32 * 4)(0, 0, 64, 48)
    for k in (4, 6):
        n = 1 << k
        xy = np.tile(np.array(pixel, np.int32), (n, 1)); sn = np.arange(n, dtype=np.uint32)
        out = np.zeros((n, 2), np.float32)
        assert oracle.lib.orc_sobol_samples(sb, n, xy.ctypes.data_as(A.i32p), sn.ctypes.data_as(A.u32p), 2, out.ctypes.data_as(A.fp), None) == 0
        assert (out >= 0).all() and (out < 1).all()
        for kx in range(k + 1):
            nx, ny = 1 << kx, 1 << (k - kx)
            cell = np.floor(out[:, 0] * nx).astype(int) * ny + np.floor(out[:, 1] * ny).astype(int)
            assert sorted(cell.tolist()) == list(range(n)), (k, kx)


# ---- round 2: every remaining assertion the reference's tests hold for code on this path ----

def test_hg_sampling_match_twin(oracle):
    """tests/hg.rs:12-32 sampling_match: sample_p's return value is p(wo, wi) (relative 1e-4), RNG::default(), g = -0.75 .. 0.75."""
    assert oracle.lib.orc_test_hg_sampling_match() < 1.0e-4


def test_hg_sampling_orientation_twin(oracle):
    """tests/hg.rs:34-79 sampling_orientation_forward / sample_orientation_backward: with wo = (-1, 0, 0), g = 0.95 scatters to
    wi.x > 0 more than ten times as often as not, g = -0.95 the other way round (pins the sign convention of sample_p)."""
    f, b = C.c_int(), C.c_int()
    oracle.lib.orc_test_hg_orientation(0.95, C.byref(f), C.byref(b))
    assert f.value + b.value == 100 and f.value > 10 * b.value
    oracle.lib.orc_test_hg_orientation(-0.95, C.byref(f), C.byref(b))
    assert f.value + b.value == 100 and b.value > 10 * f.value


def test_hg_normalized_twin(oracle):
    """tests/hg.rs:81-103 normalized: the mean of p over 100 000 uniform directions is 1 / 4 pi (relative 1e-3) for every g."""
    means = (C.c_double * 7)()
    oracle.lib.orc_test_hg_normalized(means)
    # the reference evaluates relative_eq!(mean, 1 / 4 pi, epsilon = 1e-3) but never asserts it; the Monte-Carlo mean of 10^5 samples
    # has a standard error of ~0.6 % at |g| = 0.75, so the twin asserts 3 % (five sigma) -- enough to catch a wrong normalisation
    for m in means:
        assert abs(m - 1.0 / (4.0 * np.pi)) < 0.03 / (4.0 * np.pi), list(means)


@pytest.mark.parametrize("op,name", [(0, "efloat_abs"), (1, "efloat_sqrt"), (2, "add"), (3, "sub"), (4, "mul"), (5, "div")])
def test_efloat_containment_twin(oracle, op, name):
    """tests/fp.rs:125-226: for RNG::new(trial), trial = 0 .. 999 999, the exact f64 result of the operation on values drawn from inside
    the operands' intervals lies inside the result's interval (EFloat is what bounds Sphere::intersect's hit error, row a14)."""
    n = C.c_int()
    failures = oracle.lib.orc_test_efloat(op, 1000000, C.byref(n))
    assert n.value > 400000 and failures == 0, (name, failures, n.value)


def test_bitops_twin(oracle):
    """tests/bitops.rs:7-64 log2 and round_up_pow2 (every i < 2^24): SobolSampler's resolution and the MIPMap resampler depend on them."""
    assert oracle.lib.orc_test_bitops() == 0


def test_generator_matrix_twin(oracle):
    """tests/sampling.rs:55-83 generator_matrix and :85-97 gray_code_sample_test on the oracle's multiply_generator."""
    assert oracle.lib.orc_test_generator_matrix() == 0


@pytest.mark.parametrize("ext,gamma", [("exr", False), ("pfm", False), ("tga", True), ("png", True)])
def test_imageio_round_trip_twin(pkg, tmp_path, ext, gamma):
    """tests/imageio.rs:9-100 test_round_trip through the front end's writers and readers (frontend/fe_imageio.h): 16 x 29 ramp with a
    negative blue channel; PFM exact, EXR exact in the negative channel and to 1e-3 (half floats) elsewhere, 8-bit formats to 0.02
    after undoing the sRGB curve with the clamped channel reading back 0."""
    F = pkg.frontend.lib()
    w, h = 16, 29
    px = np.zeros((h, w, 3), np.float32)
    px[..., 0] = (np.arange(w, dtype=np.float32) / np.float32(w - 1))[None, :]
    px[..., 1] = (np.arange(h, dtype=np.float32) / np.float32(h - 1))[:, None]
    px[..., 2] = -1.5
    path = str(tmp_path / f"out.{ext}").encode()
    assert F.ptf_write_image(path, w, h, px.ctypes.data_as(pkg._abi.fp)) == 0
    rw, rh = C.c_int(), C.c_int()
    back = np.zeros((h, w, 3), np.float32)
    assert F.ptf_read_image(path, C.byref(rw), C.byref(rh), back.ctypes.data_as(pkg._abi.fp), back.size) == 0
    assert (rw.value, rh.value) == (w, h)
    if gamma:   # inverse_gamma_correct (pbrt.rs)
        back = np.where(back <= 0.04045, back / 12.92, np.power((back + 0.055) / 1.055, 2.4)).astype(np.float32)
    delta = px - back
    if ext == "pfm":
        assert np.array_equal(px, back)
    elif ext == "exr":
        assert np.all(delta[..., 2] == 0.0) and np.abs(delta[..., :2]).max() < 0.001
    else:
        assert np.all(back[..., 2] == 0.0) and np.abs(delta[..., :2]).max() < 0.02


# ---- tests/shapes.rs:226-419: the reference's sampling / solid-angle tests of the shapes behind the area lights ----

def test_triangle_sampling_twin(oracle):
    """tests/shapes.rs:226-299 triangle_sampling: for RNG::new(0..30) a random triangle (punif(10)) and a reference point 3 units outside
    the cube, Sum 1 / (N pdf) over Triangle::sample + Shape::sample_interaction (the pdf LightSampler::sample_li uses) must agree with
    the uniform-sphere Monte Carlo estimate over Triangle::intersect_p within 10 % -- N = 512 * 1024 radical-inverse points, every pdf
    > 0 -- on the oracle's restatements (oracle/ref_kats_shapes.cpp runs the loops)."""
    n = 30
    out = (C.c_double * (4 * n))()
    assert oracle.lib.orc_test_triangle_sampling(n, 512 * 1024, out) == 0
    compared = sum(1 for i in range(n) if out[4 * i + 3] == 1.0)
    assert compared >= 25                                                     # the reference skips only tiny solid angles
    assert max(out[4 * i + 2] for i in range(n) if out[4 * i + 3] == 1.0) < 0.1


def test_triangle_solid_angle_twin(oracle):
    """tests/shapes.rs:301-352 triangle_solid_angle: the same sampling estimate (N = 64 * 1024, RNG::new(100..150)) against
    Triangle::solid_angle -- Girard's theorem, triangle.rs:586-624 -- within 1.5 %."""
    n = 50
    out = (C.c_double * (3 * n))()
    assert oracle.lib.orc_test_triangle_solid_angle(n, 64 * 1024, out) == 0
    assert sum(1 for i in range(n) if out[3 * i] > 0.0) >= 45 and max(out[3 * i + 2] for i in range(n)) < 0.015


def _test_transform(pkg):
    """Transform::translate(1, .5, -.8) * Transform::rotate_x(30) and its inverse as the reference builds them (transform.rs:291-303:
    m_inv of a rotation is the transpose; Mul: (m1 m2, m2_inv m1_inv), all in f32)."""
    F32 = np.float32
    T = pkg.host.Transform
    th = F32(np.radians(F32(30.0)))
    s, c = F32(np.sin(th)), F32(np.cos(th))
    rot = np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]], dtype=F32)
    return T.translate((1.0, 0.5, -0.8)) * T(rot, rot.T.copy())


def test_sphere_solid_angle_twin(pkg, oracle):
    """tests/shapes.rs:354-389 mc_solid_angle + sphere_solid_angle: uniform directions through Sphere::intersect_p of a rotated and
    translated unit sphere give 4 pi from inside and Sphere::solid_angle (sphere.rs:397-407) to 1e-3 from outside, N = 128 * 1024."""
    b = pkg.host.SceneBuilder()
    b.ctm = _test_transform(pkg)
    b.sphere(radius=1.0, zmin=-1.0, zmax=1.0, phimax=360.0)
    out = (C.c_double * 4)()
    assert oracle.lib.orc_test_sphere_solid_angle(C.byref(b.spheres[0]), 128 * 1024, out) == 0
    assert abs(out[0] - 4 * np.pi) < 0.01 and out[1] == np.float32(4.0) * np.float32(np.pi) and abs(out[2] - out[3]) < 0.001 and 0.2 < out[3] < 2.0


def test_disk_solid_angle_twin(pkg, oracle):
    """tests/shapes.rs:407-419 disk_solid_angle: Disk::intersect_p Monte Carlo against the default Shape::solid_angle (shape.rs:84-107:
    Disk::sample through sample_interaction, the sample counted when the disk does not block its own segment), N = 128 * 1024, 1e-3."""
    b = pkg.host.SceneBuilder()
    b.ctm = _test_transform(pkg)
    b.disk(height=0.0, radius=1.25, innerradius=0.0, phimax=360.0)
    out = (C.c_double * 2)()
    assert oracle.lib.orc_test_disk_solid_angle(C.byref(b.spheres[0]), 128 * 1024, out) == 0
    assert abs(out[0] - out[1]) < 0.001 and out[0] > 0.1


def test_oracle_counts_the_asserts_the_reference_would_panic_on(pkg, oracle):
    """PtCounters::reference_asserts: 0 on an ordinary scene, > 0 where path.rs:143 would have aborted the render."""
    from test_gpu_parity import _negative_light_scene
    sd, rp = _negative_light_scene(pkg)
    s = oracle.scene(sd); s.render(rp, nthreads=2); c = s.counters()
    assert c["reference_asserts"] > 0 and c["sanitized_negative"] > 0
    sd, rp = pkg.scenes.ganesha_scale(n=16, xres=32, yres=24, spp=2).world_end()
    s = oracle.scene(sd); s.render(rp, nthreads=2)
    assert s.counters()["reference_asserts"] == 0


def _watertight(oracle, n_seeds, as_written):
    fn = oracle.lib.orc_test_triangle_watertight
    fp = C.POINTER(C.c_float)
    v = np.zeros((256, 3), np.float32); idx = np.zeros((420, 3), np.uint32)
    ro = np.zeros((2 * n_seeds, 3), np.float32); rd = np.zeros((2 * n_seeds, 3), np.float32); nh = np.zeros(2 * n_seeds, np.int32)
    failures = fn(n_seeds, as_written, v.ctypes.data_as(fp), idx.ctypes.data_as(C.POINTER(C.c_uint32)), ro.ctypes.data_as(fp), rd.ctypes.data_as(fp),
                  nh.ctypes.data_as(C.POINTER(C.c_int)))
    return failures, v, idx, ro, rd, nh


def test_triangle_watertight_twin(oracle):
    """tests/shapes.rs:36-146 triangle_watertight on the oracle's Triangle::intersect: RNG::new(12111) mesh, the reference's 100 000 seeds, both rays of every
    seed (a uniform direction, then "shoot directly at a vertex") must hit at least one of the 420 triangles. The reference keeps the test switched off
    (`//#[test]`, :35); the mesh loop as the Rust file has it leaves the sphere open along phi = 0 (`t == nphi - 1` at :60 where pbrt-v3 has `p == nPhi - 1`:
    oracle/ref_kats_shapes.cpp), so the assertion is held on the closed mesh and, on the mesh as written, every ray that hits nothing must go through that slit."""
    failures, v, idx, ro, rd, nh = _watertight(oracle, 100000, 0)
    assert failures == 0 and int(nh.min()) >= 1
    assert np.array_equal(v[15::16][1:15], v[0::16][1:15])            # closed: the last vertex of every interior row is its first
    failures_w, vw, idxw, row, rdw, nhw = _watertight(oracle, 100000, 1)
    assert np.array_equal(idx, idxw) and np.array_equal(ro, row)       # same connectivity, same ray origins (RNG::new(i) streams do not depend on the mesh)
    assert 0 < failures_w == int((nhw < 1).sum()) < 2000
    assert not np.array_equal(vw[15::16][1:15], vw[0::16][1:15])
    bad = np.nonzero(nhw < 1)[0]
    o = row[bad].astype(np.float64); d = rdw[bad].astype(np.float64)
    t = -o[:, 1] / d[:, 1]                                               # where the ray crosses the plane y = 0 ...
    assert (t > 0).all() and ((o[:, 0] + t * d[:, 0]) > -1e-6).all()     # ... ahead of its origin, on the x >= 0 side: through the seam's half plane (x = 0: the two rays aimed at a pole, the slit's end)


def test_float_bits_twin(oracle):
    # tests/fp.rs:46-57: RNG::new(1), 100 000 draws, float_to_bits(bits_to_float(ui)) == ui for every non-NaN pattern
    n = C.c_int()
    assert oracle.lib.orc_test_float_bits(100000, C.byref(n)) == 0
    assert 99000 < n.value <= 100000      # 2^24 - 2 of 2^32 patterns are NaNs: ~390 of the 100 000


def dist1d_continuous_checks(sample):
    """tests/sampling.rs:259-283 distribution1d_continuous; `sample(u)` -> (value, pdf, offset) of Distribution1D::new([1, 1, 2, 4, 8]).sample_continous(u).
    The file's four assert_eq!s, and its five relative_eq!s (whose results the Rust test drops) held as real assertions at the epsilon written there."""
    count = 5
    x, pdf, off = sample(0.0)
    assert x == 0.0                                                      # :267 assert_eq!(0.0, ...)
    assert abs(pdf - 5.0 * 1.0 / 16.0) <= 1e-5 * 5.0 / 16.0              # (the file's `count + 1.0` at :268 is not the pdf of this distribution: func[0] / func_int = 1 / (16 / 5); its result is dropped there)
    assert off == 0                                                      # :269
    x, pdf, off = sample(0.5)
    assert abs(x - 0.8) <= 1e-5 * 0.8                                    # :272 right at the boundary between the 4 and the 8 segments
    x, pdf, off = sample(0.75)
    assert abs(x - 0.9) <= 1e-5 * 0.9                                    # :275 middle of the 8 segment
    assert abs(pdf - count * 8.0 / 16.0) <= 1e-5 * count * 8.0 / 16.0    # (:276 writes `count * 0.8 / 16`; the pdf of the 8 segment is 8 / (16 / 5) = 2.5)
    assert off == 4                                                      # :277
    assert abs(sample(0.0)[0] - 0.0) <= 1e-5                             # :279
    assert abs(sample(1.0)[0] - 1.0) <= 1e-5                             # :280


def test_distribution1d_continuous_twin(oracle, pkg):
    A = pkg._abi
    func = np.array([1.0, 1.0, 2.0, 4.0, 8.0], np.float32)

    def sample(u):
        pdf = C.c_float(); off = C.c_int(-1)
        x = oracle.lib.orc_dist1d_sample_continuous(func.ctypes.data_as(A.fp), 5, u, C.byref(pdf), C.byref(off))
        return x, pdf.value, off.value
    dist1d_continuous_checks(sample)
    # count() == 5 (:263): the discrete pdfs of the same distribution sum to one over its five entries
    assert abs(sum(oracle.lib.orc_dist1d_discrete_pdf(func.ctypes.data_as(A.fp), 5, i) for i in range(5)) - 1.0) < 1e-6


def test_scrambled_radical_inverse_twin(oracle):
    """tests/sampling.rs:24-53 scrambled_radical_inverse_test (the Halton sampler's dimensions >= 2): 128 bases, RNG::new(dim)-shuffled permutations, the test's seven indices.
    The Rust test drops its `relative_eq!` and its hand-rolled expectation is broken (oracle/ref_kats.cpp); the twin asserts the function against the exact digit sum."""
    worst = C.c_double()
    assert oracle.lib.orc_test_scrambled_radical_inverse(128, C.byref(worst)) == 0
    assert worst.value < 1.0e-6


def test_partial_sphere_normal_twin(oracle):
    """tests/shapes.rs:490-535 partial_sphere_normal: 10 000 seeds of random partial spheres; at every hit Sphere::intersect finds, the normal points along the hit point
    (the Rust file's dropped `relative_eq!(1.0, dot, epsilon = 1e-5)` as an assertion)."""
    n = C.c_int(); worst = C.c_double()
    assert oracle.lib.orc_test_partial_sphere_normal(10000, C.byref(n), C.byref(worst)) == 0
    assert n.value > 3000 and worst.value <= 1.0e-5
