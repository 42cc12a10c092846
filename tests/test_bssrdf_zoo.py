"""The oracle's BSSRDF (oracle/ref_bssrdf.h through orc_bssrdf_eval) against float64 models, on the queries of tests/bssrdf_zoo.py -- no GPU.

tests/test_bssrdf_probe.py holds the device equal to the oracle bit for bit, and the two share their arithmetic nearly line for line: what they share is held here against
something that does not -- closed forms, quadrature, geometry and an independent spline, in numpy float64.

Every tolerance is 4 x the worst deviation the oracle alone shows on these queries (the margin of interaction_zoo.py: room for float32 rounding on other inputs of the
same family); the measured value stands beside each bound and every test prints what it measures. The live shares of the random queries have floors
(bssrdf_zoo.FLOORS / FLOOR_EXCEPTIONS): a comparison must compare something."""
import numpy as np
import pytest
from bssrdf_zoo import (ADAPTER_FLAGS, BSDF_DIFFUSE, BSDF_REFLECTION, DEVICE_REFUSES, F, FLOOR_EXCEPTIONS, FLOORS, FRAMES, MATERIALS, N_RANDOM, NO_BSSRDF, ORTHONORMAL_FRAMES,
                        U_TOP, case, check_floors, field, frame_axes, oracle_eval)

WITH_BSSRDF = [n for n in MATERIALS if n not in NO_BSSRDF]
DISNEY = [n for n in WITH_BSSRDF if MATERIALS[n][0] == "disney"]
TABULATED = [n for n in WITH_BSSRDF if MATERIALS[n][0] != "disney"]

# ---- tolerances: 4 x the measured worst deviation of the oracle alone (the measured value in the comment) -----------------------------------------------------
DISNEY_CDF_TOL = 4 * 8.54e-8        # |1 - exp(-r / d') - u'| for the exponential sample_sr picked (d' = d or 3 d) and its remapped u': measured 8.538e-08 (all three Disney materials)
DISNEY_MIXTURE_TOL = 4 * 1.24e-5    # |share of 65536 stratified u with sample_sr(u) <= R  -  (1 - e^{-R/d} / 4 - 3 e^{-R/3d} / 4)|: measured 1.238e-05 (2 / 65536 = 3.1e-05 is what counting allows)
DISNEY_NORM_TOL = 4 * 3.44e-6       # |midpoint rule of pdf_sr 2 pi r over (0, 90 d], h = d / 64, minus 1|: measured 3.432e-06 (disney_scatter; 3.400e-06 disney_d_zero)
DISNEY_SR_TOL = 4 * 3.22e-6         # relative deviation of sr from R (e^{-r/d} + e^{-r/3d}) / (8 pi d r): measured 3.211e-06 (disney_weighted; 2.418e-06 disney_scatter, 1.503e-06 disney_d_zero)
# probe_segment, deviations over rmax of the query's channel, worst over the materials -- frame: (norms, dist, built, along) as segment_deviations returns them.
# `built` and `along` carry the float32 rounding of rmax^2 - r^2 where r is close to rmax; the far frame's carry the spacing of floats at 1e4 (9.8e-4) over rmax.
SEGMENT_MEASURED = {"canonical": dict(norms=9.983e-08, dist=7.012e-08, built=8.207e-06, along=1.641e-05),
                    "tilted": dict(built=8.232e-06, along=1.642e-05),
                    "far": dict(norms=8.504e-04, dist=6.815e-04, built=9.780e-04, along=4.915e-04)}
SEGMENT_TOL = {f: {k: 4 * v for k, v in m.items()} for f, m in SEGMENT_MEASURED.items()}
# pdf_sp, relative deviation from the float64 sum, worst over the materials: canonical 8.202e-07 (kd_textured), tilted 2.562e-06 (disney_scatter), far 8.623e-07 (ss_negative)
PDF_SP_MEASURED = {"canonical": 8.21e-7, "tilted": 2.57e-6, "far": 8.63e-7}
PDF_SP_TOL = {f: 4 * v for f, v in PDF_SP_MEASURED.items()}
CONVERSION_KD_TOL = 4 * 1.87e-5     # |float64 spline of rhoeff at the returned rho - kd|: measured 1.861e-05 (ss_scaled_eta_1.5; 1.547e-05 ss_g_0.4, 8.315e-06 the eta 1.33 table, 1.838e-06 eta 1.0)
CONVERSION_SUM_TOL = 4 * 7.89e-8    # relative deviation of sigma_a + sigma_s from 1 / mfp: measured 7.888e-08
ADAPTER_F_TOL = 4 * 1.05e-5         # relative deviation of f and the sampled f from sw eta^2: measured 1.042e-05 (ss_eta_0.8, tilted; 9.331e-06 in the other frames)
ADAPTER_PDF_TOL = 4 * 1.14e-5       # relative deviation of pdf and the sampled pdf from |cos| / pi: measured 1.139e-05 (a sample at z = 0.05: 5e-8 / z^2)
ADAPTER_WI_TOL = 4 * 6.87e-7        # |sampled wi - the float64 cosine-hemisphere sample of the clamped u, carried to the world|: measured 6.863e-07


def _rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


# ---- floors ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MATERIALS))
def test_the_zoo_compares_something(pkg, oracle, name):
    c = case(pkg, oracle, name)
    assert c["has"] == (name not in NO_BSSRDF), name   # status 2 exactly for the materials whose diffuse weight is 0 or that are thin
    if not c["has"]: return
    shares = check_floors(name, c)
    fl = FLOOR_EXCEPTIONS.get(name, FLOORS)
    for fname, sh in shares.items():
        fc = c["frames"][fname]
        sizes = ", ".join(f"{k} {len(v['q'])} ({v['random']} random, {len(v['q']) - v['random']} structured)" for k, v in fc["sets"].items())
        print(f"\n{name} {fname}: {sizes}; live shares " + ", ".join(f"{k} {v:.3f} (floor {fl[k]})" for k, v in sh.items()))
    for k, v in c["frames"]["canonical"]["sets"].items():
        assert v["random"] == N_RANDOM and len(v["q"]) > N_RANDOM and (v["tag"][:N_RANDOM] == "random").all() and (v["tag"][N_RANDOM:] != "random").all(), k


# ---- DisneyBSSRDF: the analytic profile ------------------------------------------------------------------------------------------------------------------
def disney_profile_deviations(oracle, c):
    """(branch CDF, mixture CDF, normalisation, sr) worst deviations of one Disney material; channels with d = 0 are left to the bit comparison alone."""
    fc = c["frames"]["canonical"]
    d = fc["state"]["sigma_t"].astype(np.float64); R = fc["state"]["rho"].astype(np.float64)
    live = [k for k in range(3) if d[k] > 0]
    u = fc["sets"]["samples"]["q"][:, 0].astype(np.float64); r = field(fc["ref"]["samples"], "samples", "r").astype(np.float64)
    # sample_sr picks ONE of the two exponentials by u (disney.rs:673-681) and inverts that one's CDF at the remapped u
    first = u < 0.25
    up = np.minimum(np.where(first, u * 4.0, (u - 0.25) / 0.75), U_TOP)
    cdf = max(float(np.abs(1.0 - np.exp(-r[:, k] / np.where(first, d[k], 3.0 * d[k])) - up).max()) for k in live)
    # ... so that the share of u with sample_sr(u) <= R is the mixture's CDF 1 - e^{-R/d} / 4 - 3 e^{-R/3d} / 4: counted over a stratified u
    n = 65536
    grid = ((np.arange(n) + 0.5) / n).astype(F)
    s = oracle.scene(c["sd"])
    try:
        rg = field(oracle_eval(oracle, s, c["mi"], fc["frames"], samples=grid)["samples"], "samples", "r").astype(np.float64)
        mix = norm = 0.0
        for k in live:
            for m in (0.1, 0.5, 1.0, 2.0, 5.0, 10.0):
                want = 1.0 - 0.25 * np.exp(-m) - 0.75 * np.exp(-m / 3.0)
                mix = max(mix, abs(float((rg[:, k] <= m * d[k]).mean()) - want))
        # pdf_sr 2 pi r integrates to 1: the midpoint rule on (0, 90 d], h = d / 64 (the tail beyond is 0.75 e^-30)
        h = 1.0 / 64.0
        t = (np.arange(int(90 / h)) + 0.5) * h
        for k in live:
            rr = (t * d[k]).astype(F)
            pdf = field(oracle_eval(oracle, s, c["mi"], fc["frames"], radii=rr)["radii"], "radii", "pdf_sr")[:, k].astype(np.float64)
            norm = max(norm, abs(float(np.sum(pdf * 2.0 * np.pi * rr.astype(np.float64)) * h * d[k]) - 1.0))
    finally:
        s.close()
    rq = fc["sets"]["radii"]["q"][:, 0].astype(np.float64); sr = field(fc["ref"]["radii"], "radii", "sr").astype(np.float64)
    rc = np.maximum(rq, float(F(1e-6)))
    worst_sr = 0.0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        for k in live:
            closed = R[k] * (np.exp(-rc / d[k]) + np.exp(-rc / (3.0 * d[k]))) / (8.0 * np.pi * d[k] * rc)
            big = np.isfinite(closed) & (closed > 1e-30)
            assert np.all(sr[~big & np.isfinite(rc), k] <= 1e-29) and np.all(sr[np.isinf(rc), k] == 0)
            worst_sr = max(worst_sr, float(_rel(sr[big, k], closed[big]).max()))
    return cdf, mix, norm, worst_sr


@pytest.mark.parametrize("name", DISNEY)
def test_disney_profile_is_the_analytic_one(pkg, oracle, name):
    cdf, mix, norm, sr = disney_profile_deviations(oracle, case(pkg, oracle, name))
    print(f"\n{name}: branch CDF {cdf:.3e} (bound {DISNEY_CDF_TOL:.1e}), mixture CDF {mix:.3e} (bound {DISNEY_MIXTURE_TOL:.1e}), normalisation {norm:.3e} "
          f"(bound {DISNEY_NORM_TOL:.1e}), sr {sr:.3e} (bound {DISNEY_SR_TOL:.1e})")
    assert cdf <= DISNEY_CDF_TOL and mix <= DISNEY_MIXTURE_TOL and norm <= DISNEY_NORM_TOL and sr <= DISNEY_SR_TOL


# ---- probe_segment: geometry ----------------------------------------------------------------------------------------------------------------------------
def segment_deviations(oracle, c, fname):
    """Worst deviations of one frame's segments, relative to rmax of the query's channel: (|start - po| and |target - po| from rmax [orthonormal frames], the distance of start
    from the axis through po from r [orthonormal frames], start and target from the float64 construction, target - start from vz l); the number accepted."""
    fc = c["frames"][fname]
    q = fc["sets"]["segments"]["q"].astype(np.float64); ref = fc["ref"]["segments"]
    ok = ref[:, 0] != 0
    start, target, u1n = (field(ref, "segments", k).astype(np.float64) for k in ("start", "target", "u1n"))
    ss, ts, ns = frame_axes(fc["state"]); po = fc["state"]["po_p"].astype(np.float64)
    u1 = q[:, 0]
    axis = np.where(u1 < 0.5, 0, np.where(u1 < 0.75, 1, 2))                       # the axis follows u1's interval
    pre = np.where(axis == 0, u1 * 2.0, np.where(axis == 1, (u1 - 0.5) * 4.0, (u1 - 0.75) * 4.0))   # (exact in float32 as in float64)
    x3 = pre.astype(F) * F(3.0)                                                  # the channel follows the float32 product's integer part
    ch = np.clip(x3.astype(np.int64), 0, 2)
    assert np.all((u1n >= 0.0) & (u1n < 1.0)), f"u1n leaves [0, 1): {u1n[(u1n < 0) | (u1n >= 1)][:4]}"
    assert np.array_equal(u1n.astype(F), x3 - ch.astype(F))
    vx = np.array([ss, ts, ns])[axis]; vy = np.array([ts, ns, ss])[axis]; vz = np.array([ns, ss, ts])[axis]
    s = oracle.scene(c["sd"])
    try:
        r3 = field(oracle_eval(oracle, s, c["mi"], fc["frames"], samples=np.ascontiguousarray(q[:, 1], F))["samples"], "samples", "r").astype(np.float64)
        rmax3 = field(oracle_eval(oracle, s, c["mi"], fc["frames"], samples=np.array([0.999], F))["samples"], "samples", "r")[0].astype(np.float64)
    finally:
        s.close()
    r = r3[np.arange(len(q)), ch]; rmax = rmax3[ch]
    with np.errstate(invalid="ignore"):
        want_ok = ~(r < 0) & ~(r >= rmax)
    assert np.array_equal(ok, want_ok), f"accepted differs from r >= 0 and r < rmax at {np.flatnonzero(ok != want_ok)[:4]}"
    assert not start[~ok].any() and not target[~ok].any()
    if not ok.any(): return None, 0
    k = np.flatnonzero(ok & np.isfinite(r) & np.isfinite(rmax))
    r, rmax, vx, vy, vz, st, tg = r[k], rmax[k], vx[k], vy[k], vz[k], start[k], target[k]
    half = np.sqrt(np.maximum(rmax * rmax - r * r, 0.0)); phi = 2.0 * np.pi * q[k, 2]
    want_start = po + (vx * np.cos(phi)[:, None] + vy * np.sin(phi)[:, None]) * r[:, None] - vz * half[:, None]
    want_target = want_start + vz * (2.0 * half)[:, None]
    built = max(float((np.linalg.norm(st - want_start, axis=1) / rmax).max()), float((np.linalg.norm(tg - want_target, axis=1) / rmax).max()))
    d = tg - st; lvz = np.linalg.norm(vz, axis=1)
    along = float((np.linalg.norm(d - vz * (2.0 * half)[:, None], axis=1) / (rmax * lvz)).max())   # parallel to vz, length 2 sqrt(rmax^2 - r^2) |vz|
    norms = dist = None
    if fname in ORTHONORMAL_FRAMES:
        norms = max(float((np.abs(np.linalg.norm(st - po, axis=1) - rmax) / rmax).max()), float((np.abs(np.linalg.norm(tg - po, axis=1) - rmax) / rmax).max()))
        rel = st - po
        dist = float((np.abs(np.linalg.norm(rel - vz * np.sum(rel * vz, axis=1)[:, None], axis=1) - r) / rmax).max())
    return dict(norms=norms, dist=dist, built=built, along=along), int(ok.sum())


@pytest.mark.parametrize("name", WITH_BSSRDF)
def test_probe_segments_are_chords_of_the_rmax_sphere(pkg, oracle, name):
    c = case(pkg, oracle, name)
    for fname in FRAMES:
        dev, n_ok = segment_deviations(oracle, c, fname)
        if dev is None:
            assert name in FLOOR_EXCEPTIONS, name
            print(f"\n{name} {fname}: no segment accepted")
            continue
        print(f"\n{name} {fname}: {n_ok} accepted segments, deviations / rmax: " + ", ".join(f"{k} {v:.3e} (bound {SEGMENT_TOL[fname][k]:.1e})" for k, v in dev.items() if v is not None))
        for k, v in dev.items():
            assert v is None or v <= SEGMENT_TOL[fname][k], (name, fname, k, v)


# ---- pdf_sp: the float64 sum over 3 axes x 3 channels of the oracle's own pdf_sr ---------------------------------------------------------------------------------
def pdf_sp_deviation(oracle, name, c, fname):
    fc = c["frames"][fname]
    q = fc["sets"]["exits"]["q"].astype(np.float64); pdf = field(fc["ref"]["exits"], "exits", "pdf_sp").astype(np.float64)
    ss, ts, ns = frame_axes(fc["state"]); po = fc["state"]["po_p"].astype(np.float64)
    d = po - q[:, :3]; nrm = q[:, 3:]
    dl = np.stack([d @ ss, d @ ts, d @ ns], axis=1); nl = np.stack([nrm @ ss, nrm @ ts, nrm @ ns], axis=1)
    rproj = np.stack([np.hypot(dl[:, 1], dl[:, 2]), np.hypot(dl[:, 2], dl[:, 0]), np.hypot(dl[:, 0], dl[:, 1])], axis=1)
    axisprob = (0.25, 0.25, 0.5)
    want = np.zeros(len(q))
    s = oracle.scene(c["sd"])
    try:
        with np.errstate(invalid="ignore", over="ignore"):
            for a in range(3):
                p3 = field(oracle_eval(oracle, s, c["mi"], fc["frames"], radii=rproj[:, a].astype(F))["radii"], "radii", "pdf_sr").astype(np.float64)
                want += p3.sum(axis=1) * np.abs(nl[:, a]) * axisprob[a] / 3.0
    finally:
        s.close()
    # compared: the exit points a probe segment can reach (within rmax of po: beyond it the profile's tail is a spline through values near the smallest floats), but
    # for those whose projected radius is itself a rounding residue (pi displaced along one axis of a frame that is not the world's): it has no float64 counterpart
    dist = np.linalg.norm(d, axis=1)
    clear = np.isfinite(want) & np.isfinite(pdf) & (want > 0) & np.all(rproj >= 1e-3 * dist[:, None], axis=1) & (dist <= fc["rmax"])
    assert clear[:N_RANDOM].mean() >= 0.5 or name in FLOOR_EXCEPTIONS, (name, fname, clear[:N_RANDOM].mean())
    return (float(_rel(pdf[clear], want[clear]).max()) if clear.any() else None), int(clear.sum())


@pytest.mark.parametrize("name", WITH_BSSRDF)
def test_pdf_sp_is_the_sum_over_axes_and_channels(pkg, oracle, name):
    c = case(pkg, oracle, name)
    for fname in FRAMES:
        dev, n = pdf_sp_deviation(oracle, name, c, fname)
        print(f"\n{name} {fname}: {n} exit points with a clear non-zero pdf_sp, relative deviation " + ("-" if dev is None else f"{dev:.3e}") + f" (bound {PDF_SP_TOL[fname]:.1e})")
        assert dev is None or dev <= PDF_SP_TOL[fname], (name, fname, dev)


# ---- subsurface_from_diffuse -----------------------------------------------------------------------------------------------------------------------------
def spline64(x, y, t):
    """The Catmull-Rom spline through (x, y) at t (interpolation.rs:52-91 catmull_rom, in float64), t within [x[0], x[-1]]."""
    x = np.asarray(x, np.float64); y = np.asarray(y, np.float64); t = np.asarray(t, np.float64)
    i = np.clip(np.searchsorted(x, t, side="right") - 1, 0, len(x) - 2)
    x0, x1, f0, f1 = x[i], x[i + 1], y[i], y[i + 1]
    w = x1 - x0
    lo = np.maximum(i - 1, 0); hi = np.minimum(i + 2, len(x) - 1)
    d0 = np.where(i > 0, w * (f1 - y[lo]) / (x1 - x[lo]), f1 - f0)
    d1 = np.where(i + 2 < len(x), w * (y[hi] - f0) / np.where(i + 2 < len(x), x[hi] - x0, 1.0), f1 - f0)
    s = (t - x0) / w; s2 = s * s; s3 = s2 * s
    return (2 * s3 - 3 * s2 + 1) * f0 + (-2 * s3 + 3 * s2) * f1 + (s3 - 2 * s2 + s) * d0 + (s3 - s2) * d1


def conversion_deviations(c):
    fc = c["frames"]["canonical"]; t = c["table"]
    q = fc["sets"]["conversion"]["q"].astype(np.float64)
    sa = field(fc["ref"]["conversion"], "conversion", "sigma_a").astype(np.float64); ss = field(fc["ref"]["conversion"], "conversion", "sigma_s").astype(np.float64)
    kd, mfp = q[:, :3].ravel(), q[:, 3:].ravel(); sa, ss = sa.ravel(), ss.ravel()
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = np.isfinite(sa) & np.isfinite(ss) & (mfp > 0) & np.isfinite(1.0 / mfp) & ((sa + ss) > 0)
        inside = ok & (kd > float(t.rhoeff[0])) & (kd < float(t.rhoeff[-1]))
        rho = ss[inside] / (sa[inside] + ss[inside])
        back = float(np.abs(spline64(t.rho_samples, t.rhoeff, rho) - kd[inside]).max())
        total = float(_rel(sa[ok] + ss[ok], 1.0 / mfp[ok]).max())
    # outside the table's range the conversion clamps: rho = 0 below the first node's rhoeff, 1 at and above the last
    below = ok & ~(kd > float(t.rhoeff[0])); above = ok & ~(kd < float(t.rhoeff[-1]))
    assert np.all(ss[below] == 0.0) and np.all(sa[above] == 0.0)
    return back, total, int(inside.sum())


@pytest.mark.parametrize("name", TABULATED)
def test_subsurface_from_diffuse_inverts_the_rhoeff_spline(pkg, oracle, name):
    c = case(pkg, oracle, name)
    if not np.any(c["table"].rhoeff > 0):   # (eta < 1: the beam-diffusion table is all zero, nothing to invert)
        assert name in FLOOR_EXCEPTIONS, name
        return
    back, total, n = conversion_deviations(c)
    print(f"\n{name}: {n} conversions inside the table: |spline(rho) - kd| {back:.3e} (bound {CONVERSION_KD_TOL:.1e}), sigma_a + sigma_s vs 1 / mfp {total:.3e} (bound {CONVERSION_SUM_TOL:.1e})")
    assert n >= 3 * N_RANDOM // 2 and back <= CONVERSION_KD_TOL and total <= CONVERSION_SUM_TOL


@pytest.mark.parametrize("name", ["ss_skin1", "ss_g_0.4", "ss_eta_1.0"])
def test_host_conversion_is_the_oracles(pkg, oracle, name):
    """A constant Kd converts on the host (pbrt_rust_amd.bssrdf.subsurface_from_diffuse), a textured one on the device: both are the reference's one function, bit for bit.
    Every structured (kd, mfp) and the first 256 random ones."""
    from test_device_probe import bits
    c = case(pkg, oracle, name)
    fc = c["frames"]["canonical"]
    rows = np.concatenate([np.arange(256), np.arange(N_RANDOM, len(fc["sets"]["conversion"]["q"]))])
    q = fc["sets"]["conversion"]["q"][rows]; ref = fc["ref"]["conversion"][rows]
    host = np.zeros((len(q), 6), F)
    with np.errstate(all="ignore"):
        for k, row in enumerate(q):
            sa, ss = pkg.bssrdf.subsurface_from_diffuse(c["table"], row[:3], row[3:])
            host[k, :3] = sa; host[k, 3:] = ss
    want = np.concatenate([field(ref, "conversion", "sigma_a"), field(ref, "conversion", "sigma_s")], axis=1)
    bad = np.flatnonzero(np.any(bits(host) != bits(want), axis=1))
    print(f"\n{name}: {len(q)} (kd, mfp) triples compared, host vs oracle")
    assert len(bad) == 0, (f"{len(bad)} of {len(q)} conversions differ; first at {fc['sets']['conversion']['tag'][rows[bad[0]]]}: (kd, mfp) {q[bad[0]]}: host {host[bad[0]]} != oracle {want[bad[0]]}")


# ---- the adapter ------------------------------------------------------------------------------------------------------------------------------------------
def _fresnel_moment1(eta):
    e2, e3, e4, e5 = eta ** 2, eta ** 3, eta ** 4, eta ** 5
    if eta < 1.0: return 0.45966 - 1.73965 * eta + 3.37668 * e2 - 3.904945 * e3 + 2.49277 * e4 - 0.68441 * e5
    return -4.61686 + 11.1136 * eta - 10.4646 * e2 + 5.11455 * e3 - 1.27198 * e4 + 0.12746 * e5


def _fr_dielectric(cos_i, eta_i, eta_t):
    cos_i = np.clip(cos_i, -1.0, 1.0)
    ei = np.where(cos_i > 0, eta_i, eta_t); et = np.where(cos_i > 0, eta_t, eta_i)
    cos_i = np.abs(cos_i)
    sin_t = ei / et * np.sqrt(np.maximum(0.0, 1.0 - cos_i * cos_i))
    cos_t = np.sqrt(np.maximum(0.0, 1.0 - sin_t * sin_t))
    with np.errstate(invalid="ignore", divide="ignore"):
        rparl = (et * cos_i - ei * cos_t) / (et * cos_i + ei * cos_t); rperp = (ei * cos_i - et * cos_t) / (ei * cos_i + et * cos_t)
    return np.where(sin_t >= 1.0, 1.0, (rparl * rparl + rperp * rperp) / 2.0)


def _cosine_hemisphere(u):
    """sampling.rs cosine_sample_hemisphere over concentric_sample_disk, float64."""
    o = 2.0 * u - 1.0
    x, y = o[:, 0], o[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        wide = np.abs(x) > np.abs(y)
        r = np.where(wide, x, y)
        th = np.where(wide, (np.pi / 4.0) * (y / x), np.pi / 2.0 - (np.pi / 4.0) * (x / y))
    zero = (x == 0) & (y == 0)
    dx = np.where(zero, 0.0, r * np.cos(th)); dy = np.where(zero, 0.0, r * np.sin(th))
    return np.stack([dx, dy, np.sqrt(np.maximum(0.0, 1.0 - dx * dx - dy * dy))], axis=1)


def adapter_deviations(c, fname):
    fc = c["frames"][fname]
    a = fc["sets"]["adapter"]; ref = fc["ref"]["adapter"]
    fr = fc["frames"][15:].astype(np.float64)
    ng, ns, dpdu = fr[3:6], fr[6:9], fr[9:12]
    ss = dpdu / np.linalg.norm(dpdu); ts = np.cross(ns, ss)
    local = lambda v: np.stack([v @ ss, v @ ts, v @ ns], axis=1)
    eta = float(fc["state"]["eta"])
    q = a["q8"].astype(np.float64); wo, wi, u = q[:, :3], q[:, 3:6], q[:, 6:]
    match = (a["flags"] & (BSDF_REFLECTION | BSDF_DIFFUSE)) == (BSDF_REFLECTION | BSDF_DIFFUSE)
    f, pdf, s_wi, s_f, s_pdf = (field(ref, "adapter", k).astype(np.float64) for k in ("f", "pdf", "s_wi", "s_f", "s_pdf"))
    s_type = ref[:, 11].astype(np.int32)
    assert not f[~match].any() and not pdf[~match].any() and not s_f[~match].any() and not s_pdf[~match].any() and not s_type[~match].any()   # flags without the lobe: nothing
    wol, wil = local(wo), local(wi)
    scale = eta * eta / ((1.0 - 2.0 * _fresnel_moment1(1.0 / eta)) * np.pi)
    sw = lambda cos: (1.0 - _fr_dielectric(cos, 1.0, eta)) * scale
    go, gi = wo @ ng, wi @ ng
    clear = match & (np.abs(go) > 1e-5) & (np.abs(gi) > 1e-5) & (np.abs(wol[:, 2]) > 1e-5) & (np.abs(wil[:, 2]) > 1e-5)   # no sign decided by rounding
    same_side = go * gi > 0
    want_f = np.where(same_side, sw(wil[:, 2]), 0.0)
    assert np.all((f[clear, 0] == 0) == (want_f[clear] == 0)) and np.all(f[:, 0] == f[:, 1]) and np.all(f[:, 1] == f[:, 2])
    # (relative deviations away from grazing: below |cos| = 0.01 the float32 cos_t = sqrt(1 - sin_t^2) of fr_dielectric is a difference of nearly equal numbers;
    # the bit comparison of the GPU test covers those directions, and the zero / non-zero agreement above holds for them too)
    # ... and away from the critical angle of a direction below the surface, where cos_t is the same kind of difference
    critical = lambda cos: np.abs(1.0 - np.where(cos > 0, 1.0 / eta, eta) ** 2 * (1.0 - np.clip(cos, -1, 1) ** 2)) < 1e-2
    nz = clear & (want_f != 0) & (np.abs(wil[:, 2]) > 1e-2) & ~critical(wil[:, 2])
    dev_f = float(_rel(f[nz, 0], want_f[nz]).max())
    want_pdf = np.where(wol[:, 2] * wil[:, 2] > 0, np.abs(wil[:, 2]) / np.pi, 0.0)
    assert np.all((pdf[clear] == 0) == (want_pdf[clear] == 0))
    nzp = clear & (want_pdf != 0)
    dev_pdf = float(_rel(pdf[nzp], want_pdf[nzp]).max())
    # the sampled direction: the cosine-hemisphere sample of (min(u.x, 1 - 2^-24), u.y), flipped to wo's side of ns, carried to the world by the frame
    uc = np.stack([np.minimum(u[:, 0], U_TOP), u[:, 1]], axis=1)
    wl = _cosine_hemisphere(uc)
    wl[:, 2] *= np.where(wol[:, 2] < 0, -1.0, 1.0)
    want_wi = wl[:, 0:1] * ss + wl[:, 1:2] * ts + wl[:, 2:3] * ns
    sampled = match & (np.abs(wol[:, 2]) > 1e-5) & (wl[:, 2] != 0)
    assert np.all(s_type[sampled & (s_pdf != 0)] == (BSDF_REFLECTION | BSDF_DIFFUSE))
    assert np.all(s_pdf[sampled] >= 0) and np.all(s_pdf[sampled] <= 1.0 / np.pi * (1 + 1e-6))
    # (compared away from the disk's rim: z = sqrt(1 - x^2 - y^2) amplifies the float32 rounding of x and y by 1 / z)
    live = sampled & (s_pdf != 0) & (np.abs(wl[:, 2]) > 0.05)
    dev_wi = float(np.linalg.norm(s_wi[live] - want_wi[live], axis=1).max())
    dev_pdf = max(dev_pdf, float(_rel(s_pdf[live], np.abs(wl[live, 2]) / np.pi).max()))
    gs = want_wi @ ng
    clear_s = live & (np.abs(gs) > 1e-5) & (np.abs(go) > 1e-5)
    want_sf = np.where(gs * go > 0, sw(wl[:, 2]), 0.0)
    assert np.all((s_f[clear_s, 0] == 0) == (want_sf[clear_s] == 0))
    nzs = clear_s & (want_sf != 0) & ~critical(wl[:, 2])
    dev_f = max(dev_f, float(_rel(s_f[nzs, 0], want_sf[nzs]).max()))
    return dev_f, dev_pdf, dev_wi, int(nz.sum()), int(live.sum())


@pytest.mark.parametrize("name", WITH_BSSRDF)
def test_adapter_is_one_diffuse_reflection_lobe_of_sw(pkg, oracle, name):
    c = case(pkg, oracle, name)
    assert len(ADAPTER_FLAGS) == 5
    for fname in FRAMES:
        dev_f, dev_pdf, dev_wi, n_f, n_s = adapter_deviations(c, fname)
        print(f"\n{name} {fname}: {n_f} non-zero f, {n_s} samples: f {dev_f:.3e} (bound {ADAPTER_F_TOL:.1e}), pdf {dev_pdf:.3e} (bound {ADAPTER_PDF_TOL:.1e}), wi {dev_wi:.3e} (bound {ADAPTER_WI_TOL:.1e})")
        assert n_f >= N_RANDOM // 20 and n_s >= N_RANDOM // 10
        assert dev_f <= ADAPTER_F_TOL and dev_pdf <= ADAPTER_PDF_TOL and dev_wi <= ADAPTER_WI_TOL
