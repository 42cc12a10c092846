"""The device's BSDFs and light sampling against the CPU oracle, CALL BY CALL (the renders of tests/test_gpu_parity.py reach these functions only with
the few tens of thousands of vertices a small scene produces, never with wo.z == 0, a zero half vector, a lobe-choice boundary or a reference point on a
light's own plane).

tests/device_probe/{bsdf,light}_probe.hip are test code: small kernels of their own around the UNMODIFIED headers of pbrt-rust_amd/csrc (dev_bsdf.h,
dev_light.h), one query per thread, on the material table / DeviceScene of a pt_scene that libmi355pt.so created. The module fixture `probe` compiles them
once per session with hipcc, with the HIPFLAGS line of pbrt-rust_amd/csrc/Makefile (a different -ffp-contract would change bits) plus
-fvisibility=hidden, into a pytest temporary directory: about half a minute, paid once; every case after that is a few kernel launches of
a few thousand threads and takes well under a second. No render, no trace_mode.

  * Bsdf<MAXL, DIFF>::f / pdf / f_pdf / sample_f == orc_bsdf_eval (oracle/ref_kats.cpp) at the oracle's canonical interaction, bit for bit, in every one of
    the nine instantiations of tu_shade.hip the material's vertices can run in: the lobe-set kernel of its shade class, the general kernel of its lobe count
    and, for the specular class, the one-lobe kernel the volumetric integrator folds it into. The class comes from pth::material_class / class_general themselves.
  * on the device, the fused f_pdf == f and pdf evaluated separately; the specialised instantiation == the general one.
  * light_sample_li / light_pdf_li == orc_light_sample_li / orc_light_pdf_li, same scene, light and (p, p_error, n), bit for bit.

Bit equality is the project's own claim (parity statement: both sides are built with -ffp-contract=off and share the dm_* transcendentals), so
values are compared as uint32 patterns: signed zeros and infinities count. The one thing IEEE 754 leaves open is the sign and payload of a NaN an
invalid operation produces (x86 SSE sets the sign bit, the GPU does not): every NaN pattern compares as one value, a NaN against a number still fails.
A test must not pass by comparing nothing: per material the shares of random queries with non-zero oracle f / pdf / sampled pdf have floors, and per light the
share of random queries with a non-zero sampled pdf."""
import ctypes as C
import os

import numpy as np
import pytest
from probe_build import probe_library

pytestmark = pytest.mark.gpu

if os.environ.get("PT_LIB_PATH"):   # a kernel-variant library: its pt_scene layout may differ from the one the probe is compiled against
    pytest.skip("PT_LIB_PATH names a variant library; the probe reads pt_scene of the tree's own headers", allow_module_level=True)

F = np.float32
U_TOP = float(np.float32(1.0) - np.float32(2.0 ** -24))   # the largest float below 1


# ---- the probe library ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(pkg, gpu, tmp_path_factory):
    """libdevprobe.so of tests/device_probe/*.hip: built once per session by tests/probe_build.py, shared with tests/test_interaction_probe.py."""
    return probe_library(pkg, tmp_path_factory.mktemp("device_probe"))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def bits(a):
    """uint32 patterns of a float32 array, every NaN as one pattern (module docstring)."""
    a = np.ascontiguousarray(a, F)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def assert_same_bits(dev, ref, what, tags=None):
    """`tags`: per query, the name of the family it belongs to (tests/bssrdf_zoo.py): the message then names the first one's and every family that differs."""
    d, r = bits(dev), bits(ref)
    if np.array_equal(d, r):
        return
    bad = np.argwhere(d != r)
    q = int(bad[0][0])
    family = "" if tags is None else f" [{tags[q]}; families that differ: {sorted({str(t) for t in np.asarray(tags)[np.unique(bad[:, 0])]})[:8]}]"
    raise AssertionError(f"{what}: {len(np.unique(bad[:, 0]))} of {len(d)} queries differ; first at query {q}{family}: device {np.atleast_1d(d[q])} "
                         f"({np.atleast_1d(np.asarray(dev, F)[q])}) != reference {np.atleast_1d(r[q])} ({np.atleast_1d(np.asarray(ref, F)[q])})")


# ---- BSDF probe -------------------------------------------------------------------------------------------------------------------------------------
# (kind, parameters, materials made before it: a mix names them by their ids 1 and 2 -- id 0 is the builder's default matte)
_PLASTIC = ("plastic", dict(Kd=(0.2, 0.3, 0.4), Ks=(0.5, 0.4, 0.3), roughness=0.3))
_MATTE_ON = ("matte", dict(Kd=(0.6, 0.5, 0.4), sigma=35.0))
_MIX = lambda amount: ("mix", dict(amount=amount, namedmaterial1=1, namedmaterial2=2), (_PLASTIC, _MATTE_ON))
MATERIALS = {
    "matte": ("matte", dict(Kd=(0.6, 0.5, 0.4), sigma=0.0)),
    "matte_oren_nayar": _MATTE_ON,
    "mirror": ("mirror", dict(Kr=(0.9, 0.8, 0.7))),
    "glass_smooth": ("glass", dict(Kr=(0.9, 1.0, 0.8), Kt=(1.0, 0.9, 0.8), eta=1.5)),
    "glass_rough": ("glass", dict(eta=1.5, uroughness=0.35, vroughness=0.35)),
    "glass_rough_aniso": ("glass", dict(Kr=(0.9, 1.0, 0.8), Kt=(1.0, 0.9, 0.8), eta=1.4, uroughness=0.2, vroughness=0.5)),
    "glass_rough_no_remap": ("glass", dict(eta=1.5, uroughness=0.3, vroughness=0.2, remaproughness=False)),
    "glass_rough_kr_black": ("glass", dict(Kr=(0.0, 0.0, 0.0), eta=1.5, uroughness=0.3, vroughness=0.3)),
    "glass_rough_kt_black": ("glass", dict(Kt=(0.0, 0.0, 0.0), eta=1.5, uroughness=0.3, vroughness=0.3)),
    "glass_smooth_kr_black": ("glass", dict(Kr=(0.0, 0.0, 0.0), eta=1.5)),
    "glass_smooth_kt_black": ("glass", dict(Kt=(0.0, 0.0, 0.0), eta=1.5)),
    "plastic": _PLASTIC,
    "plastic_kd_black": ("plastic", dict(Kd=(0.0, 0.0, 0.0), Ks=(0.5, 0.4, 0.3), roughness=0.2)),
    "plastic_ks_black": ("plastic", dict(Kd=(0.2, 0.3, 0.4), Ks=(0.0, 0.0, 0.0), roughness=0.2)),
    "metal_alpha_floor": ("metal", dict(roughness=0.001)),
    "metal_aniso": ("metal", dict(eta_rgb=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), uroughness=0.2, vroughness=0.35)),
    "uber_kd": ("uber", dict(Kd=(0.3, 0.5, 0.2), Ks=(0.0, 0.0, 0.0))),
    "uber_kd_ks": ("uber", dict(Kd=(0.3, 0.5, 0.2), Ks=(0.3, 0.3, 0.3), roughness=0.3)),
    "uber_kd_ks_kr": ("uber", dict(Kd=(0.3, 0.5, 0.2), Ks=(0.3, 0.3, 0.3), Kr=(0.2, 0.2, 0.3), roughness=0.3)),
    "uber_kd_ks_kr_kt": ("uber", dict(Kd=(0.3, 0.5, 0.2), Ks=(0.3, 0.3, 0.3), Kr=(0.2, 0.2, 0.3), Kt=(0.3, 0.2, 0.2), uroughness=0.2, vroughness=0.4, eta=1.3)),
    "uber_five_lobes": ("uber", dict(Kd=(0.3, 0.5, 0.2), Ks=(0.3, 0.3, 0.3), Kr=(0.2, 0.2, 0.3), Kt=(0.3, 0.2, 0.2), opacity=(0.7, 0.8, 0.6), roughness=0.25, eta=1.3)),
    "substrate": ("substrate", dict(Kd=(0.5, 0.3, 0.1), Ks=(0.2, 0.2, 0.2), uroughness=0.3, vroughness=0.4)),
    "translucent": ("translucent", dict(Kd=(0.3, 0.4, 0.5), Ks=(0.3, 0.3, 0.2), reflect=(0.6, 0.5, 0.4), transmit=(0.4, 0.5, 0.6), roughness=0.3)),
    "translucent_reflect_black": ("translucent", dict(Kd=(0.3, 0.4, 0.5), Ks=(0.3, 0.3, 0.2), reflect=(0.0, 0.0, 0.0), transmit=(0.4, 0.5, 0.6), roughness=0.3)),
    "translucent_transmit_black": ("translucent", dict(Kd=(0.3, 0.4, 0.5), Ks=(0.3, 0.3, 0.2), reflect=(0.6, 0.5, 0.4), transmit=(0.0, 0.0, 0.0), roughness=0.3)),
    "translucent_no_bsdf": ("translucent", dict(Kd=(0.3, 0.4, 0.5), Ks=(0.3, 0.3, 0.2), reflect=(0.0, 0.0, 0.0), transmit=(0.0, 0.0, 0.0))),
    "mix_amount_0": _MIX(0.0),
    "mix_amount_0.3": _MIX(0.3),
    "mix_amount_1": _MIX(1.0),
    "mix_amount_rgb": _MIX((0.2, 0.5, 0.9)),
    "disney_dielectric": ("disney", dict(color=(0.6, 0.4, 0.3), metallic=0.0, roughness=0.45, speculartint=0.3)),
    "disney_metallic": ("disney", dict(color=(0.8, 0.8, 0.2), metallic=1.0, roughness=0.35)),
    "disney_aniso": ("disney", dict(color=(0.8, 0.8, 0.2), metallic=0.6, roughness=0.35, anisotropic=0.7)),
    "disney_sheen": ("disney", dict(color=(0.6, 0.4, 0.3), metallic=0.3, roughness=0.45, sheen=0.5, sheentint=0.3)),
    "disney_clearcoat": ("disney", dict(color=(0.6, 0.4, 0.3), metallic=0.2, roughness=0.5, clearcoat=0.8, clearcoatgloss=0.6)),
    "disney_spectrans": ("disney", dict(color=(0.6, 0.7, 0.8), roughness=0.4, spectrans=0.6, eta=1.4)),
    "disney_thin": ("disney", dict(color=(0.6, 0.7, 0.8), roughness=0.4, thin=True, flatness=0.6, difftrans=0.8)),
    "disney_scatter": ("disney", dict(color=(0.6, 0.4, 0.3), roughness=0.4, scatterdistance=(0.5, 0.3, 0.2))),
    "subsurface_smooth": ("subsurface", dict(eta=1.33)),
    "subsurface_rough": ("subsurface", dict(eta=1.33, uroughness=0.3, vroughness=0.2)),
    "kdsubsurface": ("kdsubsurface", dict(Kd=(0.5, 0.4, 0.3), mfp=(1.0, 0.8, 0.6))),
}
RAGGED_MATERIAL = "plastic"   # the two-lobe material whose query count is 1, 255, 256, 257: a ragged last block and a full LDS column set
# class -> Bsdf<MAXL, DIFF> of its shade kernel (render_loop.hip's kernel table; tu_shade.hip instantiates exactly these nine)
CLASS_KERNEL = {0: (1, 1), 6: (1, 2), 7: (1, 3), 8: (2, 4), 9: (5, 5), 10: (1, 6), 1: (1, 0), 2: (2, 0), 3: (5, 0)}
# the floors of the random part: shares of queries with non-zero oracle f, pdf and sampled pdf. Measured with the oracle alone on 20 000 uniform pairs
# the lowest shares over these materials are 0.497, 0.497 and 0.723 (rough glass); the exceptions below are what the oracle alone shows, with their reason
FLOORS = (0.4, 0.4, 0.7)
FLOOR_EXCEPTIONS = {
    # a lone microfacet TRANSMISSION lobe: non-zero only for pairs in opposite hemispheres (half of them) whose generalised half vector has wo and wi on
    # opposite sides (about a quarter of those). The oracle alone shows 0.117, 0.133 and 0.702 on these queries
    "glass_rough_kr_black": (0.1, 0.1, 0.7),
}


def material_scene(pkg, spec):
    kind, kw = spec[0], spec[1]
    b = pkg.host.SceneBuilder()
    b.film.update(xres=8, yres=8); b.spp = 1
    b.look_at((0.0, 2.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)); b.camera(fov=40.0)
    b.world_begin()
    b.light_source("infinite", L=(1.0, 1.0, 1.0))
    for k, w in (spec[2] if len(spec) > 2 else ()):
        b.material(k, **w)
    b.material(kind, **kw)
    b.trianglemesh(np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], F), np.array([0, 1, 2, 0, 2, 3], np.uint32))
    sd, rp = b.world_end()
    return sd, int(sd.prim_material[0])


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sphere(rng, n):
    z = 1.0 - 2.0 * rng.random(n); ph = 2.0 * np.pi * rng.random(n); r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([r * np.cos(ph), r * np.sin(ph), z], axis=1)


def random_queries(n=4096, seed=1):
    rng = np.random.default_rng(seed)
    return _sphere(rng, n).astype(F), _sphere(rng, n).astype(F), rng.random((n, 2), dtype=F)


def structured_queries():
    """(wo, wi, u) at the inputs where BSDF code goes wrong; see the list in the body."""
    xz = lambda z: (np.sqrt(1.0 - z * z), 0.0, z)
    yz = lambda z: (0.0, np.sqrt(1.0 - z * z), z)
    up, down = _unit((0.3, -0.5, 0.8)), _unit((-0.4, 0.2, -0.7))
    generic = [up, down, _unit((0.6, 0.0, 0.5)), _unit((0.0, -0.7, -0.4))]
    pairs = []
    # wo.z exactly 0 (BSDF::f / pdf / sample_f return early)
    for wo in ((1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (0.6, 0.8, 0.0)):
        pairs += [(wo, w) for w in generic[:2]] + [(up, wo), (down, wo)]
    # grazing cosines, in the xz- and the yz-plane, for wo and for wi, against both hemispheres
    for z in (1e-3, -1e-3, 1e-6, -1e-6, 1e-30, -1e-30):
        for plane in (xz, yz):
            pairs += [(plane(z), up), (plane(z), down), (up, plane(z)), (down, plane(z))]
    # wo = +-z exactly; wi = -wo (zero half vector); wi the exact mirror of wo
    pairs += [((0.0, 0.0, s), w) for s in (1.0, -1.0) for w in generic + [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0)]]
    for w in generic + [xz(0.5), yz(-0.5), xz(1e-3), (0.0, 0.0, 1.0)]:
        w = np.asarray(w, np.float64).astype(F)
        pairs += [(w, -w), (w, w * np.array([-1, -1, 1], F)), (w, w)]
    # both in one plane
    pairs += [(xz(a), xz(b)) for a in (0.9, 0.3, -0.6) for b in (0.7, -0.2)] + [(yz(a), yz(b)) for a in (0.9, 0.3, -0.6) for b in (0.7, -0.2)]
    # opposite hemispheres at grazing angles; from inside beyond the critical angle (total internal reflection for the dielectrics)
    for a in (0.05, 1e-3, 0.3, 0.6, 0.74, 0.75):
        for b in (0.05, 0.5, 0.99):
            pairs += [(xz(a), yz(-b)), (yz(-a), xz(b)), (xz(-a), xz(b)), (xz(-a), _unit((-1.0, 0.2, b)))]
    # u: the four corners (1 - 2^-24 for 1), and u.x on every lobe-choice boundary k / matching and the float just below it
    us = [(a, b) for a in (0.0, U_TOP) for b in (0.0, U_TOP)]
    for m in range(2, 6):
        for k in range(1, m + 1):
            edge = F(k) / F(m)
            if k < m: us.append((float(edge), 0.37))
            us.append((float(np.nextafter(edge, F(0))), 0.61))
    us += [(0.5, 0.5), (0.25, 0.75)]
    wo = [p[0] for p in pairs]; wi = [p[1] for p in pairs]; u = [us[j % len(us)] for j in range(len(pairs))]
    for uu in us:   # every u with outgoing directions of each kind
        for o in (up, down, xz(-0.3), (0.0, 0.0, 1.0), xz(0.7), yz(-0.9)):
            wo.append(o); wi.append(generic[len(wo) % 4]); u.append(uu)
    return np.array(wo, np.float64).astype(F), np.array(wi, np.float64).astype(F), np.array(u, np.float64).astype(F)


def oracle_bsdf(oracle, s, mi, wo, wi, u):
    """orc_bsdf_eval -> dict of arrays (has_bsdf False: the oracle leaves everything unwritten, all zero here like the probe's words)."""
    n = len(wo)
    r = dict(f=np.zeros((n, 3), F), pdf=np.zeros(n, F), s_wi=np.zeros((n, 3), F), s_f=np.zeros((n, 3), F), s_pdf=np.zeros(n, F), s_type=np.zeros(n, np.int32))
    nl = C.c_int32(0)
    st = oracle.lib.orc_bsdf_eval(s.h, mi, n, _fp(wo), _fp(wi), _fp(u), _fp(r["f"]), _fp(r["pdf"]), _fp(r["s_wi"]), _fp(r["s_f"]), _fp(r["s_pdf"]),
                                  r["s_type"].ctypes.data_as(C.POINTER(C.c_int32)), C.byref(nl))
    assert st in (0, 2), st   # 2: the material leaves no BSDF
    r["has"] = st == 0; r["n"] = nl.value if st == 0 else 0
    return r


def device_bsdf(probe, scene, maxl, diff, mi, wo, wi, u):
    n = len(wo)
    out = np.zeros((n, 18), np.uint32)
    st = probe.probe_bsdf(scene.h, maxl, diff, mi, n, _fp(wo), _fp(wi), _fp(u), out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert st == 0, f"probe_bsdf<{maxl},{diff}>: status {st}"
    fl = lambda a, b: np.ascontiguousarray(out[:, a:b]).view(F).reshape(n, -1) if b - a > 1 else np.ascontiguousarray(out[:, a]).view(F)
    return dict(has=out[:, 0], n=out[:, 1], f=fl(2, 5), pdf=fl(5, 6), ff=fl(6, 9), fpdf=fl(9, 10), s_wi=fl(10, 13), s_f=fl(13, 16), s_pdf=fl(16, 17),
                s_type=out[:, 17].astype(np.int32))


def kernels_of(probe, sd, mi):
    """The Bsdf<MAXL, DIFF> instantiations material `mi` runs in, specialised first: from pth::material_class / class_general themselves."""
    cls, gen = C.c_int32(-1), C.c_int32(-1)
    assert probe.probe_material_class(sd.materials, sd.n_materials, mi, C.byref(cls), C.byref(gen)) == 0
    ks = [CLASS_KERNEL[cls.value]]
    if CLASS_KERNEL[gen.value] not in ks: ks.append(CLASS_KERNEL[gen.value])
    if cls.value == 6 and (1, 0) not in ks: ks.append((1, 0))   # volpath folds the specular class into class 1
    return cls.value, ks


_QUERIES = {}
_ORACLE_BSDF = {}


def _queries():
    if not _QUERIES:
        _QUERIES["random"] = random_queries(); _QUERIES["structured"] = structured_queries()
    return _QUERIES


def reference_bsdf(pkg, oracle, name):
    """Scene, material id and the oracle's answers to both query sets of one material: computed once, shared by the instances of the test."""
    if name not in _ORACLE_BSDF:
        sd, mi = material_scene(pkg, MATERIALS[name])
        s = oracle.scene(sd)
        _ORACLE_BSDF[name] = (sd, mi, {part: oracle_bsdf(oracle, s, mi, *q) for part, q in _queries().items()})
        s.close()
    return _ORACLE_BSDF[name]


def shares(ref):
    """Shares of queries with non-zero oracle f, pdf and sampled pdf."""
    return (float(np.any(ref["f"] != 0, axis=1).mean()), float((ref["pdf"] != 0).mean()), float((ref["s_pdf"] != 0).mean()))


def check_floors(name, ref):
    sf, sp, ss = shares(ref["random"])
    if name == "translucent_no_bsdf":
        assert not ref["random"]["has"] and not ref["structured"]["has"]
        return
    assert ref["random"]["has"] and ref["structured"]["has"], name
    if name == "mirror":   # a specular lobe: f and pdf are identically zero
        assert sf == 0.0 and sp == 0.0 and ss >= FLOORS[2], (name, sf, sp, ss)
        return
    ff, fp_, fs = FLOOR_EXCEPTIONS.get(name, FLOORS)
    assert sf >= ff and sp >= fp_ and ss >= fs, (name, sf, sp, ss)


def compare_bsdf(dev, ref, n, what):
    assert np.all(dev["has"] == (1 if ref["has"] else 0)), f"{what}: has_bsdf"
    assert np.all(dev["n"] == ref["n"]), f"{what}: lobe count {np.unique(dev['n'])} != {ref['n']}"
    for k in ("f", "pdf", "s_wi", "s_f", "s_pdf"):
        assert_same_bits(dev[k], ref[k][:n], f"{what}: {k} device vs oracle")
    assert np.array_equal(dev["s_type"], ref["s_type"][:n]), f"{what}: sampled type"
    assert_same_bits(dev["ff"], dev["f"], f"{what}: fused f_pdf's f vs f()")
    assert_same_bits(dev["fpdf"], dev["pdf"], f"{what}: fused f_pdf's pdf vs pdf()")


@pytest.mark.parametrize("name", list(MATERIALS))
def test_bsdf_calls_match_the_oracle_in_every_instantiation(pkg, gpu, oracle, probe, name):
    sd, mi, ref = reference_bsdf(pkg, oracle, name)
    check_floors(name, ref)
    scene = pkg.Scene(gpu, sd)
    try:
        cls, kernels = kernels_of(probe, sd, mi)
        results = {}
        for maxl, diff in kernels:
            for part, (wo, wi, u) in _queries().items():
                dev = device_bsdf(probe, scene, maxl, diff, mi, wo, wi, u)
                sf, sp, ss = shares(ref[part])
                print(f"{name}: class {cls}, Bsdf<{maxl},{diff}>, {part}: {len(wo)} queries compared, lobes {ref[part]['n']}, "
                      f"non-zero oracle f {sf:.3f}, pdf {sp:.3f}, sampled pdf {ss:.3f}")
                compare_bsdf(dev, ref[part], len(wo), f"{name} Bsdf<{maxl},{diff}> {part}")
                results[(maxl, diff, part)] = dev
        for maxl, diff in kernels[1:]:   # the specialised instantiation == the general one(s)
            for part in _queries():
                a, b = results[kernels[0] + (part,)], results[(maxl, diff, part)]
                for k in ("f", "pdf", "ff", "fpdf", "s_wi", "s_f", "s_pdf"):
                    assert_same_bits(a[k], b[k], f"{name} {part}: {k} of Bsdf<{kernels[0][0]},{kernels[0][1]}> vs Bsdf<{maxl},{diff}>")
                assert np.array_equal(a["s_type"], b["s_type"]) and np.array_equal(a["n"], b["n"])
    finally:
        scene.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_bsdf_probe_with_a_ragged_last_block(pkg, gpu, oracle, probe, n):
    """The two-lobe kernels keep their lobes in a 256-column LDS store: one query, one short of a block, a full block, one more than a block."""
    sd, mi, ref = reference_bsdf(pkg, oracle, RAGGED_MATERIAL)
    wo, wi, u = (a[:n] for a in _queries()["random"])
    scene = pkg.Scene(gpu, sd)
    try:
        cls, kernels = kernels_of(probe, sd, mi)
        assert (2, 4) in kernels and (2, 0) in kernels, kernels
        for maxl, diff in kernels:
            dev = device_bsdf(probe, scene, maxl, diff, mi, np.ascontiguousarray(wo), np.ascontiguousarray(wi), np.ascontiguousarray(u))
            print(f"{RAGGED_MATERIAL}: Bsdf<{maxl},{diff}>: {n} queries compared")
            compare_bsdf(dev, ref["random"], n, f"{RAGGED_MATERIAL} Bsdf<{maxl},{diff}> n={n}")
    finally:
        scene.close()


def test_probe_refuses_what_could_index_out_of_range(pkg, gpu, oracle, probe):
    sd, mi, _ = reference_bsdf(pkg, oracle, "matte")
    scene = pkg.Scene(gpu, sd)
    try:
        wo, wi, u = (np.ascontiguousarray(a[:4]) for a in _queries()["random"])
        out = np.zeros((4, 18), np.uint32); op = out.ctypes.data_as(C.POINTER(C.c_uint32))
        assert probe.probe_bsdf(scene.h, 1, 1, sd.n_materials, 4, _fp(wo), _fp(wi), _fp(u), op) == 1          # material index
        assert probe.probe_bsdf(scene.h, 1, 1, mi, 0, _fp(wo), _fp(wi), _fp(u), op) == 1                       # no query
        assert probe.probe_bsdf(scene.h, 1, 1, mi, 4, None, _fp(wi), _fp(u), op) == 1                          # null pointer
        assert probe.probe_bsdf(None, 1, 1, mi, 4, _fp(wo), _fp(wi), _fp(u), op) == 1
        for maxl, diff in ((1, 4), (1, 5), (2, 1), (2, 5), (5, 4), (3, 0), (0, 0), (5, 6)):
            assert probe.probe_bsdf(scene.h, maxl, diff, mi, 4, _fp(wo), _fp(wi), _fp(u), op) == 2, (maxl, diff)   # not one of the nine instantiations
        nl, sph = C.c_uint32(), C.c_int32()
        assert probe.probe_light_count(scene.h, C.byref(nl), C.byref(sph)) == 0 and nl.value == sd.n_lights
        z3 = np.zeros((4, 3), F); out8 = np.zeros((4, 8), np.uint32)
        assert probe.probe_light(scene.h, nl.value, 4, _fp(z3), _fp(z3), _fp(z3), _fp(u), _fp(wi), out8.ctypes.data_as(C.POINTER(C.c_uint32))) == 1   # light index
        assert probe.probe_light(scene.h, 0, 4, _fp(z3), None, _fp(z3), _fp(u), _fp(wi), out8.ctypes.data_as(C.POINTER(C.c_uint32))) == 1
        cls, gen = C.c_int32(), C.c_int32()
        assert probe.probe_material_class(sd.materials, sd.n_materials, sd.n_materials, C.byref(cls), C.byref(gen)) == 1
        assert not out.any() and not out8.any()   # nothing ran
    finally:
        scene.close()


# ---- light probe ------------------------------------------------------------------------------------------------------------------------------------
def _base(pkg):
    b = pkg.host.SceneBuilder()
    b.film.update(xres=8, yres=8); b.spp = 1
    b.look_at((0.0, 2.0, 7.0), (0.0, 0.4, 0.0), (0.0, 1.0, 0.0)); b.camera(fov=40.0)
    b.world_begin()
    return b


def _floor(pkg, b):
    b.material("matte", Kd=(0.5, 0.5, 0.5))
    P, I = pkg.scenes.quad((-6.0, -1.0, -6.0), (-6.0, -1.0, 6.0), (6.0, -1.0, 6.0), (6.0, -1.0, -6.0))
    b.trianglemesh(P, I)
    return b


def triangle_lights(pkg):
    """One triangle area light each: one-sided, two-sided, a mesh with normals that point AGAINST the geometric normal (the face_forward branch of
    Triangle::sample flips it), and ReverseOrientation."""
    b = _base(pkg)
    tri = np.array([[-0.5, 0.0, -0.4], [0.6, 0.0, -0.3], [0.1, 0.0, 0.7]], F); idx = np.array([0, 1, 2], np.uint32)
    b.attribute_begin(); b.area_light_source(L=(10.0, 9.0, 8.0)); b.translate(-2.0, 2.5, 0.0); b.rotate(20.0, 1.0, 0.0, 0.3); b.trianglemesh(tri, idx); b.attribute_end()
    b.attribute_begin(); b.area_light_source(L=(5.0, 6.0, 7.0), twosided=True); b.translate(0.0, 2.0, -1.0); b.rotate(-70.0, 0.0, 0.0, 1.0); b.trianglemesh(tri, idx); b.attribute_end()
    nrm = np.array([[0.1, 1.0, 0.0], [-0.1, 1.0, 0.1], [0.0, 1.0, -0.2]], F)   # the geometric normal cross(p1 - p0, p2 - p0) points to -y
    b.attribute_begin(); b.area_light_source(L=(4.0, 4.0, 9.0)); b.translate(2.0, 1.5, 0.5); b.rotate(35.0, 0.0, 1.0, 1.0); b.trianglemesh(tri, idx, N=nrm); b.attribute_end()
    b.attribute_begin(); b.area_light_source(L=(9.0, 4.0, 4.0)); b.translate(0.5, 3.0, 1.5); b.toggle_reverse_orientation(); b.trianglemesh(tri, idx); b.attribute_end()
    return _floor(pkg, b)


def delta_lights(pkg):
    b = _base(pkg)
    b.attribute_begin(); b.translate(0.2, 0.1, -0.3); b.light_source("point", I=(20.0, 18.0, 15.0), from_=(-1.0, 2.5, -1.0)); b.attribute_end()
    b.light_source("spot", I=(30.0, 30.0, 40.0), from_=(1.5, 3.0, 1.0), to=(0.0, 0.0, 0.2), coneangle=35.0, conedeltaangle=10.0)
    b.light_source("distant", L=(2.0, 2.5, 3.0), from_=(1.0, 3.0, 2.0), to=(0.0, 0.0, 0.0))
    return _floor(pkg, b)


def env_light(pkg):
    b = _base(pkg)
    b.attribute_begin(); b.rotate(-90.0, 1.0, 0.0, 0.0); b.rotate(30.0, 0.0, 0.0, 1.0)
    b.light_source("infinite", texels=pkg.scenes.sky_env(16, 8), L=(1.0, 1.0, 1.0)); b.attribute_end()
    return _floor(pkg, b)


LIGHT_SCENES = {
    "sphere_lights": lambda pkg: pkg.scenes.sphere_lights(xres=8, yres=8, spp=1),
    "disk_scene": lambda pkg: pkg.scenes.disk_scene(xres=8, yres=8, spp=1),
    "triangle_lights": triangle_lights,
    "delta_lights": delta_lights,
    "sky_env": env_light,
}
BOX = (np.array([-5.0, -1.0, -5.0]), np.array([5.0, 5.0, 6.0]))   # the random reference points: around every scene above
LIGHT_FLOOR = 0.3   # share of the random queries with a non-zero sampled pdf, per light


def light_geometry(pkg, sd, li):
    """What the structured reference points of light `li` are built from: read from the scene description itself."""
    A = pkg._abi
    L = sd.lights[li]
    m = np.array(list(L.light_to_world), np.float64).reshape(4, 4)
    g = dict(type=int(L.type), two_sided=bool(L.two_sided), center=m[:3, 3].copy(), axis=_unit(m[:3, 2]), pos=np.array(list(L.pos), np.float64),
             cos_total=float(L.cos_total_width), cos_falloff=float(L.cos_falloff_start), shape=None)
    if L.type == A.PT_LIGHT_DIFFUSE_AREA:
        ref = int(sd.prim_shape[L.prim])
        if (ref >> 30) == A.PT_SHAPE_SPHERE:
            S = sd.spheres[ref & 0x3FFFFFFF]
            g["shape"] = "disk" if S.kind == A.PT_QUADRIC_DISK else "sphere"; g["radius"] = float(S.radius)
            m = np.array(list(S.object_to_world), np.float64).reshape(4, 4)
            g["center"] = m[:3, 3] + m[:3, 2] * (float(S.z_min) if g["shape"] == "disk" else 0.0); g["axis"] = _unit(m[:3, 2])
        else:
            v = sd.P[sd.idx[ref & 0x3FFFFFFF]].astype(np.float64)
            g["shape"] = "triangle"; g["verts"] = v; g["center"] = v.mean(axis=0); g["axis"] = _unit(np.cross(v[1] - v[0], v[2] - v[0])); g["radius"] = float(np.linalg.norm(v[0] - g["center"]))
    return g


def _perp(a):
    t = np.cross(a, (1.0, 0.0, 0.0) if abs(a[0]) < 0.9 else (0.0, 1.0, 0.0))
    return t / np.linalg.norm(t)


def structured_points(pkg, g):
    A = pkg._abi
    c, a = g["center"], g["axis"]; t = _perp(a)
    pts = [np.array([0.3, 0.2, 0.1])]
    if g["shape"] in ("triangle", "disk"):
        r = g["radius"]
        pts += [c + t * r * k for k in (0.25, 2.0, 10.0)] + [c.copy()]                       # on the emitter's own plane (cosine 0), and on the emitter
        if g["shape"] == "triangle": pts += [g["verts"][0].copy(), 0.5 * (g["verts"][0] + g["verts"][1])]
        for s in (1.0, -1.0):                                                                # in front and behind, near and far
            pts += [c + a * s * d for d in (1e-6, 1.0, 1e6)] + [c + a * s * 0.5 + t * 3.0 * r]
    elif g["shape"] == "sphere":
        r = g["radius"]; d = _unit((0.3, 0.5, -0.8))
        pts += [c.copy(), c + d * 0.5 * r, c + d * r, c + a * r, c - a * r, c + d * r * (1.0 + 1e-6), c + d * r * (1.0 - 1e-6), c + d * (r + 1e-6), c + d * 1e6, c + d * 2.0 * r]
    elif g["type"] in (A.PT_LIGHT_POINT, A.PT_LIGHT_SPOT):
        p = g["pos"]; d = _unit((0.3, -0.8, 0.5))
        pts += [p.copy(), p + d * 1e-6, p + d * 1e6, p + d]
        if g["type"] == A.PT_LIGHT_SPOT:   # on the cone's total-width and falloff-start angles, on the axis, behind the light
            for cs in (g["cos_total"], g["cos_falloff"]):
                sn = np.sqrt(max(0.0, 1.0 - cs * cs))
                pts += [p + (a * cs + t * sn) * k for k in (1.0, 2.5)] + [p + (a * cs - t * sn) * 1.5]
            pts += [p + a * 2.0, p - a * 2.0]
    else:   # distant, infinite: no position of their own
        pts += [np.array([0.0, 0.0, 0.0]), np.array([1e6, -1e6, 1e6]), np.array([1e-6, 0.0, 0.0])]
    return np.array(pts, np.float64).astype(F)


def light_queries(pkg, sd, li, seed):
    """Reference points (p, p_error, n), sample points u and first-round directions w of one light; `random` = how many of them form the random part."""
    A = pkg._abi
    rng = np.random.default_rng(seed)
    g = light_geometry(pkg, sd, li)
    nr = 1024
    p = (BOX[0] + (BOX[1] - BOX[0]) * rng.random((nr, 3))).astype(F)
    p = np.concatenate([p, p]); nrm = np.concatenate([_sphere(rng, nr).astype(F), np.zeros((nr, 3), F)])   # a surface vertex, then the same point as a medium vertex
    perr = (np.abs(p) * F(3e-7) * (rng.random((2 * nr, 1)) < 0.5)).astype(F)
    u = rng.random((2 * nr, 2), dtype=F)
    sp = structured_points(pkg, g)
    corners = np.array([(a, b) for a in (0.0, U_TOP) for b in (0.0, U_TOP)] + [(0.37, 0.61), (0.5, 0.5)], F)
    normals = [g["axis"].astype(F), (-g["axis"]).astype(F), _perp(g["axis"]).astype(F), np.zeros(3, F)]
    sp_p, sp_n, sp_u = [], [], []
    for q in sp:
        for nn in normals:
            for uu in corners:
                sp_p.append(q); sp_n.append(nn); sp_u.append(uu)
    sp_p = np.array(sp_p, F); sp_n = np.array(sp_n, F); sp_u = np.array(sp_u, F)
    sp_err = (np.abs(sp_p) * F(3e-7) * (np.arange(len(sp_p))[:, None] % 2)).astype(F)
    p = np.concatenate([p, sp_p]); nrm = np.concatenate([nrm, sp_n]); perr = np.concatenate([perr, sp_err]); u = np.concatenate([u, sp_u])
    w = _sphere(rng, len(p))   # directions that mostly miss the light
    if g["type"] == A.PT_LIGHT_INFINITE:   # wi = +-z of the map, and phi at +-pi
        m = np.array(list(sd.lights[li].light_to_world), np.float64).reshape(4, 4)[:3, :3]
        special = [(0, 0, 1), (0, 0, -1), (-1, 0.0, 0), (-1, -0.0, 0), (-1, 1e-8, 0), (-1, -1e-8, 0), (-1, 1e-8, 0.5), (1, 0, 0), (1, -1e-8, 0)]
        for k, v in enumerate(special):
            w[2 * nr + k] = m @ _unit(v)
    return dict(p=p, perr=perr, n=nrm, u=u, w=w.astype(F), random=2 * nr, geometry=g)


def oracle_light(oracle, s, li, q, w):
    """orc_light_sample_li and orc_light_pdf_li per reference point (the oracle's hooks take one point and many samples)."""
    n = len(q["p"])
    wi = np.zeros((n, 3), F); pdf = np.zeros(n, F); L = np.zeros((n, 3), F); back = np.zeros(n, F)
    for i in range(n):
        a = (_fp(q["p"][i]), _fp(q["perr"][i]), _fp(q["n"][i]))
        assert oracle.lib.orc_light_sample_li(s.h, li, *a, 1, _fp(q["u"][i]), _fp(wi[i]), _fp(pdf[i:i + 1]), _fp(L[i])) == 0
        assert oracle.lib.orc_light_pdf_li(s.h, li, *a, 1, _fp(w[i]), _fp(back[i:i + 1])) == 0
    return dict(wi=wi, pdf=pdf, L=L, back=back)


def oracle_pdf(oracle, s, li, q, w):
    back = np.zeros(len(w), F)
    for i in range(len(w)):
        assert oracle.lib.orc_light_pdf_li(s.h, li, _fp(q["p"][i]), _fp(q["perr"][i]), _fp(q["n"][i]), 1, _fp(w[i]), _fp(back[i:i + 1])) == 0
    return back


def device_light(probe, scene, li, q, w):
    n = len(q["p"])
    out = np.zeros((n, 8), np.uint32)
    st = probe.probe_light(scene.h, li, n, _fp(q["p"]), _fp(q["perr"]), _fp(q["n"]), _fp(q["u"]), _fp(np.ascontiguousarray(w, F)), out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert st == 0, f"probe_light: status {st}"
    f = out.view(F)
    return dict(wi=f[:, 0:3], pdf=f[:, 3], L=f[:, 4:7], back=f[:, 7])


def second_round_directions(ref, w):
    """pdf_li is fed the directions sample_li returned (where it returned one: a finite, non-zero direction), else the first round's again."""
    ok = np.isfinite(ref["wi"]).all(axis=1) & (np.abs(ref["wi"]).sum(axis=1) > 0) & (ref["pdf"] != 0)
    return np.ascontiguousarray(np.where(ok[:, None], ref["wi"], w), F), ok


_ORACLE_LIGHT = {}


def reference_lights(pkg, oracle, name):
    if name not in _ORACLE_LIGHT:
        sd, rp = LIGHT_SCENES[name](pkg).world_end()
        s = oracle.scene(sd)
        per_light = []
        for li in range(sd.n_lights):
            q = light_queries(pkg, sd, li, seed=100 + li)
            ref = oracle_light(oracle, s, li, q, q["w"])
            w2, ok = second_round_directions(ref, q["w"])
            per_light.append((q, ref, w2, ok, oracle_pdf(oracle, s, li, q, w2)))
        s.close()
        _ORACLE_LIGHT[name] = (sd, per_light)
    return _ORACLE_LIGHT[name]


def check_light_floor(name, li, q, ref):
    share = float((ref["pdf"][:q["random"]] != 0).mean())
    assert share >= LIGHT_FLOOR, (name, li, share)
    return share


@pytest.mark.parametrize("name", list(LIGHT_SCENES))
def test_light_calls_match_the_oracle(pkg, gpu, oracle, probe, name):
    sd, per_light = reference_lights(pkg, oracle, name)
    assert sd.n_lights == len(per_light) > 0
    scene = pkg.Scene(gpu, sd)
    try:
        nl, sph = C.c_uint32(), C.c_int32()
        assert probe.probe_light_count(scene.h, C.byref(nl), C.byref(sph)) == 0 and nl.value == sd.n_lights
        assert bool(sph.value) == (sd.n_spheres > 0 or sd.n_instances > 0)
        for li, (q, ref, w2, ok, back2) in enumerate(per_light):
            share = check_light_floor(name, li, q, ref)
            g = q["geometry"]
            print(f"{name}: light {li} (type {g['type']}, {g['shape'] or '-'}), SPH {sph.value}: {len(q['p'])} queries compared ({q['random']} random), "
                  f"non-zero oracle sampled pdf {share:.3f}, non-zero pdf_li of random directions {float((ref['back'] != 0).mean()):.3f}, "
                  f"of sampled directions {float((back2[ok] != 0).mean()) if ok.any() else 0.0:.3f}")
            dev = device_light(probe, scene, li, q, q["w"])
            for k in ("pdf", "L", "wi", "back"):
                assert_same_bits(dev[k], ref[k], f"{name} light {li}: {'pdf_li' if k == 'back' else 'sample_li ' + k} device vs oracle")
            dev2 = device_light(probe, scene, li, q, w2)
            assert_same_bits(dev2["back"], back2, f"{name} light {li}: pdf_li of the sampled directions device vs oracle")
    finally:
        scene.close()
