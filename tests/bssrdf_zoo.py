"""Materials, frames and queries of the BSSRDF probe (tests/test_bssrdf_probe.py: the device's dev_bssrdf.h against the oracle's orc_bssrdf_eval, bit for bit;
tests/test_bssrdf_zoo.py: the oracle's answers to the same queries against float64 models, without a GPU).

A material is one 8x8 one-quad scene built through SceneBuilder, as test_device_probe.material_scene builds its own. A frame is the interaction the BSSRDF is made at
(p, n, sh_n, sh_dpdu, sh_dpdv) with the exit interaction of the adapter section beside it. Per section the queries have a random part of N_RANDOM and a structured
part; every structured query carries the name of its family, which a failure message repeats.

Sections and their words: probe_build.BSSRDF_SECTIONS (the layout of orc_bssrdf_eval, oracle/ref_kats.cpp); FIELDS names the words of each."""
import ctypes as C

import numpy as np
from probe_build import BSSRDF_SECTIONS

F = np.float32
N_RANDOM = 4096
U_TOP = float(F(1.0) - F(2.0 ** -24))   # the largest float below 1
DENORMAL = float(np.nextafter(F(0), F(1)))
BSDF_ALL, BSDF_REFLECTION, BSDF_TRANSMISSION, BSDF_DIFFUSE, BSDF_SPECULAR = 31, 1, 2, 4, 16
SECTION_INDEX = {name: k for k, (name, _, _) in enumerate(BSSRDF_SECTIONS)}
WORDS_IN = {name: a for name, a, _ in BSSRDF_SECTIONS}
WORDS_OUT = {name: b for name, _, b in BSSRDF_SECTIONS}
# section -> field -> (first word, one past the last). Words are floats but `ok` (a uint32) and `s_type` (an int32): small integers, no NaN patterns.
# state of a DisneyBSSRDF: sigma_t holds d (the scatter distance), rho holds R (colour x diffuse weight)
FIELDS = {
    "state": dict(sigma_t=(0, 3), rho=(3, 6), eta=(6, 7), ns=(7, 10), ss=(10, 13), ts=(13, 16), po_p=(16, 19)),
    "radii": dict(sr=(0, 3), pdf_sr=(3, 6)),
    "samples": dict(r=(0, 3)),
    "exits": dict(pdf_sp=(0, 1), sr=(1, 4)),
    "segments": dict(ok=(0, 1), start=(1, 4), target=(4, 7), u1n=(7, 8)),
    "adapter": dict(f=(0, 3), pdf=(3, 4), s_wi=(4, 7), s_f=(7, 10), s_pdf=(10, 11), s_type=(11, 12)),
    "conversion": dict(sigma_a=(0, 3), sigma_s=(3, 6)),
}
# no field is left out of the bit comparison: a name here would need the IEEE operation beside it that leaves the field open
FIELDS_LEFT_OUT = {}

# ---- materials ------------------------------------------------------------------------------------------------------------------------------------
# name -> (kind, parameters, textures declared before it: (name, kind, class, parameters))
_SA, _SS = (0.0011, 0.0024, 0.014), (2.55, 3.21, 3.77)
MATERIALS = {
    "ss_skin1": ("subsurface", dict(name="Skin1", eta=1.33)),
    "ss_scaled_eta_1.5": ("subsurface", dict(sigma_a=(0.02, 0.05, 0.3), sigma_s=(1.5, 2.0, 0.7), scale=2.5, eta=1.5)),
    "ss_g_0.4": ("subsurface", dict(sigma_a=_SA, sigma_s=_SS, g=0.4, eta=1.33, scale=0.1)),                    # a second table
    "ss_negative": ("subsurface", dict(sigma_a=(-0.5, 0.01, 0.02), sigma_s=(1.0, -2.0, 3.0), eta=1.33)),         # the clamp of init_medium
    "ss_sigma_s_zero": ("subsurface", dict(sigma_a=(0.5, 0.01, 0.02), sigma_s=(0.0, 2.0, 3.0), eta=1.33)),      # rho = 0: the first rho node
    "ss_sigma_a_zero": ("subsurface", dict(sigma_a=(0.0, 0.01, 0.02), sigma_s=(1.0, 2.0, 3.0), eta=1.33)),      # rho = 1: the last rho node, catmull_rom_weights refuses
    "ss_sigma_t_zero": ("subsurface", dict(sigma_a=(0.0, 0.01, 0.02), sigma_s=(0.0, 2.0, 3.0), eta=1.33)),      # sigma_t = 0: sample_sr = -1, probe_segment false
    "ss_eta_1.0": ("subsurface", dict(sigma_a=(0.02, 0.05, 0.3), sigma_s=(1.5, 2.0, 0.7), eta=1.0)),
    "ss_eta_0.8": ("subsurface", dict(sigma_a=(0.02, 0.05, 0.3), sigma_s=(1.5, 2.0, 0.7), eta=0.8)),             # the other arm of fresnel_moment1 in bssrdf_sw
    "kd_constant": ("kdsubsurface", dict(Kd=(0.5, 0.4, 0.3), mfp=(1.0, 0.8, 0.6))),                               # converted on the host
    "kd_textured": ("kdsubsurface", dict(Kd="kd", mfp=(1.0, 0.8, 0.6), scale=0.5), (("kd", "spectrum", "constant", dict(value=(0.5, 0.5, 0.5))),)),   # kd_subsurface = 1: converted on the device
    "disney_scatter": ("disney", dict(color=(0.6, 0.4, 0.3), roughness=0.4, scatterdistance=(0.5, 0.3, 0.2))),
    "disney_weighted": ("disney", dict(color=(0.6, 0.4, 1.3), roughness=0.4, metallic=0.3, spectrans=0.4, eta=1.4, scatterdistance=(0.05, 0.3, 2.0))),
    "disney_d_zero": ("disney", dict(color=(0.6, 0.4, 0.3), roughness=0.4, scatterdistance=(0.5, 0.0, 0.2))),   # d = 0 in one channel: divisions by zero
    "disney_metallic_1": ("disney", dict(color=(0.6, 0.4, 0.3), metallic=1.0, scatterdistance=(0.5, 0.3, 0.2))),   # diffuse weight 0: no BSSRDF
    "disney_spectrans_1": ("disney", dict(color=(0.6, 0.4, 0.3), spectrans=1.0, scatterdistance=(0.5, 0.3, 0.2))),
    "disney_thin": ("disney", dict(color=(0.6, 0.4, 0.3), thin=True, scatterdistance=(0.5, 0.3, 0.2))),           # thin: the BSSRDF is skipped
}
NO_BSSRDF = ("disney_metallic_1", "disney_spectrans_1", "disney_thin")   # status 2 on both sides
# pt_scene_create refuses a DisneyBSSRDF whose scatter distance is not positive in every channel (scene_plan.hip), so the device never divides by d = 0:
# the oracle alone answers this material (test_bssrdf_zoo.py), and the GPU test asserts the refusal
DEVICE_REFUSES = ("disney_d_zero",)
RAGGED_MATERIAL = "ss_skin1"


def material_scene(pkg, spec):
    kind, kw = spec[0], spec[1]
    b = pkg.host.SceneBuilder()
    b.film.update(xres=8, yres=8); b.spp = 1
    b.look_at((0.0, 2.0, 5.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)); b.camera(fov=40.0)
    b.world_begin()
    b.light_source("infinite", L=(1.0, 1.0, 1.0))
    for name, tkind, cls, tkw in (spec[2] if len(spec) > 2 else ()):
        b.texture(name, tkind, cls, **tkw)
    b.material(kind, **kw)
    b.trianglemesh(np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], F), np.array([0, 1, 2, 0, 2, 3], np.uint32))
    sd, rp = b.world_end()
    return sd, int(sd.prim_material[0])


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _frame(p, n, sh_n, sh_dpdu, sh_dpdv):
    return np.concatenate([np.asarray(v, np.float64) for v in (p, n, sh_n, sh_dpdu, sh_dpdv)]).astype(F)


# the exit interactions of the adapter section, both with ng != ns: one whose shading frame is the world's axes (local == world, so the structured directions keep
# their exact zeros), one tilted and not orthonormal
_EXIT_AXES = _frame((0.5, 0.1, -0.2), _unit((0.3, 0.1, 1.0)), (0, 0, 1), (1, 0, 0), (0, 1, 0))
_EXIT_TILTED = _frame((0.5, 0.1, -0.2), _unit((-0.2, 0.1, 1.0)), _unit((0.25, 0.3, 0.9)), (1.17, -0.13, 0.39), (0.1, 1.1, -0.2))
# name -> the 30 floats the probe takes: the entry interaction, then the exit interaction
FRAMES = {
    "canonical": np.concatenate([_frame((0, 0, 0), (0, 0, 1), (0, 0, 1), (1, 0, 0), (0, 1, 0)), _EXIT_AXES]),
    # as a bump-mapped vertex has it: sh_dpdu not unit and not orthogonal to sh_n, so ts is not unit and the frame not orthonormal
    "tilted": np.concatenate([_frame((0.3, -0.2, 0.1), _unit((0.1, 0.2, 1.0)), _unit((0.3, -0.2, 0.9)), (1.7, 0.4, 0.5), (0.1, 1.2, -0.3)), _EXIT_TILTED]),
    # cancellation in po_p - pi_p
    "far": np.concatenate([_frame((1e4, -1e4, 1e4), (0, 0, 1), (0, 0, 1), (1, 0, 0), (0, 1, 0)), _EXIT_AXES]),
}
ORTHONORMAL_FRAMES = ("canonical", "far")


# ---- the oracle -------------------------------------------------------------------------------------------------------------------------------------
def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def field(words, section, name):
    """One field of a section's (n, words) uint32 array, as float32 (n, k) -- or (n,) for a single word."""
    a, b = FIELDS[section][name]
    w = np.ascontiguousarray(words[:, a:b]).view(F)
    return w[:, 0] if b - a == 1 else w


def adapter_words(q8, flags):
    """The adapter section's nine input words per query: wo, wi, u and the flags as the ninth word's bits."""
    return np.ascontiguousarray(np.concatenate([np.ascontiguousarray(q8, F).view(np.uint32), np.asarray(flags, np.int32).astype(np.uint32)[:, None]], axis=1)).view(F)


def oracle_eval(oracle, s, mi, frames, **q):
    """orc_bssrdf_eval: the sections named in `q` (section -> input array as the probe takes it) plus the state; None where the material leaves no BSSRDF."""
    out = {k: np.zeros((len(v), WORDS_OUT[k]), np.uint32) for k, v in q.items()}
    out["state"] = np.zeros((1, WORDS_OUT["state"]), np.uint32)
    ins = {k: np.ascontiguousarray(v, F) for k, v in q.items()}
    n = lambda k: len(ins[k]) if k in ins else 0
    i = lambda k: _fp(ins[k]) if k in ins else None
    o = lambda k: _fp(out[k].view(F)) if k in out else None
    a8 = flags = None
    if "adapter" in ins:
        a8 = np.ascontiguousarray(ins["adapter"][:, :8]); flags = np.ascontiguousarray(ins["adapter"][:, 8]).view(np.int32)
    fr = np.ascontiguousarray(frames, F)
    st = oracle.lib.orc_bssrdf_eval(s.h, mi, _fp(fr[:15]), o("state"), n("radii"), i("radii"), o("radii"), n("samples"), i("samples"), o("samples"),
                                    n("exits"), i("exits"), o("exits"), n("segments"), i("segments"), _u32p(out["segments"]) if "segments" in out else None,
                                    _fp(fr[15:]), n("adapter"), _fp(a8) if a8 is not None else None,
                                    flags.ctypes.data_as(C.POINTER(C.c_int32)) if flags is not None else None, _u32p(out["adapter"]) if "adapter" in out else None,
                                    n("conversion"), i("conversion"), o("conversion"))
    assert st in (0, 2), st
    return out if st == 0 else None


# ---- queries --------------------------------------------------------------------------------------------------------------------------------------
def _near(v):
    """A float32 value with its two neighbours."""
    v = F(v)
    return [float(np.nextafter(v, F(-np.inf))), float(v), float(np.nextafter(v, F(np.inf)))]


def _sphere(rng, n):
    z = 1.0 - 2.0 * rng.random(n); ph = 2.0 * np.pi * rng.random(n); r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return np.stack([r * np.cos(ph), r * np.sin(ph), z], axis=1)


class _Set:
    """Rows and the family of each: the random part first."""

    def __init__(self):
        self.rows, self.tags = [], []

    def add(self, family, rows):
        rows = [np.atleast_1d(np.asarray(r, np.float64)) for r in rows]
        self.rows += rows; self.tags += [family] * len(rows)

    def done(self, n_random):
        return dict(q=np.array(self.rows, np.float64).astype(F), tag=np.array(self.tags), random=n_random)


def radius_queries(table, state, disney, seed=11):
    """r: random log-uniform over the table's optical range divided by sigma_t of the query's channel (Disney: over 1e-3 d .. 30 d); then the structured families."""
    rng = np.random.default_rng(seed)
    scale = state["sigma_t"].astype(np.float64)   # sigma_t, or Disney's d
    ok = np.isfinite(scale) & (scale > 0)
    ch = np.arange(N_RANDOM) % 3
    ch = np.where(ok[ch], ch, int(np.argmax(ok)) if ok.any() else 0)
    unit = np.where(ok, scale, 1.0)[ch]
    s = _Set()
    if disney:
        s.add("random", list(np.exp(rng.uniform(np.log(1e-3), np.log(30.0), N_RANDOM)) * unit))
    else:
        nodes = table.radius_samples.astype(np.float64)
        s.add("random", list(np.exp(rng.uniform(np.log(nodes[1]), np.log(nodes[-1]), N_RANDOM)) / unit))
    s.add("zero", [0.0]); s.add("denormal", [DENORMAL]); s.add("1e-6 and neighbours (Disney's clamp)", _near(1e-6))
    s.add("huge", [1e30, np.inf])
    if disney:
        for c in range(3):
            if ok[c]: s.add(f"multiples of d, channel {c}", [k * scale[c] for k in (1e-4, 0.5, 1.0, 3.0, 30.0, 100.0, 1000.0)])
    else:
        for c in range(3):
            if not ok[c]: continue
            sig = F(scale[c])
            for k, node in enumerate(table.radius_samples):
                s.add(f"radius node {k} / sigma_t, channel {c}", _near(F(node) / sig))
            s.add(f"beyond the last node, channel {c}", [float(F(table.radius_samples[-1]) / sig) * k for k in (1.0 + 1e-6, 1.5, 100.0)])
    return s.done(N_RANDOM)


def sample_queries(seed=12):
    rng = np.random.default_rng(seed)
    s = _Set()
    s.add("random", list(rng.random(N_RANDOM, dtype=F)))
    s.add("0, 1 - 2^-24, 1", [0.0, U_TOP, 1.0])
    s.add("0.25 and neighbours (Disney's branch)", _near(0.25)); s.add("0.999 and neighbours (the rmax call)", _near(0.999))
    s.add("sweep near 0", [DENORMAL] + [2.0 ** -k for k in range(1, 60)] + [k * 2.0 ** -24 for k in range(1, 64)])
    s.add("sweep near 1", [1.0 - 2.0 ** -k for k in range(2, 25)] + [1.0 - k * 2.0 ** -24 for k in range(1, 64)])
    return s.done(N_RANDOM)


def channel_edges():
    """The six u1 at which u1n * 3 crosses 1 and 2 in each axis branch of probe_segment."""
    return [1.0 / 6.0, 1.0 / 3.0, 0.5 + 1.0 / 12.0, 0.5 + 1.0 / 6.0, 0.75 + 1.0 / 12.0, 0.75 + 1.0 / 6.0]


U2_SPECIAL = [0.0, 0.25, 0.5, 0.75, U_TOP]


def segment_queries(seed=13):
    rng = np.random.default_rng(seed)
    s = _Set()
    s.add("random", list(rng.random((N_RANDOM, 3), dtype=F)))
    u1s = [(f"u1 at {v} and neighbours", w) for v in (0.0, 0.5, 0.75, U_TOP) for w in _near(v) if 0.0 <= w < 1.0]
    u1s += [(f"u1 on a channel edge {v:.4f} and neighbours", w) for v in channel_edges() for w in _near(v)]
    generic = [(0.37, 0.61), (0.8, 0.13), (0.05, 0.9)]
    for fam, u1 in u1s:
        s.add(fam, [(u1, a, b) for a, b in generic])
    for k, u1 in enumerate((0.1, 0.3, 0.45, 0.55, 0.62, 0.7, 0.8, 0.88, 0.97)):   # every axis and channel
        s.add("u2.y on the axes of phi", [(u1, 0.37, y) for y in U2_SPECIAL])
        s.add("u2.x at the special values (r >= rmax)", [(u1, x, 0.61) for x in U2_SPECIAL + _near(0.999) + [1.0, 0.9995, 0.99999]])
    return s.done(N_RANDOM)


def frame_axes(state):
    """ss, ts, ns of a state section, float64."""
    return tuple(state[k].astype(np.float64) for k in ("ss", "ts", "ns"))


def exit_queries(state, rmax, seed=14):
    """(pi_p, pi_n): random points within rmax of po with random unit normals; then the structured families."""
    rng = np.random.default_rng(seed)
    po = state["po_p"].astype(np.float64); ss, ts, ns = frame_axes(state)
    s = _Set()
    d = _sphere(rng, N_RANDOM) * (rmax * rng.random(N_RANDOM) ** (1.0 / 3.0))[:, None]
    s.add("random", list(np.concatenate([po + d, _sphere(rng, N_RANDOM)], axis=1)))
    diag = _unit((0.3, -0.5, 0.8))
    normals = [("pi_n along ss", _unit(ss)), ("pi_n along ts", _unit(ts)), ("pi_n along ns", _unit(ns)), ("pi_n zero", np.zeros(3)), ("pi_n orthogonal to ns", _unit(np.cross(ns, diag))),
               ("pi_n orthogonal to ss", _unit(np.cross(ss, diag))), ("pi_n generic", diag)]
    pof = po.astype(F)
    near = [pof.copy()]
    for k in (1, 2, 3):
        for c in range(3):
            for side in (-np.inf, np.inf):
                p = pof.copy()
                for _ in range(k): p[c] = np.nextafter(p[c], F(side))
                near.append(p)
    points = [("pi = po", near[:1]), ("pi a few ulps from po", near[1:])]
    for name, ax in (("ss", ss), ("ts", ts), ("ns", ns)):
        points.append((f"pi displaced along {name} only", [po + _unit(ax) * rmax * k for k in (1e-6, 1e-3, 0.1, 0.5, -0.25, 0.99, 1.5)]))
    points.append(("pi generic", [po + diag * rmax * k for k in (1e-4, 0.01, 0.3, 0.9, 3.0)]))
    for pname, pts in points:
        for nname, nn in normals:
            s.add(f"{pname}; {nname}", [np.concatenate([np.asarray(p, np.float64), nn]) for p in pts])
    return s.done(N_RANDOM)


ADAPTER_FLAGS = (BSDF_ALL, BSDF_ALL & ~BSDF_SPECULAR, BSDF_REFLECTION | BSDF_DIFFUSE, BSDF_SPECULAR, BSDF_TRANSMISSION)


def adapter_queries():
    """(wo, wi, u, flags): the random and the structured queries of tests/test_device_probe.py, the random ones with every set of flags in turn, the structured ones with
    all of them. World directions: in the axes-aligned exit frame they are the local ones."""
    from test_device_probe import random_queries, structured_queries   # (imported, not copied)
    wo, wi, u = random_queries(N_RANDOM)
    rows = [np.concatenate([wo, wi, u], axis=1)]; flags = [np.array([ADAPTER_FLAGS[k % len(ADAPTER_FLAGS)] for k in range(len(wo))], np.int32)]
    tags = ["random"] * len(wo)
    wo, wi, u = structured_queries()
    for fl in ADAPTER_FLAGS:
        rows.append(np.concatenate([wo, wi, u], axis=1)); flags.append(np.full(len(wo), fl, np.int32)); tags += [f"test_device_probe.structured_queries, flags {fl}"] * len(wo)
    q8 = np.concatenate(rows).astype(F); fl = np.concatenate(flags)
    return dict(q=adapter_words(q8, fl), q8=q8, flags=fl, tag=np.array(tags), random=N_RANDOM)


def conversion_queries(table, seed=15):
    """(kd, mfp) per channel triple."""
    rng = np.random.default_rng(seed)
    s = _Set()
    s.add("random", list(np.concatenate([rng.random((N_RANDOM, 3)), np.exp(rng.uniform(np.log(1e-2), np.log(1e2), (N_RANDOM, 3)))], axis=1)))
    top = float(table.rhoeff.max())
    kds = [("kd 0", 0.0), ("kd just above 0", DENORMAL), ("kd just above 0", 1e-30), ("kd 1", 1.0), ("kd above the largest rhoeff", top * 1.5 + 0.1), ("kd negative", -0.25)]
    for k, node in enumerate(table.rhoeff):
        kds += [(f"kd at rhoeff node {k} and neighbours", w) for w in _near(node)]
    mfps = (0.0, 1e-30, 1.0, 1e30)
    for j, (fam, kd) in enumerate(kds):
        others = (kds[(j + 7) % len(kds)][1], kds[(j + 13) % len(kds)][1])
        s.add(fam, [(kd, others[0], others[1], m, mfps[(k + 1) % 4], mfps[(k + 2) % 4]) for k, m in enumerate(mfps)])
    return s.done(N_RANDOM)


# ---- a material's case: scene, state per frame, queries, the oracle's answers -- computed once, shared, left unchanged --------------------------------------------
_CASES = {}


def _state_fields(words):
    return {k: field(words, "state", k)[0] for k in FIELDS["state"]}


def case(pkg, oracle, name):
    if name in _CASES:
        return _CASES[name]
    sd, mi = material_scene(pkg, MATERIALS[name])
    m = sd.materials[mi]
    disney = int(m.type) == pkg._abi.PT_MAT_DISNEY
    table = None if disney else sd.bssrdf_src[int(m.bssrdf_table)]
    c = dict(sd=sd, mi=mi, disney=disney, table=table, frames={}, has=True)
    s = oracle.scene(sd)
    try:
        for fname, fr in FRAMES.items():
            first = oracle_eval(oracle, s, mi, fr, samples=np.array([0.999], F))
            if first is None:
                c["has"] = False
                break
            state = _state_fields(first["state"])
            r999 = field(first["samples"], "samples", "r")[0].astype(np.float64)
            live = r999[np.isfinite(r999) & (r999 > 0)]
            rmax = float(live.min()) if len(live) else 1.0   # the reach of the narrowest live channel: the scale of the exit points, within every live channel's range
            sets = dict(radii=radius_queries(table, state, disney), samples=sample_queries(), segments=segment_queries(), exits=exit_queries(state, rmax), adapter=adapter_queries())
            if not disney: sets["conversion"] = conversion_queries(table)
            ref = oracle_eval(oracle, s, mi, fr, **{k: v["q"] for k, v in sets.items()})
            c["frames"][fname] = dict(frames=fr, state=state, state_words=ref["state"], rmax=rmax, sets=sets, ref=ref)
    finally:
        s.close()
    _CASES[name] = c
    return c


# ---- a comparison must compare something ------------------------------------------------------------------------------------------------------------
def live_shares(fc):
    """Per frame case, over the RANDOM part: radii with a non-zero sr, samples with r >= 0 (any channel), segments accepted, exit points with a non-zero pdf_sp."""
    n = N_RANDOM
    ref = fc["ref"]
    return dict(radii=float(np.any(field(ref["radii"][:n], "radii", "sr") != 0, axis=1).mean()),
                samples=float(np.any(field(ref["samples"][:n], "samples", "r") >= 0, axis=1).mean()),
                segments=float((ref["segments"][:n, 0] != 0).mean()),
                exits=float((field(ref["exits"][:n], "exits", "pdf_sp") != 0).mean()))


# Floors of the live shares of the random part, per section. Measured with the oracle alone over the ordinary materials x the three frames, the lowest shares are
# radii 0.916 (kd_textured: a radius drawn in one channel's range can lie past the table in another's), samples 1.000, segments 1.000, exits 1.000
# (test_bssrdf_zoo.py prints them on every run); the floors sit a little below.
FLOORS = dict(radii=0.9, samples=0.99, segments=0.98, exits=0.98)
# The materials that are degenerate by design: their floors, with the measured shares (the same in the three frames) and the reason.
FLOOR_EXCEPTIONS = {
    # channel 0 has rho = 1 (sigma_a clamped to 0: catmull_rom_weights refuses, sample_sr = 0 = rmax, the segment is refused) and channel 1 rho = 0 with the table's
    # zero row (rmax = 0 as well): one channel in three gives segments. Measured: radii 0.765, samples 1.000, segments 0.329, exits 1.000
    "ss_negative": dict(radii=0.75, samples=0.99, segments=0.32, exits=0.98),
    # one channel with rho = 0 (the table's zero row): its segments have r >= rmax = 0. Measured: 0.934, 1.000, 0.656, 1.000
    "ss_sigma_s_zero": dict(radii=0.9, samples=0.99, segments=0.64, exits=0.98),
    # one channel with rho = 1, where catmull_rom_weights refuses: sample_sr = 0 = rmax. Measured: 0.953, 1.000, 0.656, 1.000
    "ss_sigma_a_zero": dict(radii=0.9, samples=0.99, segments=0.64, exits=0.98),
    # one channel with sigma_t = 0: sample_sr = -1, probe_segment false. Measured: 0.974, 1.000, 0.656, 1.000
    "ss_sigma_t_zero": dict(radii=0.9, samples=0.99, segments=0.64, exits=0.98),
    # eta < 1: the host's beam-diffusion table is all zero (its single-scattering term takes sqrt(eta^2 - 1), and the NaNs are stored as 0), so sr = 0, pdf_sr = 0 / 0,
    # rmax = 0. The material is here for the adapter: the other arm of fresnel_moment1 in bssrdf_sw. Measured: 0.000, 1.000, 0.000, 0.000
    "ss_eta_0.8": dict(radii=0.0, samples=0.99, segments=0.0, exits=0.0),
    # d = 0 in one channel: its sample_sr = 0 * log(..) = 0 = rmax. Measured: 1.000, 1.000, 0.673, 1.000 (sr and pdf_sp are non-zero because they are NaN: x / 0)
    "disney_d_zero": dict(radii=0.98, samples=0.99, segments=0.65, exits=0.98),
}


def check_floors(name, c):
    shares = {}
    for fname, fc in c["frames"].items():
        sh = live_shares(fc); shares[fname] = sh
        floors = FLOOR_EXCEPTIONS.get(name, FLOORS)
        for k, v in sh.items():
            assert v >= floors[k], f"{name} {fname}: only {v:.3f} of the random {k} queries are live (floor {floors[k]})"
    return shares
