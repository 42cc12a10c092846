"""Test infrastructure of the ID-matte tests (test_matte_model.py, test_matte_abi.py, test_matte.py): the contract of include/mi355aov.h's pt_matte_render as a numpy
model, and the scenes the GPU tests render.

The model takes the camera samples in the oracle's words -- aov_reference.camera_hits: pixel, pfilm and the primitive of every sample --, the scene's prim_material, a
group table and the render parameters, and forms the PtMattePixel tables by the stated order in float32: sample numbers ascending, within one the source pixels in
raster order, every sample added to the pixels of FilmTile::add_sample's footprint (film.rs:292-331) with the filter table's entry as its weight. Ids are integers and
the weights table lookups of bit-exact pfilm values, so the device's tables are held to the model's bit for bit."""
import types

import numpy as np
from aov_reference import GROUND_I, GROUND_P, _builder, undulating_mesh
from model_math import F, NONE

SLOTS = 8
LAYERS = ("material", "instance", "group")
# PtMattePixel (80 bytes)
DTYPE = np.dtype([("id", "<u4", (SLOTS,)), ("w", "<f4", (SLOTS,)), ("n_ids", "<u4"), ("w_total", "<f4"), ("w_other", "<f4"), ("reserved", "<u4")])
XRES, YRES, SPP = 32, 24, 4   # 2 x 2 sample tiles, the lower row half full: gathers cross tile edges


def sample_ids(sd, h, groups=None, instance=None):
    """Per sample of camera_hits: surface (bool) and ids (N, 3) uint32 -- material, instance, group. For scenes whose primitives all carry a material (the first hit is the
    surface). `instance`: the instance layer's id per sample (None: top-level geometry, 0); `groups`: the caller's id per primitive (None: 0)."""
    prim = h["prim"]
    surface = prim != NONE
    p = np.where(surface, prim, 0).astype(np.int64)
    assert (sd.prim_material[p][surface] != NONE).all(), "the model takes the first hit for the surface: no material-less shells"
    ids = np.zeros((len(prim), 3), np.uint32)
    ids[:, 0] = sd.prim_material[p]
    if instance is not None: ids[:, 1] = instance
    if groups is not None: ids[:, 2] = np.asarray(groups, np.uint32)[p]
    ids[~surface] = 0
    return surface, ids


def empty_tables(rp, layers=LAYERS):
    cb = rp.cropped_pixel_bounds
    return {k: np.zeros((cb[3] - cb[1], cb[2] - cb[0]), DTYPE) for k in layers}


def add_samples(rp, h, surface, ids, tables):
    """Continues `tables` ({layer: (H, W) array of DTYPE}, in place) with the samples of `h` = camera_hits(.., first, n): the contract's order and arithmetic. Returns the
    number of (sample, pixel) contributions -- the render's film_splats."""
    cb, sb, pb = list(rp.cropped_pixel_bounds), list(rp.sample_bounds), list(rp.pixel_bounds)
    n = h["n"]
    rx, ry = F(rp.filter_radius[0]), F(rp.filter_radius[1])
    invrx, invry = F(1.0) / rx, F(1.0) / ry
    table = np.array(list(rp.filter_table), F)
    n_src = len(h["pix"]) // n
    assert n_src == (sb[2] - sb[0]) * (sb[3] - sb[1])
    cols = [LAYERS.index(k) for k in tables]
    flat = [t.reshape(-1) for t in tables.values()]
    W = cb[2] - cb[0]
    contributions = 0
    half, sixteen = F(0.5), F(16.0)
    for s in range(n):                     # sample numbers ascending
        for q in range(n_src):             # source pixels in raster order (camera_hits: y outer, x inner)
            i = q * n + s
            qx, qy = h["pix"][i]
            if not (pb[0] <= qx < pb[2] and pb[1] <= qy < pb[3]): continue   # integrator.rs:328: no samples outside pixel_bounds
            dx, dy = F(h["pfilm"][i, 0]) - half, F(h["pfilm"][i, 1]) - half
            x0, x1 = max(int(np.ceil(dx - rx)), cb[0]), min(int(np.floor(dx + rx)) + 1, cb[2])
            y0, y1 = max(int(np.ceil(dy - ry)), cb[1]), min(int(np.floor(dy + ry)) + 1, cb[3])
            for y in range(y0, y1):
                iy = min(int(np.floor(np.abs((F(y) - dy) * invry * sixteen))), 15)
                for x in range(x0, x1):
                    ix = min(int(np.floor(np.abs((F(x) - dx) * invrx * sixteen))), 15)
                    fw = table[iy * 16 + ix]
                    pixel = (y - cb[1]) * W + (x - cb[0])
                    for col, t in zip(cols, flat):
                        _contribute(t[pixel:pixel + 1], bool(surface[i]), ids[i, col], fw)
                    contributions += 1
    return contributions


def _contribute(t, surface, ident, fw):
    """One contribution to the table t (a one-element view): found / claims a slot / w_other; w_total always. A miss adds to w_total alone."""
    if surface:
        n = int(t["n_ids"][0])
        for k in range(n):
            if t["id"][0, k] == ident:
                t["w"][0, k] = F(t["w"][0, k]) + fw
                break
        else:
            if n < SLOTS:
                t["id"][0, n] = ident; t["w"][0, n] = fw; t["n_ids"][0] = n + 1
            else:
                t["w_other"][0] = F(t["w_other"][0]) + fw
    t["w_total"][0] = F(t["w_total"][0]) + fw


def resolve(table, ranks):
    """pt_matte_resolve: (ids (.., ranks) uint32, coverage (.., ranks) float32) -- slots by weight descending, ties to the lower id; w / w_total in float32."""
    flat = table.reshape(-1)
    ids = np.zeros((len(flat), ranks), np.uint32); cov = np.zeros((len(flat), ranks), F)
    for i, t in enumerate(flat):
        n = int(t["n_ids"])
        if F(t["w_total"]) == 0: continue
        order = sorted(range(n), key=lambda k: (-float(t["w"][k]), int(t["id"][k])))
        for r, k in enumerate(order[:ranks]):
            ids[i, r] = t["id"][k]; cov[i, r] = F(t["w"][k]) / F(t["w_total"])
    return ids.reshape(table.shape + (ranks,)), cov.reshape(table.shape + (ranks,))


def mask(table, wanted):
    """pt_matte_mask: the sum, in slot order and float32, of the weights whose id is wanted, over w_total; 0 where w_total == 0."""
    wanted = np.asarray(wanted, np.uint32)
    total = np.zeros(table.shape, F)
    for k in range(SLOTS):
        take = (k < table["n_ids"]) & np.isin(table["id"][..., k], wanted)
        total = np.where(take, total + table["w"][..., k], total).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(table["w_total"] != 0, total / table["w_total"], F(0.0)).astype(F)


def fake_rp(width, height, radius=0.5, table=None):
    """Render parameters as far as the model reads them, for hand-made cases: a width x height film at the origin, sample and pixel bounds equal to it."""
    bounds = [0, 0, width, height]
    return types.SimpleNamespace(cropped_pixel_bounds=bounds, sample_bounds=bounds, pixel_bounds=bounds, filter_radius=[radius, radius],
                                 filter_table=[1.0] * 256 if table is None else table)


def fake_hits(rp, samples):
    """camera_hits of a hand-made job: samples[s][q] = (pfilm x, pfilm y, primitive) for sample number s of source pixel q (raster order)."""
    sb = rp.sample_bounds
    n, n_src = len(samples), (sb[2] - sb[0]) * (sb[3] - sb[1])
    pix = np.zeros((n_src * n, 2), np.int32); pfilm = np.zeros((n_src * n, 2), F); prim = np.zeros(n_src * n, np.uint32)
    for s, row in enumerate(samples):
        assert len(row) == n_src
        for q, (x, y, p) in enumerate(row):
            i = q * n + s
            pix[i] = (sb[0] + q % (sb[2] - sb[0]), sb[1] + q // (sb[2] - sb[0])); pfilm[i] = (x, y); prim[i] = p
    return dict(pix=pix, pfilm=pfilm, prim=prim, n=n)


# ---- the scenes of test_matte.py -------------------------------------------------------------------------------------------------------------------------------------

def _content(b):
    """Several materials over the ground plane: four materials, a sphere, a disk and a raised quad among them."""
    b.material("matte", Kd=(0.7, 0.45, 0.2), sigma=0.0)
    b.trianglemesh(GROUND_P, GROUND_I)
    b.attribute_begin(); b.material("plastic", Kd=(0.2, 0.3, 0.7)); b.translate(-1.2, 0.6, 0.4); b.sphere(radius=0.6); b.attribute_end()
    b.attribute_begin(); b.material("mirror", Kr=(0.9, 0.9, 0.9)); b.translate(1.1, 0.5, 1.2); b.sphere(radius=0.5); b.attribute_end()
    b.attribute_begin(); b.material("matte", Kd=(0.1, 0.8, 0.1)); b.translate(0.2, 0.3, -0.8)
    b.trianglemesh(np.array([(-0.8, 0.0, -0.8), (-0.8, 0.0, 0.8), (0.8, 0.0, 0.8), (0.8, 0.0, -0.8)], F), GROUND_I); b.attribute_end()
    return b


def materials_scene(pkg, sampler="sobol", lensradius=0.0, crop=None):
    """Case 1. crop: the 32 x 24 film as the middle of a 64 x 48 frame (case 2: under a wide filter the sample bounds exceed the film)."""
    if crop:
        b = _builder(pkg, sampler=sampler, lensradius=lensradius, xres=2 * XRES, yres=2 * YRES, spp=SPP)
        b.film.update(crop=(0.25, 0.75, 0.25, 0.75))
        # (world_begin() has been called: the film's options are read at world_end())
    else:
        b = _builder(pkg, sampler=sampler, lensradius=lensradius, xres=XRES, yres=YRES, spp=SPP)
    return _content(b).world_end()


def orthographic_scene(pkg):
    """Case 9: case 1's content under camera_model's orthographic job, looking straight down (a 32 x 24 crop of a 64 x 32 frame)."""
    import camera_model
    return _content(camera_model.job(pkg, "orthographic", view="down")).world_end()


def overflow_scene(pkg, n):
    """Case 3: the ground as n x n flat quads. Returns (sd, rp, groups): every quad of the left half (x < 0) is a group of its own, the right half one group (0)."""
    b = _builder(pkg, xres=XRES, yres=YRES, spp=SPP)
    b.material("matte", Kd=(0.5, 0.5, 0.5), sigma=0.0)
    P, I, _ = undulating_mesh(n, amplitude=0.0)
    b.trianglemesh(P, I)
    sd, rp = b.world_end()
    quad = np.arange(2 * n * n) % (n * n)   # (undulating_mesh: the quads' first triangles, then their second ones)
    groups = np.where(quad % n < n // 2, 1 + quad, 0).astype(np.uint32)
    return sd, rp, groups


def instance_scene(pkg):
    """Case 4: one object -- a sphere on a small quad -- instanced at x = -1.6 and x = +1.6, beside the top-level ground. Returns (sd, rp, the object's primitives)."""
    b = _builder(pkg, xres=XRES, yres=YRES, spp=SPP)
    b.material("matte", Kd=(0.5, 0.5, 0.5), sigma=0.0)
    b.trianglemesh(GROUND_P, GROUND_I)
    b.object_begin("thing")
    b.material("plastic", Kd=(0.7, 0.2, 0.2))
    first = b.trianglemesh(np.array([(-0.7, 0.2, -0.7), (-0.7, 0.2, 0.7), (0.7, 0.2, 0.7), (0.7, 0.2, -0.7)], F), GROUND_I)
    b.translate(0.0, 0.8, 0.0); b.sphere(radius=0.6)
    b.object_end()
    for x in (-1.6, 1.6):
        b.attribute_begin(); b.translate(x, 0.0, 0.0); b.object_instance("thing"); b.attribute_end()
    sd, rp = b.world_end()
    return sd, rp, np.arange(first, first + 3)


def shell_scene(pkg, shell):
    """Case 5: the single-material ground; shell: a sphere without a material stands over it, wholly inside the ground's silhouette."""
    b = _builder(pkg, xres=XRES, yres=YRES, spp=SPP)
    b.material("matte", Kd=(0.5, 0.5, 0.5), sigma=0.0)
    b.trianglemesh(GROUND_P, GROUND_I)
    if shell:
        b.attribute_begin(); b.material("none"); b.translate(0.0, 0.65, 1.8); b.sphere(radius=0.6); b.attribute_end()
    return b.world_end()


_CACHE = {}


def reference(pkg, oracle, key, sd, rp, groups=None, instance_of=None, hits=None, layers=LAYERS):
    """(camera hits, surface, ids, tables, contributions) of the whole job by the model, fed by the oracle's hits; computed once per `key` and left unchanged.
    instance_of(h) -> the instance id per sample; hits(pkg, oracle, orc, rp) -> camera hits (default: aov_reference.camera_hits)."""
    if key not in _CACHE:
        from aov_reference import camera_hits
        orc = oracle.scene(sd)
        h = (hits or camera_hits)(pkg, oracle, orc, rp)
        orc.close()
        surface, ids = sample_ids(sd, h, groups, None if instance_of is None else instance_of(h))
        tables = empty_tables(rp, layers)
        count = add_samples(rp, h, surface, ids, tables)
        for t in tables.values(): t.setflags(write=False)
        _CACHE[key] = (h, surface, ids, tables, count)
    return _CACHE[key]
