"""The device's subsurface code -- dev_bssrdf.h: catmull_rom_weights, sample_catmull_rom_2d, invert_catmull_rom, subsurface_from_diffuse,
DevBssrdf::{init_medium, init_disney, init_frame, sr, sample_sr, pdf_sr, pdf_sp, probe_segment} and BssrdfAdapterBsdf -- against the CPU oracle, CALL BY CALL. Renders reach
it with one (u1, u2) per subsurface vertex, one exit point per probe chain, one adapter sample and a material or two with ordinary coefficients: never a rho on the table's
first or last node, a channel with sigma_t = 0, a radius on a table node, u1 on the edge between two axes or channels, an exit point at po, a frame that is not orthonormal.

tests/device_probe/bssrdf_probe.hip is test code beside the other three probes (tests/probe_build.py builds the four once per session): one thread per query, the material
index read per thread from memory, on the material table and the BSSRDF tables of a pt_scene that libmi355pt.so created. It builds the DevBssrdf in the two forms the render
builds it in -- at the entry point as k_shade does, at the exit point as k_bssrdf rebuilds it from the stored frame and coefficients -- and refuses (status 4) unless the two
give the same bits for every word of the state. Materials, frames and queries: tests/bssrdf_zoo.py; what holds of the oracle alone, against float64: tests/test_bssrdf_zoo.py.

  a. for every material x frame x section, in both forms: every field of probe_bssrdf == orc_bssrdf_eval (oracle/ref_kats.cpp) BIT FOR BIT, as test_device_probe.assert_same_bits
     has it: every NaN is one pattern, signed zeros and infinities count as themselves. A failure names the section, the field, how many queries differ, the first one and the
     structured families that differ. bssrdf_zoo.FIELDS_LEFT_OUT is empty: no field is left out.
  b. the live shares of the random queries have floors (bssrdf_zoo.check_floors): a comparison must compare something.
  c. a material without a BSSRDF is status 2 on both sides; pt_scene_create refuses the DisneyBSSRDF with d = 0 in a channel, which the oracle alone answers.
  d. query counts 1, 255, 256, 257; refusals leave the output untouched."""
import ctypes as C
import os

import numpy as np
import pytest
from bssrdf_zoo import (DEVICE_REFUSES, F, FIELDS, FIELDS_LEFT_OUT, FLOOR_EXCEPTIONS, FLOORS, FRAMES, MATERIALS, N_RANDOM, NO_BSSRDF, RAGGED_MATERIAL, SECTION_INDEX, WORDS_IN,
                        WORDS_OUT, case, check_floors, field)
from probe_build import probe_library
from test_device_probe import assert_same_bits

pytestmark = pytest.mark.gpu

if os.environ.get("PT_LIB_PATH"):   # a kernel-variant library: its pt_scene layout may differ from the one the probe is compiled against
    pytest.skip("PT_LIB_PATH names a variant library; the probe reads pt_scene of the tree's own headers", allow_module_level=True)

FORMS = {0: "entry form (k_shade)", 1: "exit form (k_bssrdf)"}


@pytest.fixture(scope="module")
def probe(pkg, gpu):
    return probe_library(pkg)


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def device_section(probe, scene, mi, section, form, frames, q=None, n=None):
    """probe_bssrdf: one section's (n, words) uint32 answers."""
    if section == "state":
        n, qq = 1, None
    else:
        n = len(q) if n is None else n
        qq = np.ascontiguousarray(q[:n], F).reshape(n, WORDS_IN[section])
    out = np.zeros((n, WORDS_OUT[section]), np.uint32)
    st = probe.probe_bssrdf(scene.h, mi, SECTION_INDEX[section], form, _fp(np.ascontiguousarray(frames, F)), n, _fp(qq), out.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert st != 4, f"{section}: the entry form and the exit form of the DevBssrdf differ in a word of the state"
    assert st == 0, f"probe_bssrdf {section} form {form}: status {st}"
    return out


def compare_section(dev, ref, section, tags, what):
    for name in FIELDS[section]:
        if name in FIELDS_LEFT_OUT: continue
        assert_same_bits(field(dev, section, name), field(ref, section, name), f"{what}: section {section}, field {name}, device vs oracle", tags)


@pytest.mark.parametrize("name", [n for n in MATERIALS if n not in NO_BSSRDF and n not in DEVICE_REFUSES])
def test_bssrdf_calls_match_the_oracle(pkg, gpu, oracle, probe, name):
    c = case(pkg, oracle, name)
    assert c["has"]
    shares = check_floors(name, c)
    fl = FLOOR_EXCEPTIONS.get(name, FLOORS)
    scene = pkg.Scene(gpu, c["sd"])
    try:
        for fname, fc in c["frames"].items():
            print(f"\n{name} {fname}: live shares of the random queries " + ", ".join(f"{k} {v:.3f} (floor {fl[k]})" for k, v in shares[fname].items()))
            for form in FORMS:
                what = f"{name}, frame {fname}, {FORMS[form]}"
                state = device_section(probe, scene, c["mi"], "state", form, fc["frames"])
                compare_section(state, fc["state_words"], "state", None, what)
                for section, qs in fc["sets"].items():
                    dev = device_section(probe, scene, c["mi"], section, form, fc["frames"], qs["q"])
                    if form == 0: print(f"{name} {fname} {section}: {len(dev)} queries compared ({qs['random']} random, {len(dev) - qs['random']} structured), both forms")
                    compare_section(dev, fc["ref"][section], section, qs["tag"], what)
    finally:
        scene.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_bssrdf_probe_with_a_ragged_last_block(pkg, gpu, oracle, probe, n):
    c = case(pkg, oracle, RAGGED_MATERIAL)
    fc = c["frames"]["tilted"]
    scene = pkg.Scene(gpu, c["sd"])
    try:
        for section, qs in fc["sets"].items():
            rows = np.concatenate([np.arange(0, N_RANDOM, 32), np.arange(N_RANDOM, len(qs["q"]))])[:n]   # random and structured queries
            assert len(rows) == n
            dev = device_section(probe, scene, c["mi"], section, 1, fc["frames"], np.ascontiguousarray(qs["q"][rows]))
            assert dev.shape == (n, WORDS_OUT[section])
            print(f"\n{RAGGED_MATERIAL} tilted {section}: {n} queries compared")
            compare_section(dev, fc["ref"][section][rows], section, qs["tag"][rows], f"{RAGGED_MATERIAL} n={n}")
    finally:
        scene.close()


def test_bssrdf_probe_refuses_without_touching_the_output(pkg, gpu, oracle, probe):
    c = case(pkg, oracle, RAGGED_MATERIAL)
    fc = c["frames"]["canonical"]
    q = np.ascontiguousarray(fc["sets"]["radii"]["q"][:4]); fr = np.ascontiguousarray(fc["frames"], F)
    out = np.full((4, 19), 0xA5A5A5A5, np.uint32); op = out.ctypes.data_as(C.POINTER(C.c_uint32))
    R, S, CV = SECTION_INDEX["radii"], SECTION_INDEX["state"], SECTION_INDEX["conversion"]
    scene = pkg.Scene(gpu, c["sd"])
    try:
        sd = c["sd"]
        assert probe.probe_bssrdf(None, c["mi"], R, 0, _fp(fr), 4, _fp(q), op) == 1                  # null pointers
        assert probe.probe_bssrdf(scene.h, c["mi"], R, 0, None, 4, _fp(q), op) == 1
        assert probe.probe_bssrdf(scene.h, c["mi"], R, 0, _fp(fr), 4, None, op) == 1
        assert probe.probe_bssrdf(scene.h, c["mi"], R, 0, _fp(fr), 4, _fp(q), None) == 1
        assert probe.probe_bssrdf(scene.h, c["mi"], R, 0, _fp(fr), 0, _fp(q), op) == 1               # no query
        assert probe.probe_bssrdf(scene.h, c["mi"], R, 0, _fp(fr), (1 << 20) + 1, _fp(q), op) == 1
        assert probe.probe_bssrdf(scene.h, sd.n_materials, R, 0, _fp(fr), 4, _fp(q), op) == 1        # material index out of range
        assert probe.probe_bssrdf(scene.h, 0xFFFFFFFF, R, 0, _fp(fr), 4, _fp(q), op) == 1
        assert probe.probe_bssrdf(scene.h, c["mi"], len(SECTION_INDEX), 0, _fp(fr), 4, _fp(q), op) == 1   # an unknown section, an unknown form
        assert probe.probe_bssrdf(scene.h, c["mi"], -1, 0, _fp(fr), 4, _fp(q), op) == 1
        assert probe.probe_bssrdf(scene.h, c["mi"], R, 2, _fp(fr), 4, _fp(q), op) == 1
        assert probe.probe_bssrdf(scene.h, c["mi"], S, 0, _fp(fr), 4, None, op) == 1                 # the state is one query
        assert probe.probe_bssrdf(scene.h, 0, R, 0, _fp(fr), 4, _fp(q), op) == 2                     # material 0, the builder's default matte: no BSSRDF
        assert (out == 0xA5A5A5A5).all()   # nothing ran
        assert probe.probe_bssrdf(scene.h, c["mi"], R, 0, _fp(fr), 4, _fp(q), op) == 0
        assert not (out.ravel()[:4 * WORDS_OUT["radii"]] == 0xA5A5A5A5).any() and (out.ravel()[4 * WORDS_OUT["radii"]:] == 0xA5A5A5A5).all()   # 4 x 6 words, no more
    finally:
        scene.close()
    out[:] = 0xA5A5A5A5
    d = case(pkg, oracle, "disney_scatter")
    scene = pkg.Scene(gpu, d["sd"])
    try:   # the conversion answers only for a tabulated material
        q6 = np.ascontiguousarray(c["frames"]["canonical"]["sets"]["conversion"]["q"][:4])
        assert probe.probe_bssrdf(scene.h, d["mi"], CV, 0, _fp(fr), 4, _fp(q6), op) == 1
        assert (out == 0xA5A5A5A5).all()
    finally:
        scene.close()


@pytest.mark.parametrize("name", NO_BSSRDF)
def test_materials_without_a_bssrdf_are_status_2_on_both_sides(pkg, gpu, oracle, probe, name):
    c = case(pkg, oracle, name)
    assert not c["has"]   # orc_bssrdf_eval: status 2
    out = np.full((1, 19), 0xA5A5A5A5, np.uint32)
    scene = pkg.Scene(gpu, c["sd"])
    try:
        for form in FORMS:
            assert probe.probe_bssrdf(scene.h, c["mi"], SECTION_INDEX["state"], form, _fp(np.ascontiguousarray(FRAMES["canonical"], F)), 1, None, out.ctypes.data_as(C.POINTER(C.c_uint32))) == 2
        assert (out == 0xA5A5A5A5).all()
    finally:
        scene.close()


@pytest.mark.parametrize("name", DEVICE_REFUSES)
def test_scene_creation_refuses_a_zero_scatter_distance(pkg, gpu, oracle, name):
    """The oracle answers a DisneyBSSRDF with d = 0 in a channel (tests/test_bssrdf_zoo.py); the device never meets one: pt_scene_create refuses it."""
    c = case(pkg, oracle, name)
    assert c["has"]
    with pytest.raises(Exception, match="scatterdistance"):
        pkg.Scene(gpu, c["sd"]).close()
