"""The kernel symbol behind every launch kind, and the host scheduler's per-call state.

pt_get_kernel_stats reports, per launch kind ("trace", "route", "shade_metal", ...), the symbol of the kernel instantiation the host launched, as
rocprofv3 prints it. The symbol is a key: bench.py looks a kernel's PMC traffic record up by it and infers the node size from the trace symbol's last
argument. The host picks each instantiation from run-time conditions (geometry kinds, textures, integrator, sampler, walk), so a symbol that no longer
names the launched instantiation would attach another kernel's counters to the headline without any film changing.

Part 1 pins the whole {launch kind: symbol} map of one tiny render per variant axis. The literals were recorded from the library of the commit before
the host driver took launch and name from one variant table; they are not taken from the code under test.
Part 2: the lobe-set kernels in a TEXTURED scene -- metal, plastic-like and uber classes with textured parameters, one texture black.
Part 3: the wavefront-iteration cap (PT_TEST_MAX_ITERATIONS) is read per pt_render call, also by the replicas' threads of pt_multi_render."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT, trace_env
from parity import assert_same_film, assert_same_render

pytestmark = pytest.mark.gpu


def _volpath(b):
    b.integ.update(kind="volpath")
    return b


def _halton(b):
    b.sampler = "halton"
    return b


def _lazy_grid(pkg, b):
    sd, rp = b.world_end()
    rp.light_strategy = pkg._abi.PT_LS_SPATIAL_LAZY
    return sd, rp


# one tiny render per variant axis: name -> (scene description, render parameters)
SCENES = {
    "material_zoo": lambda pkg: pkg.scenes.material_zoo(n=16, xres=96, yres=64, spp=4).world_end(),                 # shade mode 0, nine classes
    "spheres_c1": lambda pkg: pkg.scenes.spheres_c1(xres=64, yres=64, spp=4).world_end(),                           # trace mode 1, k_film_final<true>
    "instanced_garden": lambda pkg: pkg.scenes.instanced_garden(xres=64, yres=48, spp=4).world_end(),               # trace mode 3
    "alpha_foliage": lambda pkg: pkg.scenes.alpha_foliage(xres=64, yres=48, spp=4).world_end(),                     # trace mode 2
    "textured": lambda pkg: pkg.scenes.textured(xres=64, yres=48, spp=4).world_end(),                               # shade mode 2
    "subsurface_c5": lambda pkg: pkg.scenes.subsurface_c5(n=16, xres=64, yres=48, spp=4).world_end(),               # probe launch, k_bssrdf, class 10
    "foggy_room": lambda pkg: _volpath(pkg.scenes.foggy_room(xres=64, yres=48, spp=4)).world_end(),                 # shade mode 3, k_medium_route
    "shell_media": lambda pkg: _volpath(pkg.scenes.shell_media(xres=64, yres=48, spp=4)).world_end(),               # ... and stage B
    "emissive_field": lambda pkg: _lazy_grid(pkg, pkg.scenes.emissive_field(n_lights=2000)),                        # k_light_touch
    "ganesha_halton": lambda pkg: _halton(pkg.scenes.ganesha_scale(n=24, xres=64, yres=48, spp=4)).world_end(),     # shade mode 1 without spheres
}

# {launch kind: symbol} of each, recorded from the parent commit's library in the production walk; the two-wide (exact) walk differs in k_trace's last argument only (_expected)
EXPECTED = {
    "alpha_foliage": {
        "extend_camera": "k_trace<0, 2, false, 1>", "film": "k_film_final<true>", "film_finish": "k_film_finish", "generate": "k_generate",
        "light_grid": "k_light_grid_contrib", "route": "k_route<6, 2048>", "shade_matte": "k_shade<1, 2, 1>", "trace": "k_trace<2, 2, false, 1>"},
    "emissive_field": {
        "extend_camera": "k_trace<0, 0, false, 1>", "film": "k_film_final<false>", "film_finish": "k_film_finish", "generate": "k_generate",
        "light_grid": "k_light_grid_contrib", "light_touch": "k_light_touch<false>", "route": "k_route<6, 2048>", "shade_matte": "k_shade<1, 0, 1>",
        "shade_plastic": "k_shade<2, 0, 4>", "trace": "k_trace<2, 0, false, 1>"},
    "foggy_room": {
        "extend_camera": "k_trace<0, 1, false, 1>", "film": "k_film", "film_finish": "k_film_finish", "generate": "k_generate", "light_grid": "k_light_grid_contrib",
        "route": "k_medium_route", "shade_1lobe": "k_shade<1, 3, 0>", "shade_2lobe": "k_shade<2, 3, 0>", "shade_matte": "k_shade<1, 3, 1>",
        "shade_medium": "k_shade_medium", "shade_miss": "k_shade_miss<true, true>", "trace": "k_trace<2, 1, false, 1>"},
    "ganesha_halton": {
        "extend_camera": "k_trace<0, 0, false, 1>", "film": "k_film_final<false>", "film_finish": "k_film_finish", "generate": "k_generate",
        "light_grid": "k_light_grid_contrib", "route": "k_route<6, 2048>", "shade_matte": "k_shade<1, 1, 1>", "trace": "k_trace<2, 0, false, 1>"},
    "instanced_garden": {
        "extend_camera": "k_trace<0, 3, false, 1>", "film": "k_film_final<true>", "film_finish": "k_film_finish", "generate": "k_generate",
        "light_grid": "k_light_grid_contrib", "route": "k_route<6, 2048>", "shade_matte": "k_shade<1, 1, 1>", "shade_plastic": "k_shade<2, 1, 4>",
        "trace": "k_trace<2, 3, false, 1>"},
    "material_zoo": {
        "extend_camera": "k_trace<0, 0, false, 1>", "film": "k_film_final<false>", "film_finish": "k_film_finish", "generate": "k_generate",
        "light_grid": "k_light_grid_contrib", "route": "k_route<12, 1024>", "shade_1lobe": "k_shade<1, 0, 0>", "shade_2lobe": "k_shade<2, 0, 0>",
        "shade_matte": "k_shade<1, 0, 1>", "shade_metal": "k_shade<1, 0, 3>", "shade_plastic": "k_shade<2, 0, 4>", "shade_specular": "k_shade<1, 0, 2>",
        "shade_uber": "k_shade<5, 0, 5>", "trace": "k_trace<2, 0, false, 1>"},
    "shell_media": {
        "extend": "k_trace<0, 1, false, 1>", "extend_camera": "k_trace<0, 1, false, 1>", "film": "k_film", "film_finish": "k_film_finish", "generate": "k_generate",
        "light_grid": "k_light_grid_contrib", "route": "k_medium_route", "shade_1lobe": "k_shade<1, 3, 0>", "shade_2lobe": "k_shade<2, 3, 0>",
        "shade_matte": "k_shade<1, 3, 1>", "shade_medium": "k_shade_medium", "shade_miss": "k_shade_miss<true, true>", "trace": "k_trace<2, 1, false, 1>"},
    "spheres_c1": {
        "extend_camera": "k_trace<0, 1, false, 1>", "film": "k_film_final<true>", "film_finish": "k_film_finish", "generate": "k_generate",
        "light_grid": "k_light_grid_contrib", "route": "k_route<6, 2048>", "shade_matte": "k_shade<1, 1, 1>", "shade_plastic": "k_shade<2, 1, 4>",
        "shade_specular": "k_shade<1, 1, 2>", "trace": "k_trace<2, 1, false, 1>"},
    "subsurface_c5": {
        "bssrdf": "k_bssrdf<true, false>", "extend_camera": "k_trace<0, 1, false, 1>", "extend_probe": "k_trace<0, 1, true, 1>", "film": "k_film_final<true>",
        "film_finish": "k_film_finish", "generate": "k_generate", "light_grid": "k_light_grid_contrib", "route": "k_route<6, 2048>", "shade_matte": "k_shade<1, 1, 1>",
        "shade_sss": "k_shade<1, 1, 6>", "trace": "k_trace<2, 1, false, 1>"},
    "textured": {
        "extend_camera": "k_trace<0, 1, false, 1>", "film": "k_film_final<true>", "film_finish": "k_film_finish", "generate": "k_generate",
        "light_grid": "k_light_grid_contrib", "route": "k_route<6, 2048>", "shade_matte": "k_shade<1, 2, 1>", "shade_plastic": "k_shade<2, 2, 4>",
        "trace": "k_trace<2, 1, false, 1>"},
}


def symbol_map(scene):
    return {s["name"]: s["kernel"] for s in scene.kernel_stats() if s["launches"] > 0}


def _expected(name, trace_mode):
    want = dict(EXPECTED[name])
    if trace_mode == "exact":   # pt_set_trace_exact(1): QUADK 0, whatever the production walk's was
        want = {k: (v[:v.rindex(",")] + ", 0>" if v.startswith("k_trace<") else v) for k, v in want.items()}
    return want


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_launch_kind_reports_the_symbol_it_always_did(pkg, gpu, trace_mode, name):
    sd, rp = SCENES[name](pkg)
    g = pkg.Scene(gpu, sd)
    g.render(rp)
    got = symbol_map(g)
    print(name, trace_mode, got)
    assert got == _expected(name, trace_mode)


def textured_lobe_sets(pkg):
    """A metal, a plastic and an uber ball, every one with textured parameters, over a textured matte floor. The uber's Kd is black everywhere (an image
    scaled by zero), the plastic's and the uber's Ks is a checkerboard with black squares: lobes the reference drops per vertex (plastic.rs / uber.rs:
    `if !kd.is_black()`), inside kernels whose lobe SET was fixed per material."""
    S = pkg.scenes
    b = S.SceneBuilder()
    b.film.update(xres=64, yres=48); b.spp = 4; b.integ.update(maxdepth=5)
    b.look_at((0.0, 1.6, 6.5), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0)); b.camera(fov=40.0)
    b.world_begin()
    b.light_source("infinite", L=(0.3, 0.35, 0.4))
    b.attribute_begin(); b.area_light_source(L=(22.0, 20.0, 17.0))
    P, I = S.quad((-1.5, 4.5, -1.0), (1.5, 4.5, -1.0), (1.5, 4.5, 1.5), (-1.5, 4.5, 1.5)); b.trianglemesh(P, I); b.attribute_end()
    b.texture("img", "color", "imagemap", pixels=S.test_image(), gamma=True, uscale=3.0, vscale=3.0)
    b.texture("black", "color", "scale", tex1="img", tex2=(0.0, 0.0, 0.0))
    b.texture("check", "color", "checkerboard", uscale=6.0, vscale=6.0, tex1=(0.7, 0.6, 0.2), tex2=(0.0, 0.0, 0.0))
    b.texture("rough", "float", "checkerboard", uscale=4.0, vscale=4.0, tex1=0.05, tex2=0.3)
    b.texture("ktex", "color", "checkerboard", uscale=5.0, vscale=5.0, tex1=(3.9, 2.45, 2.14), tex2=(2.0, 2.0, 2.5))
    b.material("matte", Kd="check")
    P, I = S.quad((-8.0, -1.0, -8.0), (-8.0, -1.0, 8.0), (8.0, -1.0, 8.0), (8.0, -1.0, -8.0))
    b.trianglemesh(P, I, UV=np.array([[0, 0], [0, 1], [1, 1], [1, 0]], dtype=np.float32))
    b.attribute_begin(); b.material("metal", k="ktex", roughness="rough"); b.translate(-2.2, 0.0, 0.0); b.sphere(radius=1.0); b.attribute_end()
    b.attribute_begin(); b.material("plastic", Kd="img", Ks="check", roughness="rough"); b.translate(0.0, 0.0, 0.3); b.sphere(radius=1.0); b.attribute_end()
    b.attribute_begin(); b.material("uber", Kd="black", Ks="check", Kr=(0.2, 0.2, 0.2), roughness=0.1); b.translate(2.2, 0.0, 0.0)
    P, I, N = S.displaced_sphere(12, with_normals=True); b.trianglemesh(P, I, N=N); b.attribute_end()
    return b


def test_textured_lobe_set_classes_run_their_specialised_kernels_and_change_nothing(pkg, gpu, oracle, tmp_path):
    sd, rp = textured_lobe_sets(pkg).world_end()
    g = pkg.Scene(gpu, sd); orc = oracle.scene(sd)
    film, ref = g.render(rp), orc.render(rp, nthreads=4)
    st = symbol_map(g)
    print(st)
    assert st["shade_metal"] == "k_shade<1, 2, 3>" and st["shade_plastic"] == "k_shade<2, 2, 4>" and st["shade_uber"] == "k_shade<5, 2, 5>", st
    items = {s["name"]: s["items"] for s in g.kernel_stats() if s["launches"]}
    assert all(items[k] > 0 for k in ("shade_metal", "shade_plastic", "shade_uber", "shade_matte")), items
    assert_same_render(film, ref, g.counters(), orc.counters(), rtol=3e-6, atol=1e-6)
    code = r"""
import sys, numpy as np
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from _pkg import import_pkg
pkg = import_pkg()
import torch
torch.cuda.init()
from test_kernel_symbols import textured_lobe_sets, symbol_map
lib = pkg.load_library(); lib.init(0)
sd, rp = textured_lobe_sets(pkg).world_end()
g = pkg.Scene(lib, sd); film = g.render(rp)
ks = symbol_map(g)
assert ks["shade_1lobe"] == "k_shade<1, 2, 0>" and ks["shade_2lobe"] == "k_shade<2, 2, 0>" and ks["shade_manylobe"] == "k_shade<5, 2, 0>" and "shade_metal" not in ks, ks
np.save({out!r}, film)
""".format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=str(tmp_path / "general.npy"))
    r = subprocess.run([sys.executable, "-c", code], env=trace_env(dict(os.environ, PT_SHADE_SPECIALISE="0")), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert_same_film(film, np.load(tmp_path / "general.npy"))


def test_the_iteration_cap_is_read_per_call_by_every_replica(pkg, gpu):
    """Two replicas on one device render on a host thread each. With PT_TEST_MAX_ITERATIONS=1 around the call both passes are abandoned and pt_multi_render
    returns PT_ERR_PROBE_CHAIN (a status the library produces by design); with the variable gone the next call on the same handles renders the single-device film."""
    A = pkg._abi
    sd, rp = _volpath(pkg.scenes.foggy_room(xres=32, yres=32, spp=2)).world_end()
    single = pkg.Scene(gpu, sd)
    ref = single.render(rp)
    multi = pkg.MultiScene(gpu, sd, [0, 0])
    film = np.zeros_like(ref)
    os.environ["PT_TEST_MAX_ITERATIONS"] = "1"
    try:
        st = gpu.lib.pt_multi_render(multi.h, C.byref(rp), film.ctypes.data_as(C.c_void_p), 0)
        msg = gpu.lib.pt_last_error().decode(errors="replace")
    finally:
        del os.environ["PT_TEST_MAX_ITERATIONS"]
    assert st == A.PT_ERR_PROBE_CHAIN and "1 wavefront iterations" in msg, (st, msg)
    again = multi.render(rp)
    assert_same_render(again, ref, multi.counters(), single.counters())
