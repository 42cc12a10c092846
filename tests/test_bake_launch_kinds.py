"""The launch kinds of the bake library's calls: which kernel every kind launched, and how often.

pt_get_kernel_stats reports per launch kind ("bake_rays", "bake_light_accum", "bake_probe", ...) the symbol of the kernel the host launched and the number of
launches. The four bakes and their four probes are built from one call frame (bake/bake_render.hip: selection, owner map, planes, pass loop, chunk loop, the
<true> / <false> launch pair): a frame that skipped a step, ran a pass twice or picked the other instantiation would leave planes that other tests may or may not
catch, and a kind map that differs. This pins {launch kind: (kernel symbol, launches)} of one call of each, in the manner of tests/test_kernel_symbols.py part 1.

The literals were recorded on the MI355X from the library of the commit before the call frame existed, when every entry point still wrote its steps out; they
are not taken from the code under test. Shapes: a 20 x 12 atlas (its 8 x 8 tiles hang over both edges), 3 samples of which the range (1, 2) is baked, 65 elements
per sample (two chunks, which forces one sample per pass) and then 4 elements with two samples per pass (a pass of several samples in one chunk); 70 SH points (a
partial second wave) in rows of 9 under two of the scene's three lights, 66 and then 4 elements. Once without and once with a sphere and instances in the scene,
so that both SPH instantiations launch."""
import numpy as np
import pytest
import lightmap_scenes as LS

pytestmark = pytest.mark.gpu

W, H, SPP, RANGE = 20, 12, 3, (1, 2)
SCENES = {"triangles": "open_floor", "sphere": "occluded_floor"}   # under a point light and a two-triangle quad light: three lights
QUERY = dict(texel=[0, 125, 239], sample=[0, 1, 2], element=[0, 3, 2])


def sh_points():
    """70 points on a 10 x 7 grid low above the floor, off every light's plane."""
    i = np.arange(70)
    return np.stack([-1.7 + 0.35 * (i % 10) + 0.013, -1.4 + 0.4 * (i // 10) + 0.007, 0.12 + 0.05 * (i % 3)], axis=1).astype(np.float32)


def kinds(scene):
    return {s["name"]: (s["kernel"], s["launches"]) for s in scene.kernel_stats() if s["launches"] > 0}


def calls(pkg, gpu, name):
    """{call: its kind map} of the twelve calls on the scene `name`."""
    sd, shape = LS.scene(pkg, SCENES[name], "point_quad")
    sc, src = pkg.Scene(gpu, sd), pkg.Scene(gpu, sd)
    pts = sh_points()
    got = {}
    for tag, ns, sh_ns, per_pass in (("two_chunks", 65, 66, 0), ("one_chunk", 4, 4, 2)):
        sc.bake(shape, W, H, SPP, nsamples=ns, samples=RANGE, spp_per_pass=per_pass); got["bake " + tag] = kinds(sc)
        sc.bake_light(shape, W, H, SPP, nsamples=ns, samples=RANGE, spp_per_pass=per_pass); got["light " + tag] = kinds(sc)
        sc.bake_transfer(src, shape, W, H, 0.3, 0.3, spp=SPP, nsamples=ns, samples=RANGE, spp_per_pass=per_pass); got["transfer " + tag] = kinds(src)
        sc.bake_sh(pts, SPP, nsamples=sh_ns, lights=[0, 1], row=9, samples=RANGE, spp_per_pass=per_pass); got["sh " + tag] = kinds(sc)
    q = QUERY
    sc.bake_rays(shape, W, H, SPP, q["texel"], q["sample"], q["element"], nsamples=4); got["bake probe"] = kinds(sc)
    sc.bake_light_rays(shape, W, H, SPP, q["texel"], q["sample"], q["element"], nsamples=4); got["light probe"] = kinds(sc)
    sc.bake_transfer_rays(src, shape, W, H, 0.3, 0.3, SPP, q["texel"], q["sample"], q["element"], nsamples=4); got["transfer probe"] = kinds(src)
    sc.bake_sh_rays(pts, SPP, [0, 69, 64], q["sample"], q["element"], nsamples=4, lights=[0, 1], row=9); got["sh probe"] = kinds(sc)
    return got


# {scene: {call: {launch kind: (symbol, launches)}}} in the production walk; the two-wide (exact) walk differs in k_trace's last argument only (_expected)
_ATLAS = {"bake_select": ("ptbake::k_bake_check", 1), "bake_raster": ("ptbake::k_bake_raster", 1)}
_PLANES = dict(_ATLAS, bake_points=("ptbake::k_bake_points", 1))
_PROJECT = dict(_ATLAS, bake_select=("ptbake::k_bake_top", 2), bake_project=("ptbake::k_bake_project", 1), bake_transfer_points=("ptbake::k_bake_transfer_points", 1))
EXPECTED = {
    "sphere": {
        "bake two_chunks": dict(_PLANES, bake_rays=("ptbake::k_bake_rays", 4), shadow=("k_trace<1, 2, false, 1>", 4), bake_accum=("ptbake::k_bake_accum", 4)),
        "bake one_chunk": dict(_PLANES, bake_rays=("ptbake::k_bake_rays", 1), shadow=("k_trace<1, 2, false, 1>", 1), bake_accum=("ptbake::k_bake_accum", 1)),
        "bake probe": dict(_ATLAS, bake_probe=("ptbake::k_bake_probe", 1)),
        "light two_chunks": dict(_PLANES, bake_light_rays=("ptbake::k_bake_light_rays<true>", 4), shadow=("k_trace<1, 2, false, 1>", 4), bake_light_accum=("ptbake::k_bake_light_accum", 4)),
        "light one_chunk": dict(_PLANES, bake_light_rays=("ptbake::k_bake_light_rays<true>", 1), shadow=("k_trace<1, 2, false, 1>", 1), bake_light_accum=("ptbake::k_bake_light_accum", 1)),
        "light probe": dict(_ATLAS, bake_probe=("ptbake::k_bake_light_probe<true>", 1)),
        "transfer two_chunks": dict(_PROJECT, extend=("k_trace<0, 2, false, 1>", 1), bake_transfer_rays=("ptbake::k_bake_transfer_rays", 4), shadow=("k_trace<1, 2, false, 1>", 4),
                                    bake_accum=("ptbake::k_bake_accum", 4)),
        "transfer one_chunk": dict(_PROJECT, extend=("k_trace<0, 2, false, 1>", 1), bake_transfer_rays=("ptbake::k_bake_transfer_rays", 1), shadow=("k_trace<1, 2, false, 1>", 1),
                                   bake_accum=("ptbake::k_bake_accum", 1)),
        "transfer probe": dict(_PROJECT, extend=("k_trace<0, 2, false, 1>", 1), bake_probe=("ptbake::k_bake_transfer_probe", 1)),
        "sh two_chunks": {"bake_sh_rays": ("ptbake::k_bake_sh_rays<true>", 4), "shadow": ("k_trace<1, 2, false, 1>", 4), "bake_sh_accum": ("ptbake::k_bake_sh_accum", 4)},
        "sh one_chunk": {"bake_sh_rays": ("ptbake::k_bake_sh_rays<true>", 1), "shadow": ("k_trace<1, 2, false, 1>", 1), "bake_sh_accum": ("ptbake::k_bake_sh_accum", 1)},
        "sh probe": {"bake_probe": ("ptbake::k_bake_sh_probe<true>", 1)},
    },
    "triangles": {
        "bake two_chunks": dict(_PLANES, bake_rays=("ptbake::k_bake_rays", 4), shadow=("k_trace<1, 0, false, 1>", 4), bake_accum=("ptbake::k_bake_accum", 4)),
        "bake one_chunk": dict(_PLANES, bake_rays=("ptbake::k_bake_rays", 1), shadow=("k_trace<1, 0, false, 1>", 1), bake_accum=("ptbake::k_bake_accum", 1)),
        "bake probe": dict(_ATLAS, bake_probe=("ptbake::k_bake_probe", 1)),
        "light two_chunks": dict(_PLANES, bake_light_rays=("ptbake::k_bake_light_rays<false>", 4), shadow=("k_trace<1, 0, false, 1>", 4), bake_light_accum=("ptbake::k_bake_light_accum", 4)),
        "light one_chunk": dict(_PLANES, bake_light_rays=("ptbake::k_bake_light_rays<false>", 1), shadow=("k_trace<1, 0, false, 1>", 1), bake_light_accum=("ptbake::k_bake_light_accum", 1)),
        "light probe": dict(_ATLAS, bake_probe=("ptbake::k_bake_light_probe<false>", 1)),
        "transfer two_chunks": dict(_PROJECT, extend=("k_trace<0, 0, false, 1>", 1), bake_transfer_rays=("ptbake::k_bake_transfer_rays", 4), shadow=("k_trace<1, 0, false, 1>", 4),
                                    bake_accum=("ptbake::k_bake_accum", 4)),
        "transfer one_chunk": dict(_PROJECT, extend=("k_trace<0, 0, false, 1>", 1), bake_transfer_rays=("ptbake::k_bake_transfer_rays", 1), shadow=("k_trace<1, 0, false, 1>", 1),
                                   bake_accum=("ptbake::k_bake_accum", 1)),
        "transfer probe": dict(_PROJECT, extend=("k_trace<0, 0, false, 1>", 1), bake_probe=("ptbake::k_bake_transfer_probe", 1)),
        "sh two_chunks": {"bake_sh_rays": ("ptbake::k_bake_sh_rays<false>", 4), "shadow": ("k_trace<1, 0, false, 1>", 4), "bake_sh_accum": ("ptbake::k_bake_sh_accum", 4)},
        "sh one_chunk": {"bake_sh_rays": ("ptbake::k_bake_sh_rays<false>", 1), "shadow": ("k_trace<1, 0, false, 1>", 1), "bake_sh_accum": ("ptbake::k_bake_sh_accum", 1)},
        "sh probe": {"bake_probe": ("ptbake::k_bake_sh_probe<false>", 1)},
    },
}


def _expected(name, trace_mode):
    def symbol(v):
        return v[:v.rindex(",")] + ", 0>" if trace_mode == "exact" and v.startswith("k_trace<") else v
    return {call: {kind: (symbol(k), n) for kind, (k, n) in want.items()} for call, want in EXPECTED[name].items()}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_bake_call_launches_the_kinds_and_kernels_it_always_did(pkg, gpu, trace_mode, name):
    got = calls(pkg, gpu, name)
    print(name, trace_mode, got)
    assert got == _expected(name, trace_mode)
