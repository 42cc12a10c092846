#!/usr/bin/env python3
"""bake_light.py -- bake the direct lighting of a UV-mapped shape of a .pbrt scene into its UV atlas: an irradiance lightmap (libmi355bake.so, include/mi355bake.h "Lightmap").

    tools/bake_light.py scene.pbrt --shape N [--shape M ...] --size W[xH] --spp S [--nsamples K] [--lights i,j,...] [--dilate D] --out light.pfm

--shape: the ordinal of a Shape directive in file order (the front end's prim_group); every triangle of the named shapes is a bake target, the whole scene occludes.
--lights: indices of the scene's lights in file order (area lights: one per emissive primitive); default all. --nsamples: light samples per sample, default one per
selected light; spp x nsamples must be a multiple of the number of selected lights. The map is pt_bake_light_resolve's irradiance (RGB, the surface's albedo not applied),
dilated by --dilate rings (pt_bake_dilate) so that bilinear lookups at island borders find values. Row y of the file is row y of the atlas: v = 0 first.
The format follows the file name's extension (pfm, exr, png, tga). Prints one JSON line with the owned texels, the rays and the ms per launch kind."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bake_ao import parse_size   # noqa: E402


def bake_file(pkg, lib, path, shapes, size, spp, nsamples=None, lights=None, dilate=0, sampler="sobol", profile=False):
    """(irradiance (H, W, 3), reached (H, W), owner (H, W), scene, kernel statistics, counters) of the shapes `shapes` of the scene file `path`."""
    import numpy as np
    fs = pkg.frontend.FrontScene(path=path)
    scene = pkg.Scene(lib, fs)
    w, h = size
    _, _, n_sel = scene.bake_light_select(lights)
    nsamples = n_sel if nsamples is None else nsamples
    planes = scene.bake_light(list(shapes), w, h, spp, nsamples=nsamples, lights=lights, sampler=sampler, planes=("owner", "light_w"), profile=profile)
    stats, counters = scene.kernel_stats(), scene.counters()
    irradiance, reached = pkg.runtime.resolve_lightmap(planes["light_w"], spp, nsamples)
    if dilate > 0:
        irradiance = scene.bake_dilate(planes["owner"], irradiance, dilate)
    return np.ascontiguousarray(irradiance), reached, planes["owner"], scene, stats, counters


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("scene")
    ap.add_argument("--shape", type=int, action="append", required=True)
    ap.add_argument("--size", type=parse_size, default=(1024, 1024))
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--nsamples", type=int, default=None)
    ap.add_argument("--lights", type=lambda t: [int(v) for v in t.split(",")], default=None)
    ap.add_argument("--dilate", type=int, default=0)
    ap.add_argument("--sampler", choices=("sobol", "halton"), default="sobol")
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    from _pkg import import_pkg
    pkg = import_pkg()
    lib = pkg.load_library()
    lib.init(0)
    irradiance, reached, owner, scene, stats, counters = bake_file(pkg, lib, a.scene, a.shape, a.size, a.spp, a.nsamples, a.lights, a.dilate, a.sampler, profile=True)
    pkg.frontend.write_image(a.out, irradiance)
    print(json.dumps(dict(out=a.out, width=a.size[0], height=a.size[1], owned_texels=int((owner != pkg._abi.PT_NONE).sum()), rays=counters["shadow_tests"],
                          ms={s["name"]: round(s["total_ms"], 4) for s in stats if s["launches"]})))
    return 0


if __name__ == "__main__":
    sys.exit(main())
