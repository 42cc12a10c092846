#!/usr/bin/env python3
"""bake_ao.py -- bake the ambient occlusion (and the bent normals) of a UV-mapped shape of a .pbrt scene into its UV atlas (libmi355bake.so, include/mi355bake.h).

    tools/bake_ao.py scene.pbrt --shape N [--shape M ...] --size W[xH] --spp S --nsamples K [--dilate D] --out ao.pfm [--bent bent.pfm]

--shape: the ordinal of a Shape directive in file order (the front end's prim_group); every triangle of the named shapes is a bake target, the whole scene occludes.
The AO map is pt_bake_resolve's (1 = open), written to all three channels; the bent-normal map holds the unit vectors as they are (not packed to [0, 1]). Both are
dilated by --dilate rings (pt_bake_dilate) so that bilinear lookups at island borders find values. Row y of the file is row y of the atlas: v = 0 first.
The format follows the file name's extension (pfm, exr, png, tga). Prints one JSON line with the owned texels, the rays and the ms per launch kind."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_size(text):
    w, _, h = text.lower().partition("x")
    return int(w), int(h or w)


def bake_file(pkg, lib, path, shapes, size, spp, nsamples, dilate=0, cos_sample=True, max_distance=float("inf"), sampler="sobol", profile=False):
    """(ao (H, W), bent (H, W, 3), owner (H, W), scene) of the shapes `shapes` of the scene file `path`."""
    import numpy as np
    fs = pkg.frontend.FrontScene(path=path)
    scene = pkg.Scene(lib, fs)
    w, h = size
    planes = scene.bake(list(shapes), w, h, spp, nsamples=nsamples, cos_sample=cos_sample, max_distance=max_distance, sampler=sampler, planes=("owner", "ao_w"), profile=profile)
    stats, counters = scene.kernel_stats(), scene.counters()
    ao, bent = pkg.runtime.resolve_bake(planes["ao_w"], spp)
    if dilate > 0:
        ao = scene.bake_dilate(planes["owner"], ao, dilate)
        bent = scene.bake_dilate(planes["owner"], bent, dilate)
    return np.ascontiguousarray(ao), np.ascontiguousarray(bent), planes["owner"], scene, stats, counters


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("scene")
    ap.add_argument("--shape", type=int, action="append", required=True)
    ap.add_argument("--size", type=parse_size, default=(1024, 1024))
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--nsamples", type=int, default=64)
    ap.add_argument("--dilate", type=int, default=0)
    ap.add_argument("--max-distance", type=float, default=float("inf"))
    ap.add_argument("--sampler", choices=("sobol", "halton"), default="sobol")
    ap.add_argument("--uniform", action="store_true", help="uniform-sphere directions instead of cosine-weighted ones (ao.rs cossample false)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--bent", default=None)
    a = ap.parse_args(argv)
    import numpy as np
    from _pkg import import_pkg
    pkg = import_pkg()
    lib = pkg.load_library()
    lib.init(0)
    ao, bent, owner, scene, stats, counters = bake_file(pkg, lib, a.scene, a.shape, a.size, a.spp, a.nsamples, a.dilate, not a.uniform, a.max_distance, a.sampler, profile=True)
    pkg.frontend.write_image(a.out, np.repeat(ao[..., None], 3, axis=2))
    if a.bent:
        pkg.frontend.write_image(a.bent, bent)
    print(json.dumps(dict(out=a.out, bent=a.bent, width=a.size[0], height=a.size[1], owned_texels=int((owner != pkg._abi.PT_NONE).sum()), rays=counters["shadow_tests"],
                          ms={s["name"]: round(s["total_ms"], 4) for s in stats if s["launches"]})))
    return 0


if __name__ == "__main__":
    sys.exit(main())
