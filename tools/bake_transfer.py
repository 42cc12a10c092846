#!/usr/bin/env python3
"""bake_transfer.py -- bake a detailed scene's normals, height and ambient occlusion into the UV atlas of a low-polygon shape (libmi355bake.so, include/mi355bake.h "Transfer").

    tools/bake_transfer.py low.pbrt high.pbrt --shape N [--shape M ...] --size W[xH] --front F --back B [--spp S --nsamples K --dilate D]
                           [--normal n.pfm] [--height h.pfm] [--ao ao.pfm]

low.pbrt holds the UV-mapped mesh: --shape is the ordinal of a Shape directive there in file order (the front end's prim_group). high.pbrt is what gets projected: per
texel one ray from F above the low mesh's surface, along its shading normal, to B below it. --normal: the tangent-space normal map, n * 0.5 + 0.5, flat (0.5, 0.5, 1) where
no triangle of the scene's own meshes was hit; --height: front - t of the hit in all three channels, 0 without one; --ao: pt_bake_resolve's map of the AO at the hit (1 =
open; traced only when asked for). The maps are dilated by --dilate rings (pt_bake_dilate) before the normal map is encoded: the height from the texels with a hit, the
normal and the AO from those whose hit has a normal (a sphere, a disk or an instanced object leaves a height only). Row y of a file is row y of the atlas: v = 0 first. The format follows the file name's extension (pfm, exr, png, tga). Prints one JSON line with the owned texels, the hits, the AO rays and the ms per launch kind."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_size(text):
    w, _, h = text.lower().partition("x")
    return int(w), int(h or w)


def transfer_files(pkg, lib, low, high, shapes, size, front, back, spp=1, nsamples=64, dilate=0, want_ao=True, cos_sample=True, max_distance=float("inf"), sampler="sobol", profile=False):
    """dict(normal (H, W, 3) encoded, height (H, W), ao (H, W) or None, planes: what Scene.bake_transfer returned, stats, counters) of the scene file `high` projected
    onto the shapes `shapes` of the scene file `low`."""
    import numpy as np
    target = pkg.Scene(lib, pkg.frontend.FrontScene(path=low))
    source = pkg.Scene(lib, pkg.frontend.FrontScene(path=high))
    w, h = size
    wanted = ("owner", "hit_prim", "height", "tangent_normal") + (("ao_w",) if want_ao else ())
    planes = target.bake_transfer(source, list(shapes), w, h, front, back, spp=spp, nsamples=nsamples, cos_sample=cos_sample, max_distance=max_distance, sampler=sampler, planes=wanted,
                                  profile=profile)
    stats, counters = source.kernel_stats(), source.counters()
    tn, height = planes["tangent_normal"], planes["height"]
    # (a hit on a sphere, a disk or an instance has a height and no normal: the normal map is covered where a detail hit left a unit vector)
    detail = np.where((tn != 0).any(axis=-1), planes["hit_prim"], np.uint32(pkg._abi.PT_NONE)).astype(np.uint32)
    covered = detail != pkg._abi.PT_NONE
    ao = pkg.runtime.resolve_bake(planes["ao_w"], spp)[0] if want_ao else None
    if dilate > 0:
        tn, height = source.bake_dilate(detail, tn, dilate), source.bake_dilate(planes["hit_prim"], height, dilate)
        if want_ao:
            ao = source.bake_dilate(detail, ao, dilate)
        covered = source.bake_dilate(detail, covered.astype(np.float32), dilate) > 0
    return dict(normal=pkg.runtime.encode_normal_map(tn, covered), height=np.ascontiguousarray(height), ao=ao, planes=planes, stats=stats, counters=counters)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("low")
    ap.add_argument("high")
    ap.add_argument("--shape", type=int, action="append", required=True)
    ap.add_argument("--size", type=parse_size, default=(1024, 1024))
    ap.add_argument("--front", type=float, required=True)
    ap.add_argument("--back", type=float, required=True)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--nsamples", type=int, default=16)
    ap.add_argument("--dilate", type=int, default=0)
    ap.add_argument("--max-distance", type=float, default=float("inf"))
    ap.add_argument("--sampler", choices=("sobol", "halton"), default="sobol")
    ap.add_argument("--uniform", action="store_true", help="uniform-sphere AO directions instead of cosine-weighted ones (ao.rs cossample false)")
    ap.add_argument("--normal", default=None)
    ap.add_argument("--height", default=None)
    ap.add_argument("--ao", default=None)
    a = ap.parse_args(argv)
    if not (a.normal or a.height or a.ao):
        ap.error("nothing to write: give --normal, --height or --ao")
    import numpy as np
    from _pkg import import_pkg
    pkg = import_pkg()
    lib = pkg.load_library()
    lib.init(0)
    r = transfer_files(pkg, lib, a.low, a.high, a.shape, a.size, a.front, a.back, a.spp, a.nsamples, a.dilate, a.ao is not None, not a.uniform, a.max_distance, a.sampler, profile=True)
    if a.normal:
        pkg.frontend.write_image(a.normal, r["normal"])
    if a.height:
        pkg.frontend.write_image(a.height, np.repeat(r["height"][..., None], 3, axis=2))
    if a.ao:
        pkg.frontend.write_image(a.ao, np.repeat(r["ao"][..., None], 3, axis=2))
    none = pkg._abi.PT_NONE
    print(json.dumps(dict(normal=a.normal, height=a.height, ao=a.ao, width=a.size[0], height_px=a.size[1], owned_texels=int((r["planes"]["owner"] != none).sum()),
                          hits=int((r["planes"]["hit_prim"] != none).sum()), rays=r["counters"]["shadow_tests"], ms={s["name"]: round(s["total_ms"], 4) for s in r["stats"] if s["launches"]})))
    return 0


if __name__ == "__main__":
    sys.exit(main())
