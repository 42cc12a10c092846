#!/usr/bin/env python3
"""bake_sh.py -- bake the direct lighting of a .pbrt scene at a grid of free points into order-2 spherical harmonics: light probes (libmi355bake.so, include/mi355bake.h "SH points").

    tools/bake_sh.py scene.pbrt --grid NX,NY,NZ [--bounds x0,y0,z0,x1,y1,z1] --spp S [--nsamples K] [--lights i,j,...] --out probes.npz

--grid: the number of cells along x, y and z; a point sits at every cell's centre, x fastest, then y, then z. --bounds: the box the grid divides; default the bounds of
the scene's mesh vertices; write a box that begins with a minus sign as --bounds=-1,-1,0,1,1,2. --lights: indices of the scene's lights in file order (area lights: one per emissive primitive); default all. --nsamples: light samples per
sample, default one per selected light; spp x nsamples must be a multiple of the number of selected lights. Keep the points off the lights themselves.
The .npz holds `points` (n, 3), `sh` (n, 9, 3) = pt_bake_sh_resolve's coefficients of the incident radiance per colour channel (evaluate with runtime.sh_irradiance or
pt_bake_sh_irradiance) and `reached` (n,). Prints one JSON line with the points, the rays and the ms per launch kind."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def grid_points(grid, bounds):
    """The cell centres (n, 3) float32 of `grid` = (nx, ny, nz) cells over `bounds` = (x0, y0, z0, x1, y1, z1), x fastest."""
    import numpy as np
    lo, hi = np.asarray(bounds[:3], np.float64), np.asarray(bounds[3:], np.float64)
    axes = [lo[a] + (np.arange(grid[a]) + 0.5) / grid[a] * (hi[a] - lo[a]) for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x, y, z], axis=-1).reshape(-1, 3), dtype=np.float32)


def scene_bounds(scene):
    """The bounds of the scene's mesh vertices (x0, y0, z0, x1, y1, z1)."""
    import numpy as np
    d = scene.data.desc()
    if d.n_vertices == 0:
        raise SystemExit("bake_sh: the scene has no mesh vertices: give --bounds")
    P = np.ctypeslib.as_array(d.P, shape=(d.n_vertices, 3))
    return tuple(P.min(axis=0)) + tuple(P.max(axis=0))


def bake_file(pkg, lib, path, grid, bounds, spp, nsamples=None, lights=None, sampler="sobol", profile=False):
    """(points (n, 3), sh (n, 9, 3), reached (n,), scene, kernel statistics, counters) of the grid `grid` over `bounds` (None: the vertices') of the scene file `path`."""
    fs = pkg.frontend.FrontScene(path=path)
    scene = pkg.Scene(lib, fs)
    points = grid_points(grid, scene_bounds(scene) if bounds is None else bounds)
    _, _, n_sel = scene.bake_light_select(lights)
    nsamples = n_sel if nsamples is None else nsamples
    sh_w = scene.bake_sh(points, spp, nsamples=nsamples, lights=lights, sampler=sampler, profile=profile)
    stats, counters = scene.kernel_stats(), scene.counters()
    sh, reached = pkg.runtime.resolve_sh(sh_w, spp, nsamples)
    return points, sh, reached, scene, stats, counters


def numbers(kind, count):
    """argparse type: `count` comma-separated values of type `kind`."""
    def parse(text):
        values = text.split(",")
        if len(values) != count:
            raise argparse.ArgumentTypeError(f"{count} comma-separated values expected")
        return tuple(kind(v) for v in values)
    return parse


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("scene")
    ap.add_argument("--grid", type=numbers(int, 3), required=True)
    ap.add_argument("--bounds", type=numbers(float, 6), default=None)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--nsamples", type=int, default=None)
    ap.add_argument("--lights", type=lambda t: [int(v) for v in t.split(",")], default=None)
    ap.add_argument("--sampler", choices=("sobol", "halton"), default="sobol")
    ap.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    if min(a.grid) < 1:
        ap.error("--grid: every count must be >= 1")
    import numpy as np
    from _pkg import import_pkg
    pkg = import_pkg()
    lib = pkg.load_library()
    lib.init(0)
    points, sh, reached, scene, stats, counters = bake_file(pkg, lib, a.scene, a.grid, a.bounds, a.spp, a.nsamples, a.lights, a.sampler, profile=True)
    with open(a.out, "wb") as f:   # (np.savez would append .npz to a name without it)
        np.savez(f, points=points, sh=sh, reached=reached)
    print(json.dumps(dict(out=a.out, points=len(points), grid=list(a.grid), rays=counters["shadow_tests"], ms={s["name"]: round(s["total_ms"], 4) for s in stats if s["launches"]})))
    return 0


if __name__ == "__main__":
    sys.exit(main())
