#!/usr/bin/env python3
"""ao_bench.py -- throughput of the ambient-occlusion integrator (libmi355ao.so, include/mi355ao.h) on the C2 scene.

Renders ganesha_scale() at full size (1920x1080, 4.3 M triangles) with Integrator "ambientocclusion" (nsamples 64, cossample) at a few
spp into a device film and prints one JSON line: Msamples/s (camera samples), AO rays/s, and the AO any-hit launch ("shadow")
average ms by HIP events (pt_get_kernel_stats), next to the per-ray cost of C2's path-tracing trace launch from the committed record
profiles/r6/final/kernel_stats_spp256.csv (whose shadow rays share the mixed k_trace<2, ..> launch with the continuation rays).
Scene generation, BVH build and upload are outside the timed region. `--out FILE` also writes the line to FILE."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def c2_trace_record():
    """C2's mixed trace launch (continuation + MIS + shadow rays of one wavefront iteration) from the committed record: ns per ray."""
    final = os.path.join(ROOT, "profiles", "r6", "final")
    rows = [r for r in csv.DictReader(open(os.path.join(final, "kernel_stats_spp256.csv"))) if r["Name"].startswith("void k_trace<2,")]
    kinds = json.load(open(os.path.join(final, "stats_bench.json")))["trace_kinds"]
    rays = sum(v["Mrays_per_step"] for v in kinds.values()) * 1e6
    total_ns = float(rows[0]["TotalDurationNs"])
    return dict(source="profiles/r6/final/kernel_stats_spp256.csv + stats_bench.json", kernel=rows[0]["Name"], calls=int(rows[0]["Calls"]),
                total_ms=total_ns / 1e6, rays=rays, ns_per_ray=total_ns / rays, shadow_nodes_per_ray=kinds["shadow"]["nodes_per_ray"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--nsamples", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from _pkg import import_pkg
    pkg = import_pkg()
    lib = pkg.load_library(); lib.init(0)
    b = pkg.scenes.ganesha_scale(spp=a.spp)
    b.integ.update(kind="ao", nsamples=a.nsamples, cossample=True)
    sd, rp = b.world_end()
    sc = pkg.Scene(lib, sd)
    cb = rp.cropped_pixel_bounds
    film = torch.zeros((cb[3] - cb[1], cb[2] - cb[0], 4), dtype=torch.float32, device="cuda:0")
    for _ in range(a.warmup):
        sc.render(rp, device_ptr=film.data_ptr())
    walls = []
    for _ in range(a.steps):
        t0 = time.perf_counter(); sc.render(rp, device_ptr=film.data_ptr()); walls.append(time.perf_counter() - t0)
    c = sc.counters()
    rp.profile = 1
    sc.render(rp, device_ptr=film.data_ptr())
    ks = {s["name"]: s for s in sc.kernel_stats()}
    wall = min(walls)
    sh = ks.get("shadow", {})
    line = dict(metric="ao_msamples_per_s", config="C2 ganesha_scale 1920x1080, ambientocclusion nsamples %d cossample" % a.nsamples, spp=a.spp,
                pass_spp=sc.ao_pass_size(rp), value=c["camera_rays"] / wall / 1e6, wall_s=wall, ao_rays_per_s=c["shadow_tests"] / wall,
                camera_rays=c["camera_rays"], ao_rays=c["shadow_tests"], camera_hits_fraction=c["shadow_tests"] / a.nsamples / max(1, c["camera_rays"]),
                ao_launches=sh.get("launches", 0), ao_launch_avg_ms=(sh.get("total_ms", 0.0) / sh["launches"]) if sh.get("launches") else None,
                ao_ns_per_ray=(sh.get("total_ms", 0.0) * 1e6 / c["shadow_tests"]) if c["shadow_tests"] else None, ao_kernel=sh.get("kernel"),
                kernel_stats={k: dict(launches=v["launches"], total_ms=round(v["total_ms"], 3), kernel=v["kernel"]) for k, v in ks.items()},
                c2_path_trace_record=c2_trace_record(), device=torch.cuda.get_device_name(0))
    s = json.dumps(line)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
