#!/usr/bin/env python3
"""bench.py -- headline benchmark of the hot path (BASELINE.json: Msamples/s at 1920x1080).

A "step" is one full render (pt_render / pt_multi_render) of the named workload. Default: S2 / config C2, the Ganesha-scale
synthetic scene (4,298,312-triangle displaced sphere, matte, quad area light + constant environment),
1920x1080 x 256 spp, PathIntegrator maxdepth 5, Sobol sampler, box filter, spatial light sampling.
`--config C3|C4|C5` selects the other BASELINE configs built to SURVEY 8(d)'s S3 / S4 / S5 specification
(pbrt-rust_amd/scenes.py: country_kitchen_s3, ecosystem_s4, dragon_s5) at their named spp (override: --spp).
A plain run does what `value` needs and nothing more: it builds the scene, runs the warm-up and the timed steps, writes --dump-outputs and
prints the JSON line (roofline and per-kernel figures in it come from the timed steps' own HIP events and the committed PMC record, not from runs
of their own). `--full` adds the side measurements after the timed region: the CPU baseline (cpu_baseline), the film read-back
(film_readback_ms, value_with_readback) and, for the default C2 run on one GPU, the 8-rank scaling projection (scaling_projection) and
one render each of C3 / C4 / C5 (one pass of the pass size) under "other_configs", so every BASELINE config has a number on the record.
Scene generation, BVH build and upload are outside the timed region. The film stays on the device
(pt_render's film_is_device path): the 33 MB read-back of SURVEY 8(d)'s definition (0.6 ms over PCIe) is not in `value`;
for N > 1 the film merge is inside the timed region.

N > 1, two launch forms on the same kernels and the same tile shards (16x16 sample tiles of integrator.rs:276-283 round-robin,
every shard renders all spp of its tiles into a device film, the films are summed onto the first GPU; total work is fixed, so
scaling is "strong"):
  * under a launcher (WORLD_SIZE set: `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N`): one process per
    GPU, the merge is one dist.reduce (backend nccl == RCCL over xGMI);
  * plain `python bench.py --gpus N` (no WORLD_SIZE): ONE process drives devices 0..N-1 through pt_multi_render, the C ABI's own
    multi-device path (the reference is one process too: integrator.rs:294-296), the merge is N-1 concurrent peer copies + one sum
    kernel. The line then carries per-device busy ms and the merge ms. `--devices 0,0,...` repeats ordinals (replicas share a GPU).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from code_hash import code_hash   # noqa: E402  (hash of the device library's sources: does a committed PMC record still belong to this tree?)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (~6.3 TB/s achievable)
GATHER_CEILING_GREQ_S = 54.0  # profiles/r2_gather_calibration.json: dependent random 64-byte gathers, 128-byte fabric requests per ns, whole chip
TRACE_KINDS = ("trace", "extend", "extend_mis", "shadow", "extend_camera", "extend_probe")   # "trace" = the mixed launch: continuation + MIS + shadow rays of one wavefront iteration
OTHER_CONFIG_SPP = {"C3": 1024, "C4": -1, "C5": -1}   # one step each after the headline: C3 (a 1-GPU config in BASELINE.json) as its WHOLE job (1024 spp = four passes); C4 / C5 (8-GPU configs) ONE pass of the size the library picks at their named spp (-1: asked of the library, pt_pass_size)
                                                     # (so the rate is the named-spp rate and the committed PMC profile applies): C3 1.4 s, C4 5.6 s, C5 0.4 s of render per step


def algo_bytes(name, s):
    """ALGORITHMIC bytes of a launch kind: trace kernels 128 B per four-wide BVH record fetched (32 B per reference node
    visited in the exact walk) + 48 B per shape packet tested + 44 B per ray (pid 4, ray 24, hit record 16); shade kernels count their
    path-state / mesh / queue quads in-kernel."""
    if name in TRACE_KINDS:
        # production traversal (kernel symbol k_trace<.., 1> / <.., 2>): the node counter counts four-wide records fetched, 128 B each; the exact walk
        # (pt_set_trace_exact, k_trace<.., 0>) counts the reference's node visits, 32 B each
        node_bytes = 32 if str(s.get("kernel", "")).rstrip().endswith(", 0>") else 128
        return node_bytes * s["bvh_nodes"] + 48 * s["triangle_tests"] + 44 * s["items"]
    if name.startswith("shade_") or name == "bssrdf":
        return s["bvh_nodes"]
    return None


_TRAFFIC = {}


def traffic_record(config, kernel, eff_spp_per_pass, workload_key):
    """(record, code_match) of profiles/pmc_traffic.json for one kernel symbol of one config at this pass size, or (None, None). The byte counts are a
    property of the CODE that was profiled: code_match says whether the committed record was taken from these sources (tools/code_hash.py)."""
    if "data" not in _TRAFFIC:
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        try:
            _TRAFFIC["data"] = json.load(open(tpath)) if os.path.exists(tpath) else {}
        except Exception:
            _TRAFFIC["data"] = {}
        _TRAFFIC["hash"] = code_hash(ROOT)
    r = _TRAFFIC["data"].get(config, {}).get(kernel)
    if r and r.get("spp_per_pass") == eff_spp_per_pass and r.get("workload") == workload_key:
        return r, r.get("code_hash") == _TRAFFIC["hash"]
    return None, None


def build_roofline(kstats, config, eff_spp_per_pass, workload_key):
    """Dominant kernel = the kernel symbol (what rocprofv3 --stats reports) with the largest HIP-event time in the timed region.

    `achieved` is ALGORITHMIC bytes / launch time: cache-inclusive, most of those bytes are served by L1 / L2, so against the HBM peak it
    is NOT bounded by 1 (`algorithmic_over_hbm_peak`). `frac` is the fabric-side byte rate of the same kernel (L2 misses, counted by
    request size, + writes; profiles/pmc_traffic.json, collected by tools/profile_gpu.sh in separate --pmc passes) over the HBM peak:
    Infinity-Cache hits are included in those bytes, so it is an upper bound on the DRAM rate and a true fraction. It is null when
    no committed PMC record matches this kernel / config / pass size. The byte counts come from the committed profile, only the
    launch time is measured in this run."""
    groups = {}
    for n, v in kstats.items():
        ab = algo_bytes(n, v)
        if ab is None or v["launches"] == 0:
            continue
        g = groups.setdefault(v["kernel"] or n, dict(ms=0.0, launches=0, bytes=0, kinds=[]))
        g["ms"] += v["total_ms"]; g["launches"] += v["launches"]; g["bytes"] += ab; g["kinds"].append(n)
    if not groups:
        return None
    name, g = max(groups.items(), key=lambda kv: kv[1]["ms"])
    avg_ms = g["ms"] / max(1, g["launches"])
    achieved = g["bytes"] / (g["ms"] * 1e-3) / 1e9
    rec, code_match = traffic_record(config, name, eff_spp_per_pass, workload_key)
    traffic = hbm_achieved = hbm_frac = l2_hit = gather_frac = valu_busy = None
    if rec:
        traffic, l2_hit = rec.get("hbm_bytes_per_launch"), rec.get("l2_hit_rate")
        valu_busy = rec.get("valu_busy_frac")
        if code_match:
            hbm_achieved = traffic / (avg_ms * 1e-3) / 1e9
            hbm_frac = hbm_achieved / HBM_PEAK_GBS
            rd = rec.get("rdreq", {}).get("TCC_EA0_RDREQ_sum")
            disp = rec.get("dispatches") or 1
            if rd:
                gather_frac = rd / disp / (avg_ms * 1e-3) / 1e9 / GATHER_CEILING_GREQ_S
    is_trace = any(k in TRACE_KINDS for k in g["kinds"])
    # `bound` names the limiter the committed counters of THIS kernel show (profiles/pmc_traffic.json, code-hash-gated), not the roof one would like to be measured
    # against: "hbm" when its fabric bytes run at >= 60 % of the HBM peak, "valu_issue" when vector instructions issue in >= 60 % of its SIMD cycles, "gather_latency"
    # when neither does (dependent gathers: the CU's line requests in flight x the loaded latency), "unknown" without a record taken from these sources.
    if not (rec and code_match):
        bound = "unknown"
    elif hbm_frac is not None and hbm_frac >= 0.6:
        bound = "hbm"
    elif valu_busy is not None and valu_busy >= 0.6:
        bound = "valu_issue"
    else:
        bound = "gather_latency"
    limiter = {"hbm": "fabric bytes at %s of the HBM peak" % (None if hbm_frac is None else round(hbm_frac, 3)),
               "valu_issue": "vector-instruction issue (valu_busy_frac %s) of a per-lane %s; fabric bytes at %s of the HBM peak, %s of the dependent-gather request ceiling"
                             % (valu_busy, "BVH walk" if is_trace else "shading loop", None if hbm_frac is None else round(hbm_frac, 3), None if gather_frac is None else round(gather_frac, 3)),
               "gather_latency": "neither bytes (%s of the HBM peak) nor vector issue (valu_busy_frac %s): scattered 32-128-byte gathers, bounded by the CU's 64 line requests in flight at "
                                 "the memory system's loaded latency (profiles/r4/tcp_counters_*.txt; DESIGN.md section 7)" % (None if hbm_frac is None else round(hbm_frac, 3), valu_busy),
               "unknown": "no committed counter record of this kernel from these sources (profiles/pmc_traffic.json: traffic_code_match)"}[bound]
    return dict(
        bound=bound, roof="hbm",   # `roof`: the roofline `achieved` / `peak` / `frac` / `traffic` are stated against (HBM, never MFMA -- no dense contraction on this path); `bound`: what the kernel's own counters show limits it
        kernel=name, launch_kinds=g["kinds"], unit="GB/s", peak=HBM_PEAK_GBS,
        achieved=round(achieved, 2),
        achieved_kind="ALGORITHMIC bytes / launch time (cache-inclusive: mostly L1/L2-served, can exceed the HBM peak)",
        algorithmic_over_hbm_peak=round(achieved / HBM_PEAK_GBS, 5),
        frac=None if hbm_frac is None else round(hbm_frac, 5),
        frac_kind="fabric-side bytes (L2 read misses by request size + writes; Infinity-Cache hits included, so an upper bound on DRAM bytes) / this run's launch time / 8 TB/s",
        hbm_achieved=None if hbm_achieved is None else round(hbm_achieved, 2), hbm_frac=None if hbm_frac is None else round(hbm_frac, 5),
        valu_busy_frac=valu_busy if code_match else None,
        valu_busy_kind="vector-instruction issue cycles / SIMD cycles of this kernel, SQ counters of the committed profile (4 cycles x SQ_INSTS_VALU / (1024 SIMDs x GRBM_GUI_ACTIVE per XCD))",
        traffic=traffic if code_match else None,
        traffic_code_match=code_match, traffic_code_hash=None if rec is None else rec.get("code_hash"), code_hash=code_hash(ROOT),
        traffic_source="committed profile profiles/pmc_traffic.json (rocprofv3 --pmc TCC_EA0_RDREQ_{128B,64B,32B}_sum + WRITE_SIZE, separate passes), not this run" if traffic else None,
        traffic_over_algorithmic=None if not (traffic and code_match) else round(traffic / (g["bytes"] / max(1, g["launches"])), 3),
        l2_hit_rate=l2_hit if code_match else None,
        frac_of_gather_ceiling=None if gather_frac is None else round(gather_frac, 4),
        gather_ceiling="fabric read requests per second of this kernel / 54 G/s, the measured chip-wide rate of dependent random 64-byte gathers (profiles/r2_gather_calibration.json)",
        limiter=limiter,
        launches=g["launches"], avg_launch_ms=round(avg_ms, 4),
        algorithmic_bytes_per_launch=int(g["bytes"] / max(1, g["launches"])))


def kernel_table(kstats, steps, config=None, eff_spp_per_pass=None, workload_key=None):
    def gbs(n, v):
        ab = algo_bytes(n, v)
        out = {} if ab is None else {"algo_GBs": round(ab / max(1e-9, v["total_ms"]) / 1e6, 1)}
        # fabric-side bytes of the kernel symbol from the committed PMC profile (code-hash-gated like roofline.frac) over THIS run's launch times: hbm_frac and,
        # where the kernel counts its algorithmic bytes, traffic_over_algorithmic (> 1: lines fetched for bytes nobody asked for)
        rec, match = traffic_record(config, v["kernel"], eff_spp_per_pass, workload_key) if config and v.get("kernel") else (None, None)
        if rec and match and rec.get("hbm_bytes_per_launch") and v["launches"] and v["total_ms"] > 0:
            fabric = rec["hbm_bytes_per_launch"] * v["launches"]
            out["hbm_frac"] = round(fabric / (v["total_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
            if ab:
                out["traffic_over_algorithmic"] = round(fabric / ab, 3)
            if rec.get("valu_busy_frac") is not None:
                out["valu_busy_frac"] = rec["valu_busy_frac"]
        return out
    kernels = {n: dict(ms=round(v["total_ms"] / steps, 3), launches=v["launches"] // steps, kernel=v["kernel"], **gbs(n, v),
                       **({"Mitems": round(v["items"] / steps / 1e6, 2), "ns_per_item": round(v["total_ms"] * 1e6 / v["items"], 3)} if v["items"] and n not in TRACE_KINDS else {}),
                       **({"Mrays_s": round(v["items"] / max(1e-9, v["total_ms"]) / 1e3, 1), "nodes_per_ray": round(v["bvh_nodes"] / max(1, v["items"]), 1)} if n in TRACE_KINDS else {}))
               for n, v in kstats.items() if v["launches"] and ":" not in n}
    # what the mixed traversal launches did per ray kind (counters only: the kinds share the launches' time)
    trace_kinds = {n.split(":", 1)[1]: dict(Mrays_per_step=round(v["items"] / steps / 1e6, 2), nodes_per_ray=round(v["bvh_nodes"] / max(1, v["items"]), 1), tris_per_ray=round(v["triangle_tests"] / max(1, v["items"]), 2))
                   for n, v in kstats.items() if n.startswith("trace:")}
    return kernels, trace_kinds


def accumulate(kstats, entries):
    for ks in entries:
        a = kstats.setdefault(ks["name"], dict(launches=0, total_ms=0.0, items=0, bvh_nodes=0, triangle_tests=0, kernel=ks.get("kernel", "")))
        for k in ("launches", "total_ms", "items", "bvh_nodes", "triangle_tests"):
            a[k] += ks[k]


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, film):
    """--dump-outputs: what pt_render hands its caller after the last timed step, the (H, W, 4) float32 film (XYZ sums + weight sum), as
    out_dir/film.npy. A film above DUMP_MAX_BYTES is written as a fixed sample instead: the rows (pixel index y * W + x, ascending) that a
    seed-0 generator picks, shape (n, 4), so two runs with the same arguments write the same pixels."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    if film.nbytes > DUMP_MAX_BYTES - 4096:   # (room for the .npy header)
        flat = film.reshape(-1, film.shape[-1])
        keep = np.sort(np.random.default_rng(0).choice(len(flat), (DUMP_MAX_BYTES - 4096) // flat[0].nbytes, replace=False))
        film = flat[keep]
    np.save(os.path.join(out_dir, "film.npy"), np.ascontiguousarray(film, dtype=np.float32))


def measure(pkg, lib, torch, dev, dist, args, config, spp, steps, warmup, devices, in_process, rank, world, want_cpu_baseline, proj_world=0):
    """Build the config's scene, run `warmup` untimed + `steps` timed renders, return the result dict (rank 0) or None."""
    builder_fn, named_spp, workload_desc = pkg.scenes.CONFIG_SCENES[config]
    one_pass = spp == -1    # one wavefront pass of the size the library picks for the whole job at the named spp
    spp = spp if spp > 0 else named_spp
    t_gen = time.time()
    kw = dict(xres=args.xres, yres=args.yres, spp=spp)
    if config in ("C2", "C5"):
        kw["n"] = args.mesh_n
    b = builder_fn(**kw)
    sd, rp = b.world_end()
    d = sd.desc()
    n_tris, n_inst = int(d.n_triangles), int(d.n_instances)
    t_gen = time.time() - t_gen
    t_up = time.time()
    scene = multi = None
    if in_process:
        multi = pkg.MultiScene(lib, sd, devices)   # scene replicated on every listed device, one host thread + stream each
    else:
        scene = pkg.Scene(lib, sd)                 # host SAH build + upload + packet build
    t_up = time.time() - t_up
    rp.tile_rank, rp.tile_world = rank, world
    if args.sim_world > 1 and world == 1:
        rp.tile_rank, rp.tile_world = args.sim_rank, args.sim_world
    rp.spp_per_pass = args.spp_per_pass
    if one_pass and scene is not None:
        spp = scene.pass_size(rp); rp.spp = spp
    rp.profile = int(os.environ.get("PT_BENCH_PROFILE", "1"))   # 1: HIP events around every launch, on the render stream; 2: + exact per-class launch sizes
    cb = rp.cropped_pixel_bounds
    W, H = cb[2] - cb[0], cb[3] - cb[1]
    film = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    pb = rp.pixel_bounds
    n_samples = (pb[2] - pb[0]) * (pb[3] - pb[1]) * spp

    host_staged = dist is not None and args.dist_backend == "gloo"   # rehearsal form (ranks may share one GPU): the film merge goes through host memory

    def step():
        film.zero_()
        torch.cuda.synchronize()
        if multi is not None:
            multi.render(rp, device_ptr=film.data_ptr())          # tiles % n_replicas, films summed onto the first device inside the call
        else:
            scene.render(rp, device_ptr=film.data_ptr())
        if dist is not None:
            if host_staged:
                h = film.cpu()
                dist.reduce(h, dst=0, op=dist.ReduceOp.SUM)
                if rank == 0:
                    film.copy_(h)
            else:
                dist.reduce(film, dst=0, op=dist.ReduceOp.SUM)    # merge_film_tile across ranks (RCCL over xGMI)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(warmup):
        step()
    barrier()
    nrep = len(devices) if multi is not None else 1
    kstats = {}
    rep_kernel_ms = [0.0] * nrep      # per replica: sum of its kernels' HIP-event times over the timed steps
    rep_render_ms = [0.0] * nrep      # per replica: wall time of its pt_render
    rep_copy_ms = [0.0] * nrep
    merge_ms = 0.0
    counters = None
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
        if multi is not None:
            for r in range(nrep):
                ks = multi.kernel_stats(r)
                rep_kernel_ms[r] += sum(k["total_ms"] for k in ks if ":" not in k["name"])
                accumulate(kstats, ks)
            tm = multi.timing()
            merge_ms += tm["merge_ms"]
            for r in range(nrep):
                rep_render_ms[r] += tm["render_ms"][r]; rep_copy_ms[r] += tm["copy_ms"][r]
            counters = multi.counters()
        else:
            ks = scene.kernel_stats()
            rep_kernel_ms[0] += sum(k["total_ms"] for k in ks if ":" not in k["name"])
            accumulate(kstats, ks)
            counters = scene.counters()
    barrier()
    elapsed = time.perf_counter() - t0
    busy_all = None
    if dist is not None:
        cdev = torch.device("cpu") if host_staged else dev
        t = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        busy = torch.tensor([rep_kernel_ms[0] / steps], dtype=torch.float64, device=cdev)
        gathered = [torch.zeros_like(busy) for _ in range(world)]
        dist.all_gather(gathered, busy)
        busy_all = [round(float(x.item()), 2) for x in gathered]
    if rank != 0:
        return None
    if args.dump_film and config == args.config:
        import numpy as np
        np.save(args.dump_film, film.cpu().numpy())
    if args.dump_outputs and config == args.config:
        dump_outputs(args.dump_outputs, film.cpu().numpy())

    # --full: SURVEY 8(d)'s definition of the metric includes the film read-back: timed apart (pinned host buffer, the 4 x f32 x W x H film of the last step)
    # and reported beside `value`, which stays the device-resident figure the contract asks for
    film_readback_ms = None
    if args.full:
        hostbuf = torch.empty((H, W, 4), dtype=torch.float32, pin_memory=True)
        torch.cuda.synchronize()
        t_rb = time.perf_counter()
        for _ in range(3):
            hostbuf.copy_(film, non_blocking=True)
            torch.cuda.synchronize()
        film_readback_ms = (time.perf_counter() - t_rb) / 3 * 1e3
        del hostbuf

    # strong-scaling projection as far as ONE device can tell: rank 0's shard of a `proj_world`-rank job (every proj_world-th 16x16 tile, all of the
    # config's NAMED spp) against full-frame time / proj_world. Fixed per-launch costs and the tail of each traversal launch do not shrink with the shard.
    projection = None
    if proj_world > 1 and scene is not None and world == 1 and args.sim_world <= 1:
        named = pkg.scenes.CONFIG_SCENES[config][1]
        save = (rp.tile_rank, rp.tile_world, rp.spp)
        rp.tile_rank, rp.tile_world, rp.spp = 0, proj_world, named
        try:
            if named * n_samples // spp <= 2 ** 31:   # short shards get a warm-up (workspace re-sized for the shard)
                film.zero_(); scene.render(rp, device_ptr=film.data_ptr())
            film.zero_(); torch.cuda.synchronize()
            t_s = time.perf_counter()
            scene.render(rp, device_ptr=film.data_ptr())
            torch.cuda.synchronize()
            shard_ms = (time.perf_counter() - t_s) * 1e3
            full_ms = elapsed / steps * 1e3 * named / spp   # the whole job on one device at the named spp (passes of this size back to back)
            projection = dict(world=proj_world, named_spp=named, full_job_ms_one_gpu=round(full_ms, 2), ideal_ms=round(full_ms / proj_world, 2), shard_ms=round(shard_ms, 2),
                              efficiency=round(full_ms / proj_world / shard_ms, 4), passes=[s_["launches"] for s_ in scene.kernel_stats() if s_["name"] == "generate"][0],
                              film_reduce="not included: one 33 MB reduce per render (~0.6 ms by construction, DESIGN.md section 5)")
        except Exception as e:
            projection = dict(error=f"{type(e).__name__}: {e}")
        rp.tile_rank, rp.tile_world, rp.spp = save

    eff_spp_per_pass = None   # what the library chose (0 = as many samples per pass as the free memory holds, up to 2^28 paths): from the number of k_generate launches
    if kstats.get("generate", {}).get("launches"):
        n_pass = max(1, kstats["generate"]["launches"] // (steps * nrep))
        eff_spp_per_pass = -(-spp // n_pass)
    n_gpus = len(set(devices)) if in_process else world
    value = n_samples * steps / elapsed / 1e6
    roofline = build_roofline(kstats, config, eff_spp_per_pass, [args.mesh_n, args.xres, args.yres]) if nrep == 1 or in_process else None
    if roofline and nrep > 1:
        roofline["note"] = f"launch times and bytes are summed over the {nrep} replicas (each renders 1/{nrep} of the tiles)"
    kernels, trace_kinds = kernel_table(kstats, steps, config, eff_spp_per_pass, [args.mesh_n, args.xres, args.yres])

    cpu_baseline = None
    if want_cpu_baseline and args.cpu_seconds > 0 and world == 1:
        cpu_baseline = run_cpu_baseline(pkg, sd, rp, spp, args)

    if args.dump_image and config == args.config:
        from tools.imgio import write_png
        write_png(args.dump_image, (scene or multi).resolve(film.cpu().numpy()))

    if n_gpus > 1 or nrep > 1:
        if in_process:
            par = (f"16x16 sample tiles round-robin over {nrep} replica(s) on {n_gpus} GPU(s) (devices {devices}); ONE process, pt_multi_render: one host thread + stream per "
                   "replica, film merge = concurrent hipMemcpyPeerAsync (one xGMI link per source, issued as each replica finishes) + one sum kernel on the first device; "
                   "no RCCL in this form (a single 33 MB reduction per render; the launcher form below uses RCCL)")
        else:
            par = f"16x16 sample tiles round-robin over {n_gpus} GPU(s); one process per GPU (torch.distributed), film merge = one RCCL reduce (dist.reduce SUM) onto rank 0"
    else:
        par = "1 GPU"
    multi_gpu = None
    if in_process:
        multi_gpu = dict(form="one process, pt_multi_render", devices=devices,
                         per_replica_kernel_busy_ms=[round(x / steps, 2) for x in rep_kernel_ms],
                         per_replica_render_wall_ms=[round(x / steps, 2) for x in rep_render_ms],
                         per_replica_peer_copy_ms=[round(x / steps, 3) for x in rep_copy_ms],
                         merge_ms=round(merge_ms / steps, 3), film_path_per_replica=multi.peer_access(),
                         merge_def="from the last replica's render end to the summed film on the first device (tail of the peer copies + the sum kernel)")
    elif busy_all is not None:
        multi_gpu = dict(form="one process per GPU, RCCL reduce", per_rank_kernel_busy_ms=busy_all)
    out = {
        "metric": "Msamples/s (camera rays x spp) at 1920x1080",
        "value": round(value, 3), "unit": "Msamples/s", "n_gpus": n_gpus, "steps": steps, "warmup": warmup,
        "ms_per_step": round(elapsed / steps * 1e3, 2), "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{config}: {workload_desc}; {n_tris} triangles" + (f", {n_inst} instances" if n_inst else "") +
                               f", {args.xres}x{args.yres}x{spp}spp, path maxdepth 5, sobol, box filter, spatial light sampling",
                   "name": config, "triangles": n_tris, "instances": n_inst, "spp": spp, "spp_per_pass": eff_spp_per_pass, "resolution": [args.xres, args.yres],
                   "film": "stays on the device (no read-back in the timed region; with --full, film_readback_ms / value_with_readback give SURVEY 8(d)'s read-back-inclusive figure)",
                   "parallelism": par},
        "code_hash": code_hash(ROOT),   # tools/code_hash.py: the device sources this line was measured on (tools/check_profiles.py holds committed records against it)
        **({"film_readback_ms": round(film_readback_ms, 3),
            "value_with_readback": round(n_samples / (elapsed / steps + film_readback_ms * 1e-3) / 1e6, 3)} if film_readback_ms is not None else {}),
        "roofline": roofline, "cpu_baseline": cpu_baseline,
        **({"scaling_projection": projection} if projection else {}),
        **({"multi_gpu": multi_gpu} if multi_gpu else {}),
        "kernels_ms_per_step": kernels, **({"trace_kinds": trace_kinds} if trace_kinds else {}),
        "rays_per_sample": round((counters["intersect_tests"] + counters["shadow_tests"]) / max(1, counters["camera_rays"]), 3) if counters else None,
        "nodes_per_ray": round(counters["bvh_nodes_visited"] / max(1, counters["intersect_tests"] + counters["shadow_tests"]), 2) if counters else None,
        "setup_s": {"scene_gen": round(t_gen, 1), "bvh_build_upload": round(t_up, 1),
                    **({"multi_scene_create": {k: (round(v / 1e3, 2) if not isinstance(v, list) else [round(x / 1e3, 2) for x in v]) for k, v in multi.create_timing().items()},
                        "multi_scene_create_note": "wall_ms / replica_ms in seconds: replica 0 builds the BVH, replicas 1.. adopt it and upload concurrently, one host thread each"} if multi is not None else {})},
    }
    if args.sim_world > 1 and world == 1:
        out["sim_world"] = args.sim_world
        out["value_note"] = f"rank 0's shard of a {args.sim_world}-rank job only; ideal = full-frame ms_per_step / {args.sim_world}"
    (scene or multi).close()
    del film
    torch.cuda.empty_cache()
    return out


def side_measurements(args, world, in_process):
    """Which side measurements a run makes after its headline's timed region: (projection world or 0, other configs on / off). With --projection /
    --other-configs "auto" they belong to a --full run of the default C2 workload on one GPU; "on" / "off" decide either way."""
    default_run = (args.config == "C2" and world == 1 and not in_process and args.sim_world <= 1 and args.spp == 0 and (args.xres, args.yres, args.mesh_n) == (1920, 1080, 1466))
    proj = 8 if (args.projection == "on" or (args.projection == "auto" and args.full and default_run)) else 0
    others = world == 1 and (args.other_configs == "on" or (args.other_configs == "auto" and args.full and default_run))
    return proj, others


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", default="C2", choices=["C2", "C3", "C3M", "C4", "C5"], help="BASELINE config (default: the headline C2)")
    ap.add_argument("--spp", type=int, default=0, help="samples per pixel per step (default: the config's named spp; C2: 256)")
    ap.add_argument("--mesh-n", type=int, default=1466, help="C2 / C5: displaced-sphere grid (1466 -> 4,298,312 triangles)")
    ap.add_argument("--xres", type=int, default=1920)
    ap.add_argument("--yres", type=int, default=1080)
    ap.add_argument("--spp-per-pass", type=int, default=0)
    ap.add_argument("--full", action="store_true", help="also the side measurements a plain run leaves out: cpu_baseline, the film read-back and, for the default C2 run "
                    "on one GPU, scaling_projection and other_configs")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="--full: target CPU time of the cpu_baseline sample (0 disables)")
    ap.add_argument("--dump-image", default="")
    ap.add_argument("--sim-rank", type=int, default=0, help="with --sim-world: which rank's shard")
    ap.add_argument("--sim-world", type=int, default=0, help="single-GPU study: render rank 0's shard of an N-rank job (value is then this rank's share only)")
    ap.add_argument("--in-process", action="store_true", help="force the one-process pt_multi_render form (it is the default for --gpus N > 1 without a launcher)")
    ap.add_argument("--devices", default="", help="one-process form: explicit device ordinals, e.g. 0,1,2,3 (an ordinal may repeat: replicas share the device; default 0..gpus-1)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"], help="launcher form: nccl (= RCCL, one GPU per rank) or gloo (film staged through the host; ranks may share a GPU: rehearsal on a one-GPU box)")
    ap.add_argument("--dump-film", default="", help="rank 0 writes the (merged) film of the last step as .npy")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="rank 0 writes the (merged) film of the last timed step as DIR/film.npy (float32, at most 64 MB: a fixed sample of a larger film)")
    ap.add_argument("--projection", default="auto", choices=["auto", "on", "off"], help="scaling_projection: rank 0's shard of an 8-rank job at the named spp, for the headline and for C4 / C5 (auto: --full default C2 run on one GPU)")
    ap.add_argument("--other-configs", default="auto", choices=["auto", "on", "off"], help="after the headline, one step (one wavefront pass) each of C3 / C4 / C5 under 'other_configs' (auto: --full default C2 run on one GPU)")
    return ap


def main():
    ap = parser()
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        args.gpus = world
    devices = [int(x) for x in args.devices.split(",") if x != ""] or list(range(args.gpus))
    # no launcher and more than one device (or replica) asked for: ONE process drives them all through pt_multi_render
    in_process = world == 1 and (len(devices) > 1 or args.in_process)

    import torch
    from _pkg import import_pkg
    pkg = import_pkg()
    lib = pkg.load_library()          # raises if libmi355pt.so is missing: there is no CPU fallback
    if in_process:
        import ctypes
        n_dev = ctypes.c_int(0)
        lib.check(lib.lib.pt_device_count(ctypes.byref(n_dev)), "pt_device_count")
        if max(devices) >= n_dev.value:
            raise SystemExit(f"bench.py: --gpus {args.gpus} asks for device ordinals {devices}, but this process sees {n_dev.value} device(s)")
    first = devices[0] if in_process else (devices[local_rank] if (world > 1 and args.devices and local_rank < len(devices)) else local_rank)
    lib.init(first)
    torch.cuda.set_device(first)
    dev = torch.device("cuda", first)
    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        if args.dist_backend == "gloo":
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    proj, others = side_measurements(args, world, in_process)
    out = measure(pkg, lib, torch, dev, dist, args, args.config, args.spp, args.steps, args.warmup, devices, in_process, rank, world, want_cpu_baseline=args.full, proj_world=proj)
    if out is not None and others:
        oc = {}
        for cfg, cspp in OTHER_CONFIG_SPP.items():
            if cfg == args.config:
                continue
            try:
                r = measure(pkg, lib, torch, dev, None, args, cfg, cspp, 1, 1, devices, in_process, 0, 1, want_cpu_baseline=False, proj_world=proj if cfg in ("C4", "C5") else 0)
                rf = r["roofline"] or {}
                oc[cfg] = dict(value=r["value"], unit=r["unit"], ms_per_step=r["ms_per_step"], steps=1, warmup=1, spp=r["config"]["spp"], named_spp=pkg.scenes.CONFIG_SCENES[cfg][1],
                               workload=r["config"]["workload"], spp_per_pass=r["config"]["spp_per_pass"],
                               dominant_kernel=rf.get("kernel"), dominant_avg_launch_ms=rf.get("avg_launch_ms"), algorithmic_GBs=rf.get("achieved"),
                               hbm_frac=rf.get("hbm_frac"), rays_per_sample=r["rays_per_sample"], nodes_per_ray=r["nodes_per_ray"],
                               **({"scaling_projection": r["scaling_projection"]} if r.get("scaling_projection") else {}),
                               bound=rf.get("bound"), valu_busy_frac=rf.get("valu_busy_frac"),
                               kernels_ms_per_step={k: {kk: v[kk] for kk in ("ms", "kernel", "hbm_frac", "traffic_over_algorithmic") if kk in v} for k, v in r["kernels_ms_per_step"].items()})
            except Exception as e:   # the headline line must not be lost to a side measurement
                oc[cfg] = dict(error=f"{type(e).__name__}: {e}")
        out["other_configs"] = oc
        out["other_configs_note"] = "one timed step after one warm-up; C3: the whole job at its named 1024 spp; C4 / C5: one wavefront pass of the size the library picks at the config's named spp (the per-sample cost does not depend on the spp beyond the pass size), with scaling_projection = rank 0's shard of the whole 8-GPU job; the value is Msamples/s of that step"
    if out is not None:
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


def host_cpu_info():
    """What this process may actually run on: the CPUs of its affinity mask, the distinct physical cores among them (/proc/cpuinfo `physical id` / `core id`) and
    the cgroup CPU quota (v2 cpu.max, v1 cpu.cfs_quota_us) -- os.cpu_count() is the machine, not the share a job was given."""
    try:
        aff = sorted(os.sched_getaffinity(0))
    except AttributeError:
        aff = list(range(os.cpu_count() or 1))
    cores, model, cur = set(), "", {}
    try:
        for line in open("/proc/cpuinfo"):
            if ":" in line:
                k, v = [x.strip() for x in line.split(":", 1)]
                cur[k] = v
                if k == "model name" and not model:
                    model = v
            elif not line.strip():
                if cur.get("processor", "").isdigit() and int(cur["processor"]) in aff:
                    cores.add((cur.get("physical id", "0"), cur.get("core id", cur["processor"])))
                cur = {}
        if cur.get("processor", "").isdigit() and int(cur["processor"]) in aff:
            cores.add((cur.get("physical id", "0"), cur.get("core id", cur["processor"])))
    except OSError:
        pass
    quota = None
    for path, parse in (("/sys/fs/cgroup/cpu.max", lambda t: None if t.split()[0] == "max" else float(t.split()[0]) / float(t.split()[1])),
                        ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", lambda t: None if int(t) <= 0 else int(t) / float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read()))):
        try:
            quota = parse(open(path).read().strip())
            break
        except (OSError, ValueError, IndexError, ZeroDivisionError):
            continue
    return dict(logical_cpus=len(aff), physical_cores=len(cores) or None, cgroup_cpu_quota=quota, model=model)


def run_cpu_baseline(pkg, sd, rp_full, spp, args):
    """The CPU oracle (C++ restatement of the reference path, tile-parallel std::thread like the reference's rayon loop, main.rs:115-124 /
    integrator.rs:294-296) timed on this box's host cores on a bounded sample of the SAME workload: every K-th 16x16 tile of the whole frame
    (tile_rank / tile_world sharding of integrator.rs:276-283's tile list with a stride coprime to the tiles per row), so sky, ground and dense
    geometry enter in the proportion they have in the frame. Timed with ONE thread first, then with the thread counts that can make sense here
    (the cgroup quota, the physical cores, the logical CPUs of the affinity mask); `value` is the best of them and the line says how far from linear it is --
    a GPU box hands a job a share of a 256-thread host, and one thread per logical CPU of the machine is then mostly time slicing."""
    import copy
    from oracle.oracle_binding import Oracle
    orc = Oracle(pkg._abi, pkg.runtime.TABLES_PATH)
    oscene = orc.scene(sd)
    info = host_cpu_info()
    sb = rp_full.sample_bounds
    ntx, nty = -(-(sb[2] - sb[0]) // 16), -(-(sb[3] - sb[1]) // 16)
    ntiles = ntx * nty

    def coprime_stride(k):
        from math import gcd
        k = max(1, min(int(k), ntiles))
        while k > 1 and gcd(k, ntx) != 1:
            k += 1
        return k

    cpu_spp = min(spp, 64)   # bounded sample: the per-sample cost does not depend on how many samples a pixel gets (each has its own Sobol' index)

    def render(stride, threads):
        rp = copy.copy(rp_full)
        rp.tile_rank, rp.tile_world, rp.profile, rp.spp = 0, stride, 0, cpu_spp
        oscene.render(rp, nthreads=threads)
        n = oscene.counters()["camera_rays"]
        return n, oscene.seconds()

    budget = args.cpu_seconds
    # one thread: ~ a fifth of the budget, on a sparse sample of the same tile list (calibrated on 8 tiles)
    n, secs = render(coprime_stride(ntiles // 8), 1)
    rate1 = n / max(1e-6, secs)
    want = max(8, int(rate1 * budget * 0.2 / (256 * cpu_spp)))
    n1, s1 = render(coprime_stride(max(1, ntiles // want)), 1)
    single = n1 / s1 / 1e6
    cands = sorted({t for t in (info["logical_cpus"], info["physical_cores"], int(info["cgroup_cpu_quota"] + 0.5) if info["cgroup_cpu_quota"] else None, 16) if t and 1 < t <= info["logical_cpus"]})
    cap = max(2, int(info["cgroup_cpu_quota"] + 0.5) if info["cgroup_cpu_quota"] else (info["physical_cores"] or info["logical_cpus"]))
    tried, best = [], None
    for t in cands:
        want = max(t, int(single * 1e6 * min(t, cap) * budget * 0.8 / max(1, len(cands)) / (256 * cpu_spp)))   # (sized as if it scaled up to the CPU share: bounds the oversubscribed runs)
        stride = coprime_stride(max(1, ntiles // want))
        nt, st = render(stride, t)
        r = dict(threads=t, msamples_s=round(nt / st / 1e6, 4), samples=int(nt), seconds=round(st, 2), tiles=-(-ntiles // stride), parallel_efficiency=round(nt / st / 1e6 / (single * t), 3))
        tried.append(r)
        if best is None or r["msamples_s"] > best["msamples_s"]:
            best = r
    if best is None:
        best = dict(threads=1, msamples_s=round(single, 4), samples=int(n1), seconds=round(s1, 2), tiles=0, parallel_efficiency=1.0)
    return dict(value=best["msamples_s"], unit="Msamples/s", cores=best["threads"], kind="port",
                single_thread_msamples_s=round(single, 4), threads=best["threads"], parallel_efficiency=best["parallel_efficiency"],
                physical_cores=info["physical_cores"], logical_cpus=info["logical_cpus"], cgroup_cpu_quota=info["cgroup_cpu_quota"], thread_counts_tried=tried,
                sample=f"every K-th 16x16 tile of the whole {args.xres}x{args.yres} frame at {cpu_spp} spp ({best['tiles']} of {ntiles} tiles, {best['samples']} samples, {best['seconds']} s with "
                       f"{best['threads']} threads; one thread: {n1} samples in {s1:.1f} s), oracle = C++ restatement of pbrt-rust's path, one std::thread per worker over 16x16 tiles",
                note="a reported baseline, not a target: `cores` = the thread count of `value`; parallel_efficiency = value / (threads x single-thread rate) on THIS host share",
                cpu=info["model"])


if __name__ == "__main__":
    main()
