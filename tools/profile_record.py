#!/usr/bin/env python3
"""The profile record that tools/check_profiles.py holds the tree against, one part per command:

    python3 tools/profile_record.py <part> [args] [--dry-run] [--out DIR] [--work DIR]

  pmc <C2|C3|C4|C5>             the library's pass size for the config (one bench step), rocprofv3 kernel stats and the four PMC traffic passes over
                                exactly one such pass, the three SQ issue-counter passes -> <out>/<config>/{summary.txt,summary.json,pmc_traffic.json,
                                sq_counters.txt}, and the config's records (traffic, sq, valu_busy_frac) merged into profiles/pmc_traffic.json
  final                         the -m gpu suite, the driver-form bench line, the C3/C4/C5 --full lines, rocprofv3 --stats of the bench command
                                -> <out>/final/ with the MANIFEST.json of check_profiles.write_manifest
  parity                        tools/full_frame_parity.py over the whole 1080p frame of all four configs -> <out>/full_frame_parity.jsonl
  util                          the PT_TRACE_UTIL library (tools/build_variant.sh qutil), its C2 and C4 trace-util lines -> <out>/<config>_trace_util.txt
  counters <config> "<set>"...  any counter sets, one rocprofv3 run each over one pass of the config; printed, nothing committed

<out> is profiles/r<ROUND> (check_profiles.ROUND); with --out, the committed outputs, the merged pmc_traffic.json included, go to DIR instead.
Every step runs under `timeout -k 10 <s>`. The first step that ends with a non-zero status (a failure, a time limit, an abort, a signal) ends the part:
nothing after it starts, nothing is retried, nothing is written to <out>, and the tool exits 1 naming the step and its log. Raw rocprofv3 output
stays under --work (default build/profile_record/, ignored by git), its large trace CSVs pruned. --dry-run prints every step and runs none.

Every counter pass is a rocprofv3 run of its own with --kernel-trace as its only other option: gfx950 counters, corrected as MI355X_MICROARCH.md
prescribes (FETCH_SIZE counts 64 B per 128-B request), and never combined with other tracing."""
import argparse
import csv
import dataclasses
import glob
import json
import os
import re
import shlex
import shutil
import subprocess
import sys
from collections import defaultdict

TOOLS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TOOLS)
sys.path.insert(0, TOOLS)
import check_profiles  # noqa: E402
from code_hash import code_hash  # noqa: E402

PY = sys.executable
BENCH = os.path.join(ROOT, "bench.py")
CONFIGS = ("C2", "C3", "C4", "C5")
WORKLOAD = [1466, 1920, 1080]   # bench.py matches a record's workload (mesh size, resolution) against its run's
PMC_PASSES = {"pmc_fetch": ["FETCH_SIZE"],
              "pmc_rd": ["TCC_EA0_RDREQ_sum", "TCC_EA0_RDREQ_128B_sum", "TCC_EA0_RDREQ_64B_sum", "TCC_EA0_RDREQ_32B_sum"],
              "pmc_write": ["WRITE_SIZE"],
              "pmc_l2": ["TCC_HIT_sum", "TCC_MISS_sum"]}
SQ_PASSES = {"sq1": ["SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_ACTIVE_INST_VALU", "SQ_WAVES", "GRBM_GUI_ACTIVE"],
             "sq2": ["SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR", "SQ_INSTS_LDS", "SQ_INSTS_SMEM", "SQ_INST_CYCLES_VMEM", "SQ_ACTIVE_INST_LDS"],
             "sq3": ["SQ_ACTIVE_INST_VMEM", "SQ_ACTIVE_INST_SCA", "SQ_ACTIVE_INST_FLAT", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "SQ_INSTS_FLAT", "SQ_WAIT_INST_LDS",
                     "SQ_INSTS_VALU_FMA_F64"]}
SQ_SPP = 64   # the SQ passes render 64 spp, as the committed records' sq / valu_busy_frac were taken
SQ_KEPT = ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_VMEM_RD", "SQ_INSTS_LDS", "GRBM_GUI_ACTIVE", "SQ_WAVE_CYCLES", "SQ_WAIT_INST_ANY")
VALU_BUSY_DEF = "4 cycles x SQ_INSTS_VALU / (1024 SIMDs x GRBM_GUI_ACTIVE / 8 XCDs), tools/sq_profile.sh"   # the committed records' text, kept as they carry it
FINAL_FILES = ("gpu_tests.log", "bench.json", "bench_C3.json", "bench_C4.json", "bench_C5.json", "stats_bench.json")


class StepFailed(Exception):
    pass


@dataclasses.dataclass
class Step:
    name: str
    argv: list              # as it runs: `timeout -k 10 <s>` first
    stdout: str
    stderr: str = None      # None: into stdout's file
    env: dict = dataclasses.field(default_factory=dict)   # additions to the environment
    cwd: str = ROOT
    outputs: tuple = ()     # what the command writes besides its stdout / stderr


def step(name, seconds, cmd, stdout, stderr=None, **kw):
    return Step(name, ["timeout", "-k", "10", str(seconds), *cmd], stdout, stderr, **kw)


def run_step(s):
    with open(s.stdout, "w") as out:
        err = open(s.stderr, "w") if s.stderr else None
        try:
            return subprocess.run(s.argv, stdout=out, stderr=err or subprocess.STDOUT, cwd=s.cwd, env={**os.environ, **s.env}).returncode
        finally:
            if err:
                err.close()


class Session:
    """Runs (or, dry, prints) one part's steps in order; the first non-zero status raises StepFailed."""

    def __init__(self, out, merged, work, dry_run):
        self.out, self.merged, self.work, self.dry_run = out, merged, work, dry_run

    def workdir(self, name):
        d = os.path.join(self.work, name)
        if not self.dry_run:
            shutil.rmtree(d, ignore_errors=True)
            os.makedirs(d)
        return d

    def run(self, s):
        if self.dry_run:
            print(f"{s.name}: {shlex.join(s.argv)}")
            print(f"    cwd {s.cwd}" + "".join(f"  {k}={v}" for k, v in s.env.items()))
            print(f"    writes {', '.join([s.stdout] + ([s.stderr] if s.stderr else []) + list(s.outputs))}")
            return
        print(f"== {s.name}", flush=True)
        rc = run_step(s)
        if rc != 0:
            raise StepFailed(f"step {s.name} ended with status {rc}; log {s.stderr or s.stdout}")

    def writes(self, *paths):
        """Prints the committed outputs a part is about to write; False in a dry run, which writes nothing."""
        print(("would write " if self.dry_run else "writing ") + ", ".join(paths), flush=True)
        return not self.dry_run


def profiled(w, tag, opts, bench_args, seconds):
    """bench.py under rocprofv3 (`opts`: --kernel-trace plus --stats or one --pmc set), its CSVs under <w>/<tag>."""
    d = os.path.join(w, tag)
    return step(tag, seconds, ["rocprofv3", *opts, "--output-format", "csv", "-d", d, "--", PY, BENCH, *bench_args],
                os.path.join(w, tag + "_bench.json"), os.path.join(w, tag + ".err"), env={"TMPDIR": "/tmp"}, cwd="/tmp", outputs=(d,))


def one_pass(config, spp):
    return ["--config", config, "--steps", "1", "--warmup", "0", "--spp", str(spp), "--cpu-seconds", "0"]


def probe_pass_size(sess, config, w):
    """The samples per pass the library picks for the config: one bench step's config.spp_per_pass."""
    s = step("probe", 400, [PY, BENCH, "--config", config, "--steps", "1", "--warmup", "1", "--cpu-seconds", "0", "--other-configs", "off"],
             os.path.join(w, "probe.json"), os.path.join(w, "probe.err"))
    sess.run(s)
    if sess.dry_run:
        return "<spp_per_pass>"
    line = check_profiles.last_json_line(s.stdout)
    if not line or not line["config"].get("spp_per_pass"):
        raise StepFailed(f"step probe printed no spp_per_pass; log {s.stdout}")
    return line["config"]["spp_per_pass"]


# ---- rocprofv3 CSVs -> per-kernel numbers

def short(name):
    """The kernel key of the records: `k_name<template args>`, or the symbol without its parameter list."""
    m = re.search(r"(k_[a-z_0-9]+(<[^>()]*>)?)", name)
    return m.group(1) if m else name.split("(")[0].replace("void ", "").strip()


def aggregate(d, counters):
    """{kernel: {"dispatches": n, counter: sum over dispatches}} of one counter pass (every *counter_collection.csv under d), kernels in
    descending order of their summed values. A dispatch is a row of the pass's first counter; a counter the profiler reported no rows of is left out."""
    acc = defaultdict(lambda: defaultdict(float))
    n = defaultdict(int)
    for f in sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                k, c = short(r["Kernel_Name"]), r["Counter_Name"]
                acc[k][c] += float(r["Counter_Value"])
                n[k] += c == counters[0]
    return {k: dict(dispatches=n[k], **{c: acc[k][c] for c in counters if c in acc[k]}) for k in sorted(acc, key=lambda k: -sum(acc[k].values()))}


def stats_rows(d):
    rows = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    return rows


def traffic(summary, spp_per_pass, chash):
    """HBM bytes per launch per kernel from a summary.json-shaped dict, the records of profiles/pmc_traffic.json.
    Reads: the memory-side read requests of the L2 by size, 128 * RDREQ_128B + 64 * RDREQ_64B + 32 * RDREQ_32B -- exact for any mix of wide streaming
    reads (128-byte requests, which FETCH_SIZE tallies at 64 bytes: the guide's "double it") and 64-byte gathers (which FETCH_SIZE counts exactly;
    profiles/r2_gather_calibration.json). Fallback when that pass is missing: FETCH_SIZE x 2 (upper bound).
    Writes: WRITE_SIZE (exact for 16-byte streaming stores and float atomics). FETCH_SIZE / WRITE_SIZE are in KiB."""
    out = {}
    for k, w in summary.get("pmc_write", {}).items():
        rd, fe, l2 = (summary.get(tag, {}).get(k) for tag in ("pmc_rd", "pmc_fetch", "pmc_l2"))
        if not w["dispatches"]:
            continue
        if rd and rd["dispatches"] and rd.get("TCC_EA0_RDREQ_sum"):
            read_b = (128.0 * rd["TCC_EA0_RDREQ_128B_sum"] + 64.0 * rd["TCC_EA0_RDREQ_64B_sum"] + 32.0 * rd["TCC_EA0_RDREQ_32B_sum"]) / rd["dispatches"]
            src = "rocprofv3 --pmc TCC_EA0_RDREQ_{128B,64B,32B}_sum (read bytes by request size) + WRITE_SIZE, separate passes"
        elif fe and fe["dispatches"]:
            read_b = fe["FETCH_SIZE"] * 1024.0 * 2.0 / fe["dispatches"]
            src = "rocprofv3 --pmc FETCH_SIZE x 2 (upper bound: exact for 128-byte streaming requests, 2x over for 64-byte gathers) + WRITE_SIZE"
        else:
            continue
        write_b = w["WRITE_SIZE"] * 1024.0 / w["dispatches"]
        out[k] = dict(hbm_bytes_per_launch=int(read_b + write_b), read_bytes_per_launch=int(read_b), write_bytes_per_launch=int(write_b),
                      fetch_size_kib_raw=fe["FETCH_SIZE"] if fe else None, rdreq=({c: rd[c] for c in rd if c != "dispatches"} if rd else None),
                      l2_hit_rate=(round(l2["TCC_HIT_sum"] / max(1.0, l2["TCC_HIT_sum"] + l2["TCC_MISS_sum"]), 4) if l2 else None),
                      dispatches=w["dispatches"], spp_per_pass=spp_per_pass, workload=WORKLOAD, source=src, code_hash=chash)
    return out


def valu_busy_frac(sq):
    """Vector-issue share of the SIMDs' cycles: 4 cycles per wave instruction over 1024 SIMDs x the active cycles of one of 8 XCDs."""
    return round(4.0 * sq["SQ_INSTS_VALU"] / (1024.0 * sq["GRBM_GUI_ACTIVE"] / 8.0), 4)


def with_sq(records, sq_passes):
    """The traffic records, each kernel the SQ passes saw with its SQ_KEPT counters and valu_busy_frac."""
    seen = defaultdict(dict)
    for agg in sq_passes.values():
        for k, a in agg.items():
            seen[k].update(a)
    out = {}
    for k, rec in records.items():
        v = seen.get(k, {})
        rec = dict(rec)
        if "SQ_INSTS_VALU" in v and v.get("GRBM_GUI_ACTIVE"):
            rec.update(sq={n: v[n] for n in SQ_KEPT if n in v}, valu_busy_frac=valu_busy_frac(v), valu_busy_def=VALU_BUSY_DEF)
        out[k] = rec
    return out


def summary_text(stats, summary):
    lines = ["== kernel stats (rocprofv3 --kernel-trace --stats)"]
    for r in stats[:16]:
        lines.append(f"{short(r['Name']):32s} calls={r['Calls']:>6s} total_ms={float(r['TotalDurationNs'])/1e6:10.3f} avg_us={float(r['AverageNs'])/1e3:10.2f} "
                     f"pct={r['Percentage']}")
    for tag, counters in PMC_PASSES.items():
        lines.append(f"== {tag}")
        for k, a in summary[tag].items():
            n = a["dispatches"]
            lines.append(f"{k:32s} dispatches={n:5d} " + " ".join(f"{c}={a[c]:.4g} (per dispatch {a[c]/max(1, n):.4g})" for c in counters))
    return "\n".join(lines) + "\n"


def counters_text(passes, top, width):
    """The largest `top` kernels of each counter pass, one line each: `<kernel> n=<dispatches> NAME=value ...`."""
    lines = []
    for tag, agg in passes.items():
        lines.append(f"== {tag}")
        for k in list(agg)[:top]:
            a = agg[k]
            lines.append(f"{k:{width}s} n={a['dispatches']:3d} " + " ".join(f"{c}={a[c]:.4g}" for c in sorted(c for c in a if c != "dispatches")))
    return "\n".join(lines) + "\n"


def counter_passes(w, sets, steps):
    """Aggregates of the passes that ran; a pass with no counter rows is a failed step."""
    out = {}
    for tag, counters in sets.items():
        out[tag] = aggregate(os.path.join(w, tag), counters)
        if not out[tag]:
            raise StepFailed(f"step {tag} left no counter rows; log {steps[tag].stderr}")
    return out


def write(path, text):
    with open(path, "w") as f:
        f.write(text)


# ---- parts

def part_pmc(sess, config):
    w = sess.workdir(config)
    spp = probe_pass_size(sess, config, w)
    steps = {"stats": profiled(w, "stats", ["--kernel-trace", "--stats"], one_pass(config, spp), 400)}
    steps.update({tag: profiled(w, tag, ["--pmc", *c, "--kernel-trace"], one_pass(config, spp), 400) for tag, c in PMC_PASSES.items()})
    steps.update({tag: profiled(w, tag, ["--pmc", *c, "--kernel-trace"], one_pass(config, SQ_SPP), 200) for tag, c in SQ_PASSES.items()})
    for s in steps.values():
        sess.run(s)
    dst = os.path.join(sess.out, config)
    if not sess.writes(*(os.path.join(dst, f) for f in ("summary.txt", "summary.json", "pmc_traffic.json", "sq_counters.txt")), sess.merged):
        return
    stats = stats_rows(os.path.join(w, "stats"))
    if not stats:
        raise StepFailed(f"step stats wrote no kernel_stats.csv; log {steps['stats'].stderr}")
    summary = {"kernel_stats": [dict(name=short(r["Name"]), calls=int(r["Calls"]), total_ms=float(r["TotalDurationNs"]) / 1e6,
                                     avg_us=float(r["AverageNs"]) / 1e3, pct=float(r["Percentage"])) for r in stats[:16]]}
    summary.update(counter_passes(w, PMC_PASSES, steps))
    sq = counter_passes(w, SQ_PASSES, steps)
    summary["traffic"] = traffic(summary, spp, code_hash(ROOT))
    os.makedirs(dst, exist_ok=True)
    write(os.path.join(dst, "summary.txt"), summary_text(stats, summary))
    json.dump(summary, open(os.path.join(dst, "summary.json"), "w"), indent=1)
    json.dump({config: summary["traffic"]}, open(os.path.join(dst, "pmc_traffic.json"), "w"), indent=1)
    write(os.path.join(dst, "sq_counters.txt"), counters_text(sq, 6, 28))
    data = json.load(open(sess.merged)) if os.path.exists(sess.merged) else {}
    data[config] = with_sq(summary["traffic"], sq)
    json.dump(data, open(sess.merged, "w"), indent=1)
    print(open(os.path.join(dst, "summary.txt")).read()[:2000])


def part_final(sess):
    w = sess.workdir("final")
    sess.run(step("gpu_tests", 1100, [PY, "-m", "pytest", "tests", "-m", "gpu", "-q", "--durations=12"], os.path.join(w, "gpu_tests.log")))
    sess.run(step("bench", 600, [PY, BENCH, "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"], os.path.join(w, "bench.json"), os.path.join(w, "bench.err")))
    for c in ("C3", "C4", "C5"):
        sess.run(step(f"bench_{c}", 500, [PY, BENCH, "--config", c, "--steps", "1", "--warmup", "1", "--full", "--cpu-seconds", "8", "--projection", "off"],
                      os.path.join(w, f"bench_{c}.json"), os.path.join(w, f"bench_{c}.err")))
    sess.run(profiled(w, "stats", ["--kernel-trace", "--stats"], ["--steps", "2", "--warmup", "1", "--cpu-seconds", "0", "--other-configs", "off", "--projection", "off"], 400))
    dst = os.path.join(sess.out, "final")
    if not sess.writes(*(os.path.join(dst, f) for f in FINAL_FILES + ("kernel_stats_spp256.csv", "MANIFEST.json"))):
        return
    kstats = sorted(glob.glob(os.path.join(w, "stats", "**", "*kernel_stats.csv"), recursive=True))
    if not kstats:
        raise StepFailed(f"step stats wrote no kernel_stats.csv; log {os.path.join(w, 'stats.err')}")
    shutil.rmtree(dst, ignore_errors=True)   # the record is replaced as a whole: its manifest must not bless a file of the previous one
    os.makedirs(dst)
    for f in FINAL_FILES:
        shutil.copy(os.path.join(w, f), dst)
    shutil.copy(kstats[0], os.path.join(dst, "kernel_stats_spp256.csv"))
    check_profiles.write_manifest(dst)


def part_parity(sess):
    w = sess.workdir("parity")
    s = step("full_frame_parity", 1100, [PY, os.path.join(TOOLS, "full_frame_parity.py"), "C2:64", "C5:32", "C3:16", "C4:8"],
             os.path.join(w, "full_frame_parity.jsonl"), os.path.join(w, "parity_err.log"))
    sess.run(s)
    dst = os.path.join(sess.out, "full_frame_parity.jsonl")
    if sess.writes(dst):
        os.makedirs(sess.out, exist_ok=True)
        shutil.copy(s.stdout, dst)


def part_util(sess):
    w = sess.workdir("util")
    lib = os.path.join(ROOT, "pbrt-rust_amd", "csrc", "variants", "qutil")
    sess.run(step("build_qutil", 900, [os.path.join(TOOLS, "build_variant.sh"), "qutil", "-DPT_TRACE_UTIL"], os.path.join(w, "build.log"), outputs=(lib,)))
    runs = {c: step(f"{c}_trace_util", 400, [PY, BENCH, "--config", c, "--spp", str(spp), "--steps", "1", "--warmup", "0", "--cpu-seconds", "0",
                                             "--other-configs", "off", "--projection", "off"],
                    os.path.join(w, f"{c}.json"), os.path.join(w, f"{c}.err"), env={"PT_LIB_PATH": lib})
            for c, spp in (("C2", 128), ("C4", 32))}
    for s in runs.values():
        sess.run(s)
    if not sess.writes(*(os.path.join(sess.out, f"{c}_trace_util.txt") for c in runs)):
        return
    os.makedirs(sess.out, exist_ok=True)
    for c, s in runs.items():
        write(os.path.join(sess.out, f"{c}_trace_util.txt"), "".join(l for l in open(s.stderr) if "trace-util" in l))


def part_counters(sess, config, *sets):
    w = sess.workdir("counters_" + config)
    spp = probe_pass_size(sess, config, w)
    passes = {f"p{i}": s.split() for i, s in enumerate(sets, 1)}
    steps = {tag: profiled(w, tag, ["--pmc", *c, "--kernel-trace"], one_pass(config, spp), 400) for tag, c in passes.items()}
    for s in steps.values():
        sess.run(s)
    if sess.dry_run:
        return
    text = counters_text(counter_passes(w, passes, steps), 5, 24)
    write(os.path.join(w, "counters.txt"), text)
    print(text)


def prune(work):
    """Keeps the work directory small: raw traces and counter CSVs above a few MiB go, the summaries stay."""
    for pattern, limit in (("*kernel_trace.csv", 4 << 20), ("*counter_collection.csv", 8 << 20)):
        for f in glob.glob(os.path.join(work, "**", pattern), recursive=True):
            if os.path.getsize(f) > limit:
                os.remove(f)


def main(argv=None):
    common = argparse.ArgumentParser(add_help=False)
    common.add_argument("--dry-run", action="store_true", help="print every step (argv, environment additions, timeout, outputs) and run none")
    common.add_argument("--out", help="where the committed outputs go (default profiles/r<ROUND>, merged records profiles/pmc_traffic.json)")
    common.add_argument("--work", default=os.path.join(ROOT, "build", "profile_record"), help="raw rocprofv3 output and logs")
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="part", required=True)
    p = sub.add_parser("pmc", parents=[common])
    p.add_argument("config", choices=CONFIGS)
    p.set_defaults(run=lambda sess, a: part_pmc(sess, a.config))
    sub.add_parser("final", parents=[common]).set_defaults(run=lambda sess, a: part_final(sess))
    sub.add_parser("parity", parents=[common]).set_defaults(run=lambda sess, a: part_parity(sess))
    sub.add_parser("util", parents=[common]).set_defaults(run=lambda sess, a: part_util(sess))
    p = sub.add_parser("counters", parents=[common])
    p.add_argument("config", choices=CONFIGS)
    p.add_argument("sets", nargs="+", help="one quoted, space-separated counter set per rocprofv3 run")
    p.set_defaults(run=lambda sess, a: part_counters(sess, a.config, *a.sets))
    a = ap.parse_args(argv)
    if a.out:
        out = os.path.abspath(a.out)
        merged = os.path.join(out, "pmc_traffic.json")
    else:
        out = os.path.join(ROOT, "profiles", f"r{check_profiles.ROUND}")
        merged = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    sess = Session(out, merged, os.path.abspath(a.work), a.dry_run)
    try:
        a.run(sess, a)
    except StepFailed as e:
        print(f"profile_record {a.part}: {e}; nothing after it was started", file=sys.stderr)
        return 1
    finally:
        if not a.dry_run:
            prune(sess.work)
    return 0


if __name__ == "__main__":
    sys.exit(main())
