"""tools/profile_record.py without a GPU: its traffic formula reproduces the committed record, its aggregator sums rocprofv3 counter CSVs, its plan keeps every
counter set in a --pmc run of its own under a time limit, and the first failing step ends a part."""
import csv
import json
import os
import re
import shlex
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import profile_record as pr  # noqa: E402

PROFILES = os.path.join(ROOT, "profiles")
RECORD = os.path.join(PROFILES, f"r{pr.check_profiles.ROUND}")


@pytest.mark.parametrize("config", pr.CONFIGS)
def test_committed_record_reproduces(config):
    summary = json.load(open(os.path.join(RECORD, config, "summary.json")))
    committed = json.load(open(os.path.join(RECORD, config, "pmc_traffic.json")))[config]
    spp = {r["spp_per_pass"] for r in committed.values()}
    assert len(spp) == 1
    derived = pr.traffic(summary, spp.pop(), "hash")
    assert list(derived) == list(committed)
    for k, rec in committed.items():
        assert {f: v for f, v in derived[k].items() if f != "code_hash"} == {f: v for f, v in rec.items() if f != "code_hash"}, k
    merged = json.load(open(os.path.join(PROFILES, "pmc_traffic.json")))[config]
    assert set(merged) == set(derived)
    with_sq = [r for r in merged.values() if "sq" in r]
    assert with_sq
    for r in with_sq:
        assert pr.valu_busy_frac(r["sq"]) == r["valu_busy_frac"] and r["valu_busy_def"] == pr.VALU_BUSY_DEF
    # the PMC sections of summary.txt are the text form of summary.json
    text = open(os.path.join(RECORD, config, "summary.txt")).read()
    assert pr.summary_text([], summary).split("\n", 1)[1] == text[text.index("== pmc_fetch"):]


def write_counters(path, rows):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Dispatch_Id", "Kernel_Name", "Counter_Name", "Counter_Value"])
        w.writerows(rows)


TRACE = "void k_trace<2, 0, false, 1>(TraceParams const*, unsigned int)"
SHADE = "void k_shade<1, 0, 1>(ShadeParams const*)"
COPY = "__amd_rocclr_copyBuffer"


def test_aggregator_and_traffic(tmp_path):
    d = str(tmp_path)
    # two dispatches of k_trace (split over two files, as rocprofv3 writes one per process), one each of k_shade and a runtime copy kernel
    write_counters(f"{d}/pmc_fetch/host/1_counter_collection.csv", [[1, TRACE, "FETCH_SIZE", 100.0], [2, SHADE, "FETCH_SIZE", 5.0], [3, COPY, "FETCH_SIZE", 2.0]])
    write_counters(f"{d}/pmc_fetch/host/2_counter_collection.csv", [[4, TRACE, "FETCH_SIZE", 300.0]])
    write_counters(f"{d}/pmc_write/host/1_counter_collection.csv",
                   [[1, TRACE, "WRITE_SIZE", 10.0], [2, SHADE, "WRITE_SIZE", 2.0], [3, COPY, "WRITE_SIZE", 1.0], [4, TRACE, "WRITE_SIZE", 30.0]])
    write_counters(f"{d}/pmc_l2/host/1_counter_collection.csv",
                   [[1, TRACE, "TCC_HIT_sum", 30.0], [1, TRACE, "TCC_MISS_sum", 10.0], [4, TRACE, "TCC_HIT_sum", 30.0], [4, TRACE, "TCC_MISS_sum", 30.0]])
    write_counters(f"{d}/pmc_rd/host/1_counter_collection.csv",   # only k_shade has read requests
                   [[2, SHADE, "TCC_EA0_RDREQ_sum", 10.0], [2, SHADE, "TCC_EA0_RDREQ_128B_sum", 8.0], [2, SHADE, "TCC_EA0_RDREQ_64B_sum", 2.0],
                    [2, SHADE, "TCC_EA0_RDREQ_32B_sum", 0.0]])
    summary = {tag: pr.aggregate(os.path.join(d, tag), counters) for tag, counters in pr.PMC_PASSES.items()}
    tr, sh, cp = "k_trace<2, 0, false, 1>", "k_shade<1, 0, 1>", COPY
    assert summary["pmc_fetch"] == {tr: {"dispatches": 2, "FETCH_SIZE": 400.0}, sh: {"dispatches": 1, "FETCH_SIZE": 5.0}, cp: {"dispatches": 1, "FETCH_SIZE": 2.0}}
    assert list(summary["pmc_fetch"]) == [tr, sh, cp]   # largest first
    assert summary["pmc_l2"] == {tr: {"dispatches": 2, "TCC_HIT_sum": 60.0, "TCC_MISS_sum": 40.0}}
    assert pr.aggregate(os.path.join(d, "no_such_pass"), ["FETCH_SIZE"]) == {}
    assert pr.aggregate(os.path.join(d, "pmc_fetch"), ["FETCH_SIZE", "NOT_REPORTED"])[cp] == {"dispatches": 1, "FETCH_SIZE": 2.0}   # no rows: left out, not 0

    t = pr.traffic(summary, 128, "h")
    # k_trace: no read requests counted -> FETCH_SIZE x 2: 400 KiB x 2 / 2 dispatches; writes 40 KiB / 2
    assert (t[tr]["read_bytes_per_launch"], t[tr]["write_bytes_per_launch"], t[tr]["hbm_bytes_per_launch"]) == (409600, 20480, 430080)
    assert t[tr]["l2_hit_rate"] == 0.6 and t[tr]["rdreq"] is None and t[tr]["dispatches"] == 2 and t[tr]["spp_per_pass"] == 128
    # k_shade: 128 B x 8 + 64 B x 2 read, 2 KiB written
    assert (t[sh]["read_bytes_per_launch"], t[sh]["hbm_bytes_per_launch"], t[sh]["l2_hit_rate"]) == (1152, 3200, None)
    assert t[sh]["rdreq"] == {"TCC_EA0_RDREQ_sum": 10.0, "TCC_EA0_RDREQ_128B_sum": 8.0, "TCC_EA0_RDREQ_64B_sum": 2.0, "TCC_EA0_RDREQ_32B_sum": 0.0}
    assert t[cp]["hbm_bytes_per_launch"] == 2 * 2048 + 1024
    # the whole RDREQ pass missing: every kernel falls back to FETCH_SIZE x 2
    t = pr.traffic({k: v for k, v in summary.items() if k != "pmc_rd"}, 128, "h")
    assert t[sh]["hbm_bytes_per_launch"] == 5 * 2048 + 2048 and "FETCH_SIZE x 2" in t[sh]["source"]


def plan(capsys, *argv):
    assert pr.main([*argv, "--dry-run"]) == 0
    lines = capsys.readouterr().out.replace(ROOT, "<root>").replace(sys.executable, "<python>").splitlines()
    steps = [(l.split(":", 1)[0], shlex.split(l.split(":", 1)[1])) for l in lines if not l.startswith((" ", "would write"))]
    return "\n".join(lines), steps


@pytest.mark.parametrize("part", [["pmc", "C2"], ["pmc", "C5"], ["final"], ["parity"], ["util"], ["counters", "C3", "GRBM_COUNT SQ_WAVES", "TCC_HIT_sum"]])
def test_dry_run_plan(capsys, part):
    text, steps = plan(capsys, *part)
    assert steps
    pmc_sets = []
    for name, argv in steps:
        assert argv[:3] == ["timeout", "-k", "10"] and int(argv[3]) > 0, name
        if "rocprofv3" not in argv:
            continue
        cmd = argv[argv.index("rocprofv3") + 1:]
        program = cmd[cmd.index("--") + 1:]
        assert program[:2] == ["<python>", "<root>/bench.py"], name
        opts = [a for a in cmd[:cmd.index("--")] if a.startswith("--")]
        assert "--kernel-trace" in opts and set(opts) <= {"--kernel-trace", "--stats", "--pmc", "--output-format"}, name
        if "--pmc" in opts:
            assert opts.count("--pmc") == 1 and "--stats" not in opts, name
            pmc_sets.append(cmd[cmd.index("--pmc") + 1:cmd.index("--kernel-trace")])
    if part[0] == "pmc":
        assert pmc_sets == list(pr.PMC_PASSES.values()) + list(pr.SQ_PASSES.values())
    if part[0] == "counters":
        assert pmc_sets == [["GRBM_COUNT", "SQ_WAVES"], ["TCC_HIT_sum"]]
    assert not re.search(r"(?<![A-Za-z0-9])r\d", text.replace(f"profiles/r{pr.check_profiles.ROUND}/", "")), text


def test_no_round_numbered_tools():
    assert not [f for f in os.listdir(os.path.join(ROOT, "tools")) if re.match(r"r\d", f)]


def fake_rocprof(s):
    """What a successful step leaves behind: the probe's bench line, one kernel's stats or counters (every counter = 1000)."""
    with open(s.stdout, "w") as f:
        f.write(json.dumps({"config": {"spp_per_pass": 256}}) + "\n")
    if "rocprofv3" in s.argv:
        d = s.argv[s.argv.index("-d") + 1]
        if "--stats" in s.argv:
            os.makedirs(f"{d}/host")
            with open(f"{d}/host/1_kernel_stats.csv", "w") as f:
                f.write('"Name","Calls","TotalDurationNs","AverageNs","Percentage"\n"k_shade<1, 0, 1>(P)",6,72046825,12007804.1,26.13\n')
        else:
            ctrs = s.argv[s.argv.index("--pmc") + 1:s.argv.index("--kernel-trace")]
            write_counters(f"{d}/host/1_counter_collection.csv", [[1, SHADE, c, 1000.0] for c in ctrs])
    return 0


def test_a_whole_pmc_part_writes_the_record(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(pr, "run_step", fake_rocprof)
    out = tmp_path / "out"
    assert pr.main(["pmc", "C3", "--out", str(out), "--work", str(tmp_path / "work")]) == 0
    assert sorted(os.listdir(out / "C3")) == ["pmc_traffic.json", "sq_counters.txt", "summary.json", "summary.txt"]
    rec = json.load(open(out / "pmc_traffic.json"))["C3"]["k_shade<1, 0, 1>"]
    assert rec["spp_per_pass"] == 256 and rec["hbm_bytes_per_launch"] == 128 * 1000 + 64 * 1000 + 32 * 1000 + 1000 * 1024
    assert rec["valu_busy_frac"] == pr.valu_busy_frac({"SQ_INSTS_VALU": 1000.0, "GRBM_GUI_ACTIVE": 1000.0}) and set(rec["sq"]) == set(pr.SQ_KEPT)
    assert json.load(open(out / "C3" / "pmc_traffic.json"))["C3"]["k_shade<1, 0, 1>"] == {k: v for k, v in rec.items() if k not in ("sq", "valu_busy_frac", "valu_busy_def")}
    assert open(out / "C3" / "sq_counters.txt").read().startswith("== sq1\nk_shade<1, 0, 1>             n=  1 GRBM_GUI_ACTIVE=1000 ")


@pytest.mark.parametrize("part,n_steps", [(["pmc", "C2"], 9), (["final"], 6), (["util"], 3), (["parity"], 1), (["counters", "C4", "SQ_WAVES"], 2)])
@pytest.mark.parametrize("status", [134, 124, -11])
def test_the_first_failing_step_ends_the_part(tmp_path, monkeypatch, capsys, part, n_steps, status):
    for k in range(1, n_steps + 1):
        started = []

        def stub(s):
            started.append(s.name)
            return status if len(started) == k else fake_rocprof(s)

        monkeypatch.setattr(pr, "run_step", stub)
        out = tmp_path / f"out{k}"
        assert pr.main([*part, "--out", str(out), "--work", str(tmp_path / "work")]) == 1
        assert len(started) == k
        assert not out.exists()
        err = capsys.readouterr().err
        assert f"step {started[-1]} ended with status {status}" in err


def test_a_whole_final_part_writes_the_record_and_its_manifest(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(pr, "run_step", fake_rocprof)
    out = tmp_path / "out"
    (out / "final").mkdir(parents=True)
    (out / "final" / "from_an_earlier_record.json").write_text("{}")
    assert pr.main(["final", "--out", str(out), "--work", str(tmp_path / "work")]) == 0
    files = sorted(pr.FINAL_FILES + ("kernel_stats_spp256.csv",))
    assert sorted(os.listdir(out / "final")) == sorted(files + ["MANIFEST.json"])
    manifest = json.load(open(out / "final" / "MANIFEST.json"))
    assert sorted(manifest["files"]) == files and manifest["code_hash"] == pr.code_hash(ROOT)
