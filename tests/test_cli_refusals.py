"""No GPU: every command line mi355pbrt refuses, in one table -- the arguments, the scene text where the refusal needs one, and a piece of the message. A refusal is
exit status 2 with the message and the usage text on stderr, before the device is touched and before any file is written. The rows marked `scene=None` are refused
before the scene file is looked for (it does not exist); the others once it is parsed. tests/cli_plan/check_cli_plan.cpp holds the same table against
frontend/cli_plan.h alone (test_cli_plan_on_the_cpu)."""
import os
import subprocess

import pytest
from abi_checks import no_device_env

SCENE = ('LookAt 0 0 -1  0 0 0  0 1 0\nCamera "perspective" "float fov" 30\nFilm "image" "integer xresolution" 16 "integer yresolution" 16\n'
         'Sampler "sobol" "integer pixelsamples" 4\n%sWorldBegin\n'
         'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-100 -100 0 100 -100 0 100 100 0 -100 100 0]\nWorldEnd\n')
PATH, AO = SCENE % "", SCENE % 'Integrator "ambientocclusion" "integer nsamples" 2\n'
USAGE = ("usage: mi355pbrt scene.pbrt [--outfile out.pfm] [--device N] [--spp N] [--quiet] [--samples A:B] [--checkpoint FILE] [--preview-every N]\n"
         "                 [--adaptive T [--adaptive-step N] [--adaptive-min N]] [--aov FILE.exr] [--denoise FILE [--denoise-iterations N]]\n")

# (arguments after `scene.pbrt --outfile o.pfm`, scene text or None, substring of the message)
REFUSALS = [
    # the seven combinations that need no scene
    (["--adaptive", "0.1", "--samples", "0:2"], None, "--adaptive with --samples: an adaptive render chooses its own sample ranges"),
    (["--adaptive", "0.1", "--checkpoint", "c.bin"], None, "--adaptive with --checkpoint: a checkpoint holds one sample count for the frame"),
    (["--adaptive", "0.1", "--aov", "f.exr"], None, "--adaptive with --aov: the feature buffers have no tile-list render"),
    (["--adaptive", "0.1", "--denoise", "d.pfm"], None, "--adaptive with --denoise: the filter takes one sample count for the frame"),
    (["--checkpoint", "c.bin", "--denoise", "d.pfm"], None, "--checkpoint with --denoise: a checkpoint holds one film"),
    (["--preview-every", "2", "--denoise", "d.pfm"], None, "--preview-every with --denoise: a preview shows the film so far"),
    (["--denoise-iterations", "3"], None, "--denoise-iterations without --denoise"),
    # a malformed --samples
    (["--samples", "3:2"], None, '--samples takes A:B with 0 <= A < B, got "3:2"'),
    (["--samples", "2:2"], None, '--samples takes A:B with 0 <= A < B, got "2:2"'),
    (["--samples", "7"], None, '--samples takes A:B with 0 <= A < B, got "7"'),
    (["--samples", "0:4294967296"], None, '--samples takes A:B with 0 <= A < B, got "0:4294967296"'),
    # the numeric flags' ranges
    (["--denoise", "d.pfm", "--denoise-iterations", "6"], None, "--denoise-iterations takes a number of levels 0..5"),
    (["--denoise", "d.pfm", "--denoise-iterations", "-1"], None, "--denoise-iterations takes a number of levels 0..5"),
    (["--denoise", "d.pfm", "--denoise-iterations", "2x"], None, "--denoise-iterations takes a number of levels 0..5"),
    (["--preview-every", "0"], None, "--preview-every takes a number of samples > 0"),
    (["--preview-every", "-3"], None, "--preview-every takes a number of samples > 0"),
    (["--preview-every", "4294967296"], None, "--preview-every takes a number of samples > 0"),
    (["--preview-every", "x"], None, "--preview-every takes a number of samples > 0"),
    (["--adaptive", "-0.5"], None, "--adaptive takes an error threshold >= 0"),
    (["--adaptive", "nan"], None, "--adaptive takes an error threshold >= 0"),
    (["--adaptive", "0.1x"], None, "--adaptive takes an error threshold >= 0"),
    (["--adaptive", "0.1", "--adaptive-step", "0"], None, "--adaptive-step takes a number of samples > 0"),
    (["--adaptive", "0.1", "--adaptive-step", "4294967296"], None, "--adaptive-step takes a number of samples > 0"),
    (["--adaptive", "0.1", "--adaptive-min", "-1"], None, "--adaptive-min takes a number of samples >= 0"),
    (["--adaptive", "0.1", "--adaptive-min", "4294967296"], None, "--adaptive-min takes a number of samples >= 0"),
    # two rules broken: a flag's own range before the combinations, the combinations in their order, a combination before the malformed range
    (["--preview-every", "0", "--denoise", "d.pfm"], None, "--preview-every takes a number of samples > 0"),
    (["--denoise", "d.pfm", "--checkpoint", "c.bin", "--adaptive", "0.1"], None, "--adaptive with --checkpoint"),
    (["--samples", "3:2", "--adaptive", "0.1"], None, "--adaptive with --samples"),
    (["--samples", "3:2", "--denoise-iterations", "3"], None, "--denoise-iterations without --denoise"),
    # known once the scene is parsed (4 samples per pixel)
    (["--samples", "0:5"], PATH, "--samples 0:5 goes beyond the job's 4 samples per pixel"),
    (["--spp", "2", "--samples", "1:3"], PATH, "--samples 1:3 goes beyond the job's 2 samples per pixel"),
    (["--spp", "1", "--denoise", "d.pfm"], PATH, "--denoise needs two samples per pixel at least"),
    (["--samples", "3:4", "--denoise", "d.pfm"], PATH, "--denoise needs two samples per pixel at least"),
    (["--adaptive", "0.1"], AO, '--adaptive with Integrator "ambientocclusion": the ambient-occlusion integrator has no tile-list render'),
    (["--samples", "0:5", "--denoise", "d.pfm", "--aov", "f.exr"], PATH, "--samples 0:5 goes beyond"),   # (two rules: the range first)
    # the usage text alone: no scene, a flag nobody knows, a flag without its value
    ([], "no scene argument", ""),
    (["--frobnicate"], None, ""),
    (["--spp"], None, ""),
]


def run(args, cwd):
    return subprocess.run(args, capture_output=True, text=True, timeout=60, env=no_device_env(), cwd=cwd)   # a refusal must come first


@pytest.mark.parametrize("extra,scene,message", REFUSALS, ids=lambda v: " ".join(v) if isinstance(v, list) else None)
def test_refused_command_lines(pkg, tmp_path, extra, scene, message):
    args = [pkg.frontend.CLI_PATH]
    if scene != "no scene argument":
        args += ["scene.pbrt", "--outfile", "o.pfm"]
        if scene is not None:
            (tmp_path / "scene.pbrt").write_text(scene)
    before = sorted(os.listdir(tmp_path))
    r = run(args + extra, tmp_path)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert r.stderr.endswith(USAGE) and r.stdout == ""
    if message:
        assert "mi355pbrt: " + message in r.stderr
    else:
        assert r.stderr == USAGE
    assert sorted(os.listdir(tmp_path)) == before   # no outfile, checkpoint, feature or denoised file


def test_cli_plan_on_the_cpu(pkg, tmp_path):
    """frontend/cli_plan.h without a device: tests/cli_plan/check_cli_plan.cpp, a program of its own over the header alone, built with the address and
    undefined-behaviour sanitizers. Its header comment lists what it holds about groups() and make_plan(); it passes when it exits 0. Then every row of the table above
    goes through its parse_options and make_plan: the same verdict and message as the binary's, at the same stage."""
    root = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "check_cli_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.dirname(pkg.frontend.CLI_PATH), "-o", exe, os.path.join(root, "cli_plan", "check_cli_plan.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-4000:] + r.stderr[-2000:]
    for extra, scene, message in REFUSALS:
        args = [] if scene == "no scene argument" else ["scene.pbrt", "--outfile", "o.pfm"]
        parsed = scene in (PATH, AO)
        r = subprocess.run([exe, "verdict", "4" if parsed else "0", "1" if scene == AO else "0"] + args + extra, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", (extra, r.stderr[-2000:])
        verdict, why = r.stdout.split("\n")[:2]
        assert verdict == ("plan 2" if parsed else "parse 2"), (extra, r.stdout)
        assert message in why and (why != "") == (message != ""), (extra, why)


def test_help_prints_both_usage_lines(pkg, tmp_path):
    r = run([pkg.frontend.CLI_PATH, "--help"], tmp_path)
    assert r.returncode == 2 and r.stderr == USAGE and r.stdout == ""
    assert len(USAGE.splitlines()) == 2
