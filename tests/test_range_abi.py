"""No GPU: the range / film-tool entry points as a C compiler and ctypes see them, mi355pbrt's usage errors for --samples, and the checkpoint file's round trip."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from abi_checks import INC, ROOT, assert_mirror, c99_probe, no_device_env

# the prototypes as the feature defines them: C type of the function, and the ctypes signature the mirrors must carry
PROTOTYPES = {
    "pt_render_samples": ("int(pt_scene *, const PtRenderParams *, uint32_t, uint32_t, float *, int)", "pt"),
    "pt_multi_render_samples": ("int(pt_multi_scene *, const PtRenderParams *, uint32_t, uint32_t, float *, int)", "pt"),
    "pt_ao_render_samples": ("int(pt_scene *, const PtRenderParams *, const PtAOParams *, uint32_t, uint32_t, float *, int)", "ao"),
    "pt_film_resolve_device": ("int(pt_scene *, const float *, uint32_t, float, float *, uint8_t *)", "pt"),
    "pt_film_halves_error": ("int(pt_scene *, const float *, const float *, uint32_t, uint32_t, float *, float *, float *)", "pt"),
}


def _ctype_of(c_param, A, AO):
    c_param = c_param.strip()
    if c_param == "const PtRenderParams *": return C.POINTER(A.PtRenderParams)
    if c_param == "const PtAOParams *": return C.POINTER(AO.PtAOParams)
    if c_param.endswith("*"): return (C.c_void_p, A.fp)   # handles and buffers: an address (device pointers are integers on the Python side)
    return {"uint32_t": C.c_uint32, "int": C.c_int, "float": C.c_float}[c_param]


def test_range_entry_points_match_the_headers(pkg, tmp_path):
    A, AO = pkg._abi, pkg._abi_ao
    src = ['#include "mi355ao.h"']
    for name, (ctype, _) in PROTOTYPES.items():
        src.append(f'_Static_assert(__builtin_types_compatible_p(__typeof__({name}), {ctype}), "{name}");')
    src.append("int main(void) { return 0; }")
    cfile = tmp_path / "probe.c"; cfile.write_text("\n".join(src))
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, "-c", str(cfile), "-o", str(tmp_path / "probe.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    libs = {"pt": C.CDLL(pkg.runtime.LIB_PATH), "ao": C.CDLL(pkg.runtime.AO_LIB_PATH)}
    for name, (ctype, where) in PROTOTYPES.items():
        res, args = (A.ENTRY_POINTS if where == "pt" else AO.ENTRY_POINTS)[name]
        params = ctype[ctype.index("(") + 1:-1].split(",")
        assert res is C.c_int and len(args) == len(params), name
        for got, c_param in zip(args, params):
            want = _ctype_of(c_param, A, AO)
            assert got in want if isinstance(want, tuple) else got is want, (name, c_param, got)
        getattr(libs[where], name)   # exported


SCENE = ('LookAt 0 0 -1  0 0 0  0 1 0\nCamera "perspective" "float fov" 30\nFilm "image" "integer xresolution" 16 "integer yresolution" 16\n'
         'Sampler "sobol" "integer pixelsamples" 4\nWorldBegin\n'
         'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-100 -100 0 100 -100 0 100 100 0 -100 100 0]\nWorldEnd\n')


@pytest.mark.parametrize("arg", ["3:2", "2:2", "1", ":3", "2:", "a:b", "-1:2", "0:5", "4:9", "0:99999999999"])
def test_mi355pbrt_refuses_malformed_sample_ranges_before_any_gpu_call(pkg, tmp_path, arg):
    scene = tmp_path / "s.pbrt"; scene.write_text(SCENE)
    out = tmp_path / "o.pfm"
    r = subprocess.run([pkg.frontend.CLI_PATH, str(scene), "--outfile", str(out), "--samples", arg], capture_output=True, text=True, timeout=60, env=no_device_env())   # a usage error must come first
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "usage:" in r.stderr and "--samples" in r.stderr and not out.exists()


def test_checkpoint_round_trip_and_refusal(pkg, tmp_path):
    F = pkg.frontend
    rp = F.FrontScene(text=SCENE).render_params()
    hdr = F.checkpoint_header(rp, first_sample=1, samples_done=2)
    assert (hdr.width, hdr.height, hdr.spp, hdr.magic, hdr.version) == (16, 16, 4, F.PTF_CHECKPOINT_MAGIC, 1)
    film = np.random.default_rng(3).normal(size=(16, 16, 4)).astype(np.float32)
    path = tmp_path / "job.ckpt"
    assert F.read_checkpoint(path, hdr)[0] == 0   # no file: nothing done
    F.write_checkpoint(path, hdr, film)
    assert os.path.getsize(path) == C.sizeof(F.PtfCheckpointHeader) + film.nbytes and not os.path.exists(str(path) + ".tmp")
    done, back = F.read_checkpoint(path, F.checkpoint_header(rp, first_sample=1))
    assert done == 2 and np.array_equal(back.view(np.uint32), film.view(np.uint32))
    # schedule knobs do not change the job; anything that changes the film does
    rp.spp_per_pass = 3; rp.profile = 1
    assert F.read_checkpoint(path, F.checkpoint_header(rp, first_sample=1))[0] == 2
    for change in (dict(spp=8), dict(max_depth=rp.max_depth + 1), dict(sampler_type=1), dict(first_sample=0)):
        rp2 = F.FrontScene(text=SCENE).render_params(); first = change.pop("first_sample", 1)
        for k, v in change.items():
            setattr(rp2, k, v)
        with pytest.raises(ValueError, match="not of this job"):
            F.read_checkpoint(path, F.checkpoint_header(rp2, first_sample=first))
    ao = pkg._abi_ao.PtAOParams(8, 1)
    with pytest.raises(ValueError, match="not of this job"):
        F.read_checkpoint(path, F.checkpoint_header(rp, ao=ao, first_sample=1))
    small = F.checkpoint_header(rp, first_sample=1); small.width = 8
    with pytest.raises(ValueError, match="film size"):
        F.read_checkpoint(path, small)
    with open(path, "r+b") as f:   # a truncated film
        f.truncate(C.sizeof(F.PtfCheckpointHeader) + 100)
    with pytest.raises(ValueError, match="truncated"):
        F.read_checkpoint(path, hdr)
    path.write_bytes(b"not a checkpoint" * 4)
    with pytest.raises(ValueError, match="not a checkpoint"):
        F.read_checkpoint(path, hdr)


def test_front_end_table_names_what_the_header_declares(pkg):
    import re
    F = pkg._abi_front
    header = open(os.path.join(INC, "mi355front.h")).read()
    declared = set(re.findall(r"\b(ptf_\w+)\(", header))
    assert declared == set(F.ENTRY_POINTS) and len(declared) == 15
    for name, result in dict(ptf_last_error=C.c_char_p, ptf_output_filename=C.c_char_p, ptf_scene_desc=C.POINTER(pkg._abi.PtSceneDesc),
                             ptf_render_params=C.POINTER(pkg._abi.PtRenderParams), ptf_params_hash=C.c_uint64, ptf_scene_destroy=None).items():
        assert F.ENTRY_POINTS[name][0] is result, name
    assert all(res is C.c_int for name, (res, _) in F.ENTRY_POINTS.items() if re.search(r"\bint %s\(" % name, header))
    L = pkg.frontend.lib()   # bound through the table, and the names frontend.py had before it are still there
    assert all(getattr(L, name).argtypes == args and getattr(L, name).restype is res for name, (res, args) in F.ENTRY_POINTS.items())
    assert pkg.frontend.PtfCheckpointHeader is F.PtfCheckpointHeader and pkg.frontend.PTF_CHECKPOINT_MAGIC == F.PTF_CHECKPOINT_MAGIC and pkg.frontend.ENTRY_POINTS is F.ENTRY_POINTS


def test_checkpoint_header_matches_the_ctypes_mirror(pkg):
    H = pkg._abi_front.PtfCheckpointHeader
    fields = [name for name, _ in H._fields_]
    assert_mirror("mi355front.h", {H: fields})
    assert [int(v) for v in c99_probe("mi355front.h", 'printf("%u", PTF_CHECKPOINT_MAGIC);')] == [pkg._abi_front.PTF_CHECKPOINT_MAGIC]
    assert fields == ["magic", "version", "width", "height", "spp", "first_sample", "samples_done", "reserved", "params_hash"] and C.sizeof(H) == 40


def test_one_table_of_libraries(pkg):
    R = pkg.runtime
    assert list(R.LIBRARIES) == ["pt", "ao", "aov", "dn", "bake"]
    for name, (sub, file, abi, header) in R.LIBRARIES.items():
        assert os.path.isfile(os.path.join(INC, header)) and os.path.isdir(os.path.join(os.path.dirname(R.__file__), sub)), name
        assert abi.ENTRY_POINTS and R.LIB_PATHS[name].endswith(os.path.join(sub, file)) or (name == "pt" and os.environ.get("PT_LIB_PATH")), name
    assert (R.LIB_PATH, R.AO_LIB_PATH, R.AOV_LIB_PATH, R.DN_LIB_PATH) == tuple(R.LIB_PATHS[k] for k in ("pt", "ao", "aov", "dn"))
    # build()'s checks and Library's loaders read that table: nobody else spells the files' names
    runtime = open(R.__file__).read()
    entry = "\n".join(line.split("#")[0] for line in open(os.path.join(ROOT, "__graft_entry__.py")).read().splitlines())
    for file in ("libmi355ao.so", "libmi355aov.so", "libmi355dn.so", "libmi355bake.so"):
        assert runtime.count(file) == 1 and entry.count(file) == 0, file
    assert "LIBRARIES" in entry and "ENTRY_POINTS" in entry
