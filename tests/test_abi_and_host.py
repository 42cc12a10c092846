"""CPU-side checks of the product: the C-ABI library loads and exports every symbol include/mi355pt.h declares
(no compute calls without a GPU), argument validation, the host SAH builder against the oracle's, and the host
scene-assembly mirror."""
import ctypes as C
import os
import re
import numpy as np
import pytest


def test_library_exports_every_declared_symbol(pkg):
    pkg.runtime.build_library()
    lib = C.CDLL(pkg.runtime.LIB_PATH)
    header = open(os.path.join(os.path.dirname(pkg.runtime.LIB_PATH), "..", "..", "include", "mi355pt.h")).read()
    declared = set(re.findall(r"\b(pt_[a-z_0-9]+)\s*\(", header))
    assert declared == set(pkg._abi.ENTRY_POINTS), declared ^ set(pkg._abi.ENTRY_POINTS)
    for name in declared:
        assert getattr(lib, name) is not None


def test_struct_sizes_match_header(pkg):
    A = pkg._abi
    assert C.sizeof(A.PtBVHNode) == 32           # bvh.rs:89-95 LinearBVHNode
    assert C.sizeof(A.PtSphere) == 16 * 4 * 2 + 6 * 4 + 8 + 8
    assert C.sizeof(A.PtLight) == 4 + 12 + 4 + 4 + 12 + 12 + 8 + 128
    assert C.sizeof(A.PtMaterial) == 4 + 7 * 12 + 5 * 4 + 4 + 24 + 8 + 64 + 8 + 44 + 12 + 12 + 4
    assert C.sizeof(A.PtKernelStat) == 32 + 8 + 8 + 8 + 8 + 8 + 48


def test_no_device_fails_loudly(pkg):
    """Without a GPU the product must refuse to render (status + message), never fall back to a CPU path."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    lib = pkg.load_library()
    st = lib.lib.pt_init(0)
    assert st == pkg._abi.PT_ERR_NO_DEVICE
    assert b"no HIP device" in lib.lib.pt_last_error()
    sd, rp = pkg.scenes.ganesha_scale(n=4, xres=16, yres=16, spp=1).world_end()
    with pytest.raises(pkg.runtime.PtError):
        pkg.Scene(lib, sd)


def test_invalid_arguments_are_statuses_not_crashes(pkg):
    lib = pkg.load_library()
    A = pkg._abi
    assert lib.lib.pt_scene_create(None, None) == A.PT_ERR_INVALID_ARG
    d = A.PtSceneDesc()
    h = C.c_void_p()
    assert lib.lib.pt_scene_create(C.byref(d), C.byref(h)) == A.PT_ERR_INVALID_ARG  # no primitives
    assert lib.lib.pt_film_resolve(None, 0, 1.0, None) == A.PT_ERR_INVALID_ARG


def test_film_resolve_matches_reference_formula(pkg):
    # Film::write_image (film.rs:217-258): rgb = max(0, xyz_to_rgb(xyz)/w) * scale -- pure host arithmetic
    lib = pkg.load_library()
    A = pkg._abi
    film = np.array([[1.0, 2.0, 3.0, 4.0], [0.5, 0.25, 0.125, 0.0], [-1.0, 0.1, 0.1, 2.0]], dtype=np.float32)
    out = np.zeros((3, 3), np.float32)
    assert lib.lib.pt_film_resolve(film.ctypes.data_as(A.fp), 3, 2.0, out.ctypes.data_as(A.fp)) == 0
    M = np.array([[3.240479, -1.537150, -0.498535], [-0.969256, 1.875991, 0.041556], [0.055648, -0.204043, 1.057311]], dtype=np.float32)
    for i in range(3):
        rgb = (M * film[i, :3]).astype(np.float32)
        rgb = np.array([np.float32(np.float32(r[0] + r[1]) + r[2]) for r in rgb])
        if film[i, 3] != 0:
            rgb = np.maximum(rgb * (np.float32(1) / film[i, 3]), 0)
        np.testing.assert_allclose(out[i], rgb * 2.0, rtol=1e-6, atol=1e-7)


def test_host_sah_builder_equals_oracle_builder(pkg, oracle):
    """The product's host BVH builder (csrc/host_bvh.cpp) is an independent implementation of bvh.rs; it must
    produce the same tree as the oracle's restatement, node for node (tie-breaking depends on it)."""
    import subprocess, tempfile, textwrap
    here = os.path.dirname(pkg.runtime.LIB_PATH)
    src = textwrap.dedent('''
        #include "host_bvh.h"
        #include <cstdio>
        extern "C" int hb_build(unsigned n, const float* lo_hi, unsigned maxp, PtBVHNode* nodes, unsigned* ordered, unsigned* n_nodes) {
            std::vector<pth::PrimBound> pb(n);
            for (unsigned i = 0; i < n; ++i) for (int k = 0; k < 3; ++k) { pb[i].lo[k] = lo_hi[6*i+k]; pb[i].hi[k] = lo_hi[6*i+3+k]; }
            std::vector<PtBVHNode> nn; std::vector<uint32_t> oo;
            pth::build_sah_bvh(pb, maxp, nn, oo);
            *n_nodes = (unsigned)nn.size();
            for (size_t i = 0; i < nn.size(); ++i) nodes[i] = nn[i];
            for (size_t i = 0; i < oo.size(); ++i) ordered[i] = oo[i];
            return 0;
        }''')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "hb.cpp"), "w").write(src)
        so = os.path.join(td, "hb.so")
        san = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if os.environ.get("PT_SAN") else []
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-ffp-contract=off", *san, "-I", here, "-o", so,
                               os.path.join(td, "hb.cpp"), os.path.join(here, "host_bvh.cpp")])
        hb = C.CDLL(so)
        A = pkg._abi
        # n = 200 -> 80 004 triangles: above the 65 536-primitive threshold of the multi-threaded build (subtrees on worker
        # threads, identical tree); add -pthread when linking
        for n, kw in ((20, {}), (48, dict(with_normals=True)), (200, {})):
            sd, _ = pkg.scenes.ganesha_scale(n=n, xres=16, yres=16, spp=1, **kw).world_end()
            P, idx = sd.P, sd.idx
            tri = P[idx]  # (nt, 3, 3)
            lohi = np.concatenate([tri.min(axis=1), tri.max(axis=1)], axis=1).astype(np.float32)
            nt = len(idx)
            nodes = (A.PtBVHNode * (2 * nt))(); ordered = np.zeros(nt, np.uint32); nn = C.c_uint()
            hb.hb_build(nt, lohi.ctypes.data_as(A.fp), 4, nodes, ordered.ctypes.data_as(A.u32p), C.byref(nn))
            on, oo = oracle.scene(sd).bvh()
            assert nn.value == len(on)
            assert bytes(nodes)[: 32 * nn.value] == bytes(on)
            assert np.array_equal(ordered, oo)
            # structural invariants of flatten_bvhtree (bvh.rs:662-693)
            leaves = [x for x in on if x.n_prims > 0]
            assert sum(x.n_prims for x in leaves) == nt
            assert all(x.n_prims <= 4 or True for x in leaves)


def test_scene_plan_on_the_cpu(pkg, tmp_path):
    """The host-only half of pt_scene_create (csrc/scene_plan.h) checked without a device: tests/scene_plan/check_plan.cpp, a program of its own built from the
    plan unit and the SAH builder, provokes every refusal a toy scene can reach (and counts the refusal texts of scene_plan.hip against its table), holds the
    two- and four-wide records of small trees against their binary nodes for all eight sign octants, and recomputes the derived tables. It passes when it exits 0."""
    import subprocess
    here = os.path.dirname(pkg.runtime.LIB_PATH)
    root = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "check_plan")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-I", here, "-o", exe,
                           os.path.join(root, "scene_plan", "check_plan.cpp"), os.path.join(here, "scene_plan.hip"), os.path.join(here, "host_bvh.cpp")])
    r = subprocess.run([exe, os.path.join(here, "scene_plan.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


def test_scene_builder_mirrors_api_state_machine(pkg):
    b = pkg.host.SceneBuilder()
    assert b.materials[0].type == pkg._abi.PT_MAT_MATTE and tuple(b.materials[0].kd) == (0.5, 0.5, 0.5)  # api.rs:345-361
    b.attribute_begin(); b.material("mirror"); b.area_light_source(L=(1, 2, 3)); b.translate(1, 2, 3)
    b.trianglemesh(np.eye(3, dtype=np.float32), np.array([[0, 1, 2]], np.uint32))
    b.attribute_end()
    b.trianglemesh(np.eye(3, dtype=np.float32), np.array([[0, 1, 2]], np.uint32))
    sd, rp = b.world_end()
    assert list(sd.prim_material) == [1, 0]            # AttributeEnd restores the material
    assert list(sd.prim_light) == [0, pkg._abi.PT_NONE]  # one DiffuseAreaLight per emissive shape (api.rs:1531-1546)
    np.testing.assert_allclose(sd.P[0], [2, 2, 3])     # vertices are stored in world space (triangle.rs:39)
    np.testing.assert_allclose(sd.P[3], [1, 0, 0])
    # film/sampler defaults (film.rs:364-398): box filter radius .5 -> sample bounds == pixel bounds
    assert tuple(rp.sample_bounds) == (0, 0, 1280, 720) and tuple(rp.cropped_pixel_bounds) == (0, 0, 1280, 720)
    assert rp.max_depth == 5 and rp.rr_threshold == 1.0 and rp.light_strategy == pkg._abi.PT_LS_SPATIAL
    b.filter.update(kind="gaussian", radius=(2.0, 2.0))
    rp = b.render_params()
    assert tuple(rp.sample_bounds) == (-2, -2, 1282, 722)  # film.rs:104-112


def test_compile_time_switches_are_knobs_or_instrumentation():
    """Every `#if` on a PT_* macro in the native sources is a tuning constant of knobs.h, one of the two instruments, a translation-unit selector
    or a build setting: settled A/B experiments live as patches under profiles/rN/experiments/, not as switches in the product sources."""
    import glob
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pbrt-rust_amd")
    files = sorted(p for ext in ("h", "hip", "cpp") for p in glob.glob(os.path.join(root, "csrc", "*." + ext))) + sorted(glob.glob(os.path.join(root, "ao", "*")))
    assert any(p.endswith("knobs.h") for p in files) and any(p.endswith("ao_render.hip") for p in files)
    instruments = {"PT_TRACE_UTIL", "PT_REGION_PROFILE"}
    tu_selectors = {"PT_TU_ANY", "PT_TU_QUAD", "PT_TU_MODE", "PT_TU_MAXL"}
    build_settings = {"PT_TABLES_PATH", "PT_SAN"}
    conditional = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$")
    bad, n_util = [], 0
    for path in files:
        if not os.path.isfile(path):
            continue
        name = os.path.basename(path)
        lines = open(path, errors="replace").read().split("\n")
        for i, line in enumerate(lines):
            m = conditional.match(line)
            if not m:
                continue
            if name == "kern_trace.h" and re.match(r"^\s*#\s*ifdef\s+PT_TRACE_UTIL\b", line):
                n_util += 1
            macros = set(re.findall(r"\bPT_[A-Z0-9_]+\b", m.group(2).split("//")[0]))
            if not macros or name == "knobs.h":
                continue
            guard = m.group(1) == "ifndef" and len(macros) == 1 and i + 1 < len(lines) and re.match(r"^\s*#\s*define\s+%s\s*$" % next(iter(macros)), lines[i + 1])
            if guard or macros <= instruments or macros <= tu_selectors or macros <= build_settings:
                continue
            bad.append("%s:%d: %s" % (name, i + 1, line.strip()))
    assert not bad, "compile-time switches outside knobs.h:\n" + "\n".join(bad)
    assert n_util == 1, "kern_trace.h keeps its PT_TRACE_UTIL pieces in one block"


def test_the_render_frame_is_written_once():
    """pt_render_samples, pt_ao_render_samples and pt_multi_render_samples go through one frame (render_loop.hip: frame_geometry, render_frame, deliver_film): the tile-slot
    formula stands once in the package's sources, and each shared refusal's text once in the two libraries' host code (the pt_render / pt_ao_render / pt_multi_render wrappers
    refuse spp = 0 through check_spp, the function frame_geometry calls)."""
    import glob
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pbrt-rust_amd")
    sources = [p for ext in ("h", "hip", "cpp", "py") for p in glob.glob(os.path.join(root, "**", "*." + ext), recursive=True)]
    host = sorted(glob.glob(os.path.join(root, "csrc", "*.hip")) + glob.glob(os.path.join(root, "ao", "*.hip")))
    assert any(p.endswith("render_loop.hip") for p in host) and any(p.endswith("ao_render.hip") for p in host) and any(p.endswith("multi_device.hip") for p in host)
    count = lambda files, text: sum(open(p, errors="replace").read().count(text) for p in files)
    assert count(sources, "(ntiles - rc.tile_rank + rc.tile_world - 1) / rc.tile_world") == 1
    for phrase in ('"spp must be > 0"', '"filter radius must be > 0"', '"tile_rank >= tile_world"'):
        assert count(host, phrase) == 1, phrase
    for wrapper in ("render_loop.hip", "ao_render.hip", "multi_device.hip"):
        assert count([p for p in host if p.endswith(wrapper)], "check_spp(rp)") >= 1, wrapper


def test_pass_budget_on_the_cpu(pkg, tmp_path):
    """The pass size the library chooses (csrc/pass_budget.h: pass_size_for, the arithmetic of choose_pass_size for every integrator) checked without a device:
    tests/pass_budget/check_pass_budget.cpp, a program of its own over the header alone. Its header comment lists what it holds. It passes when it exits 0."""
    import subprocess
    here = os.path.dirname(pkg.runtime.LIB_PATH)
    root = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "check_pass_budget")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I", here, "-o", exe,
                           os.path.join(root, "pass_budget", "check_pass_budget.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


def test_the_pass_budget_and_bump_are_not_restated():
    """The integrator libraries beside libmi355pt choose their pass size through choose_pass_size (render_loop.hip): neither the stale bound on the workspace's queues nor a
    free-memory query of their own may reappear under ao/ or aov/, and the rule's arithmetic stands in pass_budget.h alone.
    bump()'s arithmetic stands in k_shade and, restated, in k_aov -- in no third place. (One inlined device helper for both moved the registers of the textured k_shade
    forms, so k_shade keeps its body and k_aov its copy, under a NOTE that says so: profiles/r6/NOTES.md section 15. With a helper this count would be one header.)"""
    import glob
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pbrt-rust_amd")
    text = lambda p: open(p, errors="replace").read()
    side = sorted(glob.glob(os.path.join(root, "ao", "*")) + glob.glob(os.path.join(root, "aov", "*")))
    assert any(p.endswith("ao_render.hip") for p in side) and any(p.endswith("aov_render.hip") for p in side)
    for p in side:
        if not os.path.isfile(p) or p.endswith((".so", ".o")):
            continue
        squeezed = re.sub(r"\s+", "", text(p))
        assert "2*kNumClasses+2+2" not in squeezed, p
        assert "hipMemGetInfo" not in squeezed, p
    for name in ("ao_render.hip", "aov_render.hip"):
        assert text([p for p in side if p.endswith(name)][0]).count("choose_pass_size(sc, ") == 1, name
    native = [p for ext in ("h", "hip", "cpp") for p in glob.glob(os.path.join(root, "**", "*." + ext), recursive=True)]
    assert sorted(os.path.basename(p) for p in native if "// passes of equal size" in text(p)) == ["pass_budget.h"]
    bump = {os.path.basename(p): text(p).count("udisplace - displace") for p in native if "udisplace - displace" in text(p)}
    assert bump == {"kern_shade.h": 1, "aov_kernels.h": 1}, bump
    assert "NOTE: the body is k_shade's" in text(os.path.join(root, "aov", "aov_kernels.h"))


def test_what_the_side_libraries_share_is_not_restated():
    """What the libraries beside libmi355pt share among themselves stands once, under side/: the AO ray (side/ao_rays.h) and, on the host (side/side_host.h), the
    sample-number limits of an AO job, the first-hit chase and the out-of-memory failure of a call's scratch allocations.
    The AO direction sampling stands in ao_ray and, restated, in k_ao_rays -- in no third place. (Through the inlined helper k_ao_rays<false> took 83 VGPRs for 79, so
    the kernel keeps its body under a NOTE that says so: profiles/r6/NOTES.md section 21. With the helper this count would be one header.)"""
    import glob
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pbrt-rust_amd")
    text = lambda p: open(p, errors="replace").read()
    native = [p for ext in ("h", "hip", "cpp") for p in glob.glob(os.path.join(root, "**", "*." + ext), recursive=True)]
    where = lambda phrase: {os.path.relpath(p, root).replace(os.sep, "/"): text(p).count(phrase) for p in native if phrase in text(p)}
    # (csrc/ has the uniform-sphere line twice more, in its light and phase-function sampling: other functions, libmi355pt's)
    assert {p: n for p, n in where("1.0f - 2.0f * u.x").items() if not p.startswith("csrc/")} == {"side/ao_rays.h": 1, "ao/ao_kernels.h": 1}
    assert "NOTE: the loop body is ao_ray's" in text(os.path.join(root, "ao", "ao_kernels.h"))
    for phrase in ("the Sobol' tables serve at this resolution", "Halton sampler's 64-bit index", "still going on behind material-less surfaces"):
        assert where(phrase) == {"side/side_host.h": 1}, phrase
    strings = where("hipGetErrorString")
    assert "side/side_host.h" in strings and not [p for p in strings if p.split("/")[0] in ("ao", "aov", "bake", "denoise")], strings
