"""Test infrastructure: libdevprobe.so, the device probes of tests/device_probe/*.hip (test code around the UNMODIFIED headers of pbrt-rust_amd/csrc),
built once per session. The translation units compile in parallel with the HIPFLAGS line of pbrt-rust_amd/csrc/Makefile (a different -ffp-contract would
change bits) plus -fvisibility=hidden, and link against libmi355pt.so the way libmi355ao.so does (pth::material_class, pth::launch_trace)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pbrt-rust_amd", "csrc")
PROBE_SRC = os.path.join(ROOT, "tests", "device_probe")
UNITS = ("bsdf_probe", "light_probe", "interaction_probe", "bssrdf_probe")
BSDF_WORDS, LIGHT_WORDS, INTERACTION_WORDS = 18, 8, 45
# bssrdf_probe.hip's sections in order, each with its words in and out per query: the layout of the oracle's orc_bssrdf_eval
BSSRDF_SECTIONS = (("state", 0, 19), ("radii", 1, 6), ("samples", 1, 3), ("exits", 6, 4), ("segments", 3, 8), ("adapter", 9, 12), ("conversion", 6, 6))
_BUILT = {}


def makefile_hipflags():
    """(hipcc, flags, arch) as pbrt-rust_amd/csrc/Makefile holds them: the HIPFLAGS line with $(ARCH) expanded and $(EXTRA_HIPFLAGS) empty."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M).group(1).strip()
    flags = var("HIPFLAGS").replace("$(ARCH)", var("ARCH")).replace("$(EXTRA_HIPFLAGS)", "")
    assert "$(" not in flags and "-ffp-contract=off" in flags, flags
    return os.environ.get("HIPCC") or var("HIPCC"), flags.split(), var("ARCH")


def compile_units(out, names=UNITS):
    """hipcc -c of tests/device_probe/<name>.hip into `out`, all at once; the object paths."""
    hipcc, flags, _ = makefile_hipflags()
    objs = [os.path.join(out, n + ".o") for n in names]
    jobs = [subprocess.Popen([hipcc] + flags + ["-fvisibility=hidden", "-c", "-o", obj, os.path.join(PROBE_SRC, n + ".hip")],
                             stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for n, obj in zip(names, objs)]
    for n, j in zip(names, jobs):
        log = j.communicate()[0]
        assert j.returncode == 0, f"hipcc {n}.hip failed:\n{log[-4000:]}"
    return objs


def probe_library(pkg, out=None):
    """The bound libdevprobe.so of this session (built into `out`, by default a temporary directory of its own, on the first call)."""
    if "lib" in _BUILT:
        return _BUILT["lib"]
    if out is None:
        _BUILT["dir"] = tempfile.TemporaryDirectory(prefix="device_probe_")   # (kept alive with the library)
        out = _BUILT["dir"].name
    out = str(out)
    hipcc, _, arch = makefile_hipflags()
    objs = compile_units(out)
    so = os.path.join(out, "libdevprobe.so")
    libdir = os.path.dirname(pkg.runtime.LIB_PATH)
    r = subprocess.run([hipcc, "-shared", "-fPIC", f"--offload-arch={arch}", "-o", so] + objs + ["-L" + libdir, "-lmi355pt", "-Wl,-rpath," + libdir],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    A = pkg._abi
    lib = C.CDLL(so)
    u32, i32, vp, u32p, i32p, fp = C.c_uint32, C.c_int32, C.c_void_p, A.u32p, A.i32p, A.fp
    for name, res, args in (("probe_bsdf_words", u32, []), ("probe_light_words", u32, []), ("probe_interaction_words", u32, []),
                            ("probe_material_class", C.c_int, [C.POINTER(A.PtMaterial), u32, u32, i32p, i32p]),
                            ("probe_bsdf", C.c_int, [vp, C.c_int, C.c_int, u32, u32, fp, fp, fp, u32p]),
                            ("probe_light_count", C.c_int, [vp, u32p, i32p]),
                            ("probe_light", C.c_int, [vp, u32, u32, fp, fp, fp, fp, fp, u32p]),
                            ("probe_interaction", C.c_int, [vp, C.c_int, u32, fp, fp, fp, u32p]),
                            ("probe_bssrdf_sections", u32, []), ("probe_bssrdf_words_in", u32, [u32]), ("probe_bssrdf_words", u32, [u32]),
                            ("probe_bssrdf", C.c_int, [vp, u32, C.c_int, C.c_int, fp, u32, fp, u32p])):
        fn = getattr(lib, name); fn.restype = res; fn.argtypes = args
    assert lib.probe_bsdf_words() == BSDF_WORDS and lib.probe_light_words() == LIGHT_WORDS and lib.probe_interaction_words() == INTERACTION_WORDS
    assert lib.probe_bssrdf_sections() == len(BSSRDF_SECTIONS)
    assert [(lib.probe_bssrdf_words_in(k), lib.probe_bssrdf_words(k)) for k in range(len(BSSRDF_SECTIONS))] == [(a, b) for _, a, b in BSSRDF_SECTIONS]
    _BUILT["lib"] = lib
    return lib
