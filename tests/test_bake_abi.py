"""The bake's C ABI without a GPU (include/mi355bake.h, libmi355bake.so): the header under C99, the structs against the ctypes mirror, the export list, the refusals
that return before the device is touched, and pt_bake_resolve (host arithmetic) against the model."""
import os
import re

import numpy as np
import bake_reference as M
from abi_checks import ROOT, assert_bound, assert_mirror, embedded_kernel_names, exported_names, run_without_device

P_FIELDS = ("width", "height", "spp", "nsamples", "cos_sample", "max_distance", "sampler_type", "spp_per_pass", "profile")
B_FIELDS = ("owner", "position", "normal", "ao_w")


def test_the_header_is_c99_and_the_structs_match_the_ctypes_mirror(pkg):
    K = pkg._abi_bake
    assert assert_mirror("mi355bake.h", {K.PtBakeParams: P_FIELDS, K.PtBakeBuffers: B_FIELDS}) == [36, 32]
    assert list(B_FIELDS) == list(K.PLANES)


def test_the_library_exports_what_its_map_names_and_the_header_declares(pkg):
    R = pkg.runtime
    assert R.LIBRARIES["bake"] == ("bake", "libmi355bake.so", pkg._abi_bake, "mi355bake.h") and not hasattr(R, "ATLAS_LIBRARIES") and not hasattr(R, "ALL_LIBRARIES")
    names = exported_names(R.LIB_PATHS["bake"])
    assert names == set(pkg._abi_bake.ENTRY_POINTS)
    pattern = re.search(r"global:\s*([^;]+);", open(os.path.join(ROOT, "pbrt-rust_amd", "bake", "exports.map")).read()).group(1).strip()
    assert pattern == "pt_bake_*" and all(n.startswith("pt_bake_") for n in names)
    header = open(os.path.join(ROOT, "include", "mi355bake.h")).read()
    declared = set(re.findall(r"^int (pt_\w+)\(", header, re.M))
    assert declared == names
    assert_bound(pkg.load_library().bake, pkg._abi_bake.ENTRY_POINTS)


def test_no_bake_kernel_uses_scratch(pkg):
    """The gfx950 code objects inside the built library: every kernel's .private_segment_fixed_size is 0, and the kernels are the ones the sources name."""
    kernels = embedded_kernel_names(pkg.runtime.LIB_PATHS["bake"])
    want = ["k_bake_top", "k_bake_check", "k_bake_raster", "k_bake_points", "k_bake_rays", "k_bake_accum", "k_bake_dilate", "k_bake_covered", "k_bake_probe"]
    assert kernels and all("6ptbake" in n for n in kernels), sorted(kernels)
    for k in want:
        assert any(k in n for n in kernels), (k, sorted(kernels))
    assert sum("k_bake_dilate" in n for n in kernels) == 4
    assert {n: v for n, v in kernels.items() if v != 0} == {}


def test_refusals_return_before_the_device_is_touched(pkg):
    """Run in a child process with no visible device: a call that reached the device would fail with another status (or not return)."""
    n = run_without_device(r'''
K = pkg._abi_bake; bake = lib.bake
scene = C.c_void_p(8)   # never looked at
def params(**kw):
    d = dict(width=8, height=8, spp=4, nsamples=8, cos_sample=1, max_distance=float("inf"), sampler_type=0, spp_per_pass=0, profile=0); d.update(kw)
    return K.PtBakeParams(*[d[k] for k, _ in K.PtBakeParams._fields_])
planes = {"owner": np.full((8, 8), 5, np.uint32), "position": np.full((8, 8, 3), 7.0, np.float32), "normal": np.full((8, 8, 3), 7.0, np.float32), "ao_w": np.full((8, 8, 4), 7.0, np.float32)}
kept = {k: v.copy() for k, v in planes.items()}
ok, none = K.buffers(planes), K.buffers({})
sel = np.ones(5, np.uint8); nosel = np.zeros(5, np.uint8)
sp, np_ = sel.ctypes.data_as(A.u8p), nosel.ctypes.data_as(A.u8p)
p = params()
refused(bake.pt_bake_render(None, C.byref(p), sp, 5, C.byref(ok), 0), b"null")
refused(bake.pt_bake_render(scene, None, sp, 5, C.byref(ok), 0), b"null")
refused(bake.pt_bake_render(scene, C.byref(p), None, 5, C.byref(ok), 0), b"null")
refused(bake.pt_bake_render(scene, C.byref(p), sp, 5, None, 0), b"null")
refused(bake.pt_bake_render_samples(None, C.byref(p), sp, 5, 0, 1, C.byref(ok), 0), b"null")
for kw, text in ((dict(width=0), b"width"), (dict(height=0), b"height"), (dict(width=1 << 15, height=1 << 14), b"2^28"), (dict(spp=0), b"spp"), (dict(nsamples=0), b"nsamples"),
                 (dict(max_distance=0.0), b"max_distance"), (dict(max_distance=-1.0), b"max_distance"), (dict(max_distance=float("nan")), b"max_distance"), (dict(sampler_type=2), b"sampler")):
    q = params(**kw)
    refused(bake.pt_bake_render(scene, C.byref(q), sp, 5, C.byref(ok), 0), text)
    refused(bake.pt_bake_render_samples(scene, C.byref(q), sp, 5, 0, 1, C.byref(ok), 0), text)
    size = C.c_uint32(5)
    refused(bake.pt_bake_pass_size(scene, C.byref(q), C.byref(size)), text)
    assert size.value == 5
refused(bake.pt_bake_render(scene, C.byref(p), sp, 5, C.byref(none), 0), b"planes")
refused(bake.pt_bake_render(scene, C.byref(p), np_, 5, C.byref(ok), 0), b"selected")
refused(bake.pt_bake_render(scene, C.byref(p), sp, 0, C.byref(ok), 0), b"selected")
for first, n in ((0, 0), (2, 3), (2 ** 32 - 1, 2)):
    refused(bake.pt_bake_render_samples(scene, C.byref(p), sp, 5, first, n, C.byref(ok), 0), b"n_samples" if n == 0 else b"sample range")
size = C.c_uint32(5)
refused(bake.pt_bake_pass_size(None, C.byref(p), C.byref(size)), b"null"); refused(bake.pt_bake_pass_size(scene, None, C.byref(size)), b"null"); refused(bake.pt_bake_pass_size(scene, C.byref(p), None), b"null")
op, pp = planes["owner"].ctypes.data_as(A.u32p), planes["position"].ctypes.data_as(A.fp)
refused(bake.pt_bake_dilate(None, op, pp, 3, 8, 8, 1, 0), b"null"); refused(bake.pt_bake_dilate(scene, None, pp, 3, 8, 8, 1, 0), b"null"); refused(bake.pt_bake_dilate(scene, op, None, 3, 8, 8, 1, 0), b"null")
refused(bake.pt_bake_dilate(scene, op, pp, 0, 8, 8, 1, 0), b"channels"); refused(bake.pt_bake_dilate(scene, op, pp, 5, 8, 8, 1, 0), b"channels")
refused(bake.pt_bake_dilate(scene, op, pp, 3, 0, 8, 1, 0), b"width"); refused(bake.pt_bake_dilate(scene, op, pp, 3, 8, 0, 1, 0), b"height")
assert bake.pt_bake_dilate(scene, op, pp, 3, 8, 8, 0, 0) == A.PT_OK   # no iteration: nothing to do
t = np.zeros(4, np.uint32); f3 = np.zeros((4, 3), np.float32); f1 = np.zeros(4, np.float32); u8 = np.zeros(4, np.uint8)
tp, fp3, fp1, up = t.ctypes.data_as(A.u32p), f3.ctypes.data_as(A.fp), f1.ctypes.data_as(A.fp), u8.ctypes.data_as(A.u8p)
refused(bake.pt_bake_rays(scene, C.byref(p), sp, 5, 4, None, tp, tp, fp3, fp3, fp1, up), b"null")
refused(bake.pt_bake_rays(scene, C.byref(p), sp, 5, 4, tp, tp, tp, fp3, fp3, fp1, None), b"null")
refused(bake.pt_bake_rays(scene, C.byref(params(nsamples=0)), sp, 5, 4, tp, tp, tp, fp3, fp3, fp1, up), b"nsamples")
refused(bake.pt_bake_rays(scene, C.byref(p), np_, 5, 4, tp, tp, tp, fp3, fp3, fp1, up), b"selected")
four = np.full(4, 4, np.uint32)
refused(bake.pt_bake_rays(scene, C.byref(p), sp, 5, 4, tp, four.ctypes.data_as(A.u32p), tp, fp3, fp3, fp1, up), b"outside the job")
ao = np.zeros(64, np.float32); bent = np.zeros((64, 3), np.float32); aw = planes["ao_w"].ctypes.data_as(A.fp)
refused(bake.pt_bake_resolve(None, 64, 4, ao.ctypes.data_as(A.fp), bent.ctypes.data_as(A.fp)), b"null"); refused(bake.pt_bake_resolve(aw, 64, 4, None, None), b"null")
refused(bake.pt_bake_resolve(aw, 64, 0, ao.ctypes.data_as(A.fp), bent.ctypes.data_as(A.fp)), b"spp")
for k in planes:
    assert planes[k].tobytes() == kept[k].tobytes(), k
assert not ao.any() and not bent.any()
''')
    assert n == 56


def test_resolve_is_the_models(pkg):
    rng = np.random.RandomState(3)
    ao_w = rng.uniform(-1, 1, (5, 7, 4)).astype(np.float32); ao_w[..., 3] = np.abs(ao_w[..., 3]) * 9
    ao_w[0, 0] = 0; ao_w[1, 1, :3] = 0   # nothing added; a sum of directions that cancels
    ao, bent = pkg.runtime.resolve_bake(ao_w, 3)
    want_ao, want_bent = M.resolve(ao_w, 3)
    assert ao.tobytes() == want_ao.tobytes() and bent.tobytes() == want_bent.tobytes()
    assert ao[0, 0] == 0 and not bent[0, 0].any() and ao[1, 1] > 0 and not bent[1, 1].any()
