"""The C ABI of the feature buffers (include/mi355aov.h, libmi355aov.so) without a GPU: the header against the ctypes mirror, the library's exports, pt_aov_resolve
(host arithmetic) and the argument errors that return before the device is touched."""
import ctypes as C
import os

import numpy as np
from abi_checks import ROOT, assert_mirror, exported_names


def test_mi355aov_header_is_c99_and_matches_the_ctypes_mirror(pkg):
    A = pkg._abi_aov
    assert_mirror("mi355aov.h", {A.PtAOVBuffers: [p + "_w" for p in A.PLANES]})
    assert A.PLANES == ("albedo", "normal", "depth")

def test_aov_library_exports_only_its_entry_points(pkg):
    assert exported_names(pkg.runtime.AOV_LIB_PATH) == set(pkg._abi_aov.ENTRY_POINTS)
    header = open(os.path.join(ROOT, "include", "mi355aov.h")).read()
    for name in pkg._abi_aov.ENTRY_POINTS:
        assert f"int {name}(" in header, name


def test_resolve_on_hand_made_sums(pkg):
    lib = pkg.load_library()
    sums = {"albedo": np.array([[[2.0, 4.0, 6.0, 2.0], [1.0, 1.0, 1.0, 0.0], [0.0, 0.0, 0.0, 3.0]]], np.float32),   # hits, nothing at all, misses only
            "normal": np.array([[[0.0, 3.0, 4.0, 2.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]]], np.float32),
            "depth": np.array([[[6.0, 2.0], [5.0, 0.0], [0.0, 0.0]]], np.float32)}
    out = pkg.runtime.resolve_aov(sums, lib)
    assert out["albedo"].shape == (1, 3, 3) and out["normal"].shape == (1, 3, 3) and out["depth"].shape == (1, 3)
    assert np.array_equal(out["albedo"][0], np.array([[1, 2, 3], [0, 0, 0], [0, 0, 0]], np.float32))
    assert np.array_equal(out["normal"][0], np.array([[0.0, np.float32(3.0) / np.float32(5.0), np.float32(4.0) / np.float32(5.0)], [0, 0, 0], [0, 0, 0]], np.float32))
    assert np.array_equal(out["depth"][0], np.array([3, 0, 0], np.float32))
    # a plane that is not there is skipped, and the others are resolved all the same
    only = pkg.runtime.resolve_aov({"depth": sums["depth"]}, lib)
    assert list(only) == ["depth"] and np.array_equal(only["depth"], out["depth"])
    assert lib.aov.pt_aov_resolve(None, 3, None, None, None) == pkg._abi.PT_ERR_INVALID_ARG


def test_argument_errors_return_before_the_device_is_touched(pkg):
    """NULL arguments, no plane at all and bad sample ranges are refused by host arithmetic: no device is needed, and the scene handle -- any non-NULL value here -- is
    never looked at. The buffers keep their contents."""
    A, V = pkg._abi, pkg._abi_aov
    lib = pkg.load_library()
    aov = lib.aov
    scene = C.c_void_p(8)
    rp = pkg.scenes.spheres_c1(xres=8, yres=8, spp=8).render_params()
    plane = np.full((8, 8, 4), 7.0, np.float32)
    bufs = V.PtAOVBuffers(plane.ctypes.data_as(A.fp), None, None)
    none = V.PtAOVBuffers(None, None, None)
    bad = A.PT_ERR_INVALID_ARG
    assert aov.pt_aov_render(None, C.byref(rp), C.byref(bufs), 0) == bad
    assert aov.pt_aov_render(scene, None, C.byref(bufs), 0) == bad
    assert aov.pt_aov_render(scene, C.byref(rp), None, 0) == bad
    assert aov.pt_aov_render(scene, C.byref(rp), C.byref(none), 0) == bad
    assert b"planes" in lib.lib.pt_last_error()
    assert aov.pt_aov_render_samples(None, C.byref(rp), 0, 1, C.byref(bufs), 0) == bad
    assert aov.pt_aov_render_samples(scene, C.byref(rp), 0, 1, C.byref(none), 0) == bad
    for first, n in ((0, 0), (6, 3), (2 ** 32 - 1, 2)):
        assert aov.pt_aov_render_samples(scene, C.byref(rp), first, n, C.byref(bufs), 0) == bad, (first, n)
    size = C.c_uint32(5)
    assert aov.pt_aov_pass_size(None, C.byref(rp), C.byref(size)) == bad and aov.pt_aov_pass_size(scene, None, C.byref(size)) == bad
    assert aov.pt_aov_pass_size(scene, C.byref(rp), None) == bad and size.value == 5
    rp.spp = 0
    assert aov.pt_aov_render(scene, C.byref(rp), C.byref(bufs), 0) == bad
    assert (plane == 7.0).all()
