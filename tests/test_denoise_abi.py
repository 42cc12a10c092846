"""The C ABI of the denoiser (include/mi355dn.h, libmi355dn.so) without a GPU: the header against the ctypes mirror, the library's exports, the default parameters and
the argument errors that return before the device is touched."""
import ctypes as C
import os

import numpy as np
from abi_checks import ROOT, assert_mirror, exported_names
FIELDS = ["iterations", "sigma_l", "sigma_z", "sigma_n", "albedo_floor", "scale"]


def test_mi355dn_header_is_c99_and_matches_the_ctypes_mirror(pkg):
    D = pkg._abi_dn
    assert_mirror("mi355dn.h", {D.PtDenoiseParams: FIELDS}, prelude="PtAOVBuffers b = {0, 0, 0}; (void)b;\n")   # (the header brings mi355aov.h's buffers along)

def test_denoise_library_exports_only_its_entry_points(pkg):
    assert exported_names(pkg.runtime.DN_LIB_PATH) == set(pkg._abi_dn.ENTRY_POINTS)
    header = open(os.path.join(ROOT, "include", "mi355dn.h")).read()
    for name in pkg._abi_dn.ENTRY_POINTS:
        assert f" {name}(" in header, name


def test_default_params(pkg):
    lib = pkg.load_library()
    p = pkg.runtime.default_denoise_params(lib)
    assert [getattr(p, f) for f in FIELDS] == [5, 4.0, 1.0, 0.25, np.float32(0.01), 1.0]
    lib.dn.pt_denoise_default_params(None)   # ignored, not dereferenced


def test_argument_errors_return_before_the_device_is_touched(pkg):
    """Every refusal of include/mi355dn.h is host arithmetic: no device is needed, and the scene handle -- any non-NULL value here -- is never looked at. The output
    keeps its contents."""
    A, V, D = pkg._abi, pkg._abi_aov, pkg._abi_dn
    lib = pkg.load_library()
    dn = lib.dn
    scene = C.c_void_p(8)
    w, h = 8, 4
    film = np.ones((h, w, 4), np.float32)
    plane = np.ones((h, w, 4), np.float32)
    out = np.full((h, w, 3), 7.0, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    bufs = V.PtAOVBuffers(plane.ctypes.data_as(A.fp), plane.ctypes.data_as(A.fp), plane.ctypes.data_as(A.fp))
    good = pkg.runtime.default_denoise_params(lib)
    bad = A.PT_ERR_INVALID_ARG

    def call(scene=scene, params=good, a=vp(film), b=vp(film), sums=bufs, w=w, h=h, rgb=vp(out), on_device=0):
        return dn.pt_denoise(scene, C.byref(params) if params is not None else None, a, b, C.byref(sums) if sums is not None else None, w, h, rgb, on_device)

    for kw in (dict(scene=None), dict(params=None), dict(a=None), dict(b=None), dict(sums=None), dict(rgb=None)):
        assert call(**kw) == bad, kw
        assert call(on_device=1, **kw) == bad, kw
    for k in range(3):   # any NULL plane
        planes = [plane.ctypes.data_as(A.fp)] * 3; planes[k] = None
        assert call(sums=V.PtAOVBuffers(*planes)) == bad, k
        assert b"planes" in lib.lib.pt_last_error()
    assert call(w=0) == bad and call(h=0) == bad
    assert call(w=2 ** 16, h=2 ** 15 + 1) == bad   # width * height > 2^31, in 64 bits
    assert call(w=2 ** 31 + 8, h=2) == bad
    assert call(w=2 ** 32 - 1, h=2 ** 32 - 1) == bad

    def params(**kw):
        p = D.PtDenoiseParams.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    assert call(params=params(iterations=6)) == bad and call(params=params(iterations=2 ** 32 - 1)) == bad
    for f in FIELDS[1:]:
        for v in (0.0, -1.0, float("inf"), float("nan")):
            assert call(params=params(**{f: v})) == bad, (f, v)
    assert (out == 7.0).all()
