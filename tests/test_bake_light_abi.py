"""The lightmap's C ABI without a GPU (include/mi355bake.h "Lightmap", libmi355bake.so): the header under C99 and the new structs against the ctypes mirror, the new
kernels in the built library, the refusals that return before the device is touched -- in the header's order --, and pt_bake_light_resolve against the model."""
import ctypes as C

import numpy as np
import lightmap_reference as LM
from abi_checks import assert_bound, assert_mirror, embedded_kernel_names, exported_names, run_without_device

P_FIELDS = ("width", "height", "spp", "nsamples", "sampler_type", "spp_per_pass", "profile")
B_FIELDS = ("owner", "position", "normal", "light_w")
ENTRIES = ("pt_bake_light", "pt_bake_light_samples", "pt_bake_light_pass_size", "pt_bake_light_resolve", "pt_bake_light_rays")


def test_the_header_is_c99_and_the_light_structs_match_the_ctypes_mirror(pkg):
    K = pkg._abi_bake
    assert assert_mirror("mi355bake.h", {K.PtBakeLightParams: P_FIELDS, K.PtBakeLightBuffers: B_FIELDS}) == [28, 32]
    assert list(B_FIELDS) == list(K.LIGHT_PLANES)
    assert C.sizeof(K.PtBakeParams) == 36 and C.sizeof(K.PtBakeBuffers) == 32 and C.sizeof(K.PtBakeTransferParams) == 44 and C.sizeof(K.PtBakeTransferBuffers) == 56   # (the layouts there were)


def test_the_library_exports_the_light_entries_and_holds_the_light_kernels(pkg):
    names = exported_names(pkg.runtime.LIB_PATHS["bake"])
    assert set(ENTRIES) <= names and set(ENTRIES) <= set(pkg._abi_bake.ENTRY_POINTS)
    assert_bound(pkg.load_library().bake, pkg._abi_bake.ENTRY_POINTS, ENTRIES)
    kernels = embedded_kernel_names(pkg.runtime.LIB_PATHS["bake"])   # (tests/test_bake_abi.py holds every kernel's scratch size)
    for kernel in ("_ZN6ptbake17k_bake_light_raysILb0EEE", "_ZN6ptbake17k_bake_light_raysILb1EEE", "_ZN6ptbake18k_bake_light_accumE", "_ZN6ptbake18k_bake_light_probeILb0EEE",
                   "_ZN6ptbake18k_bake_light_probeILb1EEE"):
        assert any(kernel in name for name in kernels), kernel


def test_light_refusals_return_before_the_device_is_touched_in_the_headers_order(pkg):
    """Run in a child process with no visible device and a scene handle that is never looked at: a call that read the handle or reached the device would crash or
    fail with another status. Every case is wrong in ONE way and in every way behind it in the header's order: the message names the first."""
    n = run_without_device(r'''
K = pkg._abi_bake; bake = lib.bake
scene = C.c_void_p(8)   # never looked at
def params(**kw):
    d = dict(width=8, height=8, spp=4, nsamples=3, sampler_type=0, spp_per_pass=0, profile=0); d.update(kw)
    return K.PtBakeLightParams(*[d[k] for k, _ in K.PtBakeLightParams._fields_])
planes = {"owner": np.full((8, 8), 5, np.uint32), "position": np.full((8, 8, 3), 7.0, np.float32), "normal": np.full((8, 8, 3), 7.0, np.float32), "light_w": np.full((8, 8, 4), 7.0, np.float32)}
kept = {k: v.copy() for k, v in planes.items()}
ok, none = K.light_buffers(planes), K.light_buffers({})
u8 = lambda a: a.ctypes.data_as(A.u8p)
sel, nosel = np.ones(5, np.uint8), np.zeros(5, np.uint8)
three, nolight, five = np.array([1, 0, 1, 1, 0], np.uint8), np.zeros(5, np.uint8), np.ones(5, np.uint8)
p = params()
# every argument wrong at once, then one fewer at a time: the order of the checks
worst = params(width=0, sampler_type=2)
refused(bake.pt_bake_light_samples(None, C.byref(worst), u8(nosel), 5, u8(nolight), 5, 3, 9, C.byref(none), 0), b"null")
refused(bake.pt_bake_light_samples(scene, None, u8(nosel), 5, u8(nolight), 5, 3, 9, C.byref(none), 0), b"null")
refused(bake.pt_bake_light_samples(scene, C.byref(worst), None, 5, u8(nolight), 5, 3, 9, C.byref(none), 0), b"null")
refused(bake.pt_bake_light_samples(scene, C.byref(worst), u8(nosel), 5, u8(nolight), 5, 3, 9, None, 0), b"null")
refused(bake.pt_bake_light(None, C.byref(p), u8(sel), 5, u8(three), 5, C.byref(ok), 0), b"null")
refused(bake.pt_bake_light_samples(scene, C.byref(worst), u8(nosel), 5, u8(nolight), 5, 3, 9, C.byref(none), 0), b"width")
for kw, text in ((dict(width=0), b"width"), (dict(height=0), b"height"), (dict(width=1 << 15, height=1 << 14), b"2^28"), (dict(spp=0), b"spp"), (dict(nsamples=0), b"nsamples"), (dict(sampler_type=2), b"sampler")):
    q = params(**kw)
    refused(bake.pt_bake_light(scene, C.byref(q), u8(sel), 5, u8(three), 5, C.byref(ok), 0), text)
    refused(bake.pt_bake_light_samples(scene, C.byref(q), u8(nosel), 5, u8(nolight), 5, 3, 9, C.byref(none), 0), text)
    size = C.c_uint32(5)
    refused(bake.pt_bake_light_pass_size(scene, C.byref(q), u8(three), 5, C.byref(size)), text)
    assert size.value == 5
refused(bake.pt_bake_light_samples(scene, C.byref(p), u8(nosel), 5, u8(nolight), 5, 3, 9, C.byref(none), 0), b"planes")
refused(bake.pt_bake_light_samples(scene, C.byref(p), u8(nosel), 5, u8(nolight), 5, 3, 9, C.byref(ok), 0), b"sample range")
refused(bake.pt_bake_light_samples(scene, C.byref(p), u8(nosel), 5, u8(nolight), 5, 0, 0, C.byref(ok), 0), b"n_samples")
refused(bake.pt_bake_light_samples(scene, C.byref(p), u8(nosel), 5, u8(nolight), 5, 2 ** 32 - 1, 2, C.byref(ok), 0), b"sample range")
refused(bake.pt_bake_light_samples(scene, C.byref(p), u8(nosel), 5, u8(nolight), 5, 0, 4, C.byref(ok), 0), b"no primitive is selected")
refused(bake.pt_bake_light(scene, C.byref(p), u8(sel), 0, u8(nolight), 5, C.byref(ok), 0), b"no primitive is selected")
refused(bake.pt_bake_light(scene, C.byref(p), u8(sel), 5, u8(nolight), 5, C.byref(ok), 0), b"no light is selected")
refused(bake.pt_bake_light(scene, C.byref(p), u8(sel), 5, None, 0, C.byref(ok), 0), b"no light is selected")
# the multiple rule: 4 x 3 = 12 light samples per texel serve 3 lights, not 5; the message names both numbers
refused(bake.pt_bake_light(scene, C.byref(p), u8(sel), 5, u8(five), 5, C.byref(ok), 0), b"12")
assert b" 5 selected lights" in lib.lib.pt_last_error()
refused(bake.pt_bake_light(scene, C.byref(p), u8(sel), 5, None, 5, C.byref(ok), 0), b"no multiple")   # NULL: all five
refused(bake.pt_bake_light(scene, C.byref(params(spp=1, nsamples=2)), u8(sel), 5, u8(three), 5, C.byref(ok), 0), b"2 light samples per texel are no multiple of the 3 selected lights")
size = C.c_uint32(5)
refused(bake.pt_bake_light_pass_size(None, C.byref(p), u8(three), 5, C.byref(size)), b"null"); refused(bake.pt_bake_light_pass_size(scene, None, u8(three), 5, C.byref(size)), b"null")
refused(bake.pt_bake_light_pass_size(scene, C.byref(p), u8(three), 5, None), b"null")
refused(bake.pt_bake_light_pass_size(scene, C.byref(p), u8(nolight), 5, C.byref(size)), b"no light is selected")
refused(bake.pt_bake_light_pass_size(scene, C.byref(p), u8(five), 5, C.byref(size)), b"no multiple")
assert size.value == 5
t = np.zeros(4, np.uint32); f3 = np.zeros((4, 3), np.float32); f1 = np.zeros(4, np.float32); f8 = np.zeros(4, np.uint8)
tp, fp3, fp1, up = t.ctypes.data_as(A.u32p), f3.ctypes.data_as(A.fp), f1.ctypes.data_as(A.fp), f8.ctypes.data_as(A.u8p)
rays = lambda par, prims, lights, n_l, texel=tp, sample=tp, light=tp, found=up: bake.pt_bake_light_rays(scene, C.byref(par), prims, 5, lights, n_l, 4, texel, sample, tp, light, fp3, fp1, fp3, fp3, fp3, fp3, found)
refused(rays(p, u8(sel), u8(three), 5, texel=None), b"null"); refused(rays(p, u8(sel), u8(three), 5, light=None), b"null"); refused(rays(p, u8(sel), u8(three), 5, found=None), b"null")
refused(rays(params(nsamples=0), u8(nosel), u8(nolight), 5), b"nsamples")
refused(rays(p, u8(nosel), u8(nolight), 5), b"no primitive is selected")
refused(rays(p, u8(sel), u8(nolight), 5), b"no light is selected")
refused(rays(p, u8(sel), u8(five), 5), b"no multiple")
four = np.full(4, 4, np.uint32)
refused(rays(p, u8(sel), u8(three), 5, sample=four.ctypes.data_as(A.u32p)), b"outside the job")
irr = np.zeros((64, 3), np.float32); reached = np.zeros(64, np.float32); lw = planes["light_w"].ctypes.data_as(A.fp)
refused(bake.pt_bake_light_resolve(None, 64, 4, 3, irr.ctypes.data_as(A.fp), reached.ctypes.data_as(A.fp)), b"null"); refused(bake.pt_bake_light_resolve(lw, 64, 4, 3, None, None), b"null")
refused(bake.pt_bake_light_resolve(lw, 64, 0, 3, irr.ctypes.data_as(A.fp), reached.ctypes.data_as(A.fp)), b"spp")
refused(bake.pt_bake_light_resolve(lw, 64, 4, 0, irr.ctypes.data_as(A.fp), reached.ctypes.data_as(A.fp)), b"nsamples")
for k in planes:
    assert planes[k].tobytes() == kept[k].tobytes(), k
assert not irr.any() and not reached.any()
''')
    assert n == 52


def test_light_resolve_is_the_models(pkg):
    rng = np.random.RandomState(4)
    lw = rng.uniform(0, 5, (5, 7, 4)).astype(np.float32); lw[..., 3] = np.floor(lw[..., 3] * 3)
    lw[0, 0] = 0; lw[1, 1, :3] = 0; lw[1, 1, 3] = 2   # nothing added; samples that arrived with E = 0 in every channel cannot be (Li is not black), but the rule is "all four sums 0"
    irr, reached = pkg.runtime.resolve_lightmap(lw, 3, 5)
    want_irr, want_reached = LM.resolve(lw, 3, 5)
    assert irr.tobytes() == want_irr.tobytes() and reached.tobytes() == want_reached.tobytes()
    assert not irr[0, 0].any() and reached[0, 0] == 0 and not irr[1, 1].any() and reached[1, 1] == np.float32(2) / (np.float32(3) * np.float32(5))
    assert irr.shape == (5, 7, 3) and reached.shape == (5, 7)
