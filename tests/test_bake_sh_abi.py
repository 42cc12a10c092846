"""The SH points' C ABI without a GPU (include/mi355bake.h "SH points", libmi355bake.so): the new struct against the ctypes mirror under C99, the six exports, the new
kernels in the built library, the refusals that return before the device is touched and before the scene handle is read -- in the header's order --, and the two
host-arithmetic entries (pt_bake_sh_resolve, pt_bake_sh_irradiance) against the model, byte for byte."""
import ctypes as C

import numpy as np
import sh_reference as SR
from abi_checks import assert_bound, assert_mirror, embedded_kernel_names, exported_names, run_without_device

P_FIELDS = ("n_points", "row", "spp", "nsamples", "sampler_type", "spp_per_pass", "profile")
ENTRIES = ("pt_bake_sh", "pt_bake_sh_samples", "pt_bake_sh_pass_size", "pt_bake_sh_resolve", "pt_bake_sh_irradiance", "pt_bake_sh_rays")


def test_the_sh_struct_matches_the_ctypes_mirror(pkg):
    K = pkg._abi_bake
    P = K.PtBakeShParams
    assert assert_mirror("mi355bake.h", {P: P_FIELDS}) == [28] and all(t is K.u32 for _, t in P._fields_)
    assert C.sizeof(K.PtBakeLightParams) == 28 and C.sizeof(K.PtBakeLightBuffers) == 32 and C.sizeof(K.PtBakeParams) == 36   # (the layouts there were)


def test_the_library_exports_the_sh_entries_and_holds_the_sh_kernels(pkg):
    K = pkg._abi_bake
    names = exported_names(pkg.runtime.LIB_PATHS["bake"])
    assert set(ENTRIES) <= names and set(ENTRIES) <= set(K.ENTRY_POINTS)
    hp, VP, fp, u8p, u32, u32p = C.POINTER(K.PtBakeShParams), pkg._abi.VP, pkg._abi.fp, pkg._abi.u8p, pkg._abi.u32, pkg._abi.u32p
    want = {"pt_bake_sh": [VP, hp, fp, u8p, u32, fp, C.c_int], "pt_bake_sh_samples": [VP, hp, fp, u8p, u32, u32, u32, fp, C.c_int], "pt_bake_sh_pass_size": [VP, hp, u8p, u32, u32p],
            "pt_bake_sh_resolve": [fp, u32, u32, u32, fp, fp], "pt_bake_sh_irradiance": [fp, fp, u32, fp],
            "pt_bake_sh_rays": [VP, hp, fp, u8p, u32, u32, u32p, u32p, u32p, u32p, fp, fp, fp, fp, fp, fp, u8p]}
    for name in ENTRIES:
        res, args = K.ENTRY_POINTS[name]
        assert res is C.c_int and args == want[name], name
    assert_bound(pkg.load_library().bake, K.ENTRY_POINTS, ENTRIES)
    kernels = embedded_kernel_names(pkg.runtime.LIB_PATHS["bake"])   # (tests/test_bake_abi.py holds every kernel's scratch size)
    for kernel in ("_ZN6ptbake14k_bake_sh_raysILb0EEE", "_ZN6ptbake14k_bake_sh_raysILb1EEE", "_ZN6ptbake15k_bake_sh_accum", "_ZN6ptbake15k_bake_sh_probeILb0EEE",
                   "_ZN6ptbake15k_bake_sh_probeILb1EEE"):
        assert any(kernel in name for name in kernels), kernel


def test_sh_refusals_return_before_the_device_is_touched_in_the_headers_order(pkg):
    """Run in a child process with no visible device and a scene handle that is never looked at: a call that read the handle or reached the device would crash or
    fail with another status. Every case is wrong in ONE way and in every way behind it in the header's order: the message names the first."""
    n = run_without_device(r'''
K = pkg._abi_bake; bake = lib.bake
scene = C.c_void_p(8)   # never looked at
def params(**kw):
    d = dict(n_points=5, row=4, spp=4, nsamples=3, sampler_type=0, spp_per_pass=0, profile=0); d.update(kw)
    return K.PtBakeShParams(*[d[k] for k, _ in K.PtBakeShParams._fields_])
fp = lambda a: a.ctypes.data_as(A.fp)
u8 = lambda a: a.ctypes.data_as(A.u8p)
good = np.arange(15, dtype=np.float32).reshape(5, 3)
nan = good.copy(); nan[3, 1] = np.nan
inf = good.copy(); inf[4, 2] = -np.inf; inf[2, 0] = np.inf
sums = np.full((5, 28), 7.0, np.float32); kept = sums.copy()
three, nolight, five = np.array([1, 0, 1, 1, 0], np.uint8), np.zeros(5, np.uint8), np.ones(5, np.uint8)
samples = lambda q, pts=nan, lights=nolight, n_l=5, first=3, n=9, scene=scene, w=sums: bake.pt_bake_sh_samples(scene, None if q is None else C.byref(q), None if pts is None else fp(pts),
    None if lights is None else u8(lights), n_l, first, n, None if w is None else fp(w), 0)
whole = lambda q, pts=good, lights=three, n_l=5, scene=scene, w=sums: bake.pt_bake_sh(scene, None if q is None else C.byref(q), None if pts is None else fp(pts),
    None if lights is None else u8(lights), n_l, None if w is None else fp(w), 0)
p = params()
# 1. NULL arguments, with everything behind them wrong as well
worst = params(n_points=0, row=0, spp=0, nsamples=0, sampler_type=2)
refused(samples(worst, scene=None), b"null"); refused(samples(None), b"null"); refused(samples(worst, pts=None), b"null"); refused(samples(worst, w=None), b"null")
refused(whole(p, scene=None), b"null"); refused(whole(None), b"null"); refused(whole(p, pts=None), b"null"); refused(whole(p, w=None), b"null")
# 2 .. 5: the parameters, each with every later one wrong too (a wrong n_points leaves nothing of `points` to read)
order = [(dict(n_points=0), b"n_points"), (dict(n_points=(1 << 28) + 1), b"2^28 points"), (dict(row=0), b"row"), (dict(row=(1 << 28) + 1), b"row"), (dict(spp=0), b"spp"),
         (dict(nsamples=0), b"nsamples"), (dict(sampler_type=2), b"sampler")]
for i, (kw, text) in enumerate(order):
    later = {}
    for k2, _ in order[i + 1:]:
        later.update({k: v for k, v in k2.items() if k not in later and k != "n_points"})
    later.update(kw)
    refused(samples(params(**later)), text)
    q = params(**kw)
    refused(whole(q), text); refused(samples(q, pts=good, lights=three, first=0, n=4), text)
    size = C.c_uint32(5)
    refused(bake.pt_bake_sh_pass_size(scene, C.byref(q), u8(three), 5, C.byref(size)), text)
    assert size.value == 5
# 6. the sample range, before the points are read
refused(samples(p), b"sample range"); refused(samples(p, first=0, n=0), b"n_samples"); refused(samples(p, first=2 ** 32 - 1, n=2), b"sample range")
# 7. a point that is not finite: the message names it
refused(samples(p, first=0, n=4), b"point 3 "); refused(samples(p, pts=inf, first=1, n=3), b"point 2 "); refused(whole(p, pts=nan, lights=nolight), b"point 3 ")
# 8. no light selected
refused(samples(p, pts=good, first=0, n=4), b"no light is selected"); refused(whole(p, lights=nolight), b"no light is selected"); refused(whole(p, lights=None, n_l=0), b"no light is selected")
# 9. the multiple rule: 4 x 3 = 12 light samples per point serve 3 lights, not 5; the message names both numbers
refused(whole(p, lights=five), b"12")
assert b" 5 selected lights" in lib.lib.pt_last_error()
refused(whole(p, lights=None), b"no multiple")   # NULL: all five
refused(whole(params(spp=1, nsamples=2)), b"2 light samples per point are no multiple of the 3 selected lights")
size = C.c_uint32(5)
refused(bake.pt_bake_sh_pass_size(None, C.byref(p), u8(three), 5, C.byref(size)), b"null"); refused(bake.pt_bake_sh_pass_size(scene, None, u8(three), 5, C.byref(size)), b"null")
refused(bake.pt_bake_sh_pass_size(scene, C.byref(p), u8(three), 5, None), b"null")
refused(bake.pt_bake_sh_pass_size(scene, C.byref(p), u8(nolight), 5, C.byref(size)), b"no light is selected")
refused(bake.pt_bake_sh_pass_size(scene, C.byref(p), u8(five), 5, C.byref(size)), b"no multiple")
assert size.value == 5
t = np.zeros(4, np.uint32); f3 = np.zeros((4, 3), np.float32); f1 = np.zeros(4, np.float32); f8 = np.zeros(4, np.uint8)
tp, fp3, fp1, up = t.ctypes.data_as(A.u32p), fp(f3), fp(f1), f8.ctypes.data_as(A.u8p)
rays = lambda par, pts, lights, point=tp, sample=tp, light=tp, found=up: bake.pt_bake_sh_rays(scene, C.byref(par), None if pts is None else fp(pts), u8(lights), 5, 4, point, sample, tp, light,
    fp3, fp1, fp3, fp3, fp3, fp3, found)
refused(rays(p, good, three, point=None), b"null"); refused(rays(p, good, three, light=None), b"null"); refused(rays(p, good, three, found=None), b"null"); refused(rays(p, None, three), b"null")
refused(rays(params(nsamples=0), nan, nolight), b"nsamples")
refused(rays(p, nan, nolight), b"point 3 ")
refused(rays(p, good, nolight), b"no light is selected")
refused(rays(p, good, five), b"no multiple")
four = np.full(4, 4, np.uint32)
refused(rays(p, good, three, sample=four.ctypes.data_as(A.u32p)), b"outside the job")
sh = np.zeros((5, 27), np.float32); reached = np.zeros(5, np.float32); irr = np.zeros((5, 3), np.float32)
refused(bake.pt_bake_sh_resolve(None, 5, 4, 3, fp(sh), fp(reached)), b"null"); refused(bake.pt_bake_sh_resolve(fp(sums), 5, 4, 3, None, None), b"null")
refused(bake.pt_bake_sh_resolve(fp(sums), 5, 0, 3, fp(sh), fp(reached)), b"spp"); refused(bake.pt_bake_sh_resolve(fp(sums), 5, 4, 0, fp(sh), fp(reached)), b"nsamples")
refused(bake.pt_bake_sh_irradiance(None, fp(good), 5, fp(irr)), b"null"); refused(bake.pt_bake_sh_irradiance(fp(sh), None, 5, fp(irr)), b"null"); refused(bake.pt_bake_sh_irradiance(fp(sh), fp(good), 5, None), b"null")
assert sums.tobytes() == kept.tobytes() and not sh.any() and not reached.any() and not irr.any()
assert bake.pt_bake_sh_resolve(fp(sums), 5, 4, 3, None, fp(reached)) == A.PT_OK and (reached == np.float32(7.0) / (np.float32(4) * np.float32(3))).all() and not sh.any()   # a NULL output is skipped
''')
    assert n == 69


def test_sh_resolve_and_irradiance_are_the_models(pkg):
    rng = np.random.RandomState(6)
    w = rng.uniform(-3, 5, (11, 28)).astype(np.float32); w[:, 27] = np.floor(np.abs(w[:, 27]) * 3)
    w[0] = 0; w[1, :27] = 0; w[1, 27] = 2; w[2, 27] = 0   # nothing added; a count alone; sums without a count cannot be, but the rule is "all 28 sums 0"
    sh, reached = pkg.runtime.resolve_sh(w, 3, 5)
    want_sh, want_reached = SR.resolve(w, 3, 5)
    assert sh.shape == (11, 9, 3) and reached.shape == (11,) and sh.tobytes() == want_sh.tobytes() and reached.tobytes() == want_reached.tobytes()
    assert not sh[0].any() and reached[0] == 0 and not sh[1].any() and reached[1] == np.float32(2) / (np.float32(3) * np.float32(5)) and sh[2].any() and reached[2] == 0
    assert sh[3, 2, 1] == w[3, 3 * 2 + 1] / np.float32(3)   # coefficient q, channel c at 3 q + c
    nrm = rng.normal(size=(11, 3)); nrm = (nrm / np.sqrt((nrm * nrm).sum(axis=1))[:, None]).astype(np.float32)
    got = pkg.runtime.sh_irradiance(sh, nrm)
    assert got.shape == (11, 3) and got.dtype == np.float32 and got.tobytes() == SR.irradiance(sh, nrm).tobytes() and (got < 0).any()   # not clamped
    one = pkg.runtime.sh_irradiance(sh[4], nrm)   # one set of coefficients under many normals
    assert one.tobytes() == SR.irradiance(np.broadcast_to(sh[4], (11, 9, 3)), nrm).tobytes()
