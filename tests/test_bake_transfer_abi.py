"""The transfer bake's C ABI without a GPU (include/mi355bake.h "Transfer", libmi355bake.so): the header under C99, the structs against the ctypes mirror, the
refusals that return before the device is touched, the kernels in the built library, and encode_normal_map."""
import numpy as np
from abi_checks import assert_mirror, embedded_kernel_names, run_without_device

P_FIELDS = ("width", "height", "front", "back", "spp", "nsamples", "cos_sample", "max_distance", "sampler_type", "spp_per_pass", "profile")
B_FIELDS = ("owner", "hit_prim", "height", "src_position", "src_normal", "tangent_normal", "ao_w")


def test_the_header_is_c99_and_the_transfer_structs_match_the_ctypes_mirror(pkg):
    K = pkg._abi_bake
    assert assert_mirror("mi355bake.h", {K.PtBakeTransferParams: P_FIELDS, K.PtBakeTransferBuffers: B_FIELDS, K.PtBakeParams: [n for n, _ in K.PtBakeParams._fields_],
                                         K.PtBakeBuffers: K.PLANES}) == [44, 56, 36, 32]
    assert list(B_FIELDS) == list(K.TRANSFER_PLANES)
    assert set(K.TRANSFER_CHANNELS) == set(K.TRANSFER_DTYPES) == set(B_FIELDS) and K.PLANES == ("owner", "position", "normal", "ao_w")
    for name in ("pt_bake_transfer", "pt_bake_transfer_samples", "pt_bake_transfer_pass_size", "pt_bake_transfer_rays"):
        assert name in K.ENTRY_POINTS
    assert len(pkg.runtime.LIBRARIES) == 5


def test_the_transfer_kernels_are_in_the_library_and_use_no_scratch(pkg):
    kernels = embedded_kernel_names(pkg.runtime.LIB_PATHS["bake"])
    for k in ("k_bake_project", "k_bake_transfer_points", "k_bake_transfer_rays", "k_bake_transfer_probe"):
        mine = {n: v for n, v in kernels.items() if k in n}
        assert len(mine) == 1 and list(mine.values()) == [0] and "6ptbake" in list(mine)[0], (k, sorted(kernels))


def test_transfer_refusals_return_before_the_device_is_touched(pkg):
    """Run in a child process with no visible device: a call that reached the device would fail with another status (or not return). The scene handles are never looked
    at; the check of n_prims against the target, which reads the handle, is tests/test_bake_transfer.py's."""
    n = run_without_device(r'''
K = pkg._abi_bake; bake = lib.bake
tg, src = C.c_void_p(8), C.c_void_p(16)   # never looked at
def params(**kw):
    d = dict(width=8, height=8, front=0.5, back=0.5, spp=4, nsamples=8, cos_sample=1, max_distance=float("inf"), sampler_type=0, spp_per_pass=0, profile=0); d.update(kw)
    return K.PtBakeTransferParams(*[d[k] for k, _ in K.PtBakeTransferParams._fields_])
planes = {k: np.full((8, 8) + ((K.TRANSFER_CHANNELS[k],) if K.TRANSFER_CHANNELS[k] > 1 else ()), 7, K.TRANSFER_DTYPES[k]) for k in K.TRANSFER_PLANES}
kept = {k: v.copy() for k, v in planes.items()}
ok, none = K.transfer_buffers(planes), K.transfer_buffers({})
no_ao = K.transfer_buffers({k: v for k, v in planes.items() if k != "ao_w"})
sel = np.ones(5, np.uint8); nosel = np.zeros(5, np.uint8)
sp, np_ = sel.ctypes.data_as(A.u8p), nosel.ctypes.data_as(A.u8p)
p = params()
size = C.c_uint32(5)
# NULL arguments
for a in range(5):
    args = [tg, src, C.byref(p), sp, 5, C.byref(ok), 0]
    args[a if a < 4 else 5] = None
    refused(bake.pt_bake_transfer(*args), b"null")
    refused(bake.pt_bake_transfer_samples(*args[:5], 0, 1, *args[5:]), b"null")
for a in range(4):
    args = [tg, src, C.byref(p), C.byref(size)]; args[a] = None
    refused(bake.pt_bake_transfer_pass_size(*args), b"null")
# atlas limits, then front / back -- with and without ao_w
nan, inf = float("nan"), float("inf")
for kw, text in ((dict(width=0), b"width"), (dict(height=0), b"height"), (dict(width=1 << 15, height=1 << 14), b"2^28"), (dict(front=-0.1), b"front"), (dict(back=-0.1), b"front"),
                 (dict(front=0.0, back=0.0), b"front"), (dict(front=nan), b"front"), (dict(back=nan), b"front"), (dict(front=inf), b"front"), (dict(back=inf), b"front")):
    q = params(**kw)
    for bufs in (ok, no_ao):
        refused(bake.pt_bake_transfer(tg, src, C.byref(q), sp, 5, C.byref(bufs), 0), text)
        refused(bake.pt_bake_transfer_samples(tg, src, C.byref(q), sp, 5, 0, 1, C.byref(bufs), 0), text)
    refused(bake.pt_bake_transfer_pass_size(tg, src, C.byref(q), C.byref(size)), text)
# the atlas comes before front / back, front / back before the planes, the planes before the AO numbers
refused(bake.pt_bake_transfer(tg, src, C.byref(params(width=0, front=-1.0)), sp, 5, C.byref(none), 0), b"width")
refused(bake.pt_bake_transfer(tg, src, C.byref(params(front=-1.0)), sp, 5, C.byref(none), 0), b"front")
refused(bake.pt_bake_transfer(tg, src, C.byref(params(spp=0)), np_, 5, C.byref(none), 0), b"planes")
refused(bake.pt_bake_transfer(tg, src, C.byref(p), sp, 5, C.byref(none), 0), b"planes")
# the AO numbers and the sample range: only with ao_w
for kw, text in ((dict(spp=0), b"spp"), (dict(nsamples=0), b"nsamples"), (dict(max_distance=0.0), b"max_distance"), (dict(max_distance=nan), b"max_distance"), (dict(sampler_type=2), b"sampler")):
    q = params(**kw)
    refused(bake.pt_bake_transfer(tg, src, C.byref(q), sp, 5, C.byref(ok), 0), text)
    refused(bake.pt_bake_transfer_samples(tg, src, C.byref(q), sp, 5, 0, 1, C.byref(ok), 0), text)
    refused(bake.pt_bake_transfer_pass_size(tg, src, C.byref(q), C.byref(size)), text)
    refused(bake.pt_bake_transfer(tg, src, C.byref(q), np_, 5, C.byref(no_ao), 0), b"selected")   # (not read without ao_w: the next refusal is the selection's)
for first, n in ((0, 0), (2, 3), (2 ** 32 - 1, 2)):
    refused(bake.pt_bake_transfer_samples(tg, src, C.byref(p), sp, 5, first, n, C.byref(ok), 0), b"n_samples" if n == 0 else b"sample range")
    refused(bake.pt_bake_transfer_samples(tg, src, C.byref(p), np_, 5, first, n, C.byref(no_ao), 0), b"selected")
refused(bake.pt_bake_transfer_samples(tg, src, C.byref(p), np_, 5, 2, 3, C.byref(ok), 0), b"sample range")   # the range comes before the selection
# nothing selected
refused(bake.pt_bake_transfer(tg, src, C.byref(p), np_, 5, C.byref(ok), 0), b"selected")
refused(bake.pt_bake_transfer(tg, src, C.byref(p), sp, 0, C.byref(ok), 0), b"selected")
assert size.value == 5
# the parity entry
t = np.zeros(4, np.uint32); f3 = np.zeros((4, 3), np.float32); f1 = np.zeros(4, np.float32); u8 = np.zeros(4, np.uint8)
tp, fp3, fp1, up = t.ctypes.data_as(A.u32p), f3.ctypes.data_as(A.fp), f1.ctypes.data_as(A.fp), u8.ctypes.data_as(A.u8p)
rays = lambda q, s, smp=tp, found=up: bake.pt_bake_transfer_rays(tg, src, C.byref(q), s, 5, 4, tp, smp, tp, fp3, fp3, fp1, fp3, fp3, fp1, found)
refused(rays(p, sp, found=None), b"null")
refused(bake.pt_bake_transfer_rays(tg, None, C.byref(p), sp, 5, 4, tp, tp, tp, fp3, fp3, fp1, fp3, fp3, fp1, up), b"null")
refused(rays(params(back=-1.0), sp), b"front")
refused(rays(params(nsamples=0), sp), b"nsamples")
refused(rays(p, np_), b"selected")
four = np.full(4, 4, np.uint32)
refused(rays(p, sp, smp=four.ctypes.data_as(A.u32p)), b"outside the job")
for k in planes:
    assert planes[k].tobytes() == kept[k].tobytes(), k
assert not f3.any() and not f1.any() and not u8.any()
''')
    assert n == 103


def test_encode_normal_map(pkg):
    tn = np.zeros((2, 3, 3), np.float32); tn[0, 0] = (0, 0, 1); tn[0, 1] = (-1, 0.5, 0.25); tn[1, 2] = (0.6, -0.8, 0)
    covered = np.zeros((2, 3), bool); covered[0, 0] = covered[0, 1] = covered[1, 2] = True
    img = pkg.runtime.encode_normal_map(tn, covered)
    assert img.dtype == np.float32 and img.shape == (2, 3, 3)
    assert np.array_equal(img[0, 0], np.array([0.5, 0.5, 1], np.float32)) and np.array_equal(img[0, 1], np.array([0, 0.75, 0.625], np.float32))
    assert np.array_equal(img[1, 2], tn[1, 2] * np.float32(0.5) + np.float32(0.5))
    assert (img[~covered] == np.array([0.5, 0.5, 1], np.float32)).all()
