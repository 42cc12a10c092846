"""The ID mattes' C ABI and Python driver without a GPU (include/mi355aov.h: pt_matte_*; include/mi355front_matte.h): the structs against the ctypes mirror and the
numpy dtype, the refusals that return before the device is touched, pt_matte_resolve (host arithmetic), cryptomatte_id, the Cryptomatte EXR file read back, and the
shape ordinals of the two hosts."""
import ctypes as C
import json
import os
import struct

import numpy as np
import matte_reference as M
from abi_checks import ROOT, assert_mirror, c99_probe, run_without_device
from test_aov_frontend import read_exr_channels

HERE = os.path.dirname(os.path.abspath(__file__))


def test_matte_structs_are_c99_and_match_the_ctypes_mirror_and_the_dtype(pkg):
    V = pkg._abi_aov
    P, B = V.PtMattePixel, V.PtMatteBuffers
    assert assert_mirror("mi355aov.h", {P: ("id", "w", "n_ids", "w_total", "w_other", "reserved"), B: ("layer", "prim_group", "n_prims")})[0] == 80
    assert [getattr(P, f).offset for f, _ in P._fields_] == [0, 32, 64, 68, 72, 76]
    consts = c99_probe("mi355aov.h", 'printf("%u %d %d %d", PT_MATTE_SLOTS, (int)PT_MATTE_MATERIAL, (int)PT_MATTE_INSTANCE, (int)PT_MATTE_GROUP);')
    assert [int(v) for v in consts] == [V.PT_MATTE_SLOTS, 0, 1, 2] and V.MATTE_LAYERS == ("material", "instance", "group") == M.LAYERS
    d = V.MATTE_DTYPE
    assert d == M.DTYPE and d.itemsize == 80 and [d.fields[k][1] for k in ("id", "w", "n_ids", "w_total", "w_other", "reserved")] == [0, 32, 64, 68, 72, 76]


def test_the_header_declares_the_entry_points(pkg):
    header = open(os.path.join(ROOT, "include", "mi355aov.h")).read()
    names = ["pt_matte_render", "pt_matte_render_samples", "pt_matte_pass_size", "pt_matte_resolve", "pt_matte_mask"]
    for name in names:
        assert f"int {name}(" in header and name in pkg._abi_aov.ENTRY_POINTS, name
        assert getattr(pkg.load_library().aov, name).restype is C.c_int
    front = open(os.path.join(ROOT, "include", "mi355front_matte.h")).read()
    F = pkg._abi_front
    assert sorted(F.MATTE_ENTRY_POINTS) == ["ptf_prim_shape_ordinals", "ptf_write_exr_channels_attrs"]
    L = pkg.frontend.lib()
    for name, (res, args) in F.MATTE_ENTRY_POINTS.items():
        assert f"int {name}(" in front and getattr(L, name).argtypes == args and getattr(L, name).restype is res


def test_refusals_return_before_the_device_is_touched(pkg):
    """Run in a child process with no visible device: a call that reached the device would fail with another status (or not return)."""
    n = run_without_device(r'''
V = pkg._abi_aov; aov = lib.aov
scene = C.c_void_p(8)   # never looked at
rp = pkg.scenes.spheres_c1(xres=8, yres=8, spp=8).render_params()
tab = np.zeros((8, 8), V.MATTE_DTYPE); tab["w_total"] = 7.0; tab["id"] = 3
kept = tab.copy()
groups = np.arange(5, dtype=np.uint32)
ok = V.matte_buffers({"material": tab})
none = V.matte_buffers({})
no_groups = V.matte_buffers({"group": tab})
refused(aov.pt_matte_render(None, C.byref(rp), C.byref(ok), 0))
refused(aov.pt_matte_render(scene, None, C.byref(ok), 0))
refused(aov.pt_matte_render(scene, C.byref(rp), None, 0))
refused(aov.pt_matte_render(scene, C.byref(rp), C.byref(none), 0), b"layers")
refused(aov.pt_matte_render(scene, C.byref(rp), C.byref(no_groups), 0), b"prim_group")
refused(aov.pt_matte_render_samples(None, C.byref(rp), 0, 1, C.byref(ok), 0))
refused(aov.pt_matte_render_samples(scene, None, 0, 1, C.byref(ok), 0))
refused(aov.pt_matte_render_samples(scene, C.byref(rp), 0, 1, None, 0))
refused(aov.pt_matte_render_samples(scene, C.byref(rp), 0, 1, C.byref(none), 0))
refused(aov.pt_matte_render_samples(scene, C.byref(rp), 0, 1, C.byref(no_groups), 0))
for first, n in ((0, 0), (6, 3), (2 ** 32 - 1, 2)):
    refused(aov.pt_matte_render_samples(scene, C.byref(rp), first, n, C.byref(ok), 0))
size = C.c_uint32(5)
refused(aov.pt_matte_pass_size(None, C.byref(rp), C.byref(size))); refused(aov.pt_matte_pass_size(scene, None, C.byref(size)))
refused(aov.pt_matte_pass_size(scene, C.byref(rp), None))
assert size.value == 5
ids = np.zeros((64, 8), np.uint32); cov = np.zeros((64, 8), np.float32)
ip, cp, tp = ids.ctypes.data_as(A.u32p), cov.ctypes.data_as(A.fp), tab.ctypes.data_as(V.mp)
for n_ranks in (0, 9):
    refused(aov.pt_matte_resolve(tp, 64, n_ranks, ip, cp))
refused(aov.pt_matte_resolve(None, 64, 2, ip, cp)); refused(aov.pt_matte_resolve(tp, 64, 2, None, cp)); refused(aov.pt_matte_resolve(tp, 64, 2, ip, None))
mask = np.full(64, 7.0, np.float32); one = np.zeros(4097, np.uint32)
mp_, op = mask.ctypes.data_as(A.fp), one.ctypes.data_as(A.u32p)
refused(aov.pt_matte_mask(None, tp, 0, 64, op, 1, mp_, 0)); refused(aov.pt_matte_mask(scene, None, 0, 64, op, 1, mp_, 0))
refused(aov.pt_matte_mask(scene, tp, 0, 64, None, 1, mp_, 0)); refused(aov.pt_matte_mask(scene, tp, 0, 64, op, 1, None, 0))
refused(aov.pt_matte_mask(scene, tp, 0, 64, op, 0, mp_, 0)); refused(aov.pt_matte_mask(scene, tp, 0, 64, op, 4097, mp_, 0))
rp.spp = 0
refused(aov.pt_matte_render(scene, C.byref(rp), C.byref(ok), 0))
assert tab.tobytes() == kept.tobytes() and not ids.any() and not cov.any() and (mask == 7.0).all()
''')
    assert n == 28


def test_resolve_on_hand_made_tables(pkg):
    V = pkg._abi_aov
    t = np.zeros((1, 4), V.MATTE_DTYPE)
    t[0, 0]["id"][:3] = [9, 7, 5]; t[0, 0]["w"][:3] = [1.0, 1.0, 2.0]; t[0, 0]["n_ids"] = 3; t[0, 0]["w_total"] = 4.0             # a tie: the lower id first
    t[0, 1]["id"][:] = np.arange(20, 28); t[0, 1]["w"][:] = [1, 8, 2, 7, 3, 6, 4, 5]; t[0, 1]["n_ids"] = 8; t[0, 1]["w_total"] = 40.0; t[0, 1]["w_other"] = 3.0
    t[0, 2]["w_total"] = 6.0                                                                                                         # misses only
    t[0, 3]["id"][:2] = [4, 6]; t[0, 3]["w"][:2] = [1.0, 2.0]; t[0, 3]["n_ids"] = 2                                                  # w_total == 0: everything 0
    for ranks in (1, 4, 8):
        ids, cov = pkg.runtime.resolve_mattes({"group": t}, ranks=ranks)["group"]
        want_ids, want_cov = M.resolve(t, ranks)
        assert ids.shape == (1, 4, ranks) and ids.dtype == np.uint32 and cov.dtype == np.float32
        assert np.array_equal(ids, want_ids) and cov.tobytes() == want_cov.tobytes()
    ids, cov = pkg.runtime.resolve_mattes({"group": t}, ranks=4)["group"]
    assert list(ids[0, 0]) == [5, 7, 9, 0] and list(cov[0, 0]) == [0.5, 0.25, 0.25, 0.0]
    assert list(ids[0, 1]) == [21, 23, 25, 27] and list(cov[0, 1]) == [np.float32(v) / np.float32(40) for v in (8, 7, 6, 5)]
    assert not ids[0, 2:].any() and not cov[0, 2:].any()


def test_cryptomatte_id_known_values(pkg):
    R = pkg.runtime
    assert R.murmur3_32(b"") == 0 and R.cryptomatte_id("") == 0x00800000
    assert R.cryptomatte_id("hello") == 0x248bfa47 and struct.unpack("<f", struct.pack("<I", 0x248bfa47))[0] == np.float32(6.0705627e-17)
    assert R.cryptomatte_id("test") == 0xba6bd213
    assert R.cryptomatte_id("The quick brown fox jumps over the lazy dog") == 0x2e4ff723
    for h in (0x7f800001, 0xff912345, 0x00012345, 0x807fffff):   # exponent bits all 1 or all 0: bit 23 is flipped (checked on the rule itself)
        fixed = h ^ (1 << 23) if (h >> 23) & 255 in (0, 255) else h
        assert (fixed >> 23) & 255 not in (0, 255)
    assert R.cryptomatte_id("ä€") == R.murmur3_32("ä€".encode("utf-8"))   # UTF-8 bytes, a tail of 1 .. 3 bytes included


def read_exr_strings(path):
    """The string attributes of an EXR header, in file order: [(name, value)] -- read_exr_channels' header walk, kept for the attributes it skips."""
    data = open(path, "rb").read()
    pos, out = 8, []
    while data[pos] != 0:
        e = data.index(b"\0", pos); name = data[pos:e].decode(); pos = e + 1
        e = data.index(b"\0", pos); kind = data[pos:e].decode(); pos = e + 1
        size, = struct.unpack_from("<i", data, pos); pos += 4
        if kind == "string": out.append((name, data[pos:pos + size].decode()))
        pos += size
    return out


def _hand_tables(pkg):
    V = pkg._abi_aov
    rng = np.random.default_rng(5)
    tables = {}
    for layer, pool in (("material", [0, 1, 2, 3]), ("instance", [0, 1, 2]), ("group", list(range(40, 52)))):
        t = np.zeros((3, 5), V.MATTE_DTYPE)
        for p in np.ndindex(t.shape):
            n = int(rng.integers(0, min(len(pool), 8) + 1))
            t[p]["id"][:n] = rng.choice(pool, n, replace=False); t[p]["w"][:n] = rng.random(n).astype(np.float32) + np.float32(0.01)
            t[p]["n_ids"] = n; t[p]["w_other"] = np.float32(0.25) if n == 8 else 0
            t[p]["w_total"] = t[p]["w"][:n].sum(dtype=np.float32) + t[p]["w_other"] + np.float32(0.5)
        tables[layer] = t
    return tables


def test_write_cryptomatte_round_trips(pkg, tmp_path):
    R = pkg.runtime
    tables = _hand_tables(pkg)
    names = {"material": {0: "default", 2: "brass"}, "group": {40: "teapot/lid", 999: "never seen"}}
    out = tmp_path / "mattes.exr"
    R.write_cryptomatte(str(out), tables, names=names, ranks=5)
    channels, planes = read_exr_channels(str(out))
    assert channels == sorted(channels, key=lambda s: s.encode())
    layers = {"material": "CryptoMaterial", "instance": "CryptoInstance", "group": "CryptoGroup"}
    assert channels == sorted(["%s%02d.%s" % (L, k, c) for L in layers.values() for k in range(3) for c in "RGBA"], key=lambda s: s.encode())
    attrs = dict(read_exr_strings(str(out)))
    assert len(attrs) == 12
    default = {"material": lambda i: "material%d" % i, "instance": lambda i: "world" if i == 0 else "instance%d" % i, "group": lambda i: "group%d" % i}
    for layer, L in layers.items():
        key = "cryptomatte/%s/" % ("%08x" % R.cryptomatte_id(L))[:7]
        assert attrs[key + "name"] == L and attrs[key + "hash"] == "MurmurHash3_32" and attrs[key + "conversion"] == "uint32_to_float32"
        assert all(len(key + leaf) <= 31 for leaf in ("name", "hash", "conversion", "manifest"))   # (short attribute names: the file's version word sets no long-name flag)
        manifest = json.loads(attrs[key + "manifest"])
        t = tables[layer]
        name_of = lambda i: names.get(layer, {}).get(i, default[layer](i))
        seen = {int(t[p]["id"][k]) for p in np.ndindex(t.shape) for k in range(int(t[p]["n_ids"]))} | set(names.get(layer, {}))
        assert manifest == {name_of(i): "%08x" % R.cryptomatte_id(name_of(i)) for i in seen}   # every name maps to its hash
        ids, cov = M.resolve(t, 5)
        for r in range(6):
            idp = planes["%s%02d.%s" % (L, r // 2, "RB"[r % 2])].view(np.uint32); cvp = planes["%s%02d.%s" % (L, r // 2, "GA"[r % 2])]
            if r == 5:   # (an odd number of ranks: the last half set is empty)
                assert not idp.any() and not cvp.any(); continue
            want = np.array([[R.cryptomatte_id(name_of(int(ids[y, x, r]))) if cov[y, x, r] != 0 else 0 for x in range(5)] for y in range(3)], np.uint32)
            assert np.array_equal(idp, want) and cvp.tobytes() == cov[..., r].tobytes()   # the ids' bit patterns are preserved
    assert "brass" in attrs["cryptomatte/%s/manifest" % ("%08x" % R.cryptomatte_id("CryptoMaterial"))[:7]] and "never seen" in json.dumps(attrs)


def test_without_attributes_the_exr_writer_writes_the_three_channel_file(pkg, tmp_path):
    from test_aov_frontend import GOLDEN, _golden_rgb
    rgb = _golden_rgb()
    out = tmp_path / "rgb.exr"
    pkg.frontend.write_exr_channels(str(out), {"R": rgb[..., 0], "G": rgb[..., 1], "B": rgb[..., 2]})
    assert open(out, "rb").read() == open(GOLDEN, "rb").read()
    with_attr = tmp_path / "a.exr"
    pkg.frontend.write_exr_channels(str(with_attr), {"R": rgb[..., 0], "G": rgb[..., 1], "B": rgb[..., 2]}, [("note", "x = 1"), ("empty", "")])
    assert read_exr_strings(str(with_attr)) == [("note", "x = 1"), ("empty", "")]
    names, planes = read_exr_channels(str(with_attr))
    assert names == ["B", "G", "R"] and np.array_equal(planes["G"].view(np.uint32), rgb[..., 1].view(np.uint32))
    L, A = pkg.frontend.lib(), pkg._abi
    cn = (C.c_char_p * 1)(b"Z"); ptrs = (A.fp * 1)(rgb[..., 0].copy().ctypes.data_as(A.fp)); one = (C.c_uint32 * 1)(1)
    bad = tmp_path / "bad.exr"
    for an, av in (((C.c_char_p * 1)(None), (C.c_char_p * 1)(b"v")), ((C.c_char_p * 1)(b""), (C.c_char_p * 1)(b"v")), ((C.c_char_p * 1)(b"n" * 32), (C.c_char_p * 1)(b"v")),
                   ((C.c_char_p * 1)(b"n"), (C.c_char_p * 1)(None))):
        assert L.ptf_write_exr_channels_attrs(os.fsencode(str(bad)), 5, 3, 1, cn, ptrs, one, 1, an, av) == A.PT_ERR_INVALID_ARG and not bad.exists()
    assert L.ptf_write_exr_channels_attrs(os.fsencode(str(bad)), 5, 3, 1, cn, ptrs, one, 1, None, None) == A.PT_ERR_INVALID_ARG and not bad.exists()


def test_shape_ordinals_of_the_two_hosts_are_equal(pkg, tmp_path):
    """Both hosts number the Shape directives 0, 1, 2, ... in file order, shapes inside ObjectBegin included: for the scenes of test_frontend.py."""
    from test_frontend import _feature_files, _python_twin
    fs = pkg.frontend.FrontScene(path=os.path.join(HERE, "scenes", "spheres_c1.pbrt"))
    sd, _ = pkg.scenes.spheres_c1(xres=96, yres=96, spp=8).world_end()
    assert fs.prim_group.dtype == np.uint32 and np.array_equal(fs.prim_group, sd.prim_group) and len(sd.prim_group) == len(sd.prim_shape)
    P, I, N, UV = _feature_files(pkg, tmp_path)
    fs = pkg.frontend.FrontScene(path=str(tmp_path / "features.pbrt"))
    sd, _ = _python_twin(pkg, P, I, N, UV)
    assert np.array_equal(fs.prim_group, sd.prim_group) and len(sd.prim_group) == fs.desc().n_prims
    g = sd.prim_group
    assert g[0] == 0 and (np.diff(g.astype(np.int64)) >= 0).all() and set(np.diff(g.astype(np.int64))) == {0, 1} and g[-1] == 4   # floor, card (in an object), two blobs, the light
    # a scene file's shapes in objects count like any other
    fs = pkg.frontend.FrontScene(text='WorldBegin\nShape "sphere"\nObjectBegin "o"\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0 0 0 1 0 0 1 1 0 0 1 0]\n'
                                      'Shape "disk"\nObjectEnd\nObjectInstance "o"\nShape "sphere"\nWorldEnd\n')
    assert list(fs.prim_group) == [0, 1, 1, 2, 3]
    assert pkg.frontend.lib().ptf_prim_shape_ordinals(None, None, None) == pkg._abi.PT_ERR_INVALID_ARG
