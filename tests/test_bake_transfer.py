"""The transfer bake on the GPU (libmi355bake.so, include/mi355bake.h "Transfer") against the numpy model of its contract (tests/transfer_reference.py), bit for bit:
every quantity is a stated float32 operation order and the library is compiled without contraction, so no tolerance is needed. The model's hits and occlusion come
from the oracle's closest-hit and any-hit queries over the source scene. tests/test_bake_transfer_model.py holds that the scenes reach what the cases are about."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import bake_reference as M
import transfer_reference as T
import transfer_scenes as X
from conftest import trace_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
WRITTEN = ("owner", "hit_prim", "height", "src_position", "src_normal", "tangent_normal")
_CACHE = {}   # scenes and the model's results, computed once (every test runs under both walks)


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def scene_data(pkg, name):
    make = {"smooth": lambda: X.quad_target(pkg, smooth=True), "flat": lambda: X.quad_target(pkg), "mirrored": lambda: X.mirrored_target(pkg), "bump": lambda: X.bump_source(pkg),
            "bump_n": lambda: X.bump_source(pkg, normals=True), "mixed": lambda: X.mixed_source(pkg)}
    return cached(("sd", name), make[name])


def model(oracle, pkg, target, source, size, front, back, **kw):
    key = ("model", target, source, size, front, back) + tuple(sorted(kw.items()))
    tg, src = scene_data(pkg, target), scene_data(pkg, source)
    osc = cached(("osc", source), lambda: oracle.scene(src))
    return cached(key, lambda: T.transfer(oracle, pkg, tg, src, tg.prim_group == 0, size[0], size[1], front, back, orc_source=osc, **kw))


def assert_planes(got, want, what=()):
    for k in WRITTEN:
        assert same(got[k], want[k]), (k, what, np.argwhere(got[k] != want[k])[:6])


# ---- 1. the written planes ----
@pytest.mark.parametrize("size", [(16, 16), (24, 8)])
@pytest.mark.parametrize("back", [0.3, 0.02])
@pytest.mark.parametrize("source", ["bump", "bump_n"])
@pytest.mark.parametrize("target", ["smooth", "mirrored"])
def test_the_written_planes_are_the_models(pkg, gpu, oracle, target, source, back, size):
    want = model(oracle, pkg, target, source, size, 0.3, back)
    tg, src = pkg.Scene(gpu, scene_data(pkg, target)), pkg.Scene(gpu, scene_data(pkg, source))
    got = tg.bake_transfer(src, 0, size[0], size[1], 0.3, back, planes=WRITTEN)
    assert_planes(got, want, (target, source, back, size))
    assert want["detail"].any() and (want["hit_prim"][want["owner"] != NONE] == NONE).any()
    names = {s["name"] for s in src.kernel_stats()}
    assert {"bake_select", "bake_raster", "bake_project", "extend", "bake_transfer_points"} <= names and not names & {"bake_transfer_rays", "shadow", "bake_accum"}
    assert src.counters()["shadow_tests"] == 0


@pytest.mark.parametrize("size", [(16, 16), (24, 8)])
def test_a_sphere_and_an_instance_leave_hit_prim_and_height_only(pkg, gpu, oracle, size):
    want = model(oracle, pkg, "smooth", "mixed", size, 0.3, 0.3)
    sd = scene_data(pkg, "mixed")
    tg, src = pkg.Scene(gpu, scene_data(pkg, "smooth")), pkg.Scene(gpu, sd)
    got = tg.bake_transfer(src, 0, size[0], size[1], 0.3, 0.3, planes=WRITTEN)
    assert_planes(got, want, size)
    other = (got["hit_prim"] != NONE) & ~want["detail"]
    assert ((sd.prim_shape[got["hit_prim"][other]] >> np.uint32(30)) != 0).any() and (~T.top_level_triangles(sd)[got["hit_prim"][other]]).all()
    assert got["height"][other].all() and not got["src_position"][other].any() and not got["src_normal"][other].any() and not got["tangent_normal"][other].any()


# ---- 2. single rays ----
def test_transfer_rays_are_the_models(pkg, gpu, oracle):
    tg, src = pkg.Scene(gpu, scene_data(pkg, "smooth")), pkg.Scene(gpu, scene_data(pkg, "mixed"))
    for sampler, cos in (("sobol", True), ("halton", False)):
        want = model(oracle, pkg, "smooth", "mixed", (16, 16), 0.3, 0.3, spp=2, nsamples=5, cos_sample=cos, sampler=sampler)
        pr, ar = want["rays"], want["ao_rays"]
        zero = np.zeros(len(pr["texel"]), np.uint32)
        got = tg.bake_transfer_rays(src, 0, 16, 16, 0.3, 0.3, 2, pr["texel"], zero, zero, nsamples=5, cos_sample=cos, sampler=sampler)
        assert (got["found"] & 1).all() and same(got["o"], pr["o"]) and same(got["d"], pr["d"]) and same(got["t_max"], pr["t_max"])
        assert np.array_equal((got["found"] & 2) != 0, want["detail"].reshape(-1)[pr["texel"]])
        got = tg.bake_transfer_rays(src, 0, 16, 16, 0.3, 0.3, 2, ar["texel"], ar["s"], ar["k"], nsamples=5, cos_sample=cos, sampler=sampler)
        assert (got["found"] == 3).all() and len(ar["w"]) == int(want["detail"].sum()) * 10
        assert same(got["ao_o"], ar["o"]) and same(got["ao_d"], ar["d"]) and same(got["ao_w"], ar["w"])
    unowned = np.flatnonzero(want["owner"].reshape(-1) == NONE)[:3]
    missed = np.array([t for t, k in want["kinds"].items() if k != "detail"][:3])
    got = tg.bake_transfer_rays(src, 0, 16, 16, 0.3, 0.3, 2, np.concatenate([unowned, missed]), np.zeros(6), np.zeros(6), nsamples=5)
    assert list(got["found"]) == [0, 0, 0, 1, 1, 1] and not got["o"][:3].any() and not got["ao_d"].any() and not got["ao_w"].any()


# ---- 3. ambient occlusion at the source hit ----
AO_CASES = [(ns, sampler, cos) for ns in (3, 70) for sampler in ("sobol", "halton") for cos in (True, False)]


@pytest.mark.parametrize("ns,sampler,cos", AO_CASES)
def test_ao_sums_are_the_models(pkg, gpu, oracle, ns, sampler, cos):
    tg, src = pkg.Scene(gpu, scene_data(pkg, "smooth")), pkg.Scene(gpu, scene_data(pkg, "mixed"))
    spp, occluded = 2, {}
    for dist in (float("inf"), 0.15):   # 0.15: the sphere and the card are out of most hits' reach
        want = model(oracle, pkg, "smooth", "mixed", (16, 16), 0.3, 0.3, spp=spp, nsamples=ns, cos_sample=cos, max_distance=dist, sampler=sampler)
        got = tg.bake_transfer(src, 0, 16, 16, 0.3, 0.3, spp=spp, nsamples=ns, cos_sample=cos, max_distance=dist, sampler=sampler)
        assert_planes(got, want, dist)
        assert same(got["ao_w"], want["ao_w"]), (dist, float(np.abs(got["ao_w"] - want["ao_w"]).max()))
        assert not got["ao_w"][~want["detail"]].any()
        assert src.counters()["shadow_tests"] == want["n_rays"] == int(want["detail"].sum()) * spp * ns
        assert 0 < want["occluded"].sum() < want["n_rays"]
        occluded[dist] = int(want["occluded"].sum())
    assert occluded[0.15] < occluded[float("inf")]
    names = {s["name"]: s for s in src.kernel_stats()}
    assert {"bake_select", "bake_raster", "bake_project", "extend", "bake_transfer_points", "bake_transfer_rays", "shadow", "bake_accum"} <= set(names)
    assert names["shadow"]["launches"] == spp * 2 if ns > 64 else names["shadow"]["launches"] >= 1
    assert names["extend"]["launches"] == 1 and names["bake_project"]["launches"] == 1


@pytest.mark.parametrize("ns,sampler", [(3, "halton"), (70, "sobol")])
def test_ranges_pass_sizes_and_repeats_leave_the_same_bytes(pkg, gpu, oracle, ns, sampler):
    tg, src = pkg.Scene(gpu, scene_data(pkg, "mirrored")), pkg.Scene(gpu, scene_data(pkg, "bump_n"))
    want = model(oracle, pkg, "mirrored", "bump_n", (16, 16), 0.3, 0.3, spp=2, nsamples=ns, sampler=sampler)
    kw = dict(spp=2, nsamples=ns, sampler=sampler)
    whole = tg.bake_transfer(src, 0, 16, 16, 0.3, 0.3, **kw)
    assert same(whole["ao_w"], want["ao_w"]) and np.abs(whole["ao_w"]).max() > 0
    assert_planes(whole, want)
    parts = tg.bake_transfer(src, 0, 16, 16, 0.3, 0.3, samples=(0, 1), **kw)
    first = parts["ao_w"].copy()
    tg.bake_transfer(src, 0, 16, 16, 0.3, 0.3, samples=(1, 1), sums=parts, **kw)
    assert same(parts["ao_w"], whole["ao_w"]) and not same(first, whole["ao_w"])
    assert_planes(parts, want)   # (the written planes are written again, the same)
    assert tg.bake_transfer_pass_size(src, 16, 16, 0.3, 0.3, 2, nsamples=ns) == (2 if ns <= 64 else 1) and tg.bake_transfer_pass_size(src, 16, 16, 0.3, 0.3, 2, nsamples=ns, spp_per_pass=1) == 1
    assert same(tg.bake_transfer(src, 0, 16, 16, 0.3, 0.3, spp_per_pass=1, **kw)["ao_w"], whole["ao_w"])
    assert same(tg.bake_transfer(src, 0, 16, 16, 0.3, 0.3, spp_per_pass=0, **kw)["ao_w"], whole["ao_w"])


def test_device_buffers_and_free_memory(pkg, gpu):
    torch = pytest.importorskip("torch")
    K = pkg._abi_bake
    tg, src = pkg.Scene(gpu, scene_data(pkg, "smooth")), pkg.Scene(gpu, scene_data(pkg, "mixed"))
    host = tg.bake_transfer(src, 0, 24, 8, 0.3, 0.3, spp=2, nsamples=6)
    dev = {k: torch.zeros((8, 24) + ((K.TRANSFER_CHANNELS[k],) if K.TRANSFER_CHANNELS[k] > 1 else ()), dtype=torch.int32 if K.TRANSFER_DTYPES[k] == "uint32" else torch.float32, device="cuda")
           for k in K.TRANSFER_PLANES}
    torch.cuda.synchronize()
    assert tg.bake_transfer(src, 0, 24, 8, 0.3, 0.3, spp=2, nsamples=6, device_ptrs={k: v.data_ptr() for k, v in dev.items()}) is None
    for k, v in dev.items():
        assert v.cpu().numpy().tobytes() == host[k].tobytes(), k
    before = torch.cuda.mem_get_info(0)[0]
    for _ in range(3):
        tg.bake_transfer(src, 0, 24, 8, 0.3, 0.3, spp=2, nsamples=6)
    assert torch.cuda.mem_get_info(0)[0] == before


# ---- 4. the two handles ----
def test_the_target_scene_is_not_disturbed(pkg, gpu, oracle):
    """Target and source are separate handles on one device: the target's own bake gives the same bytes before and after it served as a transfer's target, and its
    statistics are still those of its own bake."""
    tg, src = pkg.Scene(gpu, scene_data(pkg, "smooth")), pkg.Scene(gpu, scene_data(pkg, "mixed"))
    before = tg.bake(0, 16, 16, 2, nsamples=6)
    stats = [(s["name"], s["launches"]) for s in tg.kernel_stats()]
    counters = tg.counters()
    got = tg.bake_transfer(src, 0, 16, 16, 0.3, 0.3, spp=2, nsamples=6)
    assert (got["hit_prim"] != NONE).any() and np.abs(got["ao_w"]).max() > 0
    assert [(s["name"], s["launches"]) for s in tg.kernel_stats()] == stats and tg.counters() == counters
    after = tg.bake(0, 16, 16, 2, nsamples=6)
    for k in before:
        assert same(before[k], after[k]), k
    assert same(got["owner"], before["owner"])


def test_one_handle_as_target_and_source(pkg, gpu, oracle):
    """The target is all the rays see: every owned texel's ray hits the target itself -- the triangle that owns the texel or its neighbour across the diagonal -- at the
    model's t."""
    want = model(oracle, pkg, "smooth", "smooth", (16, 16), 0.3, 0.3, spp=1, nsamples=4)
    sc = pkg.Scene(gpu, scene_data(pkg, "smooth"))
    got = sc.bake_transfer(sc, 0, 16, 16, 0.3, 0.3, spp=1, nsamples=4)
    assert_planes(got, want)
    assert same(got["ao_w"], want["ao_w"])
    owned = got["owner"] != NONE
    assert owned.sum() == 196 and np.isin(got["hit_prim"][owned], (0, 1)).all() and (got["hit_prim"][~owned] == NONE).all()
    t = np.float32(0.3) - got["height"][owned]
    assert np.abs(t - 0.3).max() < 1e-6 and np.abs(got["height"][owned]).max() < 1e-6


# ---- 5. dilation ----
def test_hit_prim_is_a_coverage_map_for_the_dilation(pkg, gpu, oracle):
    want = model(oracle, pkg, "mirrored", "bump", (24, 8), 0.3, 0.02)
    tg, src = pkg.Scene(gpu, scene_data(pkg, "mirrored")), pkg.Scene(gpu, scene_data(pkg, "bump"))
    got = tg.bake_transfer(src, 0, 24, 8, 0.3, 0.02, planes=("hit_prim", "tangent_normal", "height"))
    assert 0 < (got["hit_prim"] != NONE).sum() < got["hit_prim"].size
    for k in ("tangent_normal", "height"):
        model_plane = cached(("dilate", k), lambda: M.dilate(want["hit_prim"], want[k], 2))
        assert same(src.bake_dilate(got["hit_prim"], got[k], 2), model_plane), k
        assert not same(model_plane, want[k])


# ---- errors that need a scene ----
def test_refusals_that_read_the_scenes(pkg, gpu):
    A, K = pkg._abi, pkg._abi_bake
    tgd, srd = scene_data(pkg, "smooth"), scene_data(pkg, "mixed")
    tg, src = pkg.Scene(gpu, tgd), pkg.Scene(gpu, srd)
    tp = tg.bake_transfer_params(8, 8, 0.3, 0.3)
    hit = np.full((8, 8), 5, np.uint32)
    sel = np.ones(len(srd.prim_group), np.uint8)   # the SOURCE's count: the selection names the target's primitives
    st = gpu.bake.pt_bake_transfer(tg.h, src.h, C.byref(tp), sel.ctypes.data_as(A.u8p), len(sel), C.byref(K.transfer_buffers({"hit_prim": hit})), 0)
    assert st == A.PT_ERR_INVALID_ARG and b"primitives" in gpu.lib.pt_last_error() and (hit == 5).all()
    with pytest.raises(pkg.runtime.PtError) as e:   # a sphere of the source is no target
        src.bake_transfer(tg, [1], 8, 8, 0.3, 0.3, planes=("hit_prim",))
    assert f"status {A.PT_ERR_UNSUPPORTED}" in str(e.value) and "sphere or disk" in str(e.value)
    with pytest.raises(pkg.runtime.PtError) as e:
        tg.bake_transfer(src, 0, 8, 8, 0.3, 0.3, spp=1 << 20, nsamples=1 << 31, planes=("ao_w",))
    assert "Sobol" in str(e.value)
    assert (tg.bake_transfer(src, 0, 8, 8, 0.3, 0.3, spp=1 << 20, nsamples=1 << 31, planes=("hit_prim",))["hit_prim"] != NONE).any()   # (not read without ao_w)


# ---- 6. the tool ----
LOW = ('LookAt 0 0 5  0 0 0  0 1 0\nCamera "perspective" "float fov" 30\nFilm "image" "integer xresolution" 8 "integer yresolution" 8\nWorldBegin\n'
       'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0  1 -1 0  1 1 0  -1 1 0] "float uv" [0.1 0.1 0.9 0.1 0.9 0.9 0.1 0.9]\nWorldEnd\n')
HIGH = ('LookAt 0 0 5  0 0 0  0 1 0\nCamera "perspective" "float fov" 30\nFilm "image" "integer xresolution" 8 "integer yresolution" 8\nWorldBegin\n'
        'Shape "trianglemesh" "integer indices" [0 1 4 1 2 4 2 3 4 3 0 4] "point P" [-0.8 -0.8 -0.1  0.8 -0.8 -0.1  0.8 0.8 -0.1  -0.8 0.8 -0.1  0 0 0.2]\n'
        'AttributeBegin\nTranslate 0.4 0.4 0.1\nShape "sphere" "float radius" 0.15\nAttributeEnd\nWorldEnd\n')


def test_bake_transfer_tool_writes_what_the_library_gives(pkg, gpu, tmp_path):
    low, high = tmp_path / "low.pbrt", tmp_path / "high.pbrt"
    low.write_text(LOW); high.write_text(HIGH)
    nrm, hgt, ao = tmp_path / "n.pfm", tmp_path / "h.pfm", tmp_path / "ao.pfm"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bake_transfer.py"), str(low), str(high), "--shape", "0", "--size", "24x16", "--front", "0.5", "--back", "0.25", "--spp", "2",
                        "--nsamples", "8", "--dilate", "2", "--normal", str(nrm), "--height", str(hgt), "--ao", str(ao)], capture_output=True, text=True, timeout=300, env=trace_env())
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    tg, src = pkg.Scene(gpu, pkg.frontend.FrontScene(path=str(low))), pkg.Scene(gpu, pkg.frontend.FrontScene(path=str(high)))
    p = tg.bake_transfer(src, [0], 24, 16, 0.5, 0.25, spp=2, nsamples=8, planes=("owner", "hit_prim", "height", "tangent_normal", "ao_w"))
    rays = src.counters()["shadow_tests"]
    cov = p["hit_prim"] != NONE
    detail = np.where((p["tangent_normal"] != 0).any(axis=-1), p["hit_prim"], np.uint32(NONE)).astype(np.uint32)   # (the sphere's hits have a height and no normal)
    assert 0 < (detail != NONE).sum() < cov.sum()
    a = pkg.runtime.resolve_bake(p["ao_w"], 2)[0]
    tn, h, a = src.bake_dilate(detail, p["tangent_normal"], 2), src.bake_dilate(p["hit_prim"], p["height"], 2), src.bake_dilate(detail, a, 2)
    covered = src.bake_dilate(detail, (detail != NONE).astype(np.float32), 2) > 0
    assert covered.sum() > (detail != NONE).sum() and not covered.all()
    img = pkg.frontend.read_image(str(nrm))
    assert img.shape == (16, 24, 3) and same(img, pkg.runtime.encode_normal_map(tn, covered))
    assert (img[~covered] == np.array([0.5, 0.5, 1], np.float32)).all() and (img[covered][:, 2] > 0.5).all()
    assert same(pkg.frontend.read_image(str(hgt)), np.repeat(h[..., None], 3, axis=2)) and same(pkg.frontend.read_image(str(ao)), np.repeat(a[..., None], 3, axis=2))
    assert line["owned_texels"] == int((p["owner"] != NONE).sum()) and line["hits"] == int(cov.sum()) and line["rays"] == rays > 0 and {"bake_project", "extend", "shadow"} <= set(line["ms"])
    assert h[cov].max() > 0.15 and h[cov].min() < 0     # the sphere's top and apex; the pyramid's foot lies under the target
