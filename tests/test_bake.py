"""The texture-space bake on the GPU (libmi355bake.so, include/mi355bake.h) against the numpy model of its contract (tests/bake_reference.py), bit for bit: every
quantity is a stated float32 operation order and the library is compiled without contraction, so no tolerance is needed. Occlusion in the model comes from the
oracle's any-hit query over the model's rays."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import bake_reference as M
import bake_scenes as S
from conftest import trace_env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
_CACHE = {}   # the model's results, computed once (every test runs under both walks)


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1. ownership ----
def ownership_cases():
    tiny = S.small_triangles()
    return {
        "diagonal": dict(uvs=S.QUAD_UV, idx=S.QUAD_IDX),
        "overlap": dict(uvs=[(0.1, 0.1), (0.7, 0.15), (0.3, 0.8), (0.25, 0.2), (0.9, 0.3), (0.6, 0.95), (0.05, 0.5), (0.95, 0.45), (0.5, 0.62)], idx=[0, 1, 2, 3, 4, 5, 6, 7, 8]),
        "outside": dict(uvs=[(0.6, 0.4), (1.7, 0.5), (0.8, 1.4), (1.2, 1.2), (1.9, 1.3), (1.4, 1.8), (-0.5, -0.2), (0.3, 0.1), (0.1, 0.45)], idx=[0, 1, 2, 3, 4, 5, 6, 7, 8]),
        "corner": dict(uvs=[(0, 0), (0.5, 0), (0, 0.5), (1, 1), (0.5, 1), (1, 0.5)], idx=[0, 1, 2, 3, 4, 5]),
        "sub_texel": dict(uvs=[(0.501, 0.501), (0.53, 0.501), (0.501, 0.53), (0.2, 0.2), (0.45, 0.25), (0.3, 0.4)], idx=[0, 1, 2, 3, 4, 5]),
        "needle": dict(uvs=[(0.0, 0.02), (1.0, 0.97), (1.0, 0.99), (0.01, 1.0), (0.02, 0.0), (0.03, 1.0)], idx=[0, 1, 2, 3, 4, 5]),
        "zero_area": dict(uvs=[(0.1, 0.1), (0.5, 0.5), (0.9, 0.9), (0.3, 0.6), (0.3, 0.6), (0.7, 0.2), (0.2, 0.6), (0.8, 0.7), (0.4, 0.9)], idx=[0, 1, 2, 3, 4, 5, 6, 7, 8]),
        "many": dict(uvs=tiny[0], idx=tiny[1]),
        "second_shape": dict(uvs=S.QUAD_UV, idx=S.QUAD_IDX, second=([(0.2, 0.1), (0.9, 0.3), (0.4, 0.85)], [0, 1, 2]), shape=1),
    }


@pytest.mark.parametrize("size", [(16, 16), (24, 8)])
@pytest.mark.parametrize("case", sorted(ownership_cases()))
def test_ownership_is_the_models(pkg, gpu, case, size):
    c = ownership_cases()[case]
    w, h = size
    sd = S.uv_mesh(pkg, c["uvs"], c["idx"], c.get("second"))
    select = sd.prim_group == c.get("shape", 0)
    want = cached(("own", case, size), lambda: M.owner_map(M.scene_triangles(sd, select)[1], M.scene_triangles(sd, select)[0], w, h))
    sc = pkg.Scene(gpu, sd)
    got = sc.bake(c.get("shape", 0), w, h, 1, planes=("owner",))["owner"]
    assert same(got, want), (case, np.argwhere(got != want)[:8])
    if case in ("sub_texel", "zero_area", "outside"):
        assert (got == NONE).any()
    if case == "many":
        assert len(np.unique(got)) > 100   # (triangles of more than one wave and block own texels: 338 are selected)
    if case == "second_shape":
        assert set(np.unique(got)) <= {2, NONE} and (got == 2).any()
    names = {s["name"] for s in sc.kernel_stats()}
    assert {"bake_select", "bake_raster"} <= names and "shadow" not in names and sc.counters()["shadow_tests"] == 0


def test_a_quad_over_a_64x64_atlas(pkg, gpu):
    sd = S.uv_mesh(pkg, S.QUAD_UV, S.QUAD_IDX)
    select = sd.prim_group == 0
    want = cached(("own", "quad64"), lambda: M.owner_map(M.scene_triangles(sd, select)[1], M.scene_triangles(sd, select)[0], 64, 64))
    got = pkg.Scene(gpu, sd).bake(0, 64, 64, 1, planes=("owner",))["owner"]
    assert same(got, want) and (got != NONE).all() and (np.diag(got) == 0).all()


def test_a_sliver_owns_nothing_outside_its_texel_box(pkg, gpu):
    """A nearly collinear triangle (det of a few 1e-9) whose barycentrics, rounded, contain the centre of a texel far beyond its far vertex (tests/test_bake_model.py):
    the contract's texel box denies it that texel, on the device as in the model, and the higher-numbered triangle behind keeps it."""
    from test_bake_model import SLIVER, BEHIND_SLIVER
    sd = S.uv_mesh(pkg, SLIVER + BEHIND_SLIVER, [0, 1, 2, 3, 4, 5])
    prims, uv = M.scene_triangles(sd, sd.prim_group == 0)
    want = cached(("own", "sliver"), lambda: M.owner_map(uv, prims, 64, 64))
    unboxed = cached(("own", "sliver_unboxed"), lambda: M.owner_map(uv, prims, 64, 64, boxed=False))
    assert unboxed[37, 34] == 0 and want[37, 34] == 1   # (the case reaches what it is about)
    got = pkg.Scene(gpu, sd).bake(0, 64, 64, 1, planes=("owner",))["owner"]
    assert same(got, want), np.argwhere(got != want)[:8]


# ---- 2. position and normal ----
@pytest.mark.parametrize("case", ["flat", "normals", "reverse", "mirror", "normals_reverse_mirror"])
def test_position_and_normal_planes_are_the_models(pkg, gpu, case):
    sd = S.shaded(pkg, normals="normals" in case, reverse="reverse" in case, mirror="mirror" in case)
    select = sd.prim_group == 0

    def model():
        prims, uv = M.scene_triangles(sd, select)
        owner = M.owner_map(uv, prims, 16, 16)
        return (owner,) + M.planes(sd, owner)
    owner, pos, nrm = cached(("planes", case), model)
    got = pkg.Scene(gpu, sd).bake(0, 16, 16, 1, planes=("owner", "position", "normal"))
    assert same(got["owner"], owner) and (owner != NONE).sum() > 100
    assert same(got["position"], pos), float(np.abs(got["position"] - pos).max())
    assert same(got["normal"], nrm), float(np.abs(got["normal"] - nrm).max())
    if case == "flat":
        flipped = pkg.Scene(gpu, S.shaded(pkg, reverse=True)).bake(0, 16, 16, 1, planes=("normal",))["normal"]
        assert np.array_equal(flipped, -nrm)   # ReverseOrientation turns the normal round


# ---- 3. ambient occlusion ----
AO_CASES = [(ns, sampler, cos) for ns in (3, 70) for sampler in ("sobol", "halton") for cos in (True, False)]


@pytest.mark.parametrize("ns,sampler,cos", AO_CASES)
def test_ao_sums_owner_and_ray_count_are_the_models(pkg, gpu, oracle, ns, sampler, cos):
    sd = S.occluded_floor(pkg)
    select = sd.prim_group == 0
    spp = 3
    osc = cached("ao_oracle_scene", lambda: oracle.scene(sd))
    sc = pkg.Scene(gpu, sd)
    for dist in (float("inf"), 1.5):   # 1.5: the sphere (z >= 2.4) is out of reach
        want = cached(("ao", ns, sampler, cos, dist), lambda: M.bake(oracle, pkg, sd, select, 16, 16, spp, ns, cos, dist, sampler, orc_scene=osc))
        got = sc.bake(0, 16, 16, spp, nsamples=ns, cos_sample=cos, max_distance=dist, sampler=sampler, planes=("owner", "ao_w"))
        assert same(got["owner"], want["owner"]) and (want["owner"] != NONE).all()
        assert same(got["ao_w"], want["ao_w"]), (dist, float(np.abs(got["ao_w"] - want["ao_w"]).max()))
        c = sc.counters()
        assert c["shadow_tests"] == want["n_rays"] == 256 * spp * ns and c["camera_rays"] == 0
        assert 0 < want["occluded"].sum() < want["n_rays"]
    near, far = _CACHE[("ao", ns, sampler, cos, 1.5)], _CACHE[("ao", ns, sampler, cos, float("inf"))]
    assert near["occluded"].sum() < far["occluded"].sum()   # the sphere occludes only the unbounded rays
    names = {s["name"]: s for s in sc.kernel_stats()}
    assert {"bake_raster", "bake_rays", "shadow", "bake_accum"} <= set(names)
    assert names["shadow"]["launches"] == spp * 2 if ns > 64 else names["shadow"]["launches"] >= 1


def test_bake_rays_are_the_models(pkg, gpu, oracle):
    sd = S.occluded_floor(pkg)
    select = sd.prim_group == 0
    for sampler, cos in (("sobol", True), ("halton", False)):
        owner = M.owner_map(M.scene_triangles(sd, select)[1], M.scene_triangles(sd, select)[0], 16, 16)
        r = cached(("rays", sampler, cos), lambda: M.rays(oracle, pkg, sd, owner, 2, 5, cos, sampler))
        o, d, w, found = pkg.Scene(gpu, sd).bake_rays(0, 16, 16, 2, r["texel"], r["s"], r["k"], nsamples=5, cos_sample=cos, sampler=sampler)
        assert found.all() and same(o, r["o"]) and same(d, r["d"]) and same(w, r["w"])


# ---- 4. continuation ----
def test_ranges_pass_sizes_repeats_and_device_buffers_agree(pkg, gpu):
    torch = pytest.importorskip("torch")
    sd = S.occluded_floor(pkg)
    sc = pkg.Scene(gpu, sd)
    kw = dict(nsamples=6, sampler="halton", planes=("ao_w",))
    whole = sc.bake(0, 16, 16, 3, **kw)["ao_w"]
    assert np.abs(whole).max() > 0
    parts = sc.bake(0, 16, 16, 3, samples=(0, 1), **kw)
    sc.bake(0, 16, 16, 3, samples=(1, 2), sums=parts, **kw)
    assert same(parts["ao_w"], whole)
    assert sc.bake_pass_size(16, 16, 3, nsamples=6) == 3 and sc.bake_pass_size(16, 16, 3, nsamples=6, spp_per_pass=1) == 1 and sc.bake_pass_size(16, 16, 3, nsamples=70) == 1
    assert same(sc.bake(0, 16, 16, 3, spp_per_pass=1, **kw)["ao_w"], whole)
    assert same(sc.bake(0, 16, 16, 3, spp_per_pass=2, **kw)["ao_w"], whole)
    assert same(sc.bake(0, 16, 16, 3, **kw)["ao_w"], whole)
    dev = {"owner": torch.zeros((16, 16), dtype=torch.int32, device="cuda"), "position": torch.zeros((16, 16, 3), device="cuda"), "normal": torch.zeros((16, 16, 3), device="cuda"),
           "ao_w": torch.zeros((16, 16, 4), device="cuda")}
    torch.cuda.synchronize()
    host = sc.bake(0, 16, 16, 3, nsamples=6, sampler="halton")
    assert sc.bake(0, 16, 16, 3, nsamples=6, sampler="halton", device_ptrs={k: v.data_ptr() for k, v in dev.items()}) is None
    for k, v in dev.items():
        assert v.cpu().numpy().tobytes() == host[k].tobytes(), k


# ---- 5. dilation ----
@pytest.mark.parametrize("channels", [1, 4])
def test_dilation_is_the_models(pkg, gpu, channels):
    sd = S.uv_mesh(pkg, [(0.3, 0.25), (0.75, 0.4), (0.45, 0.8), (0.05, 0.05), (0.2, 0.05), (0.05, 0.2)], [0, 1, 2, 3, 4, 5])
    sc = pkg.Scene(gpu, sd)
    owner = sc.bake(0, 24, 8, 1, planes=("owner",))["owner"]
    assert 0 < (owner != NONE).sum() < owner.size
    rng = np.random.RandomState(11)
    plane = rng.uniform(-2, 2, (8, 24) + ((channels,) if channels > 1 else ())).astype(np.float32)
    for it in (0, 1, 4):
        want = cached(("dilate", channels, it), lambda: M.dilate(owner, plane, it))
        got = sc.bake_dilate(owner, plane, it)
        assert same(got, want), (it, float(np.abs(got - want).max()))
    assert not same(_CACHE[("dilate", channels, 4)], _CACHE[("dilate", channels, 1)])
    empty = np.full((8, 24), NONE, np.uint32)
    assert same(sc.bake_dilate(empty, plane, 4), plane)
    assert any(s["name"] == "bake_dilate" for s in sc.kernel_stats())


# ---- 6. memory ----
def test_bakes_leave_free_memory_unchanged(pkg, gpu):
    torch = pytest.importorskip("torch")
    sd = S.occluded_floor(pkg)
    sc = pkg.Scene(gpu, sd)
    sc.bake(0, 16, 16, 2, nsamples=8); sc.bake_dilate(np.zeros((16, 16), np.uint32), np.zeros((16, 16), np.float32), 1)   # (the scene's workspace: allocated once, lives with the scene)
    before = torch.cuda.mem_get_info(0)[0]
    for _ in range(5):
        planes = sc.bake(0, 16, 16, 2, nsamples=8)
        sc.bake_dilate(planes["owner"], planes["ao_w"], 2)
    assert torch.cuda.mem_get_info(0)[0] == before


# ---- errors that need a scene ----
def test_refusals_that_read_the_scene(pkg, gpu):
    A, K = pkg._abi, pkg._abi_bake
    b = S._builder(pkg)
    S.floor(b)                                                             # shape 0: UV-mapped
    b.trianglemesh([(0, 0, 1), (1, 0, 1), (0, 1, 1)], [0, 1, 2])           # shape 1: no UVs
    b.sphere(radius=0.3)                                                   # shape 2
    b.object_begin("o"); S.floor(b, half=0.2, z=1.5); b.object_end()       # shape 3: lives in an object
    b.object_instance("o")
    sd = b.world_end()[0]
    sc = pkg.Scene(gpu, sd)
    for shape, text in ((1, "without UVs"), (2, "sphere or disk"), (3, "instanced object")):
        with pytest.raises(pkg.runtime.PtError) as e:
            sc.bake(shape, 8, 8, 1, planes=("owner",))
        first = int(np.nonzero(sd.prim_group == shape)[0][0])
        assert f"status {A.PT_ERR_UNSUPPORTED}" in str(e.value) and text in str(e.value) and f"primitive {first} " in str(e.value)
    bp = sc.bake_params(8, 8, 1)
    owner = np.zeros((8, 8), np.uint32)
    sel = np.ones(len(sd.prim_group) + 1, np.uint8)
    st = gpu.bake.pt_bake_render(sc.h, C.byref(bp), sel.ctypes.data_as(A.u8p), len(sel), C.byref(K.buffers({"owner": owner})), 0)
    assert st == A.PT_ERR_INVALID_ARG and b"primitives" in gpu.lib.pt_last_error()
    with pytest.raises(pkg.runtime.PtError) as e:
        sc.bake(0, 8, 8, 1 << 20, nsamples=1 << 31, planes=("ao_w",))
    assert "Sobol" in str(e.value)
    with pytest.raises(pkg.runtime.PtError) as e:   # (the Halton stride of an 8 x 8 grid is 2^3 * 3^2 = 72: 64-bit indices reach 2.6e17 sample numbers, not 2^62)
        sc.bake(0, 8, 8, 1 << 31, nsamples=1 << 31, sampler="halton", planes=("ao_w",))
    assert "Halton" in str(e.value)
    assert (sc.bake(0, 8, 8, 1, planes=("owner",))["owner"] != NONE).all()   # the scene bakes after the refusals


# ---- 7. the tool ----
def test_bake_ao_tool_writes_what_the_library_gives(pkg, gpu, tmp_path):
    scene = tmp_path / "bake.pbrt"
    scene.write_text('LookAt 0 0 5  0 0 0  0 1 0\nCamera "perspective" "float fov" 30\nFilm "image" "integer xresolution" 8 "integer yresolution" 8\nWorldBegin\n'
                     'Shape "sphere" "float radius" 0.5\n'
                     'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-2 -2 -0.6  2 -2 -0.6  2 2 -0.6  -2 2 -0.6] "float uv" [0.1 0.1 0.9 0.1 0.9 0.9 0.1 0.9]\nWorldEnd\n')
    out, bent = tmp_path / "ao.pfm", tmp_path / "bent.pfm"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bake_ao.py"), str(scene), "--shape", "1", "--size", "24x16", "--spp", "2", "--nsamples", "8", "--dilate", "2",
                        "--out", str(out), "--bent", str(bent)], capture_output=True, text=True, timeout=300, env=trace_env())
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    fs = pkg.frontend.FrontScene(path=str(scene))
    sc = pkg.Scene(gpu, fs)
    planes = sc.bake(1, 24, 16, 2, nsamples=8, planes=("owner", "ao_w"))
    ao, bn = pkg.runtime.resolve_bake(planes["ao_w"], 2)
    ao, bn = sc.bake_dilate(planes["owner"], ao, 2), sc.bake_dilate(planes["owner"], bn, 2)
    got = pkg.frontend.read_image(str(out))
    assert got.shape == (16, 24, 3) and same(got, np.repeat(ao[..., None], 3, axis=2))
    assert same(pkg.frontend.read_image(str(bent)), bn)
    owned = planes["owner"] != NONE
    assert line["owned_texels"] == int(owned.sum()) and line["rays"] == int(owned.sum()) * 16 and "shadow" in line["ms"]
    assert 0 < ao[owned].min() < 0.9 and ao[owned].max() > 0.99   # dark under the sphere, open at the rim
