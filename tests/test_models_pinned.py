"""The numpy models' outputs, pinned: the SHA-256 of what every model's public entry returns on small inputs, recorded at the commit before the models were moved
onto tests/model_math.py. The GPU tests hold the device to these models byte for byte; this file holds the models to themselves, without a GPU, so that a change
of their arithmetic shows here first. An output is hashed as its dtype, shape and tobytes(); a dict by its sorted keys, a list in order."""
import hashlib

import numpy as np
import pytest

import aov_reference as AR
import bake_reference as M
import bake_scenes as S
import camera_model as cm
import lightmap_reference as LM
import lightmap_scenes as LS
import matte_reference as MR
import sh_reference as SR
import transfer_reference as T
import transfer_scenes as X
from tile_scene import with_filter

F = np.float32


def _feed(h, v):
    if isinstance(v, dict):
        for k in sorted(v, key=repr):
            h.update(repr(k).encode()); _feed(h, v[k])
    elif isinstance(v, (list, tuple)):
        h.update(b"[%d]" % len(v))
        for e in v:
            _feed(h, e)
    elif v is None or isinstance(v, str):
        h.update(repr(v).encode())
    else:
        a = np.ascontiguousarray(v)
        h.update(str(a.dtype).encode()); h.update(repr(a.shape).encode()); h.update(a.tobytes())


def digest(*values):
    h = hashlib.sha256()
    _feed(h, list(values))
    return h.hexdigest()


def hits(h):
    """camera_hits' dict as far as both ray sources always filled it."""
    return {k: h[k] for k in ("pix", "pfilm", "o", "d", "prim", "t", "b", "n")}


def check(name, *values):
    got = digest(*values)
    print(name, got)
    assert got == PINNED[name], (name, got)


PINNED = {
    "ao-flat-cos-sobol": "bf0b0521e692e625c055f6cd4df0919a2cecc2efd17a7cca1f604560e08b910a",
    "ao-mirror-normals-uniform-sobol-range": "619010d581d2e2535130e486588879a98713ffb6880c798e9c726ef2ca82982d",
    "ao-normals-uniform-halton-range": "c40dd83d298f528ac1376480c48a07d25bb65067b51c617b831b6072c49ce91d",
    "ao-reverse-cos-halton": "c476c5552a6c120fbfbf78f8cb398ce378e42ec77f3ac71047e5b503dadb2818",
    "aov-instances": "8b680ad8442d4cc52299268b352f113278369b77d18d129e0322db2393171e22",
    "aov-smooth-mesh": "39abcfa2973e6f413a4f913995893dea3b931820046f85cdb8dc71f5b6be8bfe",
    "camera-environment-lens": "69912103fbcc101a4e0200f9c9697c875a16f4b84a155475bbcc112f0776c9e6",
    "camera-environment-pinhole": "090e73f456cfa2994a3b209fd16a4c2413bdb1880de852d600b5ac856f1573ed",
    "camera-hits-orthographic": "63d7ee526b3e2a45ae6c7957b1c93159f594521b26b6f1aa7c5daa61870067b9",
    "camera-orthographic-lens": "554a991ebb3a34a4d9aed2e6ce14ea01a93e484e721defe66e2699457bf58eff",
    "camera-orthographic-pinhole": "5d6f7bf39174b3bff1c2fc5d575f740098cd55413e89f49cffcc40e6263eb2d6",
    "camera-perspective-lens": "dbba58f107b9b7c71631a0c1017b3d7f8106ad506e98c898764db8565260ceb2",
    "camera-perspective-pinhole": "9308b37bf24dfeeafa9eab1c72ef0c05cf2636d7ec902ebd256b5b6ce773aa47",
    "lightmap-all": "6c28b69510a5fab3dc0d8d52544db4fb93829170bfbd3e1bb2fc2f63e36d72e6",
    "lightmap-list": "a9566137c25aa1662e880b50f1be4bbd87ce0b21bed3b92b4a064461cad72478",
    "lightmap-mask": "ebe44448cf3ec2382418c5d501c3eca39c0c828e91afeaf4214d7c1ed4002b64",
    "lightmap-side-test": "24e0fd36720bca1138c10ed0f5bc267be1be0d55cd9d670f43ff5d21fffcfc8a",
    "matte-instances": "80b932f7d165b062c4fcfcf92ff26e1d80cb5b959a518cfe550d6f20b69ca921",
    "sh-default-row": "8cb7d717a551029f0b85bf15910f7046621a14244afa80043541358ebd5a1600",
    "sh-row-4": "df4aa04c5288620a7270bd3263ff2f724e69a7ab5f14b37369083cceea5d845c",
    "transfer-degenerate-uv": "bb41958fa4364bbab765bf1b4cf1818874cc72a17b94a913ec543c26cf802c20",
    "transfer-mirrored": "6c6287a93f4055b5ddf78943fc4787444967425bb49d0de88c1263a98c1fd963",
    "transfer-smooth-quad": "d16bcc782661d51d636490919291a5f9d5d2ef7d24e8031f991c0c05ae243553",
}


# ---- AO bake ------------------------------------------------------------------------------------------------------------------------------------------------------
AO_CASES = [
    ("ao-flat-cos-sobol", dict(), True, "sobol", None),
    ("ao-normals-uniform-halton-range", dict(normals=True), False, "halton", (1, 2)),
    ("ao-reverse-cos-halton", dict(reverse=True), True, "halton", None),
    ("ao-mirror-normals-uniform-sobol-range", dict(mirror=True, normals=True), False, "sobol", (2, 2)),
]


@pytest.mark.parametrize("name,scene_kw,cos_sample,sampler,samples", AO_CASES, ids=[c[0] for c in AO_CASES])
def test_ao_bake(pkg, oracle, name, scene_kw, cos_sample, sampler, samples):
    sd = S.shaded(pkg, **scene_kw)
    out = M.bake(oracle, pkg, sd, sd.prim_group == 0, 16, 16, 4, 3, cos_sample=cos_sample, sampler=sampler, samples=samples)
    assert out["n_rays"] > 0
    ao, bent = M.resolve(out["ao_w"], 4)
    check(name, out, ao, bent, M.dilate(out["owner"], ao, 2), M.dilate(out["owner"], bent, 1))


# ---- lightmap (device=None: the model-only path) --------------------------------------------------------------------------------------------------------------------
def _classes(pkg, sd, r):
    return {LM.light_class(pkg, sd, int(li)) for li in np.unique(r["light"][r["contributes"]])}


def test_lightmap_every_light_class(pkg, oracle):
    sd, shape = LS.scene(pkg, "occluded_floor", "all")
    out = LM.bake(oracle, pkg, sd, sd.prim_group == shape, 8, 8, 2, 4)   # 8 lights, 4 samples per sample number
    assert _classes(pkg, sd, out["samples"]) == {"position", "triangle", "other"} and out["occluded"].any()
    check("lightmap-all", out, *LM.resolve(out["light_w"], 2, 4))


@pytest.mark.parametrize("name,lights,spp,nsamples,samples", [
    ("lightmap-mask", np.array([1, 0, 0, 1, 0, 1, 0, 0], np.uint8), 2, 6, None),   # 3 lights, 6 samples per sample number
    ("lightmap-list", [5, 1, 3, 2], 4, 2, (1, 2)),                                  # 4 lights, 2 samples per sample number
], ids=["mask", "list"])
def test_lightmap_light_subsets(pkg, oracle, name, lights, spp, nsamples, samples):
    sd, shape = LS.scene(pkg, "shaded_normals", "all")
    out = LM.bake(oracle, pkg, sd, sd.prim_group == shape, 12, 12, spp, nsamples, lights=lights, samples=samples)
    assert out["n_rays"] > 0 and _classes(pkg, sd, out["samples"]) == {"position", "triangle", "other"}
    check(name, out, *LM.resolve(out["light_w"], spp, nsamples))


def test_lightmap_a_texel_fails_the_side_test(pkg, oracle):
    """A point light beside the tilted, curved patch: in front of some texels and behind others, whose samples have a pdf and a radiance and no contribution."""
    sd, shape = LS.scene(pkg, "shaded_normals", [lambda b: LS.point(b, at=(-0.6, 0.0, 0.3))])
    out = LM.bake(oracle, pkg, sd, sd.prim_group == shape, 16, 16, 1)
    r = out["samples"]
    failed = (r["pdf"] > 0) & ~(r["Li"] == 0).all(axis=1) & ~r["contributes"]
    assert failed.any() and r["contributes"].any()
    check("lightmap-side-test", out, *LM.resolve(out["light_w"], 1, 1))


# ---- SH points ------------------------------------------------------------------------------------------------------------------------------------------------------
POINTS = np.array([[-1.1, 0.9, 0.3], [1.4, -0.5, 0.2], [0.9, 1.2, 0.9], [-0.6, -1.3, 0.5], [1.3, 1.6, 0.1], [-0.7, -0.4, 0.15], [0.1, 0.2, -0.5]], F)
NORMALS = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1], [0.6, 0, 0.8], [0, -0.6, 0.8], [0.36, 0.48, 0.8]], F)


@pytest.mark.parametrize("name,row", [("sh-default-row", None), ("sh-row-4", 4)], ids=["default-row", "row-4"])
def test_sh_points(pkg, oracle, name, row):
    sd, _ = LS.scene(pkg, "occluded_floor", "all")
    assert SR.default_row(len(POINTS)) == 3   # 7 points: the last row holds one
    out = SR.bake(oracle, pkg, sd, POINTS, 2, 4, row=row)
    assert _classes(pkg, sd, out["samples"]) == {"position", "triangle", "other"}
    sh, reached = SR.resolve(out["sh_w"], 2, 4)
    check(name, out, sh, reached, SR.irradiance(sh, NORMALS), SR.basis(NORMALS))


# ---- transfer ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,target,size", [("transfer-smooth-quad", lambda pkg: X.quad_target(pkg, smooth=True), 16), ("transfer-mirrored", X.mirrored_target, 16),
                                              ("transfer-degenerate-uv", X.degenerate_uv_target, 5)], ids=["smooth-quad", "mirrored", "degenerate-uv"])
def test_transfer(pkg, oracle, name, target, size):
    sd_t = target(pkg)
    kw = dict(spp=2, nsamples=3, cos_sample=(size == 16), sampler="halton" if name == "transfer-mirrored" else "sobol", samples=(1, 1) if name == "transfer-smooth-quad" else None)
    out = [T.transfer(oracle, pkg, sd_t, X.bump_source(pkg, normals=True), sd_t.prim_group == 0, size, size, 0.5, 0.5, **kw)]
    if size == 5:   # the sliver's one texel lies beside the bump grid (a miss): a tilted plane under it gives the detail hit with the fallback partials
        assert not out[0]["detail"].any() and list(out[0]["kinds"].values()) == ["miss"]
        out.append(T.transfer(oracle, pkg, sd_t, X.plane_source(pkg, z=0.0, tilt=45.0), sd_t.prim_group == 0, size, size, 1.5, 1.5, **kw))
    assert out[-1]["detail"].any() and out[-1]["n_rays"] > 0
    check(name, *out)


# ---- cameras ------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "lens"])
@pytest.mark.parametrize("kind", ["perspective", "orthographic", "environment"])
def test_cameras(pkg, oracle, kind, lens):
    rp = cm.job(pkg, kind, sampler="halton" if lens else "sobol", lens=lens).render_params()
    pix, cs = cm.camera_samples(pkg, oracle, rp)
    if kind == "environment":
        cs = np.concatenate([cs, cm.film_corners(rp)])
    extra = [cm.differentials(oracle, rp, cs, corrected=True)] if kind == "orthographic" else []
    check("camera-%s-%s" % (kind, "lens" if lens else "pinhole"), pix, cs, cm.rays(oracle, rp, cs), cm.differentials(oracle, rp, cs), cm.dxdy_camera(rp), *extra)


def test_camera_hits_of_the_model(pkg, oracle):
    sd, rp = MR.orthographic_scene(pkg)
    orc = oracle.scene(sd)
    h = cm.camera_hits(pkg, oracle, orc, rp, first=1, n=2)
    orc.close()
    assert (h["prim"] != AR.NONE).any()
    check("camera-hits-orthographic", hits(h), h["cs"])


# ---- feature buffers and mattes -----------------------------------------------------------------------------------------------------------------------------------------
def _aov(pkg, oracle, sd, rp):
    with_filter(pkg, rp, "box", 0.5)
    orc = oracle.scene(sd)
    h = AR.camera_hits(pkg, oracle, orc, rp)
    orc.close()
    hit, albedo, normal, smooth = AR.sample_values(pkg, oracle, sd, h)
    return hits(h), hit, albedo, normal, smooth, AR.box_sums(rp, h, hit, np.nan_to_num(albedo), normal)


def test_aov_sample_values_sphere_and_instances(pkg, oracle):
    sd, rp, _ = MR.instance_scene(pkg)
    out = _aov(pkg, oracle, sd, rp)
    A = pkg._abi
    shapes = sd.prim_shape[out[0]["prim"][out[1]]] >> 30
    assert (shapes == A.PT_SHAPE_TRIANGLE).any() and (shapes != A.PT_SHAPE_TRIANGLE).any() and sd.top_refs is not None
    check("aov-instances", *out)


def test_aov_sample_values_smooth_mesh_halton_lens(pkg, oracle):
    sd, rp = AR.normal_scene(pkg, "mesh", AR.LIGHTS[0], sampler="halton", lensradius=0.05)
    out = _aov(pkg, oracle, sd, rp)
    assert out[4].any()
    check("aov-smooth-mesh", *out)


def test_matte_reference_instances(pkg, oracle):
    sd, rp, object_prims = MR.instance_scene(pkg)

    def instance_of(h):
        x = h["o"][:, 0].astype(np.float64) + h["t"].astype(np.float64) * h["d"][:, 0]
        return np.where(np.isin(h["prim"], object_prims), np.where(x < 0, 1, 2), 0).astype(np.uint32)

    h, surface, ids, tables, count = MR.reference(pkg, oracle, "pinned", sd, rp, groups=sd.prim_group, instance_of=instance_of)
    assert set(np.unique(ids[surface, 1])) == {0, 1, 2}
    resolved = {k: MR.resolve(t, 3) for k, t in tables.items()}
    check("matte-instances", hits(h), surface, ids, tables, np.int64(count), resolved, MR.mask(tables["instance"], [1]))
