"""The compiled .pbrt front end (pbrt-rust_amd/frontend/, include/mi355front.h): tokenizer, parameter
lists, graphics-state semantics, PLY / PFM readers -- checked against the independent Python mirror of core/api.rs
(pbrt_rust_amd.host.SceneBuilder) and, through the oracle, end to end."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
from parity import assert_same_render

HERE = os.path.dirname(os.path.abspath(__file__))


def _arr(p, n):
    return np.ctypeslib.as_array(p, (n,)).copy() if p and n else np.zeros(0)


def _write_pfm(path, img):          # img: (h, w, 3), top row first
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1\n" % (w, h)); f.write(np.ascontiguousarray(img[::-1], dtype="<f4").tobytes())


def _write_ply(path, P, N, UV, faces, binary):     # UV=None: no u v properties
    rows = [(*p, *n) for p, n in zip(P, N)] if UV is None else [(*p, *n, *uv) for p, n, uv in zip(P, N, UV)]
    with open(path, "wb") as f:
        hdr = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "element vertex %d" % len(P)]
        hdr += ["property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz"]
        hdr += [] if UV is None else ["property float u", "property float v"]
        hdr += ["element face %d" % len(faces), "property list uint8 int vertex_indices", "end_header"]
        f.write(("\n".join(hdr) + "\n").encode())
        if binary:
            for r in rows: f.write(struct.pack("<%df" % len(r), *r))
            for fc in faces: f.write(struct.pack("<B%di" % len(fc), len(fc), *fc))
        else:
            for r in rows: f.write((" ".join(repr(float(x)) for x in r) + "\n").encode())
            for fc in faces: f.write(("%d %s\n" % (len(fc), " ".join(str(i) for i in fc))).encode())


def test_c1_scene_file_equals_python_builder(pkg):
    fs = pkg.frontend.FrontScene(path=os.path.join(HERE, "scenes", "spheres_c1.pbrt"))
    d, rp = fs.desc(), fs.render_params()
    sd, rp2 = pkg.scenes.spheres_c1(xres=96, yres=96, spp=8).world_end()
    d2 = sd.desc()
    for f in ("n_vertices", "n_triangles", "n_spheres", "n_prims", "n_materials", "n_lights", "max_node_prims", "n_instances", "n_textures"):
        assert getattr(d, f) == getattr(d2, f), f
    assert np.array_equal(_arr(d.P, 3 * d.n_vertices), _arr(d2.P, 3 * d2.n_vertices))
    assert np.array_equal(_arr(d.indices, 3 * d.n_triangles), _arr(d2.indices, 3 * d2.n_triangles))
    for f in ("prim_shape", "prim_material", "prim_light"):
        assert np.array_equal(_arr(getattr(d, f), d.n_prims), _arr(getattr(d2, f), d2.n_prims)), f
    for i in range(d.n_spheres):
        for f in ("object_to_world", "world_to_object"):
            assert np.allclose(list(getattr(d.spheres[i], f)), list(getattr(d2.spheres[i], f)), atol=1e-6)
        for f in ("radius", "z_min", "z_max", "theta_min", "theta_max", "phi_max", "reverse_orientation", "transform_swaps_handedness"):
            assert getattr(d.spheres[i], f) == getattr(d2.spheres[i], f), f
    for i in range(d.n_lights):
        for f in ("type", "two_sided", "prim"): assert getattr(d.lights[i], f) == getattr(d2.lights[i], f)
        assert np.allclose(list(d.lights[i].L), list(d2.lights[i].L)) and np.allclose(list(d.lights[i].dir), list(d2.lights[i].dir))
    for i in range(d.n_materials):
        for f in ("type", "sigma", "eta", "roughness", "u_roughness", "v_roughness", "remap_roughness"): assert getattr(d.materials[i], f) == getattr(d2.materials[i], f), (i, f)
        for f in ("kd", "ks", "kr", "kt", "opacity", "tex"): assert list(getattr(d.materials[i], f)) == list(getattr(d2.materials[i], f)), (i, f)
    for f in ("full_resolution", "cropped_pixel_bounds", "sample_bounds", "pixel_bounds", "filter_table", "filter_radius"):
        assert list(getattr(rp, f)) == list(getattr(rp2, f)), f
    # Matrix4x4::inverse is restated in f32 (Gauss-Jordan, transform.rs:78-145); the Python mirror inverts in f64
    assert np.allclose(list(rp.raster_to_camera), list(rp2.raster_to_camera), rtol=1e-5, atol=1e-5)
    assert np.allclose(list(rp.camera_to_world), list(rp2.camera_to_world), atol=1e-6)
    assert (rp.spp, rp.max_depth, rp.light_strategy, rp.rr_threshold) == (rp2.spp, rp2.max_depth, rp2.light_strategy, rp2.rr_threshold)
    assert fs.output_filename() == "spheres_c1.exr"


FEATURES = r"""
# exercises: comments, Include, named materials, textures, instancing, PLY (binary + ascii, a quad face), PFM images,
# CoordinateSystem / CoordSysTransform, TransformBegin/End, ReverseOrientation, cropwindow, gaussian filter, spot/point/infinite
Scale -1 1 1   # flips handedness like the reference's sss-dragon scene
LookAt 0 2.5 7   0 0.4 0   0 1 0
Camera "perspective" "float fov" [42] "float lensradius" [0.02] "float focaldistance" [7]
Film "image" "integer xresolution" [80] "integer yresolution" [48] "float cropwindow" [0.1 0.95 0 0.9] "float scale" 1.5
Sampler "sobol" "integer pixelsamples" [4]
PixelFilter "gaussian" "float xwidth" [1.5] "float ywidth" [1.5] "float alpha" [1.2]
Integrator "path" "integer maxdepth" [3] "string lightsamplestrategy" "power"
Accelerator "bvh" "integer maxnodeprims" [2]
WorldBegin
AttributeBegin
  Rotate -90 1 0 0
  LightSource "infinite" "rgb L" [0.5 0.5 0.5] "string mapname" ["sky.pfm"] "float scale" 2
AttributeEnd
LightSource "spot" "point from" [1 3 2] "point to" [0 0 0] "rgb I" [40 40 30] "float coneangle" 25 "float conedeltaangle" 8
LightSource "point" "point from" [-2 2 1] "rgb I" [5 5 9]
CoordinateSystem "lightspot"
Texture "img" "color" "imagemap" "string filename" "tex.pfm" "float uscale" [4] "float vscale" [4] "bool trilinear" ["true"]
Texture "chk" "spectrum" "checkerboard" "string mapping" "planar" "vector v1" [1 0 0] "vector v2" [0 0 1] "string aamode" "closedform"
        "texture tex1" "img" "rgb tex2" [0.1 0.1 0.12]
Texture "rough" "float" "imagemap" "string filename" "tex.pfm" "float scale" [0.3]
Texture "holes" "float" "checkerboard" "float uscale" [5] "float vscale" [5] "float tex1" 1 "float tex2" 0
MakeNamedMaterial "floor" "string type" "matte" "texture Kd" "chk"
MakeNamedMaterial "shiny" "string type" "plastic" "rgb Kd" [0.5 0.2 0.2] "texture roughness" "rough" "bool remaproughness" "false"
NamedMaterial "floor"
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-8 -1 -8  -8 -1 8  8 -1 8  8 -1 -8] "float st" [0 0 0 1 1 1 1 0]
Include "objects.pbrtinc"
TransformBegin
  Translate 0 0 -2
  ObjectInstance "card"
  Translate 1.5 0 0.5
  Rotate 40 0 1 0
  ObjectInstance "card"
TransformEnd
AttributeBegin
  NamedMaterial "shiny"
  Translate -1.6 0 0.4
  Shape "plymesh" "string filename" "blob_bin.ply"
AttributeEnd
AttributeBegin
  Material "uber" "rgb Kd" [0.2 0.4 0.7] "rgb Ks" [0.3 0.3 0.3] "float index" [1.3]
  CoordSysTransform "lightspot"
  Translate 1.8 0 1
  ReverseOrientation
  Shape "plymesh" "string filename" "blob_ascii.ply" "float shadowalpha" 1
AttributeEnd
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [6 6 5] "bool twosided" "true" "float scale" 2
  Translate 0 3.5 0
  Shape "sphere" "float radius" 0.4
AttributeEnd
WorldEnd
"""

OBJECTS_INC = r"""
ObjectBegin "card"
  Material "matte" "texture Kd" "img"
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-0.5 0 0  0.5 0 0  0.5 1 0  -0.5 1 0] "float uv" [0 0 1 0 1 1 0 1] "texture alpha" "holes"
ObjectEnd
"""


def _feature_files(pkg, tmp_path):
    _write_pfm(tmp_path / "sky.pfm", pkg.scenes.sky_env(16, 8))
    _write_pfm(tmp_path / "tex.pfm", pkg.scenes.test_image(20, 12))
    P, I, N = pkg.scenes.displaced_sphere(8, with_normals=True)
    P = (P * 0.6).astype(np.float32)
    UV = np.stack([np.arctan2(P[:, 1], P[:, 0]) / (2 * np.pi) + 0.5, P[:, 2] * 0.5 + 0.5], axis=1).astype(np.float32)
    faces = [list(map(int, t)) for t in I]
    _write_ply(tmp_path / "blob_bin.ply", P, N, UV, faces, binary=True)
    _write_ply(tmp_path / "blob_ascii.ply", P, N, UV, faces, binary=False)
    (tmp_path / "objects.pbrtinc").write_text(OBJECTS_INC)
    (tmp_path / "features.pbrt").write_text(FEATURES)
    return P, I, N, UV


def _python_twin(pkg, P, I, N, UV):
    """The same scene through the Python mirror of api.rs."""
    b = pkg.host.SceneBuilder()
    b.scale(-1, 1, 1); b.look_at((0, 2.5, 7), (0, 0.4, 0), (0, 1, 0)); b.camera(fov=42.0, lensradius=0.02, focaldistance=7.0)
    b.film.update(xres=80, yres=48, crop=(0.1, 0.95, 0.0, 0.9), scale=1.5); b.spp = 4
    b.filter.update(kind="gaussian", radius=(1.5, 1.5), alpha=1.2)
    b.integ.update(maxdepth=3, strategy="power"); b.max_node_prims = 2
    b.world_begin()
    b.attribute_begin(); b.rotate(-90, 1, 0, 0); b.light_source("infinite", L=(0.5, 0.5, 0.5), texels=pkg.scenes.sky_env(16, 8), scale=2.0); b.attribute_end()
    b.light_source("spot", from_=(1, 3, 2), to=(0, 0, 0), I=(40, 40, 30), coneangle=25.0, conedeltaangle=8.0)
    b.light_source("point", from_=(-2, 2, 1), I=(5, 5, 9))
    img = pkg.scenes.test_image(20, 12)
    b.texture("img", "color", "imagemap", pixels=img, uscale=4.0, vscale=4.0, trilinear=True)
    b.texture("chk", "spectrum", "checkerboard", mapping="planar", v1=(1, 0, 0), v2=(0, 0, 1), aamode="closedform", tex1="img", tex2=(0.1, 0.1, 0.12))
    b.texture("rough", "float", "imagemap", pixels=img, scale=0.3)
    b.texture("holes", "float", "checkerboard", uscale=5.0, vscale=5.0, tex1=1.0, tex2=0.0)
    b.material("matte", Kd="chk"); floor = b.material_id
    b.material("plastic", Kd=(0.5, 0.2, 0.2), roughness="rough", remaproughness=False); shiny = b.material_id
    b.material_id = floor
    Pq, Iq = pkg.scenes.quad((-8, -1, -8), (-8, -1, 8), (8, -1, 8), (8, -1, -8))
    b.trianglemesh(Pq, Iq, UV=np.array([[0, 0], [0, 1], [1, 1], [1, 0]], dtype=np.float32))
    b.object_begin("card"); b.material("matte", Kd="img")
    Pc, Ic = pkg.scenes.quad((-0.5, 0, 0), (0.5, 0, 0), (0.5, 1, 0), (-0.5, 1, 0))
    b.trianglemesh(Pc, Ic, UV=np.array([[0, 0], [1, 0], [1, 1], [0, 1]], dtype=np.float32), alpha="holes"); b.object_end()
    saved = b.ctm
    b.translate(0, 0, -2); b.object_instance("card"); b.translate(1.5, 0, 0.5); b.rotate(40, 0, 1, 0); b.object_instance("card")
    b.ctm = saved
    b.attribute_begin(); b.material_id = shiny; b.translate(-1.6, 0, 0.4); b.trianglemesh(P, I, N=N, UV=UV); b.attribute_end()
    b.attribute_begin(); b.material("uber", Kd=(0.2, 0.4, 0.7), Ks=(0.3, 0.3, 0.3), eta=1.3); b.ctm = saved; b.translate(1.8, 0, 1)
    b.reverse_orientation = not b.reverse_orientation; b.trianglemesh(P, I, N=N, UV=UV); b.attribute_end()
    b.attribute_begin(); b.area_light_source(L=(12, 12, 10), twosided=True); b.translate(0, 3.5, 0); b.sphere(radius=0.4); b.attribute_end()
    return b.world_end()


def test_feature_scene_matches_python_builder_and_renders(pkg, oracle, tmp_path):
    P, I, N, UV = _feature_files(pkg, tmp_path)
    fs = pkg.frontend.FrontScene(path=str(tmp_path / "features.pbrt"))
    d, rp = fs.desc(), fs.render_params()
    sd, rp2 = _python_twin(pkg, P, I, N, UV)
    d2 = sd.desc()
    for f in ("n_vertices", "n_triangles", "n_spheres", "n_prims", "n_lights", "max_node_prims", "n_objects", "n_instances", "n_top", "n_images", "env_width", "env_height"):
        assert getattr(d, f) == getattr(d2, f), f
    assert np.array_equal(_arr(d.indices, 3 * d.n_triangles), _arr(d2.indices, 3 * d2.n_triangles))
    assert np.array_equal(_arr(d.tri_flags, d.n_triangles), _arr(d2.tri_flags, d2.n_triangles))
    assert np.array_equal(_arr(d.top_refs, d.n_top), _arr(d2.top_refs, d2.n_top))
    assert np.array_equal(_arr(d.prim_shape, d.n_prims), _arr(d2.prim_shape, d2.n_prims)) and np.array_equal(_arr(d.prim_light, d.n_prims), _arr(d2.prim_light, d2.n_prims))
    assert np.allclose(_arr(d.P, 3 * d.n_vertices), _arr(d2.P, 3 * d2.n_vertices), atol=1e-5)
    assert np.allclose(_arr(d.N, 3 * d.n_vertices), _arr(d2.N, 3 * d2.n_vertices), atol=1e-5)
    assert np.array_equal(_arr(d.UV, 2 * d.n_vertices), _arr(d2.UV, 2 * d2.n_vertices))
    assert np.array_equal(_arr(d.tri_alpha, d.n_triangles) >= 0, _arr(d2.tri_alpha, d2.n_triangles) >= 0)
    # the MIPMap pyramid, the environment importance image and the filter table are built by two independent
    # implementations (C++ / numpy) of the same reference code
    for i in range(d.n_images):
        a, b = d.images[i], d2.images[i]
        assert (a.width, a.height, a.n_levels, a.channels) == (b.width, b.height, b.n_levels, b.channels)
        n = sum(max(1, a.width >> l) * max(1, a.height >> l) for l in range(a.n_levels)) * a.channels
        assert np.allclose(_arr(a.texels, n), _arr(b.texels, n), rtol=2e-5, atol=2e-6)
    assert np.allclose(_arr(d.env_importance, 4 * d.env_width * d.env_height), _arr(d2.env_importance, 4 * d2.env_width * d2.env_height), rtol=1e-5)
    assert np.allclose(list(d.env_power_lookup), list(d2.env_power_lookup), rtol=1e-5) and d.env_power_lookup[0] > 0
    assert np.allclose(list(rp.filter_table), list(rp2.filter_table), rtol=1e-5, atol=1e-7)
    for f in ("cropped_pixel_bounds", "sample_bounds", "pixel_bounds", "full_resolution"): assert list(getattr(rp, f)) == list(getattr(rp2, f)), f
    assert (rp.spp, rp.max_depth, rp.light_strategy, rp.lens_radius, rp.focal_distance, rp.scale) == (rp2.spp, rp2.max_depth, rp2.light_strategy, rp2.lens_radius, rp2.focal_distance, rp2.scale)
    for i in range(d.n_lights):
        assert d.lights[i].type == d2.lights[i].type
        assert np.allclose(list(d.lights[i].L), list(d2.lights[i].L), rtol=1e-6) and np.allclose(list(d.lights[i].pos), list(d2.lights[i].pos), atol=1e-5)
    # end to end through the oracle: same image up to the float differences of the two hosts' matrix inverses
    a = oracle.scene(fs); b = oracle.scene(sd)
    ia = a.resolve(a.render(rp, nthreads=4), scale=rp.scale); ib = b.resolve(b.render(rp2, nthreads=4), scale=rp2.scale)
    assert np.isfinite(ia).all() and ia.mean() > 0.05
    diff = np.abs(ia - ib)
    assert (diff.max(axis=2) > 0.05).mean() < 0.02 and diff.mean() < 2e-3


@pytest.mark.parametrize("text,needle", [
    ("WorldBegin\nFrobnicate 1 2 3\n", "line 2: unknown directive Frobnicate"),
    ('Sampler "stratified" "integer xsamples" 4\nWorldBegin WorldEnd', "only \"sobol\" and \"halton\""),
    ('Integrator "bdpt"\n', "only \"path\""),
    ('WorldBegin\nShape "cone"\n', "shape \"cone\""),
    ('WorldBegin\nMaterial "matte" "wavelengths Kd" [5500 1]\n', "unknown parameter type wavelengths"),
    ('WorldBegin\nShape "trianglemesh" "integer indices" [0 1 5] "point P" [0 0 0 1 0 0 0 1 0]\n', "out of-bounds vertex index"),
    ('WorldBegin\nNamedMaterial "nope"\n', "not defined"),
    ('WorldBegin\nAttributeEnd\n', "unmatched AttributeEnd"),
    ('WorldBegin\nMaterial "matte" "texture Kd" "missing"\n', "not declared"),
])
def test_front_end_errors_name_the_problem(pkg, text, needle):
    with pytest.raises(ValueError) as e:
        pkg.frontend.FrontScene(text=text)
    assert needle in str(e.value)


def test_tokenizer_and_parameter_forms(pkg):
    """Numbers (lexer.rs NUMBER: sign, fraction, exponent, leading dot), bare and bracketed single values, `integer`/`int`,
    `color`/`rgb`, `point`/`point3`, comments at line ends, Transform's column-major matrix, excess array values dropped."""
    fs = pkg.frontend.FrontScene(text='''
Film "image" "int xresolution" 32 "integer yresolution" [ 16 ]   # trailing comment
Sampler "sobol" "integer pixelsamples" [2]
WorldBegin
Transform [1 0 0 0  0 1 0 0  0 0 1 0  .5 -1.5e0 +2E0 1]
Material "matte" "color Kd" [.25 0.5 7.5e-1 99]
Shape "trianglemesh" "integer indices" [0 1 2] "point3 P" [0 0 0  1 0 0  0 1 0  ]
ConcatTransform [2 0 0 0  0 2 0 0  0 0 2 0  0 0 0 1]
Shape "sphere" "float radius" .5
WorldEnd''')
    d, rp = fs.desc(), fs.render_params()
    assert list(rp.full_resolution) == [32, 16] and rp.spp == 2
    assert np.allclose(_arr(d.P, 9), [0.5, -1.5, 2.0, 1.5, -1.5, 2.0, 0.5, -0.5, 2.0])
    assert np.allclose(list(d.materials[1].kd), [0.25, 0.5, 0.75])
    o2w = np.array(list(d.spheres[0].object_to_world)).reshape(4, 4)
    assert np.allclose(o2w, [[2, 0, 0, 0.5], [0, 2, 0, -1.5], [0, 0, 2, 2.0], [0, 0, 0, 1]])


@pytest.mark.gpu
def test_front_end_scene_renders_on_gpu_like_the_oracle(pkg, gpu, oracle, tmp_path):
    _feature_files(pkg, tmp_path)
    fs = pkg.frontend.FrontScene(path=str(tmp_path / "features.pbrt"))
    rp = fs.render_params()
    g = pkg.Scene(gpu, fs); orc = oracle.scene(fs)
    film, ref = g.render(rp), orc.render(rp, nthreads=4)
    # gaussian filter: overlapping splats are summed by float atomics in a different order
    assert_same_render(film, ref, g.counters(), orc.counters(), rtol=2e-4, atol=2e-6, weights=2e-4)
    # the command-line renderer produces the same picture as the library path
    out = tmp_path / "out.pfm"
    r = subprocess.run([pkg.frontend.CLI_PATH, str(tmp_path / "features.pbrt"), "--outfile", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    with open(out, "rb") as f:
        assert f.readline() == b"PF\n"; w, h = map(int, f.readline().split()); f.readline()
        img = np.frombuffer(f.read(), dtype="<f4").reshape(h, w, 3)[::-1]
    np.testing.assert_allclose(img, g.resolve(film, scale=rp.scale), rtol=2e-4, atol=2e-5)


# ---- image readers (core/imageio.rs:18-40 read_image: pfm, hdr, png, tga) ------------------------------------------------

def _hdr_bytes(rgbe, rle=True):   # rgbe: (h, w, 4) uint8
    h, w, _ = rgbe.shape
    out = bytearray(b"#?RADIANCE\n# test\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w))
    for y in range(h):
        if not (rle and 8 <= w < 32768):
            out += rgbe[y].tobytes(); continue
        out += bytes([2, 2, w >> 8, w & 255])
        for c in range(4):
            row = rgbe[y, :, c].tolist(); x = 0
            while x < w:
                run = 1
                while x + run < w and run < 127 and row[x + run] == row[x]: run += 1
                if run >= 3: out += bytes([128 + run, row[x]]); x += run
                else:
                    lit = [row[x]]; x += 1
                    while x < w and len(lit) < 128 and not (x + 2 < w and row[x] == row[x + 1] == row[x + 2]): lit.append(row[x]); x += 1
                    out += bytes([len(lit)] + lit)
    return bytes(out)


def _png_bytes(img, ctype, depth=8, palette=None):   # img: (h, w, nch) integer samples
    import struct, zlib
    h, w = img.shape[:2]
    raw = img.astype(">u2" if depth == 16 else np.uint8).reshape(h, -1).view(np.uint8).reshape(h, -1)
    bpp = max(1, raw.shape[1] // w)
    lines = bytearray(); prev = np.zeros(raw.shape[1], np.int32)
    for y in range(h):
        cur = raw[y].astype(np.int32); ft = y % 5
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]); c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]); b = prev
        if ft == 0: pred = 0
        elif ft == 1: pred = a
        elif ft == 2: pred = b
        elif ft == 3: pred = (a + b) // 2
        else:
            pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        lines += bytes([ft]) + ((cur - pred) & 255).astype(np.uint8).tobytes(); prev = cur
    def chunk(t, body): return struct.pack(">I", len(body)) + t + body + struct.pack(">I", zlib.crc32(t + body))
    z = zlib.compress(bytes(lines)); half = len(z) // 2
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0))
    if palette is not None: out += chunk(b"PLTE", palette.astype(np.uint8).tobytes())
    return out + chunk(b"IDAT", z[:half]) + chunk(b"IDAT", z[half:]) + chunk(b"IEND", b"")


def _level0(fs, i=0):
    d = fs.desc(); im = d.images[i]
    return np.ctypeslib.as_array(im.texels, shape=(im.height * im.width * im.channels,)).reshape(im.height, im.width, im.channels).copy()


def _tex_scene(name, extra=""):
    return 'WorldBegin\nTexture "t" "color" "imagemap" "string filename" "%s" "bool gamma" "false" %s\nMaterial "matte" "texture Kd" "t"\nShape "sphere"\nWorldEnd\n' % (name, extra)


@pytest.mark.parametrize("w", [8, 4])
def test_hdr_reader_rle_and_flat(pkg, tmp_path, w):
    """Radiance .hdr (imageio.rs:142-166 -> image crate HdrDecoder, Rgbe8Pixel::to_hdr = c * 2^(e-136), zero when e == 0):
    run-length coded scanlines (width >= 8) and flat ones; the decoded image equals the same floats stored as PFM."""
    rng = np.random.default_rng(w)
    rgbe = rng.integers(0, 256, (4, w, 4)).astype(np.uint8)
    rgbe[0, :, 0] = 77; rgbe[1, 1:7 if w == 8 else 3, 3] = 130; rgbe[2, 0, 3] = 0   # runs in a plane, a zero-exponent pixel
    (tmp_path / "a.hdr").write_bytes(_hdr_bytes(rgbe))
    expect = rgbe[..., :3].astype(np.float32) * np.exp2(rgbe[..., 3:4].astype(np.float32) - 136.0).astype(np.float32)
    expect[rgbe[..., 3] == 0] = 0
    _write_pfm(tmp_path / "a.pfm", expect)
    a = _level0(pkg.frontend.FrontScene(text=_tex_scene("a.hdr"), base_dir=str(tmp_path)))
    b = _level0(pkg.frontend.FrontScene(text=_tex_scene("a.pfm"), base_dir=str(tmp_path)))
    assert a.shape == (4, w, 3) and np.array_equal(a, b)
    assert np.array_equal(a, expect[::-1])   # ImageTexture flips y (imagemap.rs:141-157)


def test_png_and_tga_readers(pkg, tmp_path):
    """PNG / TGA (imageio.rs:338-357): 8-bit RGB = v / 255; grey, grey+alpha, RGBA, palette and 16-bit variants reduce to it.
    All five scanline filters and a split IDAT stream are exercised."""
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (8, 8, 3))
    def load(name): return _level0(pkg.frontend.FrontScene(text=_tex_scene(name), base_dir=str(tmp_path)))
    (tmp_path / "rgb.png").write_bytes(_png_bytes(rgb, 2))
    want = (rgb.astype(np.float32) / np.float32(255.0))[::-1]
    assert np.array_equal(load("rgb.png"), want)
    rgba = np.concatenate([rgb, rng.integers(0, 256, (8, 8, 1))], axis=2)
    (tmp_path / "rgba.png").write_bytes(_png_bytes(rgba, 6)); assert np.array_equal(load("rgba.png"), want)
    grey = rgb[..., :1]
    (tmp_path / "g.png").write_bytes(_png_bytes(grey, 0)); assert np.array_equal(load("g.png"), np.repeat(want[..., :1], 3, axis=2))
    (tmp_path / "g16.png").write_bytes(_png_bytes(grey * 257, 0, depth=16)); assert np.array_equal(load("g16.png"), np.repeat(want[..., :1], 3, axis=2))
    pal = rng.integers(0, 256, (256, 3)); idx = rng.integers(0, 256, (8, 8, 1))
    (tmp_path / "p.png").write_bytes(_png_bytes(idx, 3, palette=pal))
    assert np.array_equal(load("p.png"), (pal[idx[..., 0]].astype(np.float32) / np.float32(255.0))[::-1])
    # inverse gamma is the default for 8-bit formats (imagemap.rs "gamma" default = has an 8-bit extension)
    g = _level0(pkg.frontend.FrontScene(text=_tex_scene("rgb.png").replace('"bool gamma" "false"', ""), base_dir=str(tmp_path)))
    assert np.allclose(g, pkg.textures.inverse_gamma_correct(want), rtol=1e-6)
    # TGA: uncompressed 24-bit, bottom-left origin, BGR
    hdr = bytes([0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 8, 0, 8, 0, 24, 0])
    (tmp_path / "t.tga").write_bytes(hdr + rgb[::-1, :, ::-1].astype(np.uint8).tobytes())
    assert np.array_equal(load("t.tga"), want)
    (tmp_path / "x.exr").write_bytes(b"12345678")
    with pytest.raises(Exception, match="not an OpenEXR"): load("x.exr")
    (tmp_path / "bad.png").write_bytes(b"not a png")
    with pytest.raises(Exception, match="not a PNG"): load("bad.png")


def test_hdr_environment_map(pkg, tmp_path):
    """LightSource "infinite" "string mapname" "*.hdr" (lights/infinite.rs:43-60): same light as the PFM of the decoded floats."""
    rng = np.random.default_rng(9)
    rgbe = np.concatenate([rng.integers(1, 256, (8, 16, 3)), rng.integers(126, 132, (8, 16, 1))], axis=2).astype(np.uint8)
    (tmp_path / "sky.hdr").write_bytes(_hdr_bytes(rgbe))
    _write_pfm(tmp_path / "sky.pfm", rgbe[..., :3].astype(np.float32) * np.exp2(rgbe[..., 3:4].astype(np.float32) - 136.0).astype(np.float32))
    scene = 'WorldBegin\nLightSource "infinite" "string mapname" "%s"\nShape "sphere"\nWorldEnd\n'
    a = pkg.frontend.FrontScene(text=scene % "sky.hdr", base_dir=str(tmp_path)).desc()
    b = pkg.frontend.FrontScene(text=scene % "sky.pfm", base_dir=str(tmp_path)).desc()
    assert (a.env_width, a.env_height) == (16, 8)
    n = 16 * 8 * 3
    assert np.array_equal(np.ctypeslib.as_array(a.env_texels, shape=(n,)), np.ctypeslib.as_array(b.env_texels, shape=(n,)))


def test_non_power_of_two_environment_map_is_resampled(pkg, tmp_path):
    """MIPMap::new resamples a 12x7 map to 16x8 (mipmap.rs:81-140) and InfiniteAreaLight reads everything from that pyramid
    (infinite.rs:60-80): C++ front end == Python mirror for texels, importance image and the power lookup; a constant map stays
    constant (the Lanczos weights are normalised), so its importance image is Y * sin(theta)."""
    rng = np.random.default_rng(21)
    rgbe = np.concatenate([rng.integers(1, 256, (7, 12, 3)), rng.integers(126, 132, (7, 12, 1))], axis=2).astype(np.uint8)
    (tmp_path / "sky.hdr").write_bytes(_hdr_bytes(rgbe))
    tex = rgbe[..., :3].astype(np.float32) * np.exp2(rgbe[..., 3:4].astype(np.float32) - 136.0).astype(np.float32)
    scene = 'WorldBegin\nLightSource "infinite" "rgb L" [0.5 1 2] "string mapname" "sky.hdr"\nShape "sphere"\nWorldEnd\n'
    fs = pkg.frontend.FrontScene(text=scene, base_dir=str(tmp_path)); d = fs.desc()
    b = pkg.host.SceneBuilder(); b.light_source("infinite", L=(0.5, 1, 2), texels=tex)
    assert (d.env_width, d.env_height) == (16, 8) and b.env["texels"].shape == (8, 16, 3)
    got = np.ctypeslib.as_array(d.env_texels, shape=(8, 16, 3))
    assert np.allclose(got, b.env["texels"], rtol=1e-5, atol=1e-7) and got.min() >= 0.0
    imp = np.ctypeslib.as_array(d.env_importance, shape=(16, 32))
    assert np.allclose(imp, b.env["importance"], rtol=1e-5, atol=1e-7)
    assert np.allclose(list(d.env_power_lookup), b.env["power_lookup"], rtol=1e-5)
    # the resampled rows interpolate the original ones: the mean radiance is kept to a few per cent
    assert abs(got.mean() / (tex * np.float32([0.5, 1, 2])).mean() - 1) < 0.1
    c = pkg.host.SceneBuilder(); c.light_source("infinite", texels=np.full((5, 10, 3), 0.75, np.float32))
    assert c.env["texels"].shape == (8, 16, 3) and np.allclose(c.env["texels"], 0.75, rtol=1e-6)
    sin_t = np.sin(np.pi * (np.arange(16) + 0.5) / 16)
    assert np.allclose(c.env["importance"], (0.75 * sin_t)[:, None] * np.ones((1, 32)), rtol=1e-5)


@pytest.mark.parametrize("shape", [(2, 32), (32, 4), (1, 16)])
def test_wide_environment_maps_read_the_importance_image_from_a_coarser_level(pkg, tmp_path, shape):
    """Aspects beyond 2:1 (round 1 refused them): MIPMap::lookup's level = log2(max / min) - 2 is >= 0, so the importance image of
    infinite.rs:62-81 is the bilinear lookup of pyramid level `level` (mipmap.rs:202-223). Front end == Python mirror, and the level
    really is the coarser one: for an 8:1 map the importance rows are those of level 1 (half the width)."""
    h, w = shape
    rng = np.random.default_rng(5)
    tex = rng.uniform(0.1, 3.0, (h, w, 3)).astype(np.float32)
    _write_pfm(tmp_path / "wide.pfm", tex)
    scene = 'WorldBegin\nLightSource "infinite" "string mapname" "wide.pfm"\nShape "sphere"\nWorldEnd\n'
    d = pkg.frontend.FrontScene(text=scene, base_dir=str(tmp_path)).desc()
    b = pkg.host.SceneBuilder(); b.light_source("infinite", texels=tex)
    assert (d.env_width, d.env_height) == (w, h)
    imp = np.ctypeslib.as_array(d.env_importance, shape=(2 * h, 2 * w))
    np.testing.assert_allclose(imp, b.env["importance"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(list(d.env_power_lookup), b.env["power_lookup"], rtol=1e-5)
    level = int(np.log2(max(w, h) / min(w, h))) - 2
    assert level >= 1
    levels, _, _ = pkg.textures.build_mipmap(tex, "repeat")
    coarse = levels[level]
    # a level-`level` texel spans 2^level level-0 texels: along the long axis the importance image changes only every 2^(level+1) samples
    # where the bilinear weights are constant -- check against a direct bilinear evaluation at one interior sample
    H, W = 2 * h, 2 * w
    v, u = H // 2, W // 2
    lh, lw, _ = coarse.shape
    sx = np.float32((u + 0.5) / W) * np.float32(lw) - np.float32(0.5); ty = np.float32((v + 0.5) / H) * np.float32(lh) - np.float32(0.5)
    s0, t0 = int(np.floor(sx)), int(np.floor(ty)); ds, dt = sx - s0, ty - t0
    tx = lambda a, c: coarse[c % lh, a % lw].astype(np.float64)
    rgb = tx(s0, t0) * (1 - ds) * (1 - dt) + tx(s0, t0 + 1) * (1 - ds) * dt + tx(s0 + 1, t0) * ds * (1 - dt) + tx(s0 + 1, t0 + 1) * ds * dt
    want = (0.212671 * rgb[0] + 0.715160 * rgb[1] + 0.072169 * rgb[2]) * np.sin(np.pi * (v + 0.5) / H)
    assert abs(imp[v, u] - want) < 1e-4 * max(1.0, want)


def _exr_zip_half(img):   # (h, w, 3) float -> scan-line EXR, ZIP (16 lines per block), HALF channels B, G, R
    import struct, zlib
    h, w, _ = img.shape
    def attr(name, typ, body): return name + b"\0" + typ + b"\0" + struct.pack("<i", len(body)) + body
    chl = b"".join(c + b"\0" + struct.pack("<iiii", 1, 0, 1, 1) for c in (b"B", b"G", b"R")) + b"\0"
    hdr = struct.pack("<ii", 20000630, 2) + attr(b"channels", b"chlist", chl) + attr(b"compression", b"compression", b"\x03") + \
        attr(b"dataWindow", b"box2i", struct.pack("<iiii", 0, 0, w - 1, h - 1)) + attr(b"displayWindow", b"box2i", struct.pack("<iiii", 0, 0, w - 1, h - 1)) + \
        attr(b"lineOrder", b"lineOrder", b"\0") + attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1)) + \
        attr(b"screenWindowCenter", b"v2f", struct.pack("<ff", 0, 0)) + attr(b"screenWindowWidth", b"float", struct.pack("<f", 1)) + b"\0"
    blocks = []
    for y0 in range(0, h, 16):
        raw = b"".join(img[y, :, c].astype(np.float16).tobytes() for y in range(y0, min(h, y0 + 16)) for c in (2, 1, 0))
        a = np.frombuffer(raw, np.uint8); t = np.concatenate([a[0::2], a[1::2]]).astype(np.int32)
        t[1:] = (t[1:] - t[:-1] + 128 + 256) & 255
        z = zlib.compress(t.astype(np.uint8).tobytes())
        blocks.append(struct.pack("<ii", y0, len(z)) + z)
    off = len(hdr) + 8 * len(blocks); table = b""
    for b in blocks: table += struct.pack("<Q", off); off += len(b)
    return hdr + table + b"".join(blocks)


def test_exr_png_pfm_writers_and_exr_reader(pkg, tmp_path):
    """write_image / read_image (core/imageio.rs:18-60): EXR written as three uncompressed FLOAT channels reads back exactly;
    a ZIP-compressed HALF file (the layout of the reference's scenes/textures/envmap.exr) decodes to the half values; PNG is
    the 8-bit gamma encoding of imageio.rs:359-381."""
    F = pkg.frontend
    rng = np.random.default_rng(11)
    img = (rng.random((21, 13, 3)) * 4).astype(np.float32); img[0, 0] = (0, 1e-8, 65000.0)
    F.write_image(str(tmp_path / "a.exr"), img)
    assert np.array_equal(F.read_image(str(tmp_path / "a.exr")), img)
    F.write_image(str(tmp_path / "a.pfm"), img)
    assert np.array_equal(F.read_image(str(tmp_path / "a.pfm")), img)
    big = (rng.random((37, 19, 3)) * 3).astype(np.float32)
    (tmp_path / "z.exr").write_bytes(_exr_zip_half(big))
    assert np.array_equal(F.read_image(str(tmp_path / "z.exr")), big.astype(np.float16).astype(np.float32))
    lin = rng.random((9, 7, 3)).astype(np.float32); lin[0, 0] = (-1, 2, 0.001)
    F.write_image(str(tmp_path / "a.png"), lin); F.write_image(str(tmp_path / "a.tga"), lin)
    g = np.where(lin <= 0.0031308, 12.92 * lin, 1.055 * np.power(np.maximum(lin, 0), 1 / 2.4) - 0.055)
    want = np.clip(255.0 * g + 0.5, 0, 255).astype(np.uint8).astype(np.float32) / np.float32(255.0)
    assert np.abs(F.read_image(str(tmp_path / "a.png")) - want).max() <= 1.01 / 255   # pow() rounding may move a value across .5
    assert np.array_equal(F.read_image(str(tmp_path / "a.png")), F.read_image(str(tmp_path / "a.tga")))
    with pytest.raises(Exception, match="Unsupported file format"): F.write_image(str(tmp_path / "a.jpg"), lin)
    assert F.FrontScene(text='WorldBegin\nShape "sphere"\nWorldEnd\n').output_filename() == "pbrt.exr"   # film.rs default


def test_mix_and_translucent_materials_from_a_scene_file(pkg):
    """api.rs:615-640 + mix.rs / translucent.rs parameter names; an undefined named material falls back to a matte."""
    A = pkg._abi
    fs = pkg.frontend.FrontScene(text='''WorldBegin
Texture "bmp" "float" "checkerboard"
MakeNamedMaterial "a" "string type" "plastic" "rgb Kd" [.1 .2 .3] "texture bumpmap" "bmp"
MakeNamedMaterial "b" "string type" "translucent" "rgb reflect" [.2 .2 .2] "rgb transmit" [.7 .6 .5] "float roughness" .3
Material "mix" "string namedmaterial1" "a" "string namedmaterial2" "b" "rgb amount" [.25 .5 .75]
Shape "sphere"
Material "mix" "string namedmaterial1" "nope" "string namedmaterial2" "a" "rgb Kd" [.9 .8 .7]
Shape "sphere"
WorldEnd
''')
    d = fs.desc()
    mats = [d.materials[i] for i in range(d.n_materials)]
    mixes = [m for m in mats if m.type == A.PT_MAT_MIX]
    assert len(mixes) == 2
    m = mixes[0]
    assert mats[m.mix[0]].type == A.PT_MAT_PLASTIC and mats[m.mix[1]].type == A.PT_MAT_TRANSLUCENT
    assert list(m.kd) == pytest.approx([.25, .5, .75]) and m.tex[A.PT_MP_BUMP] == mats[m.mix[0]].tex[A.PT_MP_BUMP] >= 0
    t = mats[m.mix[1]]
    assert list(t.kr) == pytest.approx([.2, .2, .2]) and list(t.kt) == pytest.approx([.7, .6, .5]) and t.roughness == pytest.approx(.3) and list(t.kd) == pytest.approx([.25] * 3)
    fb = mats[mixes[1].mix[0]]
    assert fb.type == A.PT_MAT_MATTE and list(fb.kd) == pytest.approx([.9, .8, .7]) and list(mixes[1].kd) == pytest.approx([.5] * 3)


def test_subsurface_sigma_textures_from_a_scene_file(pkg, oracle):
    """subsurface.rs:127-128: `sigma_a` / `sigma_s` are spectrum textures (get_spectrumtexture), evaluated at every hit; a scene file that
    names textures for them flattens like the Python mirror's and renders the same image (oracle)."""
    A = pkg._abi
    fs = pkg.frontend.FrontScene(text='''LookAt 0 1.6 6  0 .2 0  0 1 0
Camera "perspective" "float fov" 38
Sampler "sobol" "integer pixelsamples" 4
Integrator "path" "integer maxdepth" 5
Film "image" "integer xresolution" 48 "integer yresolution" 32
WorldBegin
LightSource "infinite" "rgb L" [.25 .3 .35]
Texture "siga" "spectrum" "checkerboard" "integer dimension" 3 "rgb tex1" [.0011 .0024 .014] "rgb tex2" [.02 .004 .002]
Texture "sigs" "spectrum" "checkerboard" "float uscale" 4 "float vscale" 4 "rgb tex1" [2.55 3.21 3.77] "rgb tex2" [1 1.4 2.2]
Material "subsurface" "texture sigma_a" "siga" "texture sigma_s" "sigs" "float scale" 8 "float eta" 1.33
Shape "sphere" "float radius" 1
WorldEnd
''')
    d = fs.desc()
    m = [d.materials[i] for i in range(d.n_materials) if d.materials[i].type == A.PT_MAT_SUBSURFACE][0]
    assert m.tex[A.PT_MP_SIGMA_A] >= 0 and m.tex[A.PT_MP_SIGMA_S] >= 0 and m.tex[A.PT_MP_SIGMA_A] != m.tex[A.PT_MP_SIGMA_S]
    assert list(m.sigma_a) == pytest.approx([.0011, .0024, .014]) and m.scale == pytest.approx(8.0)   # the constant fields keep create_subsurface_material's defaults
    b = pkg.host.SceneBuilder()
    b.film.update(xres=48, yres=32); b.spp = 4; b.integ.update(maxdepth=5)
    b.look_at((0, 1.6, 6), (0, .2, 0), (0, 1, 0)); b.camera(fov=38.0)
    b.world_begin(); b.light_source("infinite", L=(.25, .3, .35))
    b.texture("siga", "color", "checkerboard", dimension=3, tex1=(.0011, .0024, .014), tex2=(.02, .004, .002))
    b.texture("sigs", "color", "checkerboard", uscale=4.0, vscale=4.0, tex1=(2.55, 3.21, 3.77), tex2=(1.0, 1.4, 2.2))
    b.material("subsurface", sigma_a="siga", sigma_s="sigs", scale=8.0, eta=1.33)
    b.sphere(radius=1.0)
    sd, rp = b.world_end()
    a = oracle.scene(sd).render(rp, nthreads=4); c = oracle.scene(fs).render(fs.render_params(), nthreads=4)
    # the two hosts' float arithmetic differs by ulps (matrix inverses): a few samples land on the other side of a checker edge
    assert (np.abs(a - c) > 2e-5 * np.maximum(np.abs(a), 1e-2)).mean() < 0.01
    with pytest.raises(Exception): pkg.frontend.FrontScene(text='WorldBegin\nMaterial "kdsubsurface" "texture Kd" "nope"\nWorldEnd\n')   # an undeclared texture is an error


def test_kdsubsurface_textures_from_a_scene_file_and_constant_textures_equal_constants(pkg, oracle):
    """kdsubsurface.rs:106-126: `Kd` and `mfp` are spectrum textures. With textures the library converts at every hit
    (PtMaterial.kd_subsurface); with constants the host converts once. Two checks that pin the per-hit path: constant TEXTURES must
    render exactly what constant PARAMETERS do (the oracle's f32 Newton inversion against the Python mirror's host-side one), and a
    scene file with a real texture flattens like the Python mirror's."""
    A = pkg._abi
    def scene(kd, mfp, declare):
        b = pkg.host.SceneBuilder()
        b.film.update(xres=40, yres=28); b.spp = 4; b.integ.update(maxdepth=5)
        b.look_at((0, 1.6, 6), (0, .2, 0), (0, 1, 0)); b.camera(fov=38.0)
        b.world_begin(); b.light_source("infinite", L=(.4, .45, .5))
        declare(b)
        b.material("kdsubsurface", Kd=kd, mfp=mfp, eta=1.4, scale=1.5)
        b.sphere(radius=1.0)
        return b.world_end()
    plain = scene((0.7, 0.35, 0.2), (0.25, 0.15, 0.08), lambda b: None)
    def const_tex(b):
        b.texture("kdc", "color", "constant", value=(0.7, 0.35, 0.2)); b.texture("mfpc", "color", "constant", value=(0.25, 0.15, 0.08))
    tex = scene("kdc", "mfpc", const_tex)
    mp = [plain[0].desc().materials[i] for i in range(plain[0].desc().n_materials)][-1]; mt = [tex[0].desc().materials[i] for i in range(tex[0].desc().n_materials)][-1]
    assert mp.kd_subsurface == 0 and mt.kd_subsurface == 1 and mt.tex[A.PT_MP_KD] >= 0 and mt.tex[A.PT_MP_MFP] >= 0 and mt.scale == pytest.approx(1.5)
    sa, sc = oracle.scene(plain[0]), oracle.scene(tex[0])
    a, c = sa.render(plain[1], nthreads=4), sc.render(tex[1], nthreads=4)
    assert_same_render(a, c, sa.counters(), sc.counters(), rtol=1e-5, atol=1e-6, weights=1e-5)
    fs = pkg.frontend.FrontScene(text='''WorldBegin
Texture "kdt" "spectrum" "checkerboard" "rgb tex1" [.7 .35 .2] "rgb tex2" [.2 .5 .8]
Material "kdsubsurface" "texture Kd" "kdt" "rgb mfp" [.25 .15 .08] "float scale" 1.5 "float eta" 1.4
Shape "sphere"
WorldEnd
''')
    d = fs.desc()
    m = [d.materials[i] for i in range(d.n_materials) if d.materials[i].type == A.PT_MAT_SUBSURFACE][0]
    assert m.kd_subsurface == 1 and m.tex[A.PT_MP_KD] >= 0 and m.tex[A.PT_MP_MFP] < 0 and list(m.mfp) == pytest.approx([.25, .15, .08]) and m.scale == pytest.approx(1.5)


def test_disney_material_from_a_scene_file(pkg):
    """disney.rs:842-887 parameter names and defaults; the BSSRDF branch (scatterdistance) and textured scalar parameters other
    than eta / roughness are refused by name."""
    A = pkg._abi
    head = 'WorldBegin\nTexture "c" "color" "checkerboard"\n'
    fs = pkg.frontend.FrontScene(text=head + 'Material "disney" "texture color" "c" "float metallic" .25 "float sheen" .5 "bool thin" "true" "float difftrans" .8\nShape "sphere"\nWorldEnd\n')
    d = fs.desc()
    m = [d.materials[i] for i in range(d.n_materials) if d.materials[i].type == A.PT_MAT_DISNEY][0]
    assert m.tex[A.PT_MP_KD] >= 0 and m.disney_thin == 1 and m.eta == pytest.approx(1.5) and m.roughness == pytest.approx(0.5)
    want = {A.PT_DS_METALLIC: .25, A.PT_DS_SPECULARTINT: 0, A.PT_DS_ANISOTROPIC: 0, A.PT_DS_SHEEN: .5, A.PT_DS_SHEENTINT: .5, A.PT_DS_CLEARCOAT: 0,
            A.PT_DS_CLEARCOATGLOSS: 1, A.PT_DS_SPECTRANS: 0, A.PT_DS_FLATNESS: 0, A.PT_DS_DIFFTRANS: .8}
    for k, v in want.items(): assert m.disney[k] == pytest.approx(v), k
    sd = pkg.frontend.FrontScene(text=head + 'Material "disney" "rgb scatterdistance" [.1 .2 .3]\nShape "sphere"\nWorldEnd\n').desc()
    assert [list(sd.materials[i].disney_scatter) for i in range(sd.n_materials) if sd.materials[i].type == A.PT_MAT_DISNEY][0] == pytest.approx([.1, .2, .3])
    with pytest.raises(Exception, match="scatterdistance"):
        pkg.frontend.FrontScene(text=head + 'Material "disney" "texture color" "c" "rgb scatterdistance" [.1 .1 .1]\nShape "sphere"\nWorldEnd\n')
    with pytest.raises(Exception, match="textured \"sheen\""):
        pkg.frontend.FrontScene(text=head + 'Texture "f" "float" "checkerboard"\nMaterial "disney" "texture sheen" "f"\nShape "sphere"\nWorldEnd\n')


# ---- spectral parameter types: "xyz", "blackbody", "spectrum" (inline pairs and .spd files) -> RGB ----

_SPECTRAL_HEAD = """LookAt 0 0 5 0 0 0 0 1 0
Camera "perspective" "float fov" [30]
Film "image" "integer xresolution" [16] "integer yresolution" [16]
Sampler "sobol" "integer pixelsamples" [1]
Integrator "path"
WorldBegin
"""


def test_spectral_parameter_types_become_rgb_like_the_reference(pkg, tmp_path):
    """pbrtparser.rs:325-377 + paramset.rs:145-246 + spectrum.rs:36-70,129-154: the front end against the numpy mirror (host.py)."""
    H = pkg.host
    (tmp_path / "green.spd").write_text("# wavelength value\n400 0.1\n500 0.2 550 0.9\n600 0.3\n700 0.05\n")
    (tmp_path / "broken.spd").write_text("400 0.1\n500 oops\n")
    txt = _SPECTRAL_HEAD + """
LightSource "point" "blackbody I" [5500 125]
LightSource "point" "blackbody I" [2800 3 6500 1]
LightSource "point" "xyz I" [0.3 0.4 0.2]
LightSource "point" "spectrum I" [400 0.2 500 0.5 600 0.9 700 0.3]
LightSource "point" "spectrum I" [700 0.3 500 0.5 600 0.9 400 0.2]
LightSource "point" "spectrum I" "green.spd"
LightSource "point" "spectrum I" "broken.spd"
LightSource "point" "rgb I" [1 2 3] "blackbody I" [4000 2]
Material "matte" "spectrum Kd" [300 0.5 900 0.5] "float sigma" 0
Shape "sphere"
WorldEnd
"""
    d = pkg.frontend.FrontScene(text=txt, base_dir=str(tmp_path)).desc()
    want = [H.rgb_from_blackbody(5500, 125), H.rgb_from_blackbody(2800, 3),        # find_one_spectrum: the first of several values
            H.xyz_to_rgb((0.3, 0.4, 0.2)), H.rgb_from_sampled([400, 500, 600, 700], [0.2, 0.5, 0.9, 0.3]),
            H.rgb_from_sampled([700, 500, 600, 400], [0.3, 0.5, 0.9, 0.2]),         # unsorted: sorted wavelengths, UNSORTED values (spectrum.rs:131-136)
            H.rgb_from_spd_text((tmp_path / "green.spd").read_text()), np.zeros(3, np.float32),
            H.rgb_from_blackbody(4000, 2)]                                           # same name declared twice: the later one replaces the earlier
    assert d.n_lights == len(want)
    for i, w in enumerate(want):
        np.testing.assert_allclose(list(d.lights[i].L), w, rtol=2e-5, atol=1e-6, err_msg=str(i))
    mat = d.materials[d.n_materials - 1]   # (index 0 is the graphics state's default matte)
    np.testing.assert_allclose(list(mat.kd), H.rgb_from_sampled([300, 900], [0.5, 0.5]), rtol=2e-5)
    # sanity of the conversion itself: a 6500 K blackbody is close to white in linear sRGB; a constant spectrum is the equal-energy
    # white E, i.e. XYZ = (v, v, v) -> RGB = v * (row sums of the XYZ -> RGB matrix), slightly reddish
    bb = H.rgb_from_blackbody(6500, 1); assert 0.8 < bb[0] / bb[1] < 1.25 and 0.8 < bb[2] / bb[1] < 1.25
    np.testing.assert_allclose(list(mat.kd), 0.5 * np.array([3.240479 - 1.537150 - 0.498535, -0.969256 + 1.875991 + 0.041556, 0.055648 - 0.204043 + 1.057311]), rtol=5e-3)   # (the X and Z integrals of the tables differ from the Y integral by ~0.2 %)


# A scene file laid out like the pbrt-v3 scenes exporters write: comments and commented-out alternatives, indented parameter lines, a bare scalar
# ("float scale" 1.5), bracketed values padded with spaces, an Integrator this renderer does not have (the test swaps that line), a spot light given
# as a blackbody, and two binary PLY meshes beside it (written by the test: _vase_mesh and a two-triangle slab).
_EXPORTED_SCENE = """\

#LookAt 3 5 -6   0 1 0   0 1 0
LookAt 4 6 -7   0.5 1.5 0   0 1 0

Camera "perspective" "float fov" [35]

Film "image"
    "integer xresolution" [640] "integer yresolution" [900]
    "float scale" 1.5
    "string filename" "vase.exr"

Integrator "sppm" "integer numiterations" [64] "float radius" .05
#Integrator "bdpt" "integer maxdepth" 8

WorldBegin

LightSource "spot" "point from" [1 6 7]
  "point to" [0 1.5 0] "blackbody I" [4800 60]

AttributeBegin
LightSource "infinite" "color L" [.08 .08 .1]
AttributeEnd

AttributeBegin
    Material "glass"
            "float index" [ 1.4500000000 ]
    Shape "plymesh" "string filename" "geometry/vase.ply"
AttributeEnd

AttributeBegin
    Material "uber"
            "float roughness" [ 0.0250000000 ]
            "float index" [ 1 ]
            "rgb Kd" [ 0.5500000000 0.5000000000 0.4500000000 ]
            "rgb Ks" [ 0.1000000000 0.1000000000 0.1000000000 ]
            "rgb Kt" [ 0 0 0 ]
            "rgb opacity" [ 1 1 1 ]
    Shape "plymesh" "string filename" "geometry/slab.ply"
AttributeEnd

WorldEnd
"""


def _vase_mesh(nu=210, nv=211, h=3.0):
    """A surface of revolution, radius 0.6 + 0.25 sin(2.5 pi t) at height h t, with its analytic normals: nu x nv vertices, 2 (nu - 1)(nv - 1) = 87 780 triangles."""
    t, phi = np.linspace(0.0, 1.0, nv)[:, None], np.linspace(0.0, 2.0 * np.pi, nu)[None, :]
    r, dr = 0.6 + 0.25 * np.sin(2.5 * np.pi * t), 0.625 * np.pi * np.cos(2.5 * np.pi * t)
    P = np.stack(np.broadcast_arrays(r * np.cos(phi), h * t, r * np.sin(phi)), -1).reshape(-1, 3)
    N = np.stack(np.broadcast_arrays(h * np.cos(phi), -dr, h * np.sin(phi)), -1).reshape(-1, 3)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    i = (np.arange(nv - 1)[:, None] * nu + np.arange(nu - 1)[None, :]).reshape(-1, 1)
    tris = np.concatenate([np.hstack([i, i + nu, i + 1]), np.hstack([i + 1, i + nu, i + nu + 1])])
    return P.astype(np.float32), N.astype(np.float32), tris


def _read_ply_numpy(path):
    """Minimal PLY reader for the mirror side of the test below (ascii / binary_little_endian, float vertices, list faces)."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode().split("\n")
    fmt = [l.split()[1] for l in head if l.startswith("format")][0]
    elems = []; cur = None
    for l in head:
        t = l.split()
        if not t: continue
        if t[0] == "element": cur = [t[1], int(t[2]), []]; elems.append(cur)
        elif t[0] == "property": cur[2].append(t[1:])
    body = raw[end:]
    verts = None; faces = []
    tmap = {"float": "f4", "float32": "f4", "double": "f8", "uchar": "u1", "uint8": "u1", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "short": "i2", "ushort": "u2", "char": "i1"}
    if fmt == "ascii":
        toks = body.split(); k = 0
        for name, n, props in elems:
            if name == "vertex":
                verts = {p[-1]: np.zeros(n, np.float32) for p in props}
                for i in range(n):
                    for p in props: verts[p[-1]][i] = float(toks[k]); k += 1
            elif name == "face":
                for i in range(n):
                    c = int(toks[k]); k += 1
                    faces.append([int(x) for x in toks[k:k + c]]); k += c
    else:
        off = 0
        for name, n, props in elems:
            if name == "vertex":
                dt = np.dtype([(p[-1], "<" + tmap[p[0]]) for p in props])
                a = np.frombuffer(body, dt, n, off); off += n * dt.itemsize
                verts = {k2: a[k2].astype(np.float32) for k2 in a.dtype.names}
            elif name == "face":
                p = props[0]; ct, it = np.dtype("<" + tmap[p[1]]), np.dtype("<" + tmap[p[2]])
                for i in range(n):
                    c = int(np.frombuffer(body, ct, 1, off)[0]); off += ct.itemsize
                    faces.append(np.frombuffer(body, it, c, off).tolist()); off += c * it.itemsize
    tris = []
    for f in faces:
        if len(f) == 3: tris.append(f)
        elif len(f) == 4: tris += [[f[0], f[1], f[3]], [f[1], f[2], f[3]]]   # shapes/plymesh.rs: a quad becomes (0,1,3) and (1,2,3)
    P = np.stack([verts["x"], verts["y"], verts["z"]], axis=1)
    N = np.stack([verts["nx"], verts["ny"], verts["nz"]], axis=1) if "nx" in verts else None
    UV = np.stack([verts[a] for a in (("u", "v") if "u" in verts else ("s", "t"))], axis=1) if ("u" in verts or "s" in verts) else None
    return P, np.array(tris, np.uint32), N, UV


def test_exported_scene_with_ply_meshes_loads_like_the_mirror(pkg, oracle, tmp_path):
    """_EXPORTED_SCENE (its spot light is given as `"blackbody I" [4800 60]`) and its two binary PLY meshes read by libmi355front.so --
    only its Integrator line is swapped for "path" (the file names sppm) and a sampler line added, in memory -- and assembled independently
    through the Python mirror of api.rs with a numpy PLY reader: the flattened arrays must agree, and the oracle renders both to the same image."""
    (tmp_path / "geometry").mkdir()
    P, N, I = _vase_mesh()
    _write_ply(tmp_path / "geometry" / "vase.ply", P.tolist(), N.tolist(), None, I.tolist(), binary=True)
    _write_ply(tmp_path / "geometry" / "slab.ply", [(-4.0, 0.0, -4.0), (4.0, 0.0, -4.0), (4.0, 0.0, 4.0), (-4.0, 0.0, 4.0)], [(0.0, 1.0, 0.0)] * 4, None,
               [(0, 1, 2), (0, 2, 3)], binary=True)
    lines = []
    for l in _EXPORTED_SCENE.split("\n"):
        if l.startswith("Integrator"): lines.append('Integrator "path" "integer maxdepth" [5]\nSampler "sobol" "integer pixelsamples" [1]'); continue
        if l.startswith('    "integer xresolution"'): l = '    "integer xresolution" [70] "integer yresolution" [100]'
        lines.append(l)
    fs = pkg.frontend.FrontScene(text="\n".join(lines), base_dir=str(tmp_path))
    d, rp = fs.desc(), fs.render_params()
    H = pkg.host
    b = H.SceneBuilder()
    b.film.update(xres=70, yres=100, scale=1.5); b.spp = 1
    b.integ.update(maxdepth=5)
    b.look_at((4.0, 6.0, -7.0), (0.5, 1.5, 0.0), (0.0, 1.0, 0.0)); b.camera(fov=35.0)
    b.world_begin()
    b.light_source("spot", from_=(1.0, 6.0, 7.0), to=(0.0, 1.5, 0.0), I=tuple(float(x) for x in H.rgb_from_blackbody(4800, 60)))
    b.attribute_begin(); b.light_source("infinite", L=(0.08, 0.08, 0.1)); b.attribute_end()
    for fn, (kind, kw) in (("geometry/vase.ply", ("glass", dict(eta=1.45))),
                           ("geometry/slab.ply", ("uber", dict(roughness=0.025, eta=1.0, Kd=(0.55, 0.5, 0.45), Ks=(0.1,) * 3, Kt=(0.0, 0.0, 0.0), opacity=(1.0, 1.0, 1.0))))):
        b.attribute_begin(); b.material(kind, **kw)
        P, I, N, UV = _read_ply_numpy(str(tmp_path / fn))
        b.trianglemesh(P, I, N=N, UV=UV); b.attribute_end()
    sd, rp2 = b.world_end()
    d2 = sd.desc()
    assert d.n_triangles == d2.n_triangles > 80000 and d.n_vertices == d2.n_vertices and d.n_lights == d2.n_lights == 2 and d.n_materials == d2.n_materials
    np.testing.assert_array_equal(_arr(d.indices, 3 * d.n_triangles), _arr(d2.indices, 3 * d2.n_triangles))
    np.testing.assert_allclose(_arr(d.P, 3 * d.n_vertices), _arr(d2.P, 3 * d2.n_vertices), rtol=1e-6, atol=1e-6)
    for f in ("prim_shape", "prim_material", "prim_light"):
        np.testing.assert_array_equal(_arr(getattr(d, f), d.n_prims), _arr(getattr(d2, f), d2.n_prims))
    for i in range(d.n_lights):
        assert d.lights[i].type == d2.lights[i].type
        np.testing.assert_allclose(list(d.lights[i].L), list(d2.lights[i].L), rtol=2e-5)
        np.testing.assert_allclose(list(d.lights[i].pos), list(d2.lights[i].pos), atol=1e-5)
        assert abs(d.lights[i].cos_total_width - d2.lights[i].cos_total_width) < 1e-6
    for i in range(d.n_materials):
        for f in ("type", "eta", "roughness"): assert getattr(d.materials[i], f) == pytest.approx(getattr(d2.materials[i], f), rel=1e-6), (i, f)
        for f in ("kd", "ks", "kt", "opacity"): np.testing.assert_allclose(list(getattr(d.materials[i], f)), list(getattr(d2.materials[i], f)), rtol=1e-6)
    for f in ("full_resolution", "cropped_pixel_bounds", "sample_bounds"): assert list(getattr(rp, f)) == list(getattr(rp2, f)), f
    assert rp.scale == rp2.scale == 1.5
    a = oracle.scene(fs); c = oracle.scene(sd)
    fa, fc = a.render(rp, nthreads=8), c.render(rp2, nthreads=8)
    assert np.isfinite(fa).all() and fa[..., :3].max() > 0
    np.testing.assert_allclose(a.resolve(fa), c.resolve(fc), rtol=1e-3, atol=1e-4)


# ---- OpenEXR layouts beyond scan-line ZIP (VERDICT r2 missing #6: tiled, multi-part, RLE) ----

def _exr_bytes(parts, multipart=False):
    """An independent little OpenEXR writer for the reader's test: parts = [dict(w, h, chans=[(name, type)], compression, tile=None|(tw, th), mipmap=bool,
    pixels={name: (h, w) array})]; type 1 HALF / 2 FLOAT / 0 UINT. Layout per the OpenEXR file-layout document."""
    import struct, zlib
    def attr(name, typ, data): return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(data)) + data
    def pack_block(raw, compression):
        if compression == 0: return raw
        n = len(raw); half = (n + 1) // 2
        t = bytearray(n); t[:half] = raw[0::2]; t[half:] = raw[1::2]            # even / odd split
        p = bytearray(n); p[0] = t[0]
        for i in range(1, n): p[i] = (t[i] - t[i - 1] + 128) & 255              # byte predictor
        if compression in (2, 3): out = zlib.compress(bytes(p))
        else:                                                                   # RLE
            out = bytearray(); i = 0
            while i < n:
                j = i
                while j + 1 < n and p[j + 1] == p[i] and j - i < 126: j += 1
                if j - i >= 2: out += struct.pack("b", j - i) + bytes([p[i]]); i = j + 1
                else:
                    k = i
                    while k < n and k - i < 127 and not (k + 2 < n and p[k] == p[k + 1] == p[k + 2]): k += 1
                    out += struct.pack("b", -(k - i)) + bytes(p[i:k]); i = k
            out = bytes(out)
        return out if len(out) < n else raw
    def block_bytes(pt, x0, y0, bw, bh):
        rows = []
        for y in range(y0, y0 + bh):
            for name, typ in sorted(pt["chans"]):
                a = pt["pixels"][name][y, x0:x0 + bw]
                rows.append(a.astype(np.float16).tobytes() if typ == 1 else a.astype(np.float32).tobytes() if typ == 2 else a.astype(np.uint32).tobytes())
        return b"".join(rows)
    version = 2 | (0x1000 if multipart else (0x200 if parts[0].get("tile") else 0))
    out = struct.pack("<ii", 20000630, version)
    chunks = []
    for k, pt in enumerate(parts):
        w, h = pt["w"], pt["h"]
        ch = b"".join(n.encode() + b"\0" + struct.pack("<iiii", t, 0, 1, 1) for n, t in sorted(pt["chans"])) + b"\0"
        hdr = attr("channels", "chlist", ch) + attr("compression", "compression", bytes([pt["compression"]])) + attr("dataWindow", "box2i", struct.pack("<iiii", 0, 0, w - 1, h - 1))
        hdr += attr("displayWindow", "box2i", struct.pack("<iiii", 0, 0, w - 1, h - 1)) + attr("lineOrder", "lineOrder", b"\0") + attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
        hdr += attr("screenWindowCenter", "v2f", struct.pack("<ff", 0, 0)) + attr("screenWindowWidth", "float", struct.pack("<f", 1.0))
        mine = []
        if pt.get("tile"):
            tw, th = pt["tile"]
            hdr += attr("tiles", "tiledesc", struct.pack("<IIB", tw, th, 1 if pt.get("mipmap") else 0))
            lw, lh, lvl = w, h, 0
            while True:
                for ty in range(-(-lh // th)):
                    for tx in range(-(-lw // tw)):
                        x0, y0 = tx * tw, ty * th; bw, bh = min(tw, lw - x0), min(th, lh - y0)
                        raw = block_bytes(pt, x0, y0, bw, bh) if lvl == 0 else bytes(bw * bh * sum(2 if t == 1 else 4 for _, t in pt["chans"]))
                        data = pack_block(raw, pt["compression"])
                        mine.append(struct.pack("<iiii", tx, ty, lvl, lvl) + struct.pack("<i", len(data)) + data)
                if not pt.get("mipmap") or (lw == 1 and lh == 1): break
                lw, lh, lvl = max(1, lw // 2), max(1, lh // 2), lvl + 1
        else:
            lpb = 16 if pt["compression"] == 3 else 1
            for y0 in range(0, h, lpb):
                data = pack_block(block_bytes(pt, 0, y0, w, min(lpb, h - y0)), pt["compression"])
                mine.append(struct.pack("<ii", y0, len(data)) + data)
        if multipart:
            hdr += attr("name", "string", ("part%d" % k).encode()) + attr("type", "string", b"tiledimage" if pt.get("tile") else b"scanlineimage") + attr("chunkCount", "int", struct.pack("<i", len(mine)))
            mine = [struct.pack("<i", k) + c for c in mine]
        out += hdr + b"\0"
        chunks.append(mine)
    if multipart: out += b"\0"
    pos = len(out) + 8 * sum(len(m) for m in chunks)
    tables = b""; body = b""
    for mine in chunks:
        for c in mine: tables += struct.pack("<Q", pos); pos += len(c); body += c
    return out + tables + body


@pytest.mark.parametrize("layout", ["tiled_zip", "tiled_mipmap_zips", "scanline_rle", "multipart", "tiled_none_uint"])
def test_exr_tiled_multipart_and_rle_files_are_read(pkg, tmp_path, layout):
    """imageio.rs:68-97 reads whatever flat image the `exr` crate reads: tiled files (level 0), multi-part files (first flat part) and RLE blocks
    next to the scan-line ZIP form of the reference's own envmap.exr. Files written by an independent writer in this test."""
    F = pkg.frontend.lib()
    rng = np.random.default_rng(4)
    w, h = 19, 13
    px = {c: rng.uniform(0.0, 4.0, (h, w)).astype(np.float16).astype(np.float32) for c in "RGB"}     # (exact in half and float)
    px["A"] = np.ones((h, w), np.float32)
    base = dict(w=w, h=h, pixels=px)
    if layout == "tiled_zip": parts, mp = [dict(base, chans=[("R", 1), ("G", 1), ("B", 1), ("A", 1)], compression=3, tile=(8, 8))], False
    elif layout == "tiled_mipmap_zips": parts, mp = [dict(base, chans=[("R", 2), ("G", 1), ("B", 2)], compression=2, tile=(5, 4), mipmap=True)], False
    elif layout == "scanline_rle":
        px2 = dict(px); px2["G"] = np.full((h, w), 0.5, np.float32)             # long runs for the RLE coder
        parts, mp = [dict(base, pixels=px2, chans=[("R", 1), ("G", 2), ("B", 1)], compression=1)], False; px = px2
    elif layout == "multipart":
        other = {c: np.zeros((7, 9), np.float32) for c in "RGB"}
        parts, mp = [dict(base, chans=[("R", 1), ("G", 1), ("B", 1)], compression=1), dict(w=9, h=7, pixels=other, chans=[("R", 2), ("G", 2), ("B", 2)], compression=3, tile=(4, 4))], True
    else:
        pu = {c: rng.integers(0, 1000, (h, w)).astype(np.float32) for c in "RGB"}
        parts, mp = [dict(base, pixels=pu, chans=[("R", 0), ("G", 0), ("B", 0)], compression=0, tile=(16, 16))], False; px = pu
    path = tmp_path / (layout + ".exr")
    path.write_bytes(_exr_bytes(parts, multipart=mp))
    rw, rh = C.c_int(), C.c_int()
    back = np.zeros((h, w, 3), np.float32)
    assert F.ptf_read_image(str(path).encode(), C.byref(rw), C.byref(rh), back.ctypes.data_as(pkg._abi.fp), back.size) == 0, F.ptf_last_error()
    assert (rw.value, rh.value) == (w, h)
    for k, c in enumerate("RGB"): assert np.array_equal(back[..., k], px[c]), (layout, c)


def test_exr_codecs_that_are_not_read_are_named(pkg, tmp_path):
    F = pkg.frontend.lib()
    px = {c: np.zeros((4, 4), np.float32) for c in "RGB"}
    b = bytearray(_exr_bytes([dict(w=4, h=4, pixels=px, chans=[("R", 1), ("G", 1), ("B", 1)], compression=0)]))
    i = bytes(b).index(b"compression\0compression\0") + len(b"compression\0compression\0") + 4
    b[i] = 4                                                                   # PIZ
    path = tmp_path / "piz.exr"; path.write_bytes(bytes(b))
    rw, rh = C.c_int(), C.c_int(); back = np.zeros((4, 4, 3), np.float32)
    assert F.ptf_read_image(str(path).encode(), C.byref(rw), C.byref(rh), back.ctypes.data_as(pkg._abi.fp), back.size) != 0
    assert b"PIZ" in F.ptf_last_error()


def test_malformed_exr_headers_are_refused_not_crashed_on(pkg, tmp_path):
    """a tiled part of a multi-part file without (or with a zero) tile description used to reach `(w + tw - 1) / tw` with tw = 0 -- SIGFPE in the
    host process -- because its chunkCount attribute skipped the check; a channel list without its terminating NUL was read past the attribute. Both are
    errors with a message now, like every other malformed input of the reader (imageio.rs:68-97 surfaces the exr crate's Err the same way)."""
    F = pkg.frontend.lib()
    px = {c: np.zeros((7, 9), np.float32) for c in "RGB"}
    good = _exr_bytes([dict(w=9, h=7, pixels=px, chans=[("R", 2), ("G", 2), ("B", 2)], compression=3, tile=(4, 4)),
                       dict(w=9, h=7, pixels=px, chans=[("R", 2), ("G", 2), ("B", 2)], compression=0)], multipart=True)
    rw, rh = C.c_int(), C.c_int(); back = np.zeros((7, 9, 3), np.float32)

    def read(data, name):
        path = tmp_path / name; path.write_bytes(bytes(data))
        st = F.ptf_read_image(str(path).encode(), C.byref(rw), C.byref(rh), back.ctypes.data_as(pkg._abi.fp), back.size)
        return st, F.ptf_last_error()
    assert read(good, "good.exr")[0] == 0
    # tile width 0 in the tile description of the first (tiled) part
    b = bytearray(good)
    i = bytes(b).index(b"tiles\0tiledesc\0") + len(b"tiles\0tiledesc\0") + 4
    b[i:i + 4] = (0).to_bytes(4, "little")
    st, err = read(b, "tile0.exr")
    assert st != 0 and b"tile description" in err, err
    # tile width 2^31: would become a negative int
    b = bytearray(good); b[i:i + 4] = (1 << 31).to_bytes(4, "little")
    st, err = read(b, "tilebig.exr")
    assert st != 0 and b"tile description" in err, err
    # the attribute renamed: the part is tiled ("type" = tiledimage) and has no description at all
    b = bytearray(good); j = bytes(b).index(b"tiles\0tiledesc\0"); b[j:j + 5] = b"tilez"
    st, err = read(b, "notiles.exr")
    assert st != 0 and b"tile description" in err, err
    # channel list whose terminating NUL was overwritten: reading on would leave the attribute
    b = bytearray(good); j = bytes(b).index(b"channels\0chlist\0") + len(b"channels\0chlist\0")
    size = int.from_bytes(b[j:j + 4], "little"); b[j + 4 + size - 1] = ord("X")
    st, err = read(b, "chlist.exr")
    assert st != 0 and (b"channel list" in err or b"truncated" in err or b"subsampled" in err), err
