"""`mi355pbrt --aov FILE.exr` and the channel-list EXR writer behind it (frontend/fe_imageio.h: write_exr)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest
from conftest import trace_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "exr_parent_writer_5x3.exr")   # written by the three-channel writer as it was before it took a channel list
AOV_CHANNELS = ["N.X", "N.Y", "N.Z", "Z", "albedo.B", "albedo.G", "albedo.R"]


def _golden_rgb():
    """The 5 x 3 image the fixture holds: a ramp with a signed zero, a denormal-sized value, an infinity and the largest floats in its corners."""
    rgb = (np.arange(45, dtype=np.float32).reshape(3, 5, 3) * np.float32(0.37) - np.float32(2.5)).astype(np.float32)
    rgb[0, 0] = [0.0, -0.0, 1e-30]; rgb[2, 4] = [np.inf, 3.0e38, -1.0]
    return rgb


def read_exr_channels(path):
    """An uncompressed scan-line EXR of FLOAT channels, parsed here: ([channel names in file order], {name: (h, w) float32})."""
    data = open(path, "rb").read()
    assert struct.unpack_from("<ii", data, 0) == (20000630, 2)
    pos, attrs = 8, {}
    def cstr(p):
        e = data.index(b"\0", p); return data[p:e].decode(), e + 1
    while data[pos] != 0:
        name, pos = cstr(pos); kind, pos = cstr(pos)
        size, = struct.unpack_from("<i", data, pos); pos += 4
        attrs[name] = (kind, data[pos:pos + size]); pos += size
    pos += 1
    assert attrs["compression"][1] == b"\0" and attrs["lineOrder"][1] == b"\0"
    names, p, ch = [], 0, attrs["channels"][1]
    while ch[p] != 0:
        e = ch.index(b"\0", p); names.append(ch[p:e].decode())
        assert struct.unpack_from("<iiii", ch, e + 1) == (2, 0, 1, 1)   # FLOAT, not linear, sampling 1 x 1
        p = e + 17
    x0, y0, x1, y1 = struct.unpack("<iiii", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    offsets = struct.unpack_from("<%dQ" % h, data, pos)
    planes = {n: np.zeros((h, w), np.float32) for n in names}
    for y, off in enumerate(offsets):
        yy, size = struct.unpack_from("<ii", data, off)
        assert yy == y0 + y and size == 4 * w * len(names)
        for k, n in enumerate(names):
            planes[n][y] = np.frombuffer(data, np.float32, w, off + 8 + 4 * w * k)
    assert offsets[-1] + 8 + 4 * w * len(names) == len(data)
    return names, planes


def test_help_names_the_flag(pkg):
    r = subprocess.run([pkg.frontend.CLI_PATH, "--help"], capture_output=True, text=True)
    assert "--aov" in r.stderr + r.stdout
    r = subprocess.run([pkg.frontend.CLI_PATH, "scene.pbrt", "--adaptive", "0.1", "--aov", "x.exr"], capture_output=True, text=True)
    assert r.returncode == 2 and "--aov" in r.stderr   # (refused before the scene file is looked for)


def test_three_channel_exr_is_byte_identical_to_the_former_writer(pkg, tmp_path):
    out = tmp_path / "rgb.exr"
    pkg.frontend.write_image(str(out), _golden_rgb())
    assert open(out, "rb").read() == open(GOLDEN, "rb").read()
    names, planes = read_exr_channels(str(out))
    assert names == ["B", "G", "R"]
    assert np.array_equal(np.stack([planes[c] for c in "RGB"], -1).view(np.uint32), _golden_rgb().view(np.uint32))


def test_channel_list_writer(pkg, tmp_path):
    A = pkg._abi
    L = pkg.frontend.lib()
    h, w = 3, 4
    rng = np.random.default_rng(11)
    inter = rng.standard_normal((h, w, 3)).astype(np.float32)   # two channels of an interleaved array ...
    plane = rng.standard_normal((h, w)).astype(np.float32)      # ... and one plane

    def write(names, path):
        arrs = {"N.X": (inter[..., 0], 3), "Z": (plane, 1), "albedo.B": (inter[..., 2], 3)}
        n = len(names)
        cn = (C.c_char_p * n)(*[s.encode() for s in names])
        ptrs = (A.fp * n)(*[C.cast(C.c_void_p(inter.ctypes.data + 4 * {"N.X": 0, "albedo.B": 2}[s]) if s != "Z" else C.c_void_p(plane.ctypes.data), A.fp) for s in names])
        strides = (C.c_uint32 * n)(*[arrs[s][1] for s in names])
        return L.ptf_write_exr_channels(os.fsencode(str(path)), w, h, n, cn, ptrs, strides)

    out = tmp_path / "c.exr"
    assert write(["N.X", "Z", "albedo.B"], out) == A.PT_OK
    names, planes = read_exr_channels(str(out))
    assert names == ["N.X", "Z", "albedo.B"]
    assert np.array_equal(planes["N.X"], inter[..., 0]) and np.array_equal(planes["Z"], plane) and np.array_equal(planes["albedo.B"], inter[..., 2])
    bad = tmp_path / "bad.exr"
    assert write(["Z", "N.X"], bad) == A.PT_ERR_INVALID_ARG and not bad.exists()   # the format stores channels sorted by name, byte-wise
    assert b"sorted" in L.ptf_last_error()
    # an entry without a name, without data or with a stride of 0 is refused, not dereferenced
    one = (C.c_uint32 * 1)(1); zero = (C.c_uint32 * 1)(0)
    good_name = (C.c_char_p * 1)(b"Z"); no_name = (C.c_char_p * 1)(None)
    good_data = (A.fp * 1)(plane.ctypes.data_as(A.fp)); no_data = (A.fp * 1)(None)
    for cn, ptrs, strides in ((no_name, good_data, one), (good_name, no_data, one), (good_name, good_data, zero)):
        assert L.ptf_write_exr_channels(os.fsencode(str(bad)), w, h, 1, cn, ptrs, strides) == A.PT_ERR_INVALID_ARG and not bad.exists()
    assert L.ptf_write_exr_channels(os.fsencode(str(bad)), w, h, 1, good_name, good_data, one) == A.PT_OK


SCENE = """LookAt 2 2 5  0 -0.4 0  0 1 0
Camera "perspective" "float fov" 30
Film "image" "integer xresolution" 40 "integer yresolution" 24 "string filename" "beauty.pfm"
Sampler "sobol" "integer pixelsamples" 8
PixelFilter "box"
Integrator "path" "integer maxdepth" 3
WorldBegin
LightSource "distant" "rgb L" [3 3 3] "point from" [0 10 0] "point to" [0 0 0]
Texture "chk" "spectrum" "checkerboard" "float uscale" 6 "float vscale" 6 "rgb tex1" [0.9 0.8 0.7] "rgb tex2" [0.1 0.2 0.3]
Material "matte" "texture Kd" "chk"
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-4 -1 -4  -4 -1 4  4 -1 4  4 -1 -4] "float st" [0 0 0 1 1 1 1 0]
AttributeBegin
  Material "mirror" "rgb Kr" [0.9 0.9 0.9]
  Translate -0.6 0 0
  Shape "sphere" "float radius" 1
AttributeEnd
WorldEnd
"""


@pytest.mark.gpu
@pytest.mark.parametrize("samples", [None, (2, 7)])
def test_aov_file_holds_the_resolved_planes(pkg, gpu, tmp_path, samples):
    scene = tmp_path / "scene.pbrt"; scene.write_text(SCENE)
    out, aov = tmp_path / "beauty.pfm", tmp_path / "features.exr"
    cmd = [pkg.frontend.CLI_PATH, str(scene), "--outfile", str(out), "--aov", str(aov), "--quiet"]
    if samples: cmd += ["--samples", "%d:%d" % samples]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=trace_env())
    assert r.returncode == 0, r.stderr
    names, planes = read_exr_channels(str(aov))
    assert names == AOV_CHANNELS and names == sorted(names, key=lambda s: s.encode())
    fs = pkg.frontend.FrontScene(path=str(scene))
    rp = fs.render_params()
    g = pkg.Scene(gpu, fs)
    sums = g.render_aov(rp, samples=None if samples is None else (samples[0], samples[1] - samples[0]))
    want = pkg.runtime.resolve_aov(sums, gpu)
    assert planes["Z"].shape == (24, 40)
    hit = sums["depth"][..., 1] > 0
    assert 0.3 < hit.mean() < 0.95 and np.ptp(want["albedo"][hit], axis=0).max() > 0.3
    # (a sample on a pixel's edge reaches the neighbouring pixel by an atomic, whose place in that pixel's chain of additions varies between two renders)
    np.testing.assert_allclose(planes["Z"], want["depth"], rtol=2e-6, atol=1e-7)
    for k, c in enumerate("XYZ"):
        np.testing.assert_allclose(planes["N." + c], want["normal"][..., k], rtol=2e-6, atol=2e-7)
    for k, c in enumerate("RGB"):
        np.testing.assert_allclose(planes["albedo." + c], want["albedo"][..., k], rtol=2e-6, atol=1e-7)
    assert pkg.frontend.read_image(str(out)).shape == (24, 40, 3)
