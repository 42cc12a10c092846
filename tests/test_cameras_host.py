"""The orthographic and the environment camera on the host side (no GPU): the numpy model of tests/camera_model.py proved against the oracle where the oracle has a
camera, the .pbrt front end against the Python builder, the refusal of "realistic", and the perspective job's PtRenderParams against bytes recorded before the
cameras existed."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import camera_model as cm

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- 1. the model is right where it can be checked ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lens", [False, True], ids=["pinhole", "lens"])
@pytest.mark.parametrize("sampler", ["sobol", "halton"])
def test_the_model_of_the_perspective_camera_is_the_oracle_bit_for_bit(pkg, oracle, sampler, lens):
    """32 x 24 x 4 spp, a crop window that starts at (16, 4), camera_to_world of LookAt, Rotate and a non-uniform Scale. A mismatch is a fault of the model."""
    A = pkg._abi
    rp = cm.job(pkg, "perspective", sampler=sampler, lens=lens).render_params()
    assert list(rp.cropped_pixel_bounds) == [16, 4, 48, 28] and list(rp.sample_bounds) == [16, 4, 48, 28] and rp.spp == 4
    _, cs = cm.camera_samples(pkg, oracle, rp)
    cs = np.concatenate([cs, cm.film_corners(rp)])
    N = len(cs)
    assert N == 32 * 24 * 4 + 4
    o = np.zeros((N, 3), F); d = np.zeros((N, 3), F)
    assert oracle.lib.orc_camera_rays(C.byref(rp), N, cs.ctypes.data_as(A.fp), o.ctypes.data_as(A.fp), d.ctypes.data_as(A.fp)) == 0
    mo, md = cm.rays(oracle, rp, cs)
    assert np.array_equal(_bits(mo), _bits(o)), int((_bits(mo) != _bits(o)).any(axis=1).sum())
    assert np.array_equal(_bits(md), _bits(d)), int((_bits(md) != _bits(d)).any(axis=1).sum())
    assert abs(float(np.linalg.norm(d[0])) - 1.0) > 1e-3   # the scaled camera hands on a non-unit direction: the job exercises it


# ---- 2. front end and builder agree ---------------------------------------------------------------------------------------------------------------------------------

_HEAD = '''
Scale 1 1.25 .75
Translate .5 -1 -6
%s
Film "image" "integer xresolution" 64 "integer yresolution" 32 "float cropwindow" [.25 .75 .125 .875]
Sampler "sobol" "integer pixelsamples" 4
PixelFilter "box" "float xwidth" .5 "float ywidth" .5
Integrator "path" "integer maxdepth" 3
WorldBegin
Material "matte"
Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0  1 0 0  0 1 0]
WorldEnd
'''


def _differing_fields(A, a, b):
    out = []
    for name, _ in A.PtRenderParams._fields_:
        x, y = getattr(a, name), getattr(b, name)
        x, y = (list(x), list(y)) if hasattr(x, "__len__") else (x, y)
        if bytes(np.asarray(x)) != bytes(np.asarray(y)):
            out.append((name, x, y))
    return out


def _builder_rp(pkg, kind, **kw):
    b = cm.job(pkg, kind, view="shifted", **kw)
    b.integ.update(maxdepth=3)
    return b.render_params()


def test_a_scene_file_with_the_orthographic_camera_gives_the_builders_render_parameters(pkg):
    A = pkg._abi
    fs = pkg.frontend.FrontScene(text=_HEAD % 'Camera "orthographic" "float screenwindow" [-4 4 -1.5 1.5] "float lensradius" .05 "float focaldistance" 4')
    rp = fs.render_params()
    want = _builder_rp(pkg, "orthographic", lens=True)
    assert rp.camera_type == A.PT_CAMERA_ORTHOGRAPHIC == 1
    assert (rp.shutter_open, rp.shutter_close) == (0.0, 0.0) and rp.lens_radius == F(0.05) and rp.focal_distance == 4.0
    assert bytes(rp) == bytes(want), _differing_fields(A, rp, want)
    # raster_to_camera = inverse(orthographic(0, 1)) * raster_to_screen (orthographic.rs:40-53): raster x in [0, 64] spans the screen window's 8 units, y runs down its 3
    m = np.array(list(rp.raster_to_camera), F).reshape(4, 4)
    assert np.allclose(m, [[8 / 64, 0, 0, -4], [0, -3 / 32, 0, 1.5], [0, 0, 1, 0], [0, 0, 0, 1]], rtol=1e-6, atol=1e-7)


def test_orthographic_defaults_are_the_references(pkg):
    """create_orthographic_camera (orthographic.rs:154-207): shutter 0/0, lensradius 0, focaldistance 1e30, the screen window from the film's aspect ratio."""
    A = pkg._abi
    rp = pkg.frontend.FrontScene(text=_HEAD % 'Camera "orthographic"').render_params()
    want = _builder_rp(pkg, "orthographic", screenwindow=None)
    assert (rp.camera_type, rp.shutter_open, rp.shutter_close, rp.lens_radius, rp.focal_distance) == (1, 0.0, 0.0, 0.0, F(1e30))
    assert bytes(rp) == bytes(want), _differing_fields(A, rp, want)
    m = np.array(list(rp.raster_to_camera), F).reshape(4, 4)   # frame = 64 / 32 = 2: the window is [-2, 2] x [-1, 1]
    assert np.allclose(m, [[4 / 64, 0, 0, -2], [0, -2 / 32, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]], rtol=1e-6, atol=1e-7)
    rp = pkg.frontend.FrontScene(text=_HEAD % 'Camera "orthographic" "float shutteropen" 2 "float shutterclose" .5 "float frameaspectratio" .5').render_params()
    want = _builder_rp(pkg, "orthographic", screenwindow=None, shutteropen=2.0, shutterclose=0.5, frameaspectratio=0.5)
    assert (rp.shutter_open, rp.shutter_close) == (0.5, 2.0)   # swapped when reversed
    assert bytes(rp) == bytes(want), _differing_fields(A, rp, want)


def test_a_scene_file_with_the_environment_camera_gives_the_builders_render_parameters(pkg):
    """create_environment_camera (environment.rs:54-100): shutter 1/1; lensradius, focaldistance, frameaspectratio and screenwindow are read and ignored."""
    A = pkg._abi
    rp = pkg.frontend.FrontScene(text=_HEAD % 'Camera "environment"').render_params()
    want = _builder_rp(pkg, "environment")
    assert rp.camera_type == A.PT_CAMERA_ENVIRONMENT == 2
    assert (rp.shutter_open, rp.shutter_close, rp.lens_radius, rp.focal_distance) == (1.0, 1.0, 0.0, F(1e30))
    assert list(rp.full_resolution) == [64, 32] and list(rp.cropped_pixel_bounds) == [16, 4, 48, 28]
    assert bytes(rp) == bytes(want), _differing_fields(A, rp, want)
    assert not any(rp.raster_to_camera)   # the camera has none
    with_window = pkg.frontend.FrontScene(text=_HEAD % 'Camera "environment" "float screenwindow" [-3 3 -1 1] "float frameaspectratio" 3').render_params()
    assert bytes(with_window) == bytes(rp)


def _same_but_for_rounding_in_the_projection(A, rp, want):
    """The perspective raster_to_camera of the two hosts agrees to rounding only (numpy's matrix product sums in another order than the front end's loop, as it did
    before this camera work); every other byte is equal."""
    m, w = np.array(list(rp.raster_to_camera), F), np.array(list(want.raster_to_camera), F)
    np.testing.assert_allclose(m, w, rtol=2e-6, atol=1e-7)
    a, b = A.PtRenderParams.from_buffer_copy(bytes(rp)), A.PtRenderParams.from_buffer_copy(bytes(want))
    a.raster_to_camera = b.raster_to_camera
    assert bytes(a) == bytes(b), _differing_fields(A, a, b)


def test_perspective_takes_screenwindow_and_frameaspectratio_from_both_hosts(pkg):
    A = pkg._abi
    plain = pkg.frontend.FrontScene(text=_HEAD % 'Camera "perspective" "float fov" 40').render_params()
    _same_but_for_rounding_in_the_projection(A, plain, _builder_rp(pkg, "perspective", focaldistance=1e30))
    rp = pkg.frontend.FrontScene(text=_HEAD % 'Camera "perspective" "float fov" 40 "float screenwindow" [-1.5 1 -.5 .75]').render_params()
    assert rp.camera_type == 0 and list(rp.raster_to_camera) != list(plain.raster_to_camera)
    _same_but_for_rounding_in_the_projection(A, rp, _builder_rp(pkg, "perspective", screenwindow=(-1.5, 1.0, -0.5, 0.75), focaldistance=1e30))
    rp = pkg.frontend.FrontScene(text=_HEAD % 'Camera "perspective" "float fov" 40 "float frameaspectratio" 1.5').render_params()
    assert list(rp.raster_to_camera) != list(plain.raster_to_camera)
    _same_but_for_rounding_in_the_projection(A, rp, _builder_rp(pkg, "perspective", frameaspectratio=1.5, focaldistance=1e30))


# ---- 3. "realistic" is refused by name ---------------------------------------------------------------------------------------------------------------------------------

def test_the_realistic_camera_is_refused_with_the_cameras_that_run(pkg):
    with pytest.raises(ValueError) as e:
        pkg.frontend.FrontScene(text=_HEAD % 'Camera "realistic" "string lensfile" "wide.22mm.dat"')
    msg = str(e.value)
    assert '"realistic"' in msg and all('"%s"' % k in msg for k in ("perspective", "orthographic", "environment")), msg
    with pytest.raises(ValueError) as e:
        pkg.host.SceneBuilder().camera(kind="realistic")
    assert all(k in str(e.value) for k in ("realistic", "perspective", "orthographic", "environment"))


# ---- 4. the perspective job's PtRenderParams are the bytes they were ---------------------------------------------------------------------------------------------------

# Recorded from the commit before the cameras, whose PtRenderParams ended with camera_medium (1288 bytes): SceneBuilder, film 32 x 24, 4 spp,
# LookAt (.3, 2.5, 6) (0, 0, 0) (0, 1, 0), camera(fov=40, lensradius=0.05, focaldistance=6.5) -- and the same film with a bare camera().
_PARENT_SIZE = 1288
_PARENT_SHA = "2120235177de06b3423b2f5ddd4b408894aeb838aac815bd51326c8f24a3ada3"
_PARENT_SHA_BARE = "9d3548b2717ff34237291b5880df8561a4a747e9c0221565f1ac648bf703a6c3"
_PARENT_CAMERA = ("6878f83c00000000000000006878f8be000000006878f8bc000000004e5aba3e000000000000000071f483240000803f00000000000000007cffc7c20000c8423cae7fbfb32c9dbc5b"
                  "d83cbd9a99993e00000000ef596c3fb3b6c4be00002040648b4c3ddf77c4be710e6cbf0000c0400000000000000000000000000000803fcdcc4c3d0000d040000000000000803f")


def test_a_camera_call_without_kind_or_window_gives_the_bytes_it_gave_before(pkg):
    A = pkg._abi
    b = pkg.host.SceneBuilder()
    b.film.update(xres=32, yres=24); b.spp = 4
    b.look_at((0.3, 2.5, 6.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)); b.camera(fov=40.0, lensradius=0.05, focaldistance=6.5)
    b.world_begin()
    raw = bytes(b.render_params())
    assert len(raw) == C.sizeof(A.PtRenderParams) == _PARENT_SIZE + 4 and A.PtRenderParams.camera_type.offset == _PARENT_SIZE
    lo, hi = A.PtRenderParams.raster_to_camera.offset, A.PtRenderParams.max_depth.offset   # raster_to_camera, camera_to_world, lens, focus, shutter
    assert raw[lo:hi].hex() == _PARENT_CAMERA
    assert hashlib.sha256(raw[:_PARENT_SIZE]).hexdigest() == _PARENT_SHA and raw[_PARENT_SIZE:] == bytes(4)   # camera_type 0: perspective
    b = pkg.host.SceneBuilder()
    b.film.update(xres=32, yres=24); b.spp = 4
    b.camera()
    raw = bytes(b.render_params())
    assert hashlib.sha256(raw[:_PARENT_SIZE]).hexdigest() == _PARENT_SHA_BARE and raw[_PARENT_SIZE:] == bytes(4)


# ---- the model's own promises ---------------------------------------------------------------------------------------------------------------------------------------

def test_the_orthographic_lens_quirk_shows_in_the_model(pkg, oracle):
    """orthographic.rs:135 scales the y focus offset by 0.1: the model's ry direction differs from a corrected variant's, its rx direction does not."""
    rp = cm.job(pkg, "orthographic", lens=True).render_params()
    _, cs = cm.camera_samples(pkg, oracle, rp)
    got, has = cm.differentials(oracle, rp, cs)
    fixed, _ = cm.differentials(oracle, rp, cs, corrected=True)
    assert has.all() and np.array_equal(got[:, :9], fixed[:, :9])
    assert (np.abs(got[:, 9:] - fixed[:, 9:]).max(axis=1) > 1e-3).all()


def test_the_environment_model_covers_the_sphere_over_the_full_resolution(pkg, oracle):
    rp = cm.job(pkg, "environment", view="none").render_params()
    cs = np.array([[0, 16, 0, 0, 0], [16, 16, 0, 0, 0], [32, 16, 0, 0, 0], [48, 16, 0, 0, 0], [5, 0, 0, 0, 0], [5, 32, 0, 0, 0]], F)
    o, d = cm.rays(oracle, rp, cs)
    assert not o.any()
    want = [[1, 0, 0], [0, 0, 1], [-1, 0, 0], [0, 0, -1], [0, 1, 0], [0, -1, 0]]   # phi = 0, pi/2, pi, 3pi/2 on the equator; the poles
    assert np.allclose(d, want, atol=2e-7)
    out, has = cm.differentials(oracle, rp, cs)
    assert not has.any() and not out.any()
