"""No GPU: pt_tile_grid is the arithmetic of integrator.rs:277-279 on the sample bounds -- the grid the tile lists of pt_render_tiles / pt_tiles_select index --, and
mi355pbrt's usage errors for --adaptive."""
import ctypes as C
import subprocess

import pytest
from abi_checks import no_device_env
from range_scene import range_scene
from tile_scene import BACKGROUND_PBRT, grid_of, with_filter


def _grid(pkg, rp):
    lib = pkg._abi.bind(C.CDLL(pkg.runtime.LIB_PATH))
    ntx, nty = C.c_uint32(99), C.c_uint32(99)
    assert lib.pt_tile_grid(C.byref(rp), C.byref(ntx), C.byref(nty)) == pkg._abi.PT_OK
    return ntx.value, nty.value


@pytest.mark.parametrize("case,want", [("box", (3, 2)), ("gaussian2", (3, 2)), ("crop", (2, 1)), ("one_pixel", (1, 1)), ("one_pixel_gaussian", (1, 1)), ("hd", (120, 68))])
def test_tile_grid_is_the_arithmetic_on_the_sample_bounds(pkg, case, want):
    if case in ("box", "gaussian2"):
        _, rp = range_scene(pkg, xres=40, yres=24)
        if case == "gaussian2":
            with_filter(pkg, rp, "gaussian", 2.0)
            assert list(rp.sample_bounds) == [-2, -2, 42, 26]   # still 3 x 2, offset from the film's grid
    elif case == "crop":
        b = pkg.host.SceneBuilder(); b.film.update(xres=40, yres=24, crop=(0.25, 0.75, 0.5, 1.0))
        rp = b.render_params()
        assert list(rp.cropped_pixel_bounds) == [10, 12, 30, 24]
    elif case == "hd":
        b = pkg.host.SceneBuilder(); b.film.update(xres=1920, yres=1080)
        rp = b.render_params()
    else:
        b = pkg.host.SceneBuilder(); b.film.update(xres=1, yres=1)
        rp = b.render_params()
        if case == "one_pixel_gaussian":
            with_filter(pkg, rp, "gaussian", 2.0)   # sample bounds [-2, 3) x [-2, 3): one ragged tile
    sb = rp.sample_bounds
    assert grid_of(rp) == ((sb[2] - sb[0] + 15) // 16, (sb[3] - sb[1] + 15) // 16) == want
    assert _grid(pkg, rp) == want


def test_tile_grid_refuses_null_arguments(pkg):
    A = pkg._abi
    lib = A.bind(C.CDLL(pkg.runtime.LIB_PATH))
    _, rp = range_scene(pkg)
    n = C.c_uint32()
    assert lib.pt_tile_grid(None, C.byref(n), C.byref(n)) == A.PT_ERR_INVALID_ARG
    assert lib.pt_tile_grid(C.byref(rp), None, C.byref(n)) == A.PT_ERR_INVALID_ARG
    assert lib.pt_tile_grid(C.byref(rp), C.byref(n), None) == A.PT_ERR_INVALID_ARG
    assert b"null" in lib.pt_last_error()


@pytest.mark.parametrize("extra,why", [(["--checkpoint", "job.ckpt"], "--checkpoint"), (["--samples", "0:4"], "--samples"), ([], "Integrator \"ambientocclusion\"")])
def test_mi355pbrt_refuses_adaptive_with_what_it_cannot_keep_before_any_gpu_call(pkg, tmp_path, extra, why):
    text = BACKGROUND_PBRT if extra else BACKGROUND_PBRT.replace('Integrator "path" "integer maxdepth" 5', 'Integrator "ambientocclusion" "integer nsamples" 4')
    assert extra or "ambientocclusion" in text
    scene = tmp_path / "adaptive.pbrt"; scene.write_text(text)
    out = tmp_path / "o.pfm"
    env = no_device_env()   # the usage error must come first
    r = subprocess.run([pkg.frontend.CLI_PATH, str(scene), "--outfile", str(out), "--adaptive", "0.1", *extra], capture_output=True, text=True, timeout=60, env=env, cwd=str(tmp_path))
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "usage:" in r.stderr and "--adaptive with " + why in r.stderr and not out.exists() and not (tmp_path / "job.ckpt").exists()
    bad = subprocess.run([pkg.frontend.CLI_PATH, str(scene), "--adaptive", "-1"], capture_output=True, text=True, timeout=60, env=env, cwd=str(tmp_path))
    assert bad.returncode == 2 and "--adaptive takes" in bad.stderr
