"""pt_denoise on the GPU (include/mi355dn.h, libmi355dn.so) against tests/denoise_reference.py, the numpy model test_denoise_model.py holds in place. Inputs are uploaded
from host arrays, so the device and the model read the same bits.

Tolerance: |gpu - model64| <= 4e-5 * max(|model64|, 1e-3) -- four times the float32 model's own distance from the float64 model (test_denoise_model.FLOOR = 1e-5;
measured 8.6e-6 on the rendered inputs, 1.2e-6 on the synthetic ones). The device runs the float32 model's operations in its order and differs by its expf alone.

Shapes: 5x3 is smaller than every halo and than the reach of stride 2 (and has fewer columns and rows than the wide levels have residue classes); 37x21 has ragged
tiles; 300x70 is wider than 16 lattice cells at stride 16, so halos cross tile edges at the last level; 20x270 does the same along y, which the tile numbering of
k_dn_atrous treats apart from x. Each at 1..5 levels, so that a wrong level is named. One more boundary of this tiling: the grid is capped at 2^14 blocks, which then
take several tiles each -- a 1 x (2^18 + 40) image has 16 387 tiles at stride 1 and 16 388 at stride 2 (a one-pixel-wide tile holds 16 pixels), run at 2 levels."""
import subprocess

import numpy as np
import pytest
from conftest import trace_env
import denoise_reference as R
from test_denoise_model import ganesha

TOL = 4.0e-5
SHAPES = [(5, 3), (37, 21), (300, 70), (20, 270)]

_MODEL = {}


def model64(key, make, **params):
    """The float64 model's image of inputs `make()`, computed once per key and left unchanged (every test runs under both traversal modes)."""
    k = (key, tuple(sorted(params.items())))
    if k not in _MODEL:
        a, b, sums = make()
        out = R.denoise_reference(a, b, sums, np.float64, **params)
        out.setflags(write=False)
        _MODEL[k] = (a, b, sums, out)
    return _MODEL[k]


@pytest.fixture(scope="module")
def scene(pkg, gpu):
    """A scene handle to run the filter on: pt_denoise needs its stream and statistics, not its geometry."""
    sd, _ = pkg.scenes.spheres_c1(xres=8, yres=8, spp=8).world_end()
    s = pkg.Scene(gpu, sd)
    yield s
    s.close()


def check(got, want, what):
    dev = R.deviation(got, want)
    print("%s: largest deviation %.3g of %.3g allowed" % (what, dev, TOL))
    assert np.isfinite(got).all() and dev <= TOL, what


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_and_levels(pkg, scene, shape, iterations):
    """A normal step and a depth step through the image, every pixel a hit."""
    w, h = shape
    a, b, sums, want = model64(("steps", w, h), lambda: R.synthetic_inputs(w, h, seed=w, guides="steps"), iterations=iterations)
    got = scene.denoise(a, b, sums, R.params_struct(pkg, iterations=iterations))
    check(got, want, "%dx%d, %d levels" % (w, h, iterations))
    if iterations >= 3 and min(w, h) > 8:   # the filter did something, and stopped at the steps
        noisy = R.resolve(a + b, 1.0, np.float32)
        assert np.abs(got - noisy).max() > 0.02


@pytest.mark.gpu
def test_more_tiles_than_blocks(pkg, scene):
    """A one-pixel-wide image of 2^18 + 40 pixels: more tiles than the capped grid has blocks at both levels, so blocks loop over tiles (and restage their LDS)."""
    w, h = 1, 2 ** 18 + 40
    a, b, sums, want = model64(("thin", w, h), lambda: R.synthetic_inputs(w, h, seed=2, guides="steps", invalid=0.01), iterations=2)
    got = scene.denoise(a, b, sums, R.params_struct(pkg, iterations=2))
    check(got, want, "1 x %d, 2 levels" % h)
    assert np.abs(got - R.resolve(a + b, 1.0, np.float32)).max() > 0.02


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("boundary", 0.0, 37, 21), ("miss", 0.0, 37, 21), ("steps", 0.2, 37, 21), ("boundary", 0.15, 300, 70)], ids=lambda c: "%s-%g-%dx%d" % c)
def test_guides(pkg, scene, case):
    """A hit / miss boundary with a row of partially covered pixels; an all-miss image; scattered invalid pixels (A.w or B.w is 0), which pass through and feed nobody."""
    guides, invalid, w, h = case
    make = lambda: R.synthetic_inputs(w, h, seed=7, guides=guides, invalid=invalid)
    for params in (dict(iterations=5), dict(iterations=2, sigma_l=1.5, sigma_z=0.4, sigma_n=0.6, albedo_floor=0.3, scale=2.5)):
        a, b, sums, want = model64(case, make, **params)
        got = scene.denoise(a, b, sums, R.params_struct(pkg, **params))
        check(got, want, "%s %r" % (case, params))
        bad = (a[..., 3] == 0) | (b[..., 3] == 0)
        assert bad.any() == (invalid > 0)
        if invalid > 0:   # resolved as the film, bit for bit
            np.testing.assert_array_equal(got[bad].view(np.uint32), R.resolve(a + b, params.get("scale", 1.0), np.float32)[bad].view(np.uint32))
    if guides == "boundary":
        cov = sums["normal"][..., 3] / sums["albedo"][..., 3]
        assert ((cov > 0) & (cov < 1)).sum() >= w // 3 and (cov == 0).any() and (cov == 1).any()


@pytest.mark.gpu
def test_no_level_is_the_resolved_film(pkg, scene):
    a, b, sums, want = model64(("none", 37, 21), lambda: R.synthetic_inputs(37, 21, seed=5, guides="boundary", invalid=0.1), iterations=0, scale=1.7)
    got = scene.denoise(a, b, sums, R.params_struct(pkg, iterations=0, scale=1.7))
    check(got, want, "no level")
    np.testing.assert_allclose(got, R.resolve(a + b, 1.7, np.float32), rtol=3 * 2.0 ** -23, atol=0)
    # the float32 model's operations without an exponential: the device's bits
    np.testing.assert_array_equal(got.view(np.uint32), R.denoise_reference(a, b, sums, np.float32, iterations=0, scale=1.7).view(np.uint32))


@pytest.mark.gpu
def test_two_calls_and_both_buffer_paths_agree_bit_for_bit(pkg, scene):
    import torch
    w, h = 300, 70
    a, b, sums = R.synthetic_inputs(w, h, seed=11, guides="boundary", invalid=0.1)
    p = R.params_struct(pkg)
    first = scene.denoise(a, b, sums, p)
    again = scene.denoise(a, b, sums, p)
    np.testing.assert_array_equal(first.view(np.uint32), again.view(np.uint32))
    dev = {k: torch.from_numpy(v).cuda() for k, v in dict(sums, a=a, b=b).items()}
    keep = {k: v.clone() for k, v in dev.items()}
    out = torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()   # (the library runs on its own stream)
    scene.denoise(dev["a"].data_ptr(), dev["b"].data_ptr(), {k: dev[k].data_ptr() for k in sums}, p, device_ptrs=(w, h, out.data_ptr()))
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), first.view(np.uint32))
    for k in dev:   # the inputs are read, not written
        assert torch.equal(dev[k], keep[k]), k


@pytest.mark.gpu
def test_statistics_are_added_and_counters_left(pkg, scene):
    rp = pkg.scenes.spheres_c1(xres=8, yres=8, spp=8).world_end()[1]
    scene.render(rp)
    before, stats0 = scene.counters(), {s["name"]: s for s in scene.kernel_stats()}
    assert "denoise_prepare" not in stats0 and "denoise_atrous" not in stats0
    a, b, sums = R.synthetic_inputs(37, 21)
    scene.denoise(a, b, sums, R.params_struct(pkg, iterations=3))
    stats = {s["name"]: s for s in scene.kernel_stats()}
    assert stats["denoise_prepare"]["launches"] == 1 and stats["denoise_atrous"]["launches"] == 3 and stats["denoise_variance"]["launches"] == 3
    assert stats["denoise_prepare"]["items"] == 37 * 21 and stats["denoise_atrous"]["items"] == 3 * 37 * 21
    for name, s in stats0.items():   # the render's own kinds stay as they were
        assert stats[name]["launches"] == s["launches"], name
    assert scene.counters() == before


@pytest.mark.gpu
def test_render_denoised_end_to_end(pkg, gpu, oracle):
    """render_denoised on the model test's scene: the model applied to the GPU's own halves and sums, the quality condition (a) against the oracle's 1024-spp render,
    the launch kinds, and the counters as the last render -- the feature render -- left them."""
    sd, rp = ganesha(pkg)
    ref = R.oracle_inputs(pkg, oracle, ("ganesha", 24, 64, 48, 4), sd, rp)[3]
    s = pkg.Scene(gpu, sd)
    try:
        params = R.params_struct(pkg)
        rgb, film, (a, b, sums) = s.render_denoised(rp, params, inputs=True)
        stats = {k["name"]: k for k in s.kernel_stats()}
        counters = s.counters()
        assert stats["denoise_prepare"]["launches"] == 1 and stats["denoise_atrous"]["launches"] == params.iterations == 5
        assert counters["camera_rays"] == 64 * 48 * 4 and counters["film_splats"] >= 64 * 48 * 4   # the feature render's: every sample of the job, once
        np.testing.assert_array_equal(film, a + b)
        assert (a[..., 3] >= 2).all() and (b[..., 3] >= 2).all()
        check(rgb, R.denoise_reference(a, b, sums, np.float64), "ganesha 64x48, 4 spp, the GPU's halves and sums")
        den, raw = R.rel_mse(rgb, ref), R.rel_mse(s.resolve(film), ref)
        print("ganesha 64x48, 4 spp on the GPU: relMSE denoised %.4f, noisy %.4f, ratio %.3f" % (den, raw, den / raw))
        assert den < 0.5 * raw
        rp.spp = 1
        with pytest.raises(ValueError):
            s.render_denoised(rp)
    finally:
        s.close()


SCENE = """LookAt 2 2 5  0 -0.4 0  0 1 0
Camera "perspective" "float fov" 30
Film "image" "integer xresolution" 40 "integer yresolution" 24 "string filename" "beauty.pfm"
Sampler "sobol" "integer pixelsamples" %d
PixelFilter "box"
Integrator "path" "integer maxdepth" 3
WorldBegin
LightSource "distant" "rgb L" [3 3 3] "point from" [0 10 0] "point to" [0 0 0]
Material "matte" "rgb Kd" [0.6 0.5 0.4]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-4 -1 -4  -4 -1 4  4 -1 4  4 -1 -4]
AttributeBegin
  Material "plastic" "rgb Kd" [0.2 0.5 0.7]
  Translate -0.6 0 0
  Shape "sphere" "float radius" 1
AttributeEnd
WorldEnd
"""


def test_command_line_refusals(pkg, tmp_path):
    cli = pkg.frontend.CLI_PATH
    r = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert "--denoise FILE" in r.stderr + r.stdout and "--denoise-iterations" in r.stderr + r.stdout
    for extra in (["--adaptive", "0.1"], ["--checkpoint", "c.bin"], ["--preview-every", "2"], ["--denoise-iterations", "6"], ["--denoise-iterations", "x"]):
        r = subprocess.run([cli, "scene.pbrt", "--denoise", "d.pfm"] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "--denoise" in r.stderr and "usage:" in r.stderr, extra   # (refused before the scene file is looked for)
    r = subprocess.run([cli, "scene.pbrt", "--denoise-iterations", "3"], capture_output=True, text=True)
    assert r.returncode == 2 and "--denoise" in r.stderr
    # fewer than two samples: known once the scene file is read, refused before the device is touched
    scene = tmp_path / "one.pbrt"; scene.write_text(SCENE % 1)
    out = tmp_path / "d.pfm"
    for extra in ([], ["--spp", "8", "--samples", "3:4"]):
        r = subprocess.run([cli, str(scene), "--denoise", str(out), "--outfile", str(tmp_path / "o.pfm")] + extra, capture_output=True, text=True)
        assert r.returncode == 2 and "two samples" in r.stderr and "usage:" in r.stderr and not out.exists(), extra


@pytest.mark.gpu
def test_command_line_writes_the_library_image(pkg, gpu, tmp_path):
    scene = tmp_path / "scene.pbrt"; scene.write_text(SCENE % 8)
    plain, out, den = tmp_path / "plain.pfm", tmp_path / "beauty.pfm", tmp_path / "denoised.pfm"
    cli = pkg.frontend.CLI_PATH
    for cmd in ([cli, str(scene), "--outfile", str(plain), "--quiet"], [cli, str(scene), "--outfile", str(out), "--denoise", str(den), "--denoise-iterations", "4", "--quiet"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=trace_env())
        assert r.returncode == 0, r.stderr
    # the outfile is the plain run's: the halves' sum adds a pixel's samples in another order, nothing else
    np.testing.assert_allclose(pkg.frontend.read_image(str(out)), pkg.frontend.read_image(str(plain)), rtol=2e-6, atol=1e-7)
    fs = pkg.frontend.FrontScene(path=str(scene))
    rp = fs.render_params()
    g = pkg.Scene(gpu, fs)
    try:
        a, b = g.render(rp, samples=(0, 4)), g.render(rp, samples=(4, 4))
        want = g.denoise(a, b, g.render_aov(rp), R.params_struct(pkg, iterations=4, scale=rp.scale))
    finally:
        g.close()
    got = pkg.frontend.read_image(str(den))
    assert got.shape == (24, 40, 3)
    # (a sample on a pixel's edge reaches the neighbouring pixel by an atomic, whose place in that pixel's chain of additions varies between two renders: the inputs of
    # the two filter runs agree to rounding, not bit for bit)
    check(got, want, "mi355pbrt --denoise against Scene.denoise")
    assert np.abs(got - pkg.frontend.read_image(str(out))).max() > 0.01


@pytest.mark.gpu
def test_command_line_range_with_features_and_denoising_together(pkg, gpu, tmp_path):
    """--samples 2:8 with --aov, --denoise and --outfile in one run: each file is what the flag gives without the other two."""
    from test_aov_frontend import AOV_CHANNELS, read_exr_channels
    scene = tmp_path / "scene.pbrt"; scene.write_text(SCENE % 8)
    cli, common = pkg.frontend.CLI_PATH, [str(scene), "--samples", "2:8", "--quiet", "--outfile"]
    for extra in (["plain.pfm"], ["alone.pfm", "--aov", "alone.exr"], ["o.pfm", "--aov", "f.exr", "--denoise", "d.pfm"]):
        r = subprocess.run([cli] + common + extra, capture_output=True, text=True, timeout=300, env=trace_env(), cwd=tmp_path)
        assert r.returncode == 0, r.stderr
    read = lambda name: pkg.frontend.read_image(str(tmp_path / name))
    # the outfile is the plain run's: the halves' sum adds a pixel's samples in another order, nothing else
    np.testing.assert_allclose(read("o.pfm"), read("plain.pfm"), rtol=2e-6, atol=1e-7)
    names, planes = read_exr_channels(str(tmp_path / "f.exr"))
    alone = read_exr_channels(str(tmp_path / "alone.exr"))[1]
    assert names == AOV_CHANNELS
    for name in names:   # (test_aov_frontend's bounds: an atomic's place in a pixel's chain of additions varies between two renders)
        np.testing.assert_allclose(planes[name], alone[name], rtol=2e-6, atol=2e-7 if name.startswith("N.") else 1e-7, err_msg=name)
    fs = pkg.frontend.FrontScene(path=str(scene))
    rp = fs.render_params()
    g = pkg.Scene(gpu, fs)
    try:
        a, b = g.render(rp, samples=(2, 3)), g.render(rp, samples=(5, 3))
        want = g.denoise(a, b, g.render_aov(rp, samples=(2, 6)), R.params_struct(pkg, scale=rp.scale))
    finally:
        g.close()
    got = read("d.pfm")
    assert got.shape == (24, 40, 3)
    check(got, want, "mi355pbrt --samples 2:8 --aov --denoise against Scene.denoise")
    assert np.abs(got - read("o.pfm")).max() > 0.01
