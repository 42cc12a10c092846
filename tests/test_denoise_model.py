"""The yardstick of the denoiser's GPU tests (test_denoise.py) held in place without a GPU: tests/denoise_reference.py, the numpy model of include/mi355dn.h, on half
films from the unchanged oracle and first-hit sums from aov_reference. What it must do (a quality condition), what it must leave alone (a constant film, no level at
all), and how far its float32 run in the device's order stays from its float64 run -- the floor the device's tolerance is four times of."""
import numpy as np
import pytest
import denoise_reference as R

FLOOR = 1.0e-5   # float32 model against float64 model, relative to max(|x|, 1e-3). Measured: 8.6e-6 (ganesha), 2.3e-6 (material zoo), 1.2e-6 at most on denoise_reference.synthetic_inputs


def ganesha(pkg):
    return pkg.scenes.ganesha_scale(n=24, xres=64, yres=48, spp=4).world_end()


@pytest.fixture(scope="module")
def ganesha_inputs(pkg, oracle):
    sd, rp = ganesha(pkg)
    assert list(rp.filter_radius) == [0.5, 0.5]   # the box filter
    return R.oracle_inputs(pkg, oracle, ("ganesha", 24, 64, 48, 4), sd, rp)


def test_halves_are_what_the_recipe_says(ganesha_inputs):
    a, b, sums, ref = ganesha_inputs
    assert a.shape == b.shape == (48, 64, 4) and ref.shape == (48, 64, 3)
    assert (a[..., 3] >= 2).all() and (b[..., 3] >= 2).all() and (b[..., :3] > -1e-4).all()   # two samples of a pixel in each half (+ the odd splat from a neighbour's edge)
    np.testing.assert_array_equal(sums["albedo"][..., 3], a[..., 3] + b[..., 3])              # the sums are of the samples of A + B
    hit = sums["normal"][..., 3] > 0
    assert 0.3 < hit.mean() < 0.999   # surfaces and background both


def test_quality_on_ganesha(ganesha_inputs):
    """(a) relMSE against the oracle's 1024-spp render: the denoised image under half the noisy one's. Measured: 0.0077 against 0.0326, ratio 0.235."""
    a, b, sums, ref = ganesha_inputs
    out = R.denoise_reference(a, b, sums, np.float64)
    noisy = R.resolve((a + b).astype(np.float32), 1.0, np.float32)
    den, raw = R.rel_mse(out, ref), R.rel_mse(noisy, ref)
    print("ganesha 64x48, 4 spp: relMSE denoised %.4f, noisy %.4f, ratio %.3f" % (den, raw, den / raw))
    assert den < 0.5 * raw


def test_quality_on_the_material_zoo_is_reported(pkg, oracle):
    """Printed, not gated: glossy and specular spheres, whose look is not their first hit's albedo, and one textured surface (the half films' recipe is only
    approximately right there). Measured: relMSE 0.0305 against 0.0546 noisy, ratio 0.558, at five levels; 0.0205 after one."""
    sd, rp = pkg.scenes.material_zoo(n=16, xres=96, yres=64, spp=8).world_end()
    a, b, sums, ref = R.oracle_inputs(pkg, oracle, ("zoo", 16, 96, 64, 8), sd, rp)
    raw = R.rel_mse(R.resolve((a + b).astype(np.float32), 1.0, np.float32), ref)
    for it in (1, 5):
        o64 = R.denoise_reference(a, b, sums, np.float64, iterations=it)
        print("material zoo 96x64, 8 spp, %d levels: relMSE denoised %.4f, noisy %.4f, ratio %.3f" % (it, R.rel_mse(o64, ref), raw, R.rel_mse(o64, ref) / raw))
    dev = R.deviation(R.denoise_reference(a, b, sums, np.float32), o64)
    print("material zoo: float32 model against float64 model %.3g" % dev)
    assert dev <= FLOOR


def test_constant_film_comes_back_unchanged():
    """(b) equal halves of one colour: no variance, no edge, every weight the tap's own -- the weighted mean of equal values, to rounding."""
    h, w = 21, 37
    a, _, sums = R.synthetic_inputs(w, h, guides="boundary")
    rgb = np.array([0.7, 0.4, 0.2])
    m = R.prepare(a, a, sums, 0.01, np.float64)["m"]
    # constant AFTER demodulation is what the filter leaves alone: the film is colour * m
    film = np.concatenate([(m * rgb) @ np.linalg.inv(np.array(R.XYZ2RGB)).T * 4.0, np.full((h, w, 1), 4.0)], -1).astype(np.float32)
    for T in (np.float32, np.float64):
        out = R.denoise_reference(film, film, sums, T)
        want = R.resolve(film.astype(T) + film.astype(T), 1.0, T)
        assert R.deviation(out, want) <= 2e-6, T   # 25 roundings of a mean of equal values in float32: a few ulp


def test_no_level_is_the_resolved_film(pkg, ganesha_inputs):
    """(c) iterations = 0: max(0, (c / m) * m) * scale -- pt_film_resolve's image to the roundings of the division and the product. The model's resolve IS the
    library's, bit for bit (host arithmetic: no device)."""
    a, b, sums, _ = ganesha_inputs
    film = a + b
    lib_rgb = np.zeros(film.shape[:2] + (3,), np.float32)
    fp = pkg._abi.fp
    assert pkg.load_library().lib.pt_film_resolve(film.ctypes.data_as(fp), film.size // 4, 1.7, lib_rgb.ctypes.data_as(fp)) == pkg._abi.PT_OK
    np.testing.assert_array_equal(R.resolve(film, 1.7, np.float32).view(np.uint32), lib_rgb.view(np.uint32))
    for T, eps in ((np.float32, 2.0 ** -23), (np.float64, 2.0 ** -52)):
        out = R.denoise_reference(a, b, sums, T, iterations=0, scale=1.7)
        want = R.resolve(a.astype(T) + b.astype(T), 1.7, T)
        np.testing.assert_allclose(out, want, rtol=3 * eps, atol=0)   # (half an ulp each: c / m, d * m, and the scaling on either side)


def test_invalid_pixels_pass_through_and_feed_nobody():
    a, b, sums = R.synthetic_inputs(37, 21, seed=3, invalid=0.2)
    g = R.prepare(a, b, sums, 0.01, np.float32)
    bad = ~g["valid"]
    assert 0.1 < bad.mean() < 0.3
    out = R.denoise_reference(a, b, sums, np.float32, scale=2.0)
    np.testing.assert_array_equal(out[bad], R.resolve(a + b, 2.0, np.float32)[bad])
    # whatever an invalid pixel holds, its neighbours do not see it
    a2, b2 = a.copy(), b.copy()
    a2[..., :3][bad] *= 50.0; b2[..., :3][bad] += 7.0
    out2 = R.denoise_reference(a2, b2, sums, np.float32, scale=2.0)
    np.testing.assert_array_equal(out2[~bad], out[~bad])


@pytest.mark.parametrize("iterations", [1, 5])
def test_float32_model_floor(ganesha_inputs, iterations):
    """(d) the float32 model in the device's order against the float64 model, on the rendered inputs the device's end-to-end test reads."""
    a, b, sums, _ = ganesha_inputs
    dev = R.deviation(R.denoise_reference(a, b, sums, np.float32, iterations=iterations), R.denoise_reference(a, b, sums, np.float64, iterations=iterations))
    print("ganesha, %d levels: float32 model against float64 model %.3g" % (iterations, dev))
    assert dev <= FLOOR
