"""The device film tools (pt_film_resolve_device, pt_film_halves_error) on synthetic films, and the progressive driver built on them (runtime.Scene.render_progressive)."""
import ctypes as C

import numpy as np
import pytest
from parity import ORACLE_THREADS, assert_same_film
from range_scene import range_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def any_scene(pkg, gpu):
    sd, _ = pkg.scenes.ganesha_scale(n=4, xres=16, yres=16, spp=1, env=False).world_end()
    return pkg.Scene(gpu, sd)


def synthetic_film(n, seed):
    """XYZW sums with what a film can hold: zero weights (with and without radiance), negative channel sums, very large and very small weights."""
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.0, 2.0, (n, 4)).astype(np.float32)
    f[:, 3] = rng.uniform(0.5, 64.0, n)
    k = np.arange(n)
    f[k % 7 == 1, 3] = 0.0
    f[k % 11 == 2] = 0.0
    f[k % 5 == 3, :3] *= np.float32(-1.0)
    f[k % 13 == 4, 0] = -3.0
    f[k % 17 == 5, 3] = 1e30
    f[k % 19 == 6, 3] = 1e-30
    f[k % 23 == 7, 3] = 1e-42   # a denormal weight: 1 / w overflows
    f[k % 29 == 8, :3] *= np.float32(1e-3)   # the linear toe of the sRGB curve
    return f


def srgb8_reference(rgb):
    """write_image_png_tga (core/imageio.rs:365-366, gamma_correct core/pbrt.rs:210-216) in float64: clamp(255 * gamma_correct(v) + 0.5, 0, 255) as u8."""
    v = rgb.astype(np.float64)
    with np.errstate(all="ignore"):
        g = np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.power(np.abs(v), 1.0 / 2.4) - 0.055)
        s = np.clip(255.0 * g + 0.5, 0.0, 255.0)
    return np.where(np.isnan(s), 0.0, s).astype(np.uint8)


@pytest.mark.parametrize("n", [1037, 1])
def test_resolve_on_the_device(pkg, gpu, any_scene, n):
    import torch
    A = pkg._abi
    g = any_scene
    film = synthetic_film(n, 5 + n)
    scale = 0.75
    want = g.resolve(film, scale)
    d_film = torch.from_numpy(film).to("cuda:0")
    d_rgb = torch.full((n, 3), -1.0, dtype=torch.float32, device="cuda:0")
    d_code = torch.full((3 * n + 8,), 99, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    g.resolve_device(d_film.data_ptr(), n, scale, d_rgb.data_ptr(), d_code.data_ptr())
    rgb = d_rgb.cpu().numpy(); code = d_code.cpu().numpy()
    assert np.array_equal(rgb.view(np.uint32), want.view(np.uint32))
    assert (code[3 * n:] == 99).all()   # nothing past the image
    ref = srgb8_reference(want).reshape(-1)
    diff = np.abs(code[:3 * n].astype(np.int32) - ref.astype(np.int32))
    print("n =", n, "srgb8 codes that differ from the float64 evaluation:", int((diff > 0).sum()), "of", 3 * n, "largest difference", int(diff.max()))
    assert diff.max() <= 1
    assert len(set(ref.tolist())) > 20 or n == 1   # (the codes span the curve)
    # either output alone gives the same values, on a 4-byte aligned pointer (dword stores) and on an odd one (byte stores)
    d_rgb2 = torch.zeros_like(d_rgb); d_code2 = torch.full_like(d_code, 99)
    torch.cuda.synchronize()
    g.resolve_device(d_film.data_ptr(), n, scale, d_rgb2.data_ptr(), None)
    g.resolve_device(d_film.data_ptr(), n, scale, None, d_code2.data_ptr() + 1)
    assert torch.equal(d_rgb2, d_rgb)
    code2 = d_code2.cpu().numpy()
    assert code2[0] == 99 and np.array_equal(code2[1:3 * n + 1], code[:3 * n]) and (code2[3 * n + 1:] == 99).all()
    assert gpu.lib.pt_film_resolve_device(g.h, C.c_void_p(d_film.data_ptr()), n, scale, None, None) == A.PT_ERR_INVALID_ARG
    names = {s["name"]: s["kernel"] for s in g.kernel_stats()}
    assert names["film_resolve"] == "k_film_resolve"


def halves(w, h, seed):
    rng = np.random.default_rng(seed)
    a = synthetic_positive(rng, w, h); b = synthetic_positive(rng, w, h)
    k = np.arange(w * h).reshape(h, w)
    a[k % 9 == 1, 3] = 0.0        # zero weight in A only, in B only, in both
    b[k % 9 == 4, 3] = 0.0
    a[k % 31 == 7, 3] = 0.0; b[k % 31 == 7, 3] = 0.0
    return a, b


def synthetic_positive(rng, w, h):
    f = np.empty((h, w, 4), np.float32)
    wt = rng.uniform(1.0, 16.0, (h, w)).astype(np.float32)
    rgb = rng.uniform(0.0, 1.5, (h, w, 3)) * rng.uniform(0.0, 1.0, (h, w, 1)) ** 3   # dark and bright pixels
    m = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
    f[..., :3] = (rgb @ m.T) * wt[..., None]
    f[..., 3] = wt
    return f


def halves_reference(g, a, b):
    """The definition in float64, from the resolved rgb (f32, pt_film_resolve) of the two films: per-tile means, the film's mean, the largest tile error."""
    h, w = a.shape[:2]
    ra = g.resolve(a).astype(np.float64); rb = g.resolve(b).astype(np.float64)
    m = ((ra + rb) / 2).sum(axis=2)
    e = np.abs(ra - rb).sum(axis=2) / np.sqrt(1e-4 + m)
    e[(a[..., 3] == 0) | (b[..., 3] == 0)] = 0.0
    tiles = np.array([[e[y:y + 16, x:x + 16].mean() for x in range(0, w, 16)] for y in range(0, h, 16)])
    return tiles, e.mean(), tiles.max()


@pytest.mark.parametrize("w,h", [(37, 21), (16, 16)])
def test_halves_error(pkg, gpu, any_scene, w, h):
    import torch
    g = any_scene
    a, b = halves(w, h, 100 + w)
    da, db = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0")
    nt = ((w + 15) // 16) * ((h + 15) // 16)
    runs = []
    for _ in range(2):
        tiles = torch.full((nt + 4,), -1.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        mean, worst = g.halves_error(da.data_ptr(), db.data_ptr(), w, h, tiles.data_ptr())
        runs.append((tiles.cpu().numpy(), np.float32(mean), np.float32(worst)))
    (t0, m0, x0), (t1, m1, x1) = runs
    assert np.array_equal(t0.view(np.uint32), t1.view(np.uint32)) and m0.view(np.uint32) == m1.view(np.uint32) and x0.view(np.uint32) == x1.view(np.uint32)
    assert (t0[nt:] == -1.0).all()
    want_tiles, want_mean, want_max = halves_reference(g, a, b)
    print("tiles", t0[:nt], "want", want_tiles.reshape(-1), "mean", m0, want_mean, "max", x0, want_max)
    assert want_mean > 1e-3
    # 5e-5: an f32 sum of <= 256 terms (<= 256 * 2^-24 = 1.5e-5) plus the per-pixel rounding, with a factor of 3
    np.testing.assert_allclose(t0[:nt], want_tiles.reshape(-1), rtol=5e-5, atol=0)
    np.testing.assert_allclose(m0, want_mean, rtol=5e-5, atol=0)
    np.testing.assert_allclose(x0, want_max, rtol=5e-5, atol=0)
    # without a tile array: the same two numbers; a film against itself: exactly 0
    assert g.halves_error(da.data_ptr(), db.data_ptr(), w, h) == (float(m0), float(x0))
    tiles = torch.full((nt,), -1.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert g.halves_error(da.data_ptr(), da.data_ptr(), w, h, tiles.data_ptr()) == (0.0, 0.0)
    assert (tiles.cpu().numpy() == 0.0).all()
    names = {s["name"]: s["kernel"] for s in g.kernel_stats()}
    assert names["film_halves_error"] == "k_film_halves_error" and names["film_error_reduce"] == "k_film_error_reduce"


def test_progressive_driver(pkg, gpu, oracle):
    sd, rp = range_scene(pkg)
    g = pkg.Scene(gpu, sd); orc = oracle.scene(sd)
    steps = []
    film, done = g.render_progressive(rp, 2, on_step=lambda *a: steps.append(a))
    assert done == 8 and [s[0] for s in steps] == [2, 4, 6, 8]
    assert steps[0][1:] == (0.0, 0.0) and all(s[1] > 0.0 and s[2] >= s[1] for s in steps[1:])   # (one half empty: no estimate yet)
    assert_same_film(film, orc.render(rp, nthreads=ORACLE_THREADS))
    # a target the first estimate already meets: the driver stops after the first A / B pair, with the job's first four samples
    steps2 = []
    film2, done2 = g.render_progressive(rp, 2, on_step=lambda *a: steps2.append(a), target_error=steps[1][1] * 2.0)
    assert done2 == 4 and steps2 == steps[:2]
    assert_same_film(film2, g.render(rp, samples=(0, 4)))
    # a target nothing meets: the whole job
    assert g.render_progressive(rp, 3, target_error=0.0)[1] == 8


def test_mi355pbrt_resumes_a_checkpoint_and_refuses_another_jobs(pkg, gpu, tmp_path):
    import subprocess
    from conftest import trace_env
    from test_range_abi import SCENE
    scene = tmp_path / "s.pbrt"; scene.write_text(SCENE)
    run = lambda out, *args: subprocess.run([pkg.frontend.CLI_PATH, str(scene), "--outfile", str(tmp_path / out), "--quiet", *args], capture_output=True, text=True, timeout=120, env=trace_env())
    ck = str(tmp_path / "job.ckpt")
    r = run("half.pfm", "--samples", "0:2", "--checkpoint", ck)
    assert r.returncode == 0, r.stderr
    assert pkg.frontend.read_checkpoint(ck, pkg.frontend.checkpoint_header(pkg.frontend.FrontScene(text=SCENE).render_params()))[0] == 2
    r = run("resumed.pfm", "--checkpoint", ck, "--preview-every", "1")   # samples 2 and 3, one call each, a preview in between
    assert r.returncode == 0, r.stderr
    whole = run("whole.pfm")
    assert whole.returncode == 0, whole.stderr
    a, b = pkg.frontend.read_image(str(tmp_path / "resumed.pfm")), pkg.frontend.read_image(str(tmp_path / "whole.pfm"))
    np.testing.assert_allclose(a, b, rtol=2e-6, atol=1e-7)
    r = run("other.pfm", "--checkpoint", ck, "--spp", "8")
    assert r.returncode == 1 and "not of this job" in r.stderr and not (tmp_path / "other.pfm").exists()
