"""SURVEY §8f-4 (sampler part): HaltonSampler (samplers/halton.rs), the reference's default sampler (api.rs:215-241).
The reference's tests pin only radical_inverse(0, a) (tests/sampling.rs:16-21; its scrambled test asserts nothing), so the
oracle is additionally checked through exact integer properties of the construction; the GPU is bit-exact against it."""
import ctypes as C
import numpy as np
import pytest
from parity import assert_render_matches_oracle


def _samples(fn, A, sb, n_dims, xy, sn, at_center=0):
    out = np.zeros((len(xy), n_dims), np.float32); idx = np.zeros(len(xy), np.uint64)
    st = fn((C.c_int32 * 4)(*sb), at_center, len(xy), xy.ctypes.data_as(A.i32p), sn.ctypes.data_as(A.u32p), n_dims, out.ctypes.data_as(A.fp), idx.ctypes.data_as(A.u64p))
    assert st == 0
    return out, idx


def _digits(n, base, k):
    out = []
    for _ in range(k):
        out.append(n % base); n //= base
    return out


def test_radical_inverse_base2_kat(oracle):
    """tests/sampling.rs:16-21: radical_inverse(0, a) == reverse_bits32(a) * 2^-32 for a < 1024 (exact)."""
    for a in range(1024):
        rev = int("{:032b}".format(a)[::-1], 2)
        assert oracle.lib.orc_radical_inverse_any(0, a) == np.float32(rev) * np.float32(2.3283064365386963e-10)


def test_radical_inverse_other_bases_match_the_definition(oracle):
    primes = [2, 3, 5, 7, 11, 13, 229, 7919]
    idx = {2: 0, 3: 1, 5: 2, 7: 3, 11: 4, 13: 5, 229: 49, 7919: 999}
    for p in primes[1:]:
        for n in (0, 1, 2, p - 1, p, p * p + 1, 1151, 32351, 4363211, 2**31 + 12345, 2**40 + 7):
            d = []
            m = n
            while m: d.append(m % p); m //= p
            exact = sum(di / p ** (i + 1) for i, di in enumerate(d))
            got = oracle.lib.orc_radical_inverse_any(idx[p], n)
            assert abs(got - exact) <= 2e-6 * max(exact, 1e-3), (p, n, got, exact)   # inv_base^k accumulates one rounding per digit


def test_halton_permutations_are_permutations_from_the_default_rng(oracle):
    """compute_radical_inverse_permutations(&mut RNG::default()) (lowdiscrepancy.rs:359-378): base 2's permutation consumes
    the first two PCG32 draws of the default stream, whose first output is the published PCG32 demo value 0x55d93c75... checked
    through the oracle's RNG KAT elsewhere; here: every table entry is a permutation, and the tables are stable."""
    buf = (C.c_uint16 * 8192)()
    first = {}
    for dim in (0, 1, 2, 3, 10, 100, 999):
        p = oracle.lib.orc_halton_permutation(dim, buf)
        perm = np.array(buf[:p])
        assert sorted(perm.tolist()) == list(range(p))
        first[dim] = perm.copy()
    assert oracle.lib.orc_halton_permutation(1, buf) == 3 and np.array_equal(np.array(buf[:3]), first[1])
    assert oracle.lib.orc_halton_permutation(1000, buf) == 0
    assert not np.array_equal(first[100], np.arange(len(first[100])))   # actually shuffled


@pytest.mark.parametrize("sb", [(0, 0, 1920, 1080), (0, 0, 64, 48), (-3, -5, 61, 43), (0, 0, 1, 1)])
def test_halton_index_places_the_sample_in_its_pixel(pkg, oracle, sb):
    """get_index_for_sample (halton.rs:122-155): the low base-2 / base-3 digits of the index, reversed, are the pixel's
    coordinates modulo the 128-pixel tile, and consecutive samples of a pixel are `sample_stride` apart."""
    A = pkg._abi
    rng = np.random.default_rng(7)
    n = 2000
    xy = np.stack([rng.integers(sb[0], sb[2], n), rng.integers(sb[1], sb[3], n)], axis=1).astype(np.int32)
    sn = rng.integers(0, 1 << 16, n).astype(np.uint32)
    out, idx = _samples(oracle.lib.orc_halton_samples, A, sb, 8, xy, sn)
    res = (sb[2] - sb[0], sb[3] - sb[1])
    scale, exp = [1, 1], [0, 0]
    for i, base in enumerate((2, 3)):
        while scale[i] < min(res[i], 128): scale[i] *= base; exp[i] += 1
    stride = scale[0] * scale[1]
    for (x, y), s, ix in zip(xy.tolist(), sn.tolist(), idx.tolist()):
        assert ix // stride == s
        if stride > 1:
            dx = _digits(ix, 2, exp[0]); dy = _digits(ix, 3, exp[1])
            assert sum(d * 2 ** (exp[0] - 1 - k) for k, d in enumerate(dx)) == (x % 128) % scale[0]
            assert sum(d * 3 ** (exp[1] - 1 - k) for k, d in enumerate(dy)) == (y % 128) % scale[1]
    assert (out >= 0).all() and (out[:, 1:] < 1).all() and (out[:, 0] <= 1).all()   # dimension 0 is not clamped (pbrt_macros:101)
    c, _ = _samples(oracle.lib.orc_halton_samples, A, sb, 4, xy, sn, at_center=1)
    assert (c[:, :2] == 0.5).all() and np.array_equal(c[:, 2:], out[:, 2:4])


def test_halton_render_converges_to_the_sobol_render(pkg, oracle):
    b = pkg.scenes.ganesha_scale(n=12, xres=32, yres=24, spp=128)
    sd, rp = b.world_end()
    ref = oracle.scene(sd).render(rp, nthreads=8)
    b.sampler = "halton"
    sd2, rp2 = b.world_end()
    assert rp2.sampler_type == pkg._abi.PT_SAMPLER_HALTON
    hal = oracle.scene(sd2).render(rp2, nthreads=8)
    # dimension 0 is `reverse_bits64(n) as f32 * 2^-64` without a clamp (pbrt_macros:101): it can round to 1.0 and put the
    # sample on the next pixel, so only the total weight is comparable
    assert abs(hal[..., 3].sum() - ref[..., 3].sum()) <= 0.01 * ref[..., 3].sum()
    a, c = ref[..., :3].sum() , hal[..., :3].sum()
    assert abs(a - c) / a < 0.02
    assert np.abs(hal[..., :3] - ref[..., :3]).mean() / ref[..., :3].mean() < 0.15   # different point sets, same integrand
    assert not np.array_equal(hal, ref)


def test_front_end_default_sampler_is_halton(pkg):
    A = pkg._abi
    world = 'WorldBegin\nShape "sphere"\nWorldEnd\n'
    assert pkg.frontend.FrontScene(text=world).render_params().sampler_type == A.PT_SAMPLER_HALTON
    rp = pkg.frontend.FrontScene(text='Sampler "halton" "integer pixelsamples" 4 "bool samplepixelcenter" "true"\n' + world).render_params()
    assert rp.sampler_type == A.PT_SAMPLER_HALTON and rp.spp == 4 and rp.sample_at_pixel_center == 1
    assert pkg.frontend.FrontScene(text='Sampler "sobol"\n' + world).render_params().sampler_type == A.PT_SAMPLER_SOBOL
    with pytest.raises(Exception, match="sampler"):
        pkg.frontend.FrontScene(text='Sampler "stratified"\n' + world)


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
@pytest.mark.parametrize("sb,at_center", [((0, 0, 1920, 1080), 0), ((-3, -5, 61, 43), 0), ((0, 0, 1, 1), 0), ((0, 0, 400, 400), 1)])
def test_gpu_halton_samples_bit_exact(pkg, gpu, oracle, sb, at_center):
    A = pkg._abi
    rng = np.random.default_rng(3)
    n, nd = 4096, 96
    xy = np.stack([rng.integers(sb[0], sb[2], n), rng.integers(sb[1], sb[3], n)], axis=1).astype(np.int32)
    sn = rng.integers(0, 1 << 20, n).astype(np.uint32)
    sn[:64] = rng.integers(1 << 30, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)   # indices beyond 2^32: the 64-bit digit loop
    g = _samples(gpu.lib.pt_halton_samples, A, sb, nd, xy, sn, at_center)
    o = _samples(oracle.lib.orc_halton_samples, A, sb, nd, xy, sn, at_center)
    assert np.array_equal(g[1], o[1])
    assert np.array_equal(g[0].view(np.uint32), o[0].view(np.uint32))
    hi = _samples(gpu.lib.pt_halton_samples, A, sb, 1000, xy[:8], sn[:8], at_center)   # all 1000 dimensions
    ho = _samples(oracle.lib.orc_halton_samples, A, sb, 1000, xy[:8], sn[:8], at_center)
    assert np.array_equal(hi[0].view(np.uint32), ho[0].view(np.uint32))


def _halton(b):
    b.sampler = "halton"
    return b.world_end()


@pytest.mark.gpu
def test_gpu_halton_render_matches_oracle(pkg, gpu, oracle):
    S = pkg.scenes
    assert_render_matches_oracle(pkg, gpu, oracle, *_halton(S.ganesha_scale(n=24, xres=64, yres=48, spp=8)))
    assert_render_matches_oracle(pkg, gpu, oracle, *_halton(S.material_zoo(xres=64, yres=48, spp=8)))
    assert_render_matches_oracle(pkg, gpu, oracle, *_halton(S.spheres_c1(xres=48, yres=48, spp=8)))


@pytest.mark.gpu
def test_gpu_halton_with_textures_thin_lens_and_subsurface(pkg, gpu, oracle):
    S = pkg.scenes
    b = S.textured(xres=64, yres=48, spp=4, trilinear=False)
    b.cam.update(lensradius=0.05, focaldistance=4.0)   # lens sample re-derived for the camera-ray differentials
    assert_render_matches_oracle(pkg, gpu, oracle, *_halton(b), rtol=2e-5, atol=1e-6)
    # probe chains: the device's re-walk of a long chain is left out of its counters (see test_gpu_parity)
    assert_render_matches_oracle(pkg, gpu, oracle, *_halton(S.subsurface_c5(xres=48, yres=32, spp=4)), resolved=None)
    b = S.ganesha_scale(n=16, xres=48, yres=32, spp=4); b.sample_at_pixel_center = True
    assert_render_matches_oracle(pkg, gpu, oracle, *_halton(b))


@pytest.mark.gpu
def test_gpu_default_sampler_scene_file(pkg, gpu, oracle):
    """A .pbrt file that names no sampler renders with Halton, 16 spp (api.rs:215-241, halton.rs:226-236)."""
    text = '''LookAt 0 1.5 5  0 0.3 0  0 1 0
Camera "perspective" "float fov" 35
Film "image" "integer xresolution" 48 "integer yresolution" 32
WorldBegin
LightSource "distant" "point from" [2 8 3] "rgb L" [3 3 3]
Material "matte" "rgb Kd" [.5 .4 .3]
Shape "sphere" "float radius" 1
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-5 -1 -5  -5 -1 5  5 -1 5  5 -1 -5]
WorldEnd
'''
    fs = pkg.frontend.FrontScene(text=text)
    rp = fs.render_params()
    assert rp.sampler_type == pkg._abi.PT_SAMPLER_HALTON and rp.spp == 16
    assert_render_matches_oracle(pkg, gpu, oracle, fs, rp, resolved=None)
