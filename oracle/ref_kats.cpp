// ORACLE -- TEST INFRASTRUCTURE ONLY (see ref_math.h header).
// ref_kats.cpp: the reference's own test loops for code this oracle restates, run in C++ for speed and reported to
// tests/test_oracle_kats.py:  tests/fp.rs:125-226 (EFloat abs / sqrt / add / sub / mul / div containment, 10^6 seeds each),
// tests/fp.rs:46-57 (float_bits), tests/bitops.rs:7-64 (log2_int, round_up_pow2), tests/sampling.rs:24-97 (scrambled radical inverse,
// generator matrices, Gray-code samples), tests/hg.rs (HenyeyGreenstein::p / sample_p); then the function probes that
// tests/test_oracle_kats.py and tests/test_oracle_bsdf.py call per query: Sobol / Halton / radical inverse, next_float, find_interval,
// PCG32, Distribution1D, the deterministic math, offset_ray_origin, the BSSRDF tables, light sample_li / pdf_li, a material's BSDF and (for
// tests/test_bssrdf_probe.py and tests/test_bssrdf_zoo.py) a material's BSSRDF, section by section.
#include "ref_efloat.h"
#include "ref_bssrdf.h"
#include <cmath>

namespace {
using namespace ref;
EFloat get_efloat(RNG &rng, Float min_exp = -6.0f, Float max_exp = 6.0f) {   // tests/fp.rs:73-98
    const Float t = rng.uniform_float();
    const Float logu = min_exp * (1.0f - t) + max_exp * t;   // lerp (pbrt.rs:136-144)
    const Float val = std::pow(10.0f, logu);
    Float err = 0.0f;
    switch (rng.uniform_u32_bounded(4)) {
    case 1: { const uint32_t ulp = rng.uniform_u32_bounded(1024); err = std::fabs(bits_to_float(float_to_bits(val) + ulp) - val); break; }
    case 2: { const uint32_t ulp = rng.uniform_u32_bounded(1024 * 1024); err = std::fabs(bits_to_float(float_to_bits(val) + ulp) - val); break; }
    case 3: err = (4.0f * rng.uniform_float()) * std::fabs(val); break;
    default: break;
    }
    const Float sign = rng.uniform_float() < 0.5f ? -1.0f : 1.0f;
    return EFloat(sign * val, err);
}
double get_precise(const EFloat &ef, RNG &rng) {   // tests/fp.rs:100-114
    switch (rng.uniform_u32_bounded(3)) {
    case 0: return (double)ef.low;
    case 1: return (double)ef.high;
    default: {
        const Float t = rng.uniform_float();
        double p = (1.0 - (double)t) * (double)ef.low + (double)t * (double)ef.high;
        if (p > (double)ef.high) p = (double)ef.high;
        if (p < (double)ef.low) p = (double)ef.low;
        return p;
    }
    }
}
inline Float abs_err(const EFloat &e) { return next_float_up(fmax_(std::fabs(e.high - e.v), std::fabs(e.v - e.low))); }   // efloat.rs get_absolute_error
void kat_bssrdf(const PtBSSRDFTable *t, const float *sigma_a, const float *sigma_s, float eta, BssrdfTable &tb, TabulatedBSSRDF &b) {
    tb.n_rho = (int)t->n_rho; tb.n_radius = (int)t->n_radius;
    tb.rho_samples.assign(t->rho_samples, t->rho_samples + t->n_rho); tb.radius_samples.assign(t->radius_samples, t->radius_samples + t->n_radius);
    tb.profile.assign(t->profile, t->profile + (size_t)t->n_rho * t->n_radius); tb.rhoeff.assign(t->rhoeff, t->rhoeff + t->n_rho);
    tb.profile_cdf.assign(t->profile_cdf, t->profile_cdf + (size_t)t->n_rho * t->n_radius);
    SurfaceInteraction si; si.p = V3(0, 0, 0); si.n = V3(0, 0, 1); si.sh_n = V3(0, 0, 1); si.sh_dpdu = V3(1, 0, 0);
    b.init(si, 0, eta, RGB(sigma_a[0], sigma_a[1], sigma_a[2]), RGB(sigma_s[0], sigma_s[1], sigma_s[2]), &tb);
}
}  // namespace

extern "C" {
// op: 0 abs, 1 sqrt, 2 add, 3 sub, 4 mul, 5 div (tests/fp.rs:125-226). Returns the number of containment violations over
// trials 0..iters-1 (the reference runs 1 000 000); *n_tested = trials not skipped by the test's own preconditions.
int orc_test_efloat(int op, int iters, int *n_tested) {
    int failures = 0, tested = 0;
    for (int trial = 0; trial < iters; ++trial) {
        RNG rng((uint64_t)trial);
        if (op <= 1) {
            const EFloat ef = get_efloat(rng);
            const double precise = get_precise(ef, rng);
            if (op == 1 && abs_err(ef) > 0.25f * std::fabs(ef.low)) continue;
            const EFloat r = op == 0 ? efloat_abs(ef) : efloat_sqrt(efloat_abs(ef));
            const double pr = op == 0 ? std::fabs(precise) : std::sqrt(std::fabs(precise));
            ++tested;
            if (!(pr >= (double)r.low && pr <= (double)r.high)) ++failures;
        } else {
            const EFloat e0 = get_efloat(rng), e1 = get_efloat(rng);
            const double p0 = get_precise(e0, rng), p1 = get_precise(e1, rng);
            if (op == 5 && (e1.low * e1.high < 0.0f || abs_err(e1) > 0.25f * std::fabs(e1.low))) continue;
            const EFloat r = op == 2 ? e0 + e1 : op == 3 ? e0 - e1 : op == 4 ? e0 * e1 : e0 / e1;
            const double pr = op == 2 ? p0 + p1 : op == 3 ? p0 - p1 : op == 4 ? p0 * p1 : p0 / p1;
            ++tested;
            if (!(pr >= (double)r.low && pr <= (double)r.high)) ++failures;
        }
    }
    if (n_tested) *n_tested = tested;
    return failures;
}

// tests/fp.rs:46-57 float_bits: RNG::new(1), `iters` (the reference: 100 000) draws ui; f = bits_to_float(ui); NaNs skipped; float_to_bits(f) == ui -- on
// ref_math.h's float_to_bits / bits_to_float (pbrt.rs:57-78), the pair under next_float_up / next_float_down and offset_ray_origin.
// Returns the number of mismatches; *n_tested = the draws that were not NaN.
int orc_test_float_bits(int iters, int *n_tested) {
    RNG rng(1);
    int failures = 0, tested = 0;
    for (int i = 0; i < iters; ++i) {
        const uint32_t ui = rng.uniform_u32();
        const Float f = ref::bits_to_float(ui);
        if (f != f) continue;
        ++tested;
        if (ref::float_to_bits(f) != ui) ++failures;
    }
    if (n_tested) *n_tested = tested;
    return failures;
}

// tests/sampling.rs:24-53 scrambled_radical_inverse_test: for dim < n_dims (the reference: 128), RNG::new(dim), base = PRIMES[dim], the permutation base-1 .. 0 shuffled by
// `shuffle(&mut perm, len, 1, &mut rng)` (sampling.rs:178-186), and the seven indices of the test. The Rust file compares scrambled_radical_inverse with a hand-rolled
// digit loop through a `relative_eq!` whose result it DROPS -- and the hand-rolled loop is broken (`val *= ..` on a zero, `n *= inv_base as u32`): it computes no reference
// value at all. The twin compares the oracle's scrambled_radical_inverse_base (ref_sampler.h, lowdiscrepancy.rs:469-484: what HaltonSampler::sample_dimension calls) with
// the value the radical inverse HAS -- sum_i perm[d_i] b^-(i+1) over the index's digits plus perm[0] for every digit beyond them (perm[0] b^-k / (b - 1)), in exact
// rational arithmetic carried in long double -- to the test's epsilon 1e-5 (relative). Returns the number of violations; *worst = largest relative deviation.
int orc_test_scrambled_radical_inverse(int n_dims, double *worst) {
    const HaltonTables &T = halton_tables();
    static const uint32_t indices[7] = {0u, 1u, 2u, 1151u, 32351u, 4363211u, 681122u};
    int failures = 0; double w = 0.0;
    for (int dim = 0; dim < n_dims; ++dim) {
        RNG rng((uint64_t)dim);
        const uint32_t base = T.primes[dim];
        std::vector<uint16_t> perm(base);
        for (uint32_t i = 0; i < base; ++i) perm[i] = (uint16_t)(base - 1 - i);
        for (uint32_t i = 0; i < base; ++i) { const uint32_t other = i + rng.uniform_u32_bounded(base - i); std::swap(perm[i], perm[other]); }
        for (uint32_t index : indices) {
            long double val = 0.0L, scale = 1.0L / (long double)base; uint32_t n = index;
            while (n > 0) { val += (long double)perm[n % base] * scale; scale /= (long double)base; n /= base; }
            val += (long double)perm[0] * scale * (long double)base / ((long double)base - 1.0L);   // perm[0] * sum_{j >= k+1} b^-j
            const double got = (double)scrambled_radical_inverse_base(base, perm.data(), index);
            const double want = (double)(val < 0.99999994L ? val : 0.99999994L);   // min(.., ONE_MINUS_EPSILON) as the function clamps
            const double rel = std::fabs(got - want) / std::fmax(std::fmax(std::fabs(got), std::fabs(want)), 1e-30);
            if (rel > w) w = rel;
            if (!(rel <= 1.0e-5)) ++failures;
        }
    }
    if (worst) *worst = w;
    return failures;
}

// tests/bitops.rs:7-64 on the oracle's log2_int / round_up_pow2_32 (ref_sampler.h: SobolSampler::new and the MIPMap resampler use
// them); the i64 variants of the reference are the same bit tricks on 64 bits and are restated here only for the test.
int orc_test_bitops(void) {
    int failures = 0;
    auto log2_int64 = [](int64_t v) { return (int64_t)(63 - __builtin_clzll((uint64_t)v)); };
    auto round_up_pow2_64 = [](int64_t v) { v--; v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16; v |= v >> 32; return v + 1; };
    for (int i = 0; i < 32; ++i) { const uint32_t ui = 1u << i; failures += log2_int(ui) != i; failures += log2_int64((int64_t)ui) != i; }
    for (int i = 1; i < 32; ++i) { const uint32_t ui = 1u << i; failures += log2_int(ui + 1u) != i; failures += log2_int64((int64_t)ui + 1) != i; }
    for (int i = 0; i < 64; ++i) failures += log2_int64((int64_t)(1ull << i)) != i;
    for (int i = 1; i < 64; ++i) failures += log2_int64((int64_t)(1ull << i) + 1) != i;
    failures += round_up_pow2_32(7) != 8u;
    for (int32_t i = 1; i < (1 << 24); ++i) {
        const bool p2 = i > 0 && !((i & (i - 1)) > 0);
        if (p2) failures += round_up_pow2_32(i) != (uint32_t)i; else failures += round_up_pow2_32(i) != (1u << (log2_int((uint32_t)i) + 1));
        if (p2) failures += round_up_pow2_64(i) != i; else failures += round_up_pow2_64(i) != ((int64_t)1 << (log2_int64(i) + 1));
    }
    for (int i = 0; i < 30; ++i) {
        const int32_t v = 1 << i;
        failures += round_up_pow2_32(v) != (uint32_t)v;
        if (v > 2) failures += round_up_pow2_32(v - 1) != (uint32_t)v;
        failures += round_up_pow2_32(v + 1) != (uint32_t)(2 * v);
    }
    return failures;
}

// tests/sampling.rs:55-83 generator_matrix + :85-97 gray_code_sample_test on multiply_generator (lowdiscrepancy.rs:428-440, the
// column-XOR loop behind sobol_sample_float); reverse_bits32 / sample_generator_matrix / gray_code_sample1d restated next to it.
int orc_test_generator_matrix(void) {
    auto reverse_bits32 = [](uint32_t n) {   // lowdiscrepancy.rs:382-390
        n = (n << 16) | (n >> 16);
        n = ((n & 0x00ff00ffu) << 8) | ((n & 0xff00ff00u) >> 8);
        n = ((n & 0x0f0f0f0fu) << 4) | ((n & 0xf0f0f0f0u) >> 4);
        n = ((n & 0x33333333u) << 2) | ((n & 0xccccccccu) >> 2);
        n = ((n & 0x55555555u) << 1) | ((n & 0xaaaaaaaau) >> 1);
        return n;
    };
    auto sample_generator_matrix = [](const uint32_t *C, uint32_t a, uint32_t scramble) { return fmin_((Float)(multiply_generator(C, a) ^ scramble) * 0x1.0p-32f, ONE_MINUS_EPSILON); };
    int failures = 0;
    uint32_t c[32], crev[32];
    for (int i = 0; i < 32; ++i) { c[i] = 1u << i; crev[i] = reverse_bits32(c[i]); }
    for (uint32_t a = 0; a < 128; ++a) {
        failures += multiply_generator(c, a) != a;
        failures += radical_inverse_base(2, a) != (Float)reverse_bits32(multiply_generator(c, a)) * 2.3283064365386963e-10f;
        failures += radical_inverse_base(2, a) != sample_generator_matrix(crev, a, 0);
    }
    RNG rng;   // RNG::default()
    for (int i = 0; i < 32; ++i) { c[i] = rng.uniform_u32(); crev[i] = reverse_bits32(c[i]); }
    for (uint32_t a = 0; a < 1024; ++a) failures += reverse_bits32(multiply_generator(c, a)) != multiply_generator(crev, a);
    // gray_code_sample_test: the 64 Gray-code samples of the identity matrix are the 64 values multiply_generator produces
    for (int i = 0; i < 32; ++i) c[i] = 1u << i;
    Float v[64]; uint32_t acc = 0;
    for (int i = 0; i < 64; ++i) { v[i] = fmin_((Float)acc * 0x1.0p-32f, ONE_MINUS_EPSILON); acc ^= c[__builtin_ctz((uint32_t)(i + 1))]; }   // lowdiscrepancy.rs:444-451
    for (uint32_t a = 0; a < 64; ++a) {
        const Float u = (Float)multiply_generator(c, a) * 2.3283064365386963e-10f;
        bool found = false; for (int i = 0; i < 64; ++i) found = found || v[i] == u;
        failures += !found;
    }
    return failures;
}

// ---- tests/hg.rs restated (the reference's assertions on HenyeyGreenstein::p / sample_p, medium.rs:149-193), run inside the oracle ----
// tests/hg.rs:12-32 sampling_match: RNG::default(), g = -0.75 .. 0.75 step 0.25, 100 samples each; returns max |p0 - p(wo, wi)| / p
double orc_test_hg_sampling_match(void) {
    RNG rng;   // RNG::default()
    double worst = 0.0;
    for (Float g = -0.75f; g <= 0.75f; g += 0.25f)
        for (int i = 0; i < 100; ++i) {
            const Float a = rng.uniform_float(), b = rng.uniform_float();
            const V3 wo = uniform_sample_sphere(P2(a, b));
            V3 wi;
            const Float u0 = rng.uniform_float(), u1 = rng.uniform_float();
            const Float p0 = hg_sample_p(g, wo, wi, P2(u0, u1));
            const Float p1 = phase_hg(dot(wo, wi), g);
            worst = std::max(worst, (double)std::fabs(p0 - p1) / (double)std::fabs(p1));
        }
    return worst;
}
// tests/hg.rs:34-79 sampling_orientation_forward / sample_orientation_backward: wo = (-1, 0, 0), 100 samples, counts wi.x > 0
void orc_test_hg_orientation(float g, int *nforward, int *nbackward) {
    RNG rng;   // RNG::default()
    *nforward = *nbackward = 0;
    for (int i = 0; i < 100; ++i) {
        const Float u0 = rng.uniform_float(), u1 = rng.uniform_float();
        V3 wi;
        hg_sample_p(g, V3(-1.0f, 0.0f, 0.0f), wi, P2(u0, u1));
        if (wi.x > 0.0f) ++*nforward; else ++*nbackward;
    }
}
// tests/hg.rs:81-103 normalized: per g, the mean of p(wo, wi) over 100 000 uniform directions (expected 1 / 4 pi)
void orc_test_hg_normalized(double *means7) {
    RNG rng;   // RNG::default()
    int k = 0;
    for (Float g = -0.75f; g <= 0.75f; g += 0.25f, ++k) {
        const Float a = rng.uniform_float(), b = rng.uniform_float();
        const V3 wo = uniform_sample_sphere(P2(a, b));
        Float sum = 0.0f;
        const int n = 100000;
        for (int i = 0; i < n; ++i) { const Float c = rng.uniform_float(), d = rng.uniform_float(); sum += phase_hg(dot(wo, uniform_sample_sphere(P2(c, d))), g); }
        means7[k] = (double)(sum / (Float)n);
    }
}

// ---- function probes: oracle functions called once per query by the known-answer tests of tests/test_oracle_kats.py and tests/test_oracle_bsdf.py ----
float orc_sobol_sample_float(uint64_t index, int dim, uint32_t scramble) { return sobol_sample_float(index, dim, scramble); }
float orc_radical_inverse(int base_index, uint64_t n) { return radical_inverse(base_index, n); }
// radical_inverse(base_index, n) (pbrt_macros:92-111) and the Halton digit permutation of a dimension
float orc_radical_inverse_any(uint32_t base_index, uint64_t n) {
    if (base_index == 0) return (float)reverse_bits64_h(n) * 0x1.0p-64f;
    return radical_inverse_base(halton_tables().primes[base_index], n);
}
uint32_t orc_halton_permutation(uint32_t dim, uint16_t *out) {
    const HaltonTables &T = halton_tables();
    if (dim >= 1000) return 0;
    for (uint32_t j = 0; j < T.primes[dim]; ++j) out[j] = T.perm[T.sums[dim] + j];
    return T.primes[dim];
}
float orc_next_float_up(float v) { return next_float_up(v); }
float orc_next_float_down(float v) { return next_float_down(v); }
int orc_find_interval(int size, const float *a, float x) { return find_interval(size, [&](int i) { return a[i] <= x; }); }
uint32_t orc_rng_u32_stream(uint64_t seq, int use_default, uint32_t n, uint32_t *out, float *outf) {
    RNG r = use_default ? RNG() : RNG(seq);
    for (uint32_t i = 0; i < n; ++i) { if (out) out[i] = r.uniform_u32(); else outf[i] = r.uniform_float(); }
    return n;
}
// Distribution1D (tests/sampling.rs:202-257)
int orc_dist1d_sample_discrete(const float *func, int n, float u, float *pdf, float *uremapped) {
    Distribution1D d(std::vector<Float>(func, func + n));
    return (int)d.sample_discrete(u, pdf, uremapped);
}
float orc_dist1d_discrete_pdf(const float *func, int n, int index) { return Distribution1D(std::vector<Float>(func, func + n)).discrete_pdf((size_t)index); }
float orc_dist1d_sample_continuous(const float *func, int n, float u, float *pdf, int *offset) {   // Distribution1D::sample_continous (sampling.rs:38-64); pdf / offset may be null like the reference's Options
    size_t off = 0;
    const float x = Distribution1D(std::vector<Float>(func, func + n)).sample_continuous(u, pdf, &off);
    if (offset) *offset = (int)off;
    return x;
}
// deterministic math
float orc_dm_sin(float x) { return dm_sinf(x); }
float orc_dm_cos(float x) { return dm_cosf(x); }
float orc_dm_acos(float x) { return dm_acosf(x); }
float orc_dm_atan2(float y, float x) { return dm_atan2f(y, x); }
float orc_dm_log(float x) { return dm_logf(x); }
void orc_offset_ray_origin(const float *p, const float *perr, const float *n, const float *w, float *out) {
    V3 r = offset_ray_origin(V3(p[0], p[1], p[2]), V3(perr[0], perr[1], perr[2]), V3(n[0], n[1], n[2]), V3(w[0], w[1], w[2]));
    out[0] = r.x; out[1] = r.y; out[2] = r.z;
}
// BSSRDF restatement: Sr(r) and pdf_sr(ch, r) for n radii
int orc_bssrdf_sr(const PtBSSRDFTable *t, const float *sigma_a, const float *sigma_s, float eta, uint32_t n, const float *r, float *sr3, float *pdf3) {
    BssrdfTable tb; TabulatedBSSRDF b; kat_bssrdf(t, sigma_a, sigma_s, eta, tb, b);
    for (uint32_t i = 0; i < n; ++i) {
        RGB s = b.sr(r[i]);
        for (int c = 0; c < 3; ++c) { sr3[3 * i + c] = s.c[c]; pdf3[3 * i + c] = b.pdf_sr(c, r[i]); }
    }
    return 0;
}
int orc_bssrdf_sample_sr(const PtBSSRDFTable *t, const float *sigma_a, const float *sigma_s, float eta, int ch, uint32_t n, const float *u, float *r) {
    BssrdfTable tb; TabulatedBSSRDF b; kat_bssrdf(t, sigma_a, sigma_s, eta, tb, b);
    for (uint32_t i = 0; i < n; ++i) r[i] = b.sample_sr(ch, u[i]);
    return 0;
}
int orc_catmull_rom_weights(int size, const float *nodes, float x, int *offset, float *w4) {
    return catmull_rom_weights(size, nodes, x, *offset, w4) ? 1 : 0;
}
float orc_bssrdf_sw(float eta, float cos_theta_) { return bssrdf_sw(eta, V3(std::sqrt(fmax_(0.0f, 1.0f - cos_theta_ * cos_theta_)), 0.0f, cos_theta_)); }
// light sampling: sample_li for n sample points u (2n floats) from the reference point (p, p_error, n); outputs wi (3n), pdf (n), L (3n)
int orc_light_sample_li(orc_scene *h, uint32_t li, const float *p, const float *perr, const float *nrm, uint32_t n, const float *u,
                        float *wi_out, float *pdf_out, float *L_out) {
    LightSampler ls; ls.init(h->scene, PT_LS_UNIFORM);
    IData ref; ref.p = V3(p[0], p[1], p[2]); ref.p_error = V3(perr[0], perr[1], perr[2]); ref.n = V3(nrm[0], nrm[1], nrm[2]);
    for (uint32_t i = 0; i < n; ++i) {
        V3 wi(0, 0, 0); Float pdf = 0.0f; IData p1;
        RGB L = ls.sample_li(li, ref, P2(u[2 * i], u[2 * i + 1]), wi, pdf, p1);
        wi_out[3 * i] = wi.x; wi_out[3 * i + 1] = wi.y; wi_out[3 * i + 2] = wi.z; pdf_out[i] = pdf;
        for (int c = 0; c < 3; ++c) L_out[3 * i + c] = L.c[c];
    }
    return 0;
}
int orc_light_pdf_li(orc_scene *h, uint32_t li, const float *p, const float *perr, const float *nrm, uint32_t n, const float *wi, float *pdf_out) {
    LightSampler ls; ls.init(h->scene, PT_LS_UNIFORM);
    IData ref; ref.p = V3(p[0], p[1], p[2]); ref.p_error = V3(perr[0], perr[1], perr[2]); ref.n = V3(nrm[0], nrm[1], nrm[2]);
    for (uint32_t i = 0; i < n; ++i) pdf_out[i] = ls.pdf_li(li, ref, V3(wi[3 * i], wi[3 * i + 1], wi[3 * i + 2]));
    return 0;
}
// BSDF of a material at a canonical interaction, for the analytic lobe checks of tests/test_oracle_bsdf.py.
// The material `mi` is evaluated as Material::compute_scattering_functions would at a point with geometric and shading normal +z, dpdu = +x,
// dpdv = +y, no textures; then for each of n queries: f(wo, wi) and pdf(wo, wi) over all lobes (reflection.rs:1541-1600), and sample_f(wo, u)
// (reflection.rs:1602-1689) -> sampled wi, its f, pdf and lobe type. Directions are world = local here.
int orc_bsdf_eval(orc_scene *h, uint32_t mi, uint32_t n, const float *wo, const float *wi, const float *u,
                  float *f_out, float *pdf_out, float *s_wi_out, float *s_f_out, float *s_pdf_out, int32_t *s_type_out, int32_t *n_lobes_out) {
    if (mi >= h->scene.materials.size()) return 1;
    SurfaceInteraction si{};
    si.p = V3(0, 0, 0); si.p_error = V3(0, 0, 0); si.n = V3(0, 0, 1); si.sh_n = V3(0, 0, 1); si.wo = V3(0, 0, 1);
    si.dpdu = V3(1, 0, 0); si.dpdv = V3(0, 1, 0); si.sh_dpdu = V3(1, 0, 0); si.sh_dpdv = V3(0, 1, 0);
    si.uv = P2(0.5f, 0.5f); si.has_shape = false; si.shape_flip = false; si.prim = 0;
    BSDF bsdf;
    if (!scattering_functions_of(h->scene, mi, si, bsdf, nullptr, nullptr, nullptr)) return 2;   // (mix materials included)
    if (n_lobes_out) *n_lobes_out = bsdf.n;
    for (uint32_t i = 0; i < n; ++i) {
        const V3 o(wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]);
        if (wi && f_out && pdf_out) {
            const V3 w(wi[3 * i], wi[3 * i + 1], wi[3 * i + 2]);
            const RGB f = bsdf.f(o, w, BSDF_ALL);
            for (int c = 0; c < 3; ++c) f_out[3 * i + c] = f.c[c];
            pdf_out[i] = bsdf.pdf(o, w, BSDF_ALL);
        }
        if (u && s_wi_out && s_f_out && s_pdf_out) {
            V3 w(0, 0, 0); Float pdf = 0.0f; int sampled = 0;
            const RGB f = bsdf.sample_f(o, w, P2(u[2 * i], u[2 * i + 1]), pdf, BSDF_ALL, sampled);
            s_wi_out[3 * i] = w.x; s_wi_out[3 * i + 1] = w.y; s_wi_out[3 * i + 2] = w.z; s_pdf_out[i] = pdf;
            for (int c = 0; c < 3; ++c) s_f_out[3 * i + c] = f.c[c];
            if (s_type_out) s_type_out[i] = sampled;
        }
    }
    return 0;
}

// A material's BSSRDF, call by call, for tests/test_bssrdf_probe.py (the device's dev_bssrdf.h answers the same words) and tests/test_bssrdf_zoo.py.
// scattering_functions_of(material mi) at the interaction `frame` gives (15 floats: p, n, sh_n, sh_dpdu, sh_dpdv; uv = (0.5, 0.5), no shape, no textures);
// status 1: a bad argument, 2: the material leaves no BSSRDF there -- nothing is written in either case. Every section is optional: a null output (or a
// count of zero) skips it. Words are floats unless said otherwise.
//   state (19):          sigma_t.rgb, rho.rgb (DisneyBSSRDF: d.rgb, R.rgb), eta, ns, ss, ts, po_p
//   radii (6 per r):     sr(r).rgb, pdf_sr(ch, r) for ch = 0, 1, 2
//   samples (3 per u):   sample_sr(ch, u) for ch = 0, 1, 2
//   exits (4 per point): pdf_sp(pi_p, pi_n), sr(length(po_p - pi_p)).rgb  -- in: 6 floats (pi_p, pi_n); the two values subsurface_step takes
//   segments (8 per):    probe_segment's boolean (a uint32), start, target, u1n -- in: 3 floats (u1, u2.x, u2.y); start / target stay 0 where it returns false
//   adapter (12 per):    f.rgb, pdf, sample_f's wi, f.rgb, pdf and sampled type (an int32) of BSDF(pi, 1.0) with the one BX_BSSRDF lobe, built as subsurface_step
//                        builds it, at the exit interaction `exit_frame` (15 floats as `frame`) -- in: 8 floats (wo, wi, u) and one int32 of flags; pdf and wi are 0 on entry
//   conversion (6 per):  subsurface_from_diffuse(kd, mfp) on the material's table: sigma_a.rgb, sigma_s.rgb -- in: 6 floats; a tabulated material only (else status 1)
static SurfaceInteraction bssrdf_probe_interaction(const float *f) {
    SurfaceInteraction si{};
    si.p = V3(f[0], f[1], f[2]); si.p_error = V3(0, 0, 0); si.n = V3(f[3], f[4], f[5]); si.sh_n = V3(f[6], f[7], f[8]); si.wo = si.sh_n;
    si.sh_dpdu = V3(f[9], f[10], f[11]); si.sh_dpdv = V3(f[12], f[13], f[14]); si.dpdu = si.sh_dpdu; si.dpdv = si.sh_dpdv;
    si.uv = P2(0.5f, 0.5f); si.has_shape = false; si.shape_flip = false; si.prim = 0;
    return si;
}
int orc_bssrdf_eval(orc_scene *h, uint32_t mi, const float *frame, float *state,
                    uint32_t n_r, const float *r, float *r_out, uint32_t n_u, const float *u, float *u_out,
                    uint32_t n_x, const float *x, float *x_out, uint32_t n_s, const float *s, uint32_t *s_out,
                    const float *exit_frame, uint32_t n_a, const float *a, const int32_t *a_flags, uint32_t *a_out,
                    uint32_t n_c, const float *c, float *c_out) {
    if (!h || !frame || mi >= h->scene.materials.size()) return 1;
    if ((n_r && r_out && !r) || (n_u && u_out && !u) || (n_x && x_out && !x) || (n_s && s_out && !s) || (n_a && a_out && (!a || !a_flags || !exit_frame)) || (n_c && c_out && !c)) return 1;
    SurfaceInteraction si = bssrdf_probe_interaction(frame);
    BSDF bsdf; TabulatedBSSRDF b; bool has = false;
    if (!scattering_functions_of(h->scene, mi, si, bsdf, &b, &has, nullptr) || !has) return 2;
    if (n_c && c_out && b.disney) return 1;
    auto put3 = [](float *o, V3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; };
    auto word = [](Float v) { return float_to_bits(v); };
    if (state) {
        for (int k = 0; k < 3; ++k) { state[k] = b.disney ? b.dD.c[k] : b.sigma_t.c[k]; state[3 + k] = b.disney ? b.dR.c[k] : b.rho.c[k]; }
        state[6] = b.eta; put3(state + 7, b.ns); put3(state + 10, b.ss); put3(state + 13, b.ts); put3(state + 16, b.po_p);
    }
    if (r_out) for (uint32_t i = 0; i < n_r; ++i) {
        const RGB v = b.sr(r[i]);
        for (int k = 0; k < 3; ++k) { r_out[6 * i + k] = v.c[k]; r_out[6 * i + 3 + k] = b.pdf_sr(k, r[i]); }
    }
    if (u_out) for (uint32_t i = 0; i < n_u; ++i) for (int k = 0; k < 3; ++k) u_out[3 * i + k] = b.sample_sr(k, u[i]);
    if (x_out) for (uint32_t i = 0; i < n_x; ++i) {
        const V3 pp(x[6 * i], x[6 * i + 1], x[6 * i + 2]), pn(x[6 * i + 3], x[6 * i + 4], x[6 * i + 5]);
        x_out[4 * i] = b.pdf_sp(pp, pn);
        const RGB v = b.sr(length(b.po_p - pp));
        for (int k = 0; k < 3; ++k) x_out[4 * i + 1 + k] = v.c[k];
    }
    if (s_out) for (uint32_t i = 0; i < n_s; ++i) {
        V3 start(0, 0, 0), target(0, 0, 0); Float u1n = 0.0f;
        const bool ok = b.probe_segment(s[3 * i], P2(s[3 * i + 1], s[3 * i + 2]), start, target, u1n);
        uint32_t *o = s_out + 8 * (size_t)i;
        o[0] = ok ? 1u : 0u; o[1] = word(start.x); o[2] = word(start.y); o[3] = word(start.z);
        o[4] = word(target.x); o[5] = word(target.y); o[6] = word(target.z); o[7] = word(u1n);
    }
    if (a_out && n_a) {
        SurfaceInteraction pi = bssrdf_probe_interaction(exit_frame);
        BSDF pibsdf; pibsdf.init(pi, 1.0f);   // ref_render.cpp subsurface_step: sample_s (bssrdf.rs:559-574)
        { Bxdf bx; bx.kind = BX_BSSRDF; bx.type = BSDF_REFLECTION | BSDF_DIFFUSE; bx.etab = b.eta; pibsdf.add(bx); }
        for (uint32_t i = 0; i < n_a; ++i) {
            const float *q = a + 8 * (size_t)i;
            const V3 wo(q[0], q[1], q[2]), wi(q[3], q[4], q[5]);
            const RGB f = pibsdf.f(wo, wi, a_flags[i]);
            const Float pdf = pibsdf.pdf(wo, wi, a_flags[i]);
            V3 w(0, 0, 0); Float spdf = 0.0f; int sampled = 0;
            const RGB sf = pibsdf.sample_f(wo, w, P2(q[6], q[7]), spdf, a_flags[i], sampled);
            uint32_t *o = a_out + 12 * (size_t)i;
            o[0] = word(f.c[0]); o[1] = word(f.c[1]); o[2] = word(f.c[2]); o[3] = word(pdf);
            o[4] = word(w.x); o[5] = word(w.y); o[6] = word(w.z); o[7] = word(sf.c[0]); o[8] = word(sf.c[1]); o[9] = word(sf.c[2]); o[10] = word(spdf); o[11] = (uint32_t)sampled;
        }
    }
    if (c_out) for (uint32_t i = 0; i < n_c; ++i) {
        RGB sa(0.0f), ss(0.0f);
        subsurface_from_diffuse(*b.table, RGB(c[6 * i], c[6 * i + 1], c[6 * i + 2]), RGB(c[6 * i + 3], c[6 * i + 4], c[6 * i + 5]), sa, ss);
        for (int k = 0; k < 3; ++k) { c_out[6 * i + k] = sa.c[k]; c_out[6 * i + 3 + k] = ss.c[k]; }
    }
    return 0;
}
}  // extern "C"
