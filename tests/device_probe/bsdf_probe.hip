// bsdf_probe.hip -- TEST CODE (tests/test_device_probe.py builds it; it is no part of libmi355pt.so): one thread per query calls the device's
// Bsdf<MAXL, DIFF>::f / pdf / f_pdf / sample_f (dev_bsdf.h) on the BSDF that build_bsdf makes of one material of the scene's own material table, at the
// canonical interaction of the oracle's orc_bsdf_eval (oracle/ref_kats.cpp): n = sh_n = +z, dpdu = +x, dpdv = +y, uv = (0.5, 0.5), no shape.
// Compiled with the HIPFLAGS of ../../pbrt-rust_amd/csrc/Makefile (+ -fvisibility=hidden) against the unmodified headers, in the nine (MAXL, DIFF)
// instantiations the shade kernels use (tu_shade.hip).
#include "../../pbrt-rust_amd/csrc/host_common.h"
#include "../../pbrt-rust_amd/csrc/kern_shade_common.h"

#define PROBE_API extern "C" __attribute__((visibility("default")))

namespace {

enum { PROBE_OK = 0, PROBE_BAD_ARGUMENT = 1, PROBE_BAD_INSTANTIATION = 2, PROBE_HIP = 3 };
// per query, 18 words: has_bsdf, n, f.rgb, pdf, fused f.rgb, fused pdf, sampled wi.xyz, sampled f.rgb, sampled pdf, sampled type
constexpr uint32_t kBsdfWords = 18;

template <int MAXL, int DIFF>
__global__ __launch_bounds__(256) void k_bsdf_probe(const PtMaterial *mats, const uint32_t *mat_index, uint32_t n, const float *wo, const float *wi, const float *u, uint32_t *out) {
    __shared__ float s_lobes[lobe_store_words<MAXL>()];   // (bind() indexes it by threadIdx.x: blocks of kLobeStride threads)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    SurfaceInteraction si;
    si.p = V3(0.0f, 0.0f, 0.0f); si.p_error = V3(0.0f, 0.0f, 0.0f); si.n = V3(0.0f, 0.0f, 1.0f); si.wo = V3(0.0f, 0.0f, 1.0f);
    si.dpdu = V3(1.0f, 0.0f, 0.0f); si.dpdv = V3(0.0f, 1.0f, 0.0f); si.sh_n = V3(0.0f, 0.0f, 1.0f); si.sh_dpdu = V3(1.0f, 0.0f, 0.0f); si.sh_dpdv = V3(0.0f, 1.0f, 0.0f);
    si.sh_dndu = V3(0.0f, 0.0f, 0.0f); si.sh_dndv = V3(0.0f, 0.0f, 0.0f);
    si.uv = P2(0.5f, 0.5f); si.has_shape = false; si.shape_flip = false; si.prim = 0;
    Bsdf<MAXL, DIFF> bsdf; bsdf.bind(s_lobes);
    bsdf.n = 0; bsdf.types = 0ull;
    const uint32_t mi = mat_index[i];   // per thread, from memory, as the shade kernels get theirs from the hit: the material is no wave-uniform value to the compiler
    const bool has = build_bsdf(mats[mi], si, bsdf, ConstMatEval{}, mats);
    uint32_t *o = out + (size_t)i * kBsdfWords;
    o[0] = has ? 1u : 0u; o[1] = has ? (uint32_t)bsdf.n : 0u;
    for (uint32_t k = 2; k < kBsdfWords; ++k) o[k] = 0u;
    if (!has) return;
    const V3 vo(wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]), vi(wi[3 * i], wi[3 * i + 1], wi[3 * i + 2]);
    const RGB f = bsdf.f(vo, vi, BSDF_ALL);
    const float pdf = bsdf.pdf(vo, vi, BSDF_ALL);
    float fpdf = 0.0f;
    const RGB ff = bsdf.f_pdf(vo, vi, BSDF_ALL, fpdf);
    V3 sw(0.0f, 0.0f, 0.0f); float spdf = 0.0f; int sampled = 0;   // (pdf = 0 on entry, as in the oracle's hook: sample_f leaves it untouched on its wo.z == 0 exit)
    const RGB sf = bsdf.sample_f(vo, sw, P2(u[2 * i], u[2 * i + 1]), spdf, BSDF_ALL, sampled);
    o[2] = __float_as_uint(f.r); o[3] = __float_as_uint(f.g); o[4] = __float_as_uint(f.b); o[5] = __float_as_uint(pdf);
    o[6] = __float_as_uint(ff.r); o[7] = __float_as_uint(ff.g); o[8] = __float_as_uint(ff.b); o[9] = __float_as_uint(fpdf);
    o[10] = __float_as_uint(sw.x); o[11] = __float_as_uint(sw.y); o[12] = __float_as_uint(sw.z);
    o[13] = __float_as_uint(sf.r); o[14] = __float_as_uint(sf.g); o[15] = __float_as_uint(sf.b); o[16] = __float_as_uint(spdf); o[17] = (uint32_t)sampled;
}

using BsdfKernel = void (*)(const PtMaterial *, const uint32_t *, uint32_t, const float *, const float *, const float *, uint32_t *);
BsdfKernel bsdf_kernel(int maxl, int diff) {   // the nine instantiations of tu_shade.hip
    if (maxl == 1) switch (diff) { case 0: return k_bsdf_probe<1, 0>; case 1: return k_bsdf_probe<1, 1>; case 2: return k_bsdf_probe<1, 2>; case 3: return k_bsdf_probe<1, 3>; case 6: return k_bsdf_probe<1, 6>; default: return nullptr; }
    if (maxl == 2) switch (diff) { case 0: return k_bsdf_probe<2, 0>; case 4: return k_bsdf_probe<2, 4>; default: return nullptr; }
    if (maxl == 5) switch (diff) { case 0: return k_bsdf_probe<5, 0>; case 5: return k_bsdf_probe<5, 5>; default: return nullptr; }
    return nullptr;
}

}  // namespace

// 18 words per query
PROBE_API uint32_t probe_bsdf_words() { return kBsdfWords; }

// The shade class scene_plan.hip gives material `mi` of the table (specialised, untextured scene) and the general class it folds into (kernels.h).
PROBE_API int probe_material_class(const PtMaterial *mats, uint32_t n_materials, uint32_t mi, int32_t *cls, int32_t *general) {
    if (!mats || !cls || !general || mi >= n_materials) return PROBE_BAD_ARGUMENT;
    const uint32_t c = pth::material_class(mats[mi], true, true);
    *cls = (int32_t)c; *general = (int32_t)class_general(c);
    return PROBE_OK;
}

// n queries (wo, wi: 3n floats, u: 2n floats, host memory) of material `mi` of the scene's device material table in Bsdf<maxl, diff>; out: 18n words, host memory.
PROBE_API int probe_bsdf(const pt_scene *sc, int maxl, int diff, uint32_t mi, uint32_t n, const float *wo, const float *wi, const float *u, uint32_t *out) {
    if (!sc || !wo || !wi || !u || !out || n == 0 || n > (1u << 20)) return PROBE_BAD_ARGUMENT;
    if (!sc->ds.materials || mi >= sc->ds.n_materials) return PROBE_BAD_ARGUMENT;
    const BsdfKernel k = bsdf_kernel(maxl, diff);
    if (!k) return PROBE_BAD_INSTANTIATION;
    if (hipSetDevice(sc->device) != hipSuccess) return PROBE_HIP;
    DevTmp tmp;
    float *d_wo = nullptr, *d_wi = nullptr, *d_u = nullptr; uint32_t *d_out = nullptr, *d_mi = nullptr;
    const size_t n3 = (size_t)n * 3 * sizeof(float), n2 = (size_t)n * 2 * sizeof(float), no = (size_t)n * kBsdfWords * sizeof(uint32_t);
    if (tmp.alloc(&d_wo, n3) != hipSuccess || tmp.alloc(&d_wi, n3) != hipSuccess || tmp.alloc(&d_u, n2) != hipSuccess || tmp.alloc(&d_out, no) != hipSuccess ||
        tmp.alloc(&d_mi, (size_t)n * sizeof(uint32_t)) != hipSuccess) return PROBE_HIP;
    if (hipMemcpy(d_wo, wo, n3, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_wi, wi, n3, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_u, u, n2, hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_out, 0xff, no) != hipSuccess ||
        hipMemsetD32((hipDeviceptr_t)d_mi, (int)mi, n) != hipSuccess) return PROBE_HIP;   // (mi < n_materials: checked above)
    hipLaunchKernelGGL(k, dim3((n + 255u) / 256u), dim3(256), 0, 0, sc->ds.materials, d_mi, n, d_wo, d_wi, d_u, d_out);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return PROBE_HIP;
    if (hipMemcpy(out, d_out, no, hipMemcpyDeviceToHost) != hipSuccess) return PROBE_HIP;
    return PROBE_OK;
}
