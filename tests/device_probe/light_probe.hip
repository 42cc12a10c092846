// light_probe.hip -- TEST CODE (tests/test_device_probe.py builds it; it is no part of libmi355pt.so): one thread per query calls the device's
// light_sample_li<SPH> and light_pdf_li<SPH> (dev_light.h) on the DeviceScene of a pt_scene that libmi355pt.so created, for the oracle's
// orc_light_sample_li / orc_light_pdf_li (oracle/ref_kats.cpp) to be compared with call by call. SPH as the render chooses it (render_loop.hip).
#include "../../pbrt-rust_amd/csrc/host_common.h"
#include "../../pbrt-rust_amd/csrc/kern_shade_common.h"

#define PROBE_API extern "C" __attribute__((visibility("default")))

namespace {

enum { PROBE_OK = 0, PROBE_BAD_ARGUMENT = 1, PROBE_HIP = 3 };
// per query, 8 words: sample_li's wi.xyz, pdf, L.rgb; pdf_li of the given direction
constexpr uint32_t kLightWords = 8;

template <bool SPH>
__global__ __launch_bounds__(256) void k_light_probe(DeviceScene s, const uint32_t *light_index, uint32_t n, const float *p, const float *perr, const float *nrm, const float *u, const float *w, uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t li = light_index[i];   // per thread, from memory, as the shade kernels draw theirs: the light is no wave-uniform value to the compiler
    IData ref; ref.p = V3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); ref.p_error = V3(perr[3 * i], perr[3 * i + 1], perr[3 * i + 2]); ref.n = V3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
    V3 wi(0.0f, 0.0f, 0.0f); float pdf = 0.0f; IData p1;   // (wi and pdf as the oracle's hook leaves them before the call)
    const RGB L = light_sample_li<SPH>(s, li, ref, P2(u[2 * i], u[2 * i + 1]), wi, pdf, p1);
    const float back = light_pdf_li<SPH>(s, li, ref, V3(w[3 * i], w[3 * i + 1], w[3 * i + 2]));
    uint32_t *o = out + (size_t)i * kLightWords;
    o[0] = __float_as_uint(wi.x); o[1] = __float_as_uint(wi.y); o[2] = __float_as_uint(wi.z); o[3] = __float_as_uint(pdf);
    o[4] = __float_as_uint(L.r); o[5] = __float_as_uint(L.g); o[6] = __float_as_uint(L.b); o[7] = __float_as_uint(back);
}

}  // namespace

PROBE_API uint32_t probe_light_words() { return kLightWords; }
PROBE_API int probe_light_count(const pt_scene *sc, uint32_t *n_lights, int32_t *sph) {
    if (!sc || !n_lights || !sph) return PROBE_BAD_ARGUMENT;
    *n_lights = sc->ds.n_lights; *sph = (sc->ds.n_spheres > 0 || sc->ds.n_instances > 0) ? 1 : 0;
    return PROBE_OK;
}

// n queries of light `li`: reference points (p, p_error, n: 3n floats each), sample points u (2n floats), directions w for pdf_li (3n floats), all host memory; out: 8n words.
PROBE_API int probe_light(const pt_scene *sc, uint32_t li, uint32_t n, const float *p, const float *perr, const float *nrm, const float *u, const float *w, uint32_t *out) {
    if (!sc || !p || !perr || !nrm || !u || !w || !out || n == 0 || n > (1u << 20)) return PROBE_BAD_ARGUMENT;
    if (!sc->ds.lights || !sc->ds.light_rec || li >= sc->ds.n_lights) return PROBE_BAD_ARGUMENT;
    if (hipSetDevice(sc->device) != hipSuccess) return PROBE_HIP;
    DevTmp tmp;
    const float *src[5] = {p, perr, nrm, u, w}; const size_t words[5] = {3, 3, 3, 2, 3};
    float *dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; uint32_t *d_out = nullptr, *d_li = nullptr;
    for (int k = 0; k < 5; ++k) {
        const size_t bytes = (size_t)n * words[k] * sizeof(float);
        if (tmp.alloc(&dev[k], bytes) != hipSuccess || hipMemcpy(dev[k], src[k], bytes, hipMemcpyHostToDevice) != hipSuccess) return PROBE_HIP;
    }
    const size_t no = (size_t)n * kLightWords * sizeof(uint32_t);
    if (tmp.alloc(&d_out, no) != hipSuccess || hipMemset(d_out, 0xff, no) != hipSuccess) return PROBE_HIP;
    if (tmp.alloc(&d_li, (size_t)n * sizeof(uint32_t)) != hipSuccess || hipMemsetD32((hipDeviceptr_t)d_li, (int)li, n) != hipSuccess) return PROBE_HIP;   // (li < n_lights: checked above)
    const bool sph = sc->ds.n_spheres > 0 || sc->ds.n_instances > 0;   // general_geometry() of render_loop.hip
    if (sph) hipLaunchKernelGGL(k_light_probe<true>, dim3((n + 255u) / 256u), dim3(256), 0, 0, sc->ds, d_li, n, dev[0], dev[1], dev[2], dev[3], dev[4], d_out);
    else hipLaunchKernelGGL(k_light_probe<false>, dim3((n + 255u) / 256u), dim3(256), 0, 0, sc->ds, d_li, n, dev[0], dev[1], dev[2], dev[3], dev[4], d_out);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return PROBE_HIP;
    if (hipMemcpy(out, d_out, no, hipMemcpyDeviceToHost) != hipSuccess) return PROBE_HIP;
    return PROBE_OK;
}
