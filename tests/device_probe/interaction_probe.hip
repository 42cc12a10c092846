// interaction_probe.hip -- TEST CODE (tests/probe_build.py builds it; it is no part of libmi355pt.so): the step between a hit record and the shade kernels, on its own.
// The rays are traced by the library's own launch (pth::launch_trace, a TraceJob as parity_api.hip builds it) with out_hit2 set, so the two quads arrive exactly as
// k_trace writes them for the render: {prim, b0, b1, b2} and {inst, t, packet, packet flags}. A kernel of this file then calls the UNMODIFIED fill_hit_pkt<SPH> /
// fill_hit<SPH> (kern_common.h) once per ray and writes every field of the SurfaceInteraction as words, for the oracle's orc_intersect (oracle/ref_kats_shapes.cpp)
// to be compared with field by field. SPH as the render chooses it (pth::general_geometry).
#include "../../pbrt-rust_amd/csrc/host_common.h"
#include "../../pbrt-rust_amd/csrc/kern_common.h"

#define PROBE_API extern "C" __attribute__((visibility("default")))

namespace {

enum { PROBE_OK = 0, PROBE_BAD_ARGUMENT = 1, PROBE_BAD_FORM = 2, PROBE_HIP = 3, PROBE_NO_WORKSPACE = 4, PROBE_TRACE = 5 };
// per ray, 45 words: 0 hit flag, 1 prim, 2 inst, 3 t, 4-6 b, 7-9 p, 10-12 p_error, 13-15 n, 16-18 wo, 19-20 uv, 21-23 dpdu, 24-26 dpdv, 27-29 sh_n, 30-32 sh_dpdu,
// 33-35 sh_dpdv, 36-38 sh_dndu, 39-41 sh_dndv, 42 has_shape, 43 shape_flip (words 0-43: orc_intersect's), 44 the packet flags fill_hit_pkt returns (form 1: the record's)
constexpr uint32_t kInteractionWords = 45;

PT_DEV void put3(uint32_t *o, V3 v) { o[0] = __float_as_uint(v.x); o[1] = __float_as_uint(v.y); o[2] = __float_as_uint(v.z); }

template <bool SPH, int FORM>
__global__ __launch_bounds__(256) void k_interaction_probe(DeviceScene s, uint32_t n, const float4 *ray, const float4 *hit, const float4 *hit2, uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t *o = out + (size_t)i * kInteractionWords;
    const float4 h = hit[i], h2 = hit2[i];
    const uint32_t prim = __float_as_uint(h.x);
    if (prim == PT_NONE) {   // a miss: its packet word is no index
        for (uint32_t k = 0; k < kInteractionWords; ++k) o[k] = 0u;
        return;
    }
    const float4 r0 = ray[2 * (size_t)i], r1 = ray[2 * (size_t)i + 1];
    const V3 ro(r0.x, r0.y, r0.z), rd(r0.w, r1.x, r1.y);
    const uint32_t inst = SPH ? __float_as_uint(h2.x) : PT_NONE, pkt = __float_as_uint(h2.z);
    SurfaceInteraction si;
    uint32_t fl;
    if (FORM == 0) fl = fill_hit_pkt<SPH>(s, pkt, inst, ro, rd, h.y, h.z, h.w, si);
    else { fill_hit<SPH>(s, prim, inst, ro, rd, h.y, h.z, h.w, si); fl = __float_as_uint(h2.w); }
    o[0] = 1u; o[1] = prim; o[2] = __float_as_uint(h2.x); o[3] = __float_as_uint(h2.y);
    o[4] = __float_as_uint(h.y); o[5] = __float_as_uint(h.z); o[6] = __float_as_uint(h.w);
    put3(o + 7, si.p); put3(o + 10, si.p_error); put3(o + 13, si.n); put3(o + 16, si.wo);
    o[19] = __float_as_uint(si.uv.x); o[20] = __float_as_uint(si.uv.y);
    put3(o + 21, si.dpdu); put3(o + 24, si.dpdv); put3(o + 27, si.sh_n); put3(o + 30, si.sh_dpdu); put3(o + 33, si.sh_dpdv); put3(o + 36, si.sh_dndu); put3(o + 39, si.sh_dndv);
    o[42] = si.has_shape ? 1u : 0u; o[43] = si.shape_flip ? 1u : 0u; o[44] = fl;
}

}  // namespace

PROBE_API uint32_t probe_interaction_words() { return kInteractionWords; }

// n rays (o, d: 3n floats, tmax: n floats, host memory) traced through the scene and filled in form 0 (fill_hit_pkt) or 1 (fill_hit); out: 45n words, host memory.
// The scene must have its workspace (any pt_trace_* or render call makes it): this file creates none.
PROBE_API int probe_interaction(pt_scene *sc, int form, uint32_t n, const float *o, const float *d, const float *tmax, uint32_t *out) {
    if (!sc || !o || !d || !tmax || !out || n == 0 || n > (1u << 20)) return PROBE_BAD_ARGUMENT;
    if (form != 0 && form != 1) return PROBE_BAD_FORM;
    if (!sc->stream || !sc->qc || !sc->dc || !sc->spill || sc->spill_waves == 0) return PROBE_NO_WORKSPACE;
    if (!sc->ds.leaf || !sc->ds.prim_shape) return PROBE_BAD_ARGUMENT;
    if (hipSetDevice(sc->device) != hipSuccess) return PROBE_HIP;
    DevTmp tmp;
    std::vector<float> recs(8 * (size_t)n, 0.0f);   // 32-byte ray records {o.xyz, d.x} {d.y, d.z, t_max, -}, as pt_trace_closest builds them
    for (uint32_t i = 0; i < n; ++i) {
        float *r = recs.data() + 8 * (size_t)i;
        r[0] = o[3 * (size_t)i]; r[1] = o[3 * (size_t)i + 1]; r[2] = o[3 * (size_t)i + 2];
        r[3] = d[3 * (size_t)i]; r[4] = d[3 * (size_t)i + 1]; r[5] = d[3 * (size_t)i + 2]; r[6] = tmax[i];
    }
    float4 *d_ray = nullptr, *d_hit = nullptr, *d_hit2 = nullptr; float *d_t = nullptr; uint32_t *d_word = nullptr, *d_count = nullptr, *d_out = nullptr;
    const size_t nq = (size_t)n * sizeof(float4), no = (size_t)n * kInteractionWords * sizeof(uint32_t);
    if (tmp.alloc(&d_ray, 2 * nq) != hipSuccess || tmp.alloc(&d_hit, nq) != hipSuccess || tmp.alloc(&d_hit2, nq) != hipSuccess || tmp.alloc(&d_t, (size_t)n * 4) != hipSuccess ||
        tmp.alloc(&d_word, (size_t)n * 4) != hipSuccess || tmp.alloc(&d_count, 4) != hipSuccess || tmp.alloc(&d_out, no) != hipSuccess) return PROBE_HIP;
    if (hipMemcpy(d_ray, recs.data(), 2 * nq, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_count, &n, 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_hit, 0xff, nq) != hipSuccess || hipMemset(d_hit2, 0xff, nq) != hipSuccess || hipMemset(d_out, 0xff, no) != hipSuccess) return PROBE_HIP;   // (0xff: an unwritten record is a miss)
    if (hipMemsetAsync(sc->dc, 0, sizeof(DevCounters), sc->stream) != hipSuccess || hipMemsetAsync(sc->qc, 0, sizeof(QCounters), sc->stream) != hipSuccess) return PROBE_HIP;
    TraceJob tj{};
    TraceSub &ts = tj.sub[0];
    ts.queue = nullptr; ts.count = d_count; tj.head = &sc->qc->head[0];
    ts.ray = d_ray; ts.ray_stride = 2; ts.per_ray_tmax = 1;
    ts.out_hit = d_hit; ts.out_hit_stride = 1; ts.out_hit2 = d_hit2; ts.out_t = d_t; ts.out_t_stride = 1;
    ts.out_word = d_word; ts.out_word_stride = 1;
    ts.kind = 0; ts.any = 0u;
    tj.spill = sc->spill; tj.error = &sc->qc->error; tj.counters = sc->dc;
    if (pth::launch_trace(sc, 0, tj, n) != PT_OK) return PROBE_TRACE;
    if (hipStreamSynchronize(sc->stream) != hipSuccess) return PROBE_HIP;
    QCounters qh;
    if (hipMemcpy(&qh, sc->qc, sizeof qh, hipMemcpyDeviceToHost) != hipSuccess) return PROBE_HIP;
    if (qh.error) return PROBE_TRACE;
    const bool sph = pth::general_geometry(sc);
    const dim3 grid((n + 255u) / 256u), block(256);
    if (sph) {
        if (form == 0) hipLaunchKernelGGL((k_interaction_probe<true, 0>), grid, block, 0, 0, sc->ds, n, d_ray, d_hit, d_hit2, d_out);
        else hipLaunchKernelGGL((k_interaction_probe<true, 1>), grid, block, 0, 0, sc->ds, n, d_ray, d_hit, d_hit2, d_out);
    } else {
        if (form == 0) hipLaunchKernelGGL((k_interaction_probe<false, 0>), grid, block, 0, 0, sc->ds, n, d_ray, d_hit, d_hit2, d_out);
        else hipLaunchKernelGGL((k_interaction_probe<false, 1>), grid, block, 0, 0, sc->ds, n, d_ray, d_hit, d_hit2, d_out);
    }
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return PROBE_HIP;
    if (hipMemcpy(out, d_out, no, hipMemcpyDeviceToHost) != hipSuccess) return PROBE_HIP;
    return PROBE_OK;
}
