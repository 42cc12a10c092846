// bssrdf_probe.hip -- TEST CODE (tests/probe_build.py builds it; it is no part of libmi355pt.so): one thread per query calls the device's subsurface code
// (dev_bssrdf.h: DevBssrdf::{sr, pdf_sr, sample_sr, pdf_sp, probe_segment}, BssrdfAdapterBsdf, subsurface_from_diffuse) on the material table and the
// BSSRDF tables of a pt_scene that libmi355pt.so created, and writes the words of the oracle's orc_bssrdf_eval (oracle/ref_kats.cpp), section by section.
// Compiled with the HIPFLAGS of ../../pbrt-rust_amd/csrc/Makefile (+ -fvisibility=hidden) against the unmodified headers.
// The DevBssrdf is built in the two forms the render builds it in; the few glue lines of the kernels are RESTATED here (the kernels are not edited to share them):
//   form 0, entry: kern_shade.h:156-160 (the ConstMatEval arm: subsurface_from_diffuse when kd_subsurface is set, else the material's constants) and
//                  kern_shade.h:219-221 (init_medium / init_disney, then init_frame(si))
//   form 1, exit:  kern_bssrdf.h:70-78 (init_disney, or init_medium from the stored coefficients where bss_coef_stored, else from the material's constants;
//                  ns, ss, po_p from the frame record k_shade stored at kern_shade.h:232-233 -- si.p, bss.ns, bss.ss -- and ts = cross(ns, ss))
#include "../../pbrt-rust_amd/csrc/host_common.h"
#include "../../pbrt-rust_amd/csrc/kern_shade_common.h"

#define PROBE_API extern "C" __attribute__((visibility("default")))

namespace {

enum { PROBE_OK = 0, PROBE_BAD_ARGUMENT = 1, PROBE_NO_BSSRDF = 2, PROBE_HIP = 3, PROBE_FORMS_DIFFER = 4 };
enum { SEC_STATE = 0, SEC_RADII, SEC_SAMPLES, SEC_EXITS, SEC_SEGMENTS, SEC_ADAPTER, SEC_CONVERSION, SEC_COUNT };
// words in / out per query of each section (orc_bssrdf_eval's layout; the adapter's flags are a ninth input word)
constexpr uint32_t kWordsIn[SEC_COUNT] = {0, 1, 1, 6, 3, 9, 6};
constexpr uint32_t kWordsOut[SEC_COUNT] = {19, 6, 3, 4, 8, 12, 6};

PT_DEV void put3(uint32_t *o, V3 v) { o[0] = __float_as_uint(v.x); o[1] = __float_as_uint(v.y); o[2] = __float_as_uint(v.z); }
PT_DEV void put3(uint32_t *o, RGB v) { o[0] = __float_as_uint(v.r); o[1] = __float_as_uint(v.g); o[2] = __float_as_uint(v.b); }

PT_DEV SurfaceInteraction frame_interaction(const float *f) {   // 15 floats: p, n, sh_n, sh_dpdu, sh_dpdv
    SurfaceInteraction si;
    si.p = V3(f[0], f[1], f[2]); si.p_error = V3(0.0f, 0.0f, 0.0f); si.n = V3(f[3], f[4], f[5]); si.sh_n = V3(f[6], f[7], f[8]); si.wo = si.sh_n;
    si.sh_dpdu = V3(f[9], f[10], f[11]); si.sh_dpdv = V3(f[12], f[13], f[14]); si.dpdu = si.sh_dpdu; si.dpdv = si.sh_dpdv;
    si.sh_dndu = V3(0.0f, 0.0f, 0.0f); si.sh_dndv = V3(0.0f, 0.0f, 0.0f);
    si.uv = P2(0.5f, 0.5f); si.has_shape = false; si.shape_flip = false; si.prim = 0;
    return si;
}

PT_DEV void build_bssrdf(const PtMaterial *mats, const DevBssTable *tables, uint32_t n_textures, uint32_t mi, const SurfaceInteraction &si, int form, DevBssrdf &out) {
    const bool is_sss = mats[mi].type == PT_MAT_SUBSURFACE;   // kern_shade.h:115
    RGB bss_sa(0.0f), bss_ss(0.0f);
    if (is_sss) {   // kern_shade.h:156-160
        const PtMaterial &sm = mats[mi];
        if (sm.kd_subsurface) subsurface_from_diffuse(tables[sm.bssrdf_table], rgb3(sm.kd).clamps(0.0f, PT_INF), rgb3(sm.mfp).clamps(0.0f, PT_INF) * RGB(sm.scale), bss_sa, bss_ss);
        else { bss_sa = rgb3(sm.sigma_a); bss_ss = rgb3(sm.sigma_s); }
    }
    DevBssrdf bss;   // kern_shade.h:219-221
    if (is_sss) bss.init_medium(mats[mi], tables, bss_sa, bss_ss); else bss.init_disney(mats[mi]);
    bss.init_frame(si);
    if (form == 0) { out = bss; return; }
    // kern_shade.h:232-233, 237: what the frame and coefficient records hold
    const float4 fr0 = make_float4(si.p.x, si.p.y, si.p.z, 0.0f), fr1 = make_float4(bss.ns.x, bss.ns.y, bss.ns.z, 0.0f), fr2 = make_float4(bss.ss.x, bss.ss.y, bss.ss.z, 0.0f);
    const float4 c0 = make_float4(bss_sa.r, bss_sa.g, bss_sa.b, 0.0f), c1 = make_float4(bss_ss.r, bss_ss.g, bss_ss.b, 0.0f);
    const PtMaterial &m = mats[mi];
    DevBssrdf ex;   // kern_bssrdf.h:70-78
    if (m.type == PT_MAT_DISNEY) ex.init_disney(m);
    else if (bss_coef_stored(n_textures, m)) ex.init_medium(m, tables, RGB(c0.x, c0.y, c0.z), RGB(c1.x, c1.y, c1.z));
    else ex.init_medium(m, tables, rgb3(m.sigma_a), rgb3(m.sigma_s));
    ex.ns = V3(fr1.x, fr1.y, fr1.z); ex.ss = V3(fr2.x, fr2.y, fr2.z);
    ex.ts = cross(ex.ns, ex.ss); ex.po_p = V3(fr0.x, fr0.y, fr0.z);
    out = ex;
}

// frames: 30 floats, the entry interaction and the exit interaction of the adapter section. in / out: kWordsIn / kWordsOut words per query.
__global__ __launch_bounds__(256) void k_bssrdf_probe(const PtMaterial *mats, const DevBssTable *tables, uint32_t n_textures, const uint32_t *mat_index, const float *frames,
                                                      int section, int form, uint32_t n, const float *in, uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t mi = mat_index[i];   // per thread, from memory, as the shade kernels get theirs from the hit
    const float *q = in + (size_t)i * kWordsIn[section];
    uint32_t *o = out + (size_t)i * kWordsOut[section];
    if (section == SEC_CONVERSION) {   // a tabulated material (the host checked)
        RGB sa(0.0f), ss(0.0f);
        subsurface_from_diffuse(tables[mats[mi].bssrdf_table], RGB(q[0], q[1], q[2]), RGB(q[3], q[4], q[5]), sa, ss);
        put3(o, sa); put3(o + 3, ss);
        return;
    }
    const SurfaceInteraction si = frame_interaction(frames);
    DevBssrdf bss;
    build_bssrdf(mats, tables, n_textures, mi, si, form, bss);
    switch (section) {
    case SEC_STATE:
        for (int k = 0; k < 3; ++k) { o[k] = __float_as_uint(bss.disney ? bss.dD[k] : bss.sigma_t[k]); o[3 + k] = __float_as_uint(bss.disney ? bss.dR[k] : bss.rho[k]); }
        o[6] = __float_as_uint(bss.eta); put3(o + 7, bss.ns); put3(o + 10, bss.ss); put3(o + 13, bss.ts); put3(o + 16, bss.po_p);
        break;
    case SEC_RADII:
        put3(o, bss.sr(q[0]));
        for (int k = 0; k < 3; ++k) o[3 + k] = __float_as_uint(bss.pdf_sr(k, q[0]));
        break;
    case SEC_SAMPLES:
        for (int k = 0; k < 3; ++k) o[k] = __float_as_uint(bss.sample_sr(k, q[0]));
        break;
    case SEC_EXITS: {   // kern_bssrdf.h:84-85
        const V3 pp(q[0], q[1], q[2]), pn(q[3], q[4], q[5]);
        o[0] = __float_as_uint(bss.pdf_sp(pp, pn));
        put3(o + 1, bss.sr(length(bss.po_p - pp)));
        break;
    }
    case SEC_SEGMENTS: {   // kern_shade.h:222-224
        V3 start(0.0f, 0.0f, 0.0f), target(0.0f, 0.0f, 0.0f); float u1n = 0.0f;
        const bool ok = bss.probe_segment(q[0], P2(q[1], q[2]), start, target, u1n);
        o[0] = ok ? 1u : 0u; put3(o + 1, start); put3(o + 4, target); o[7] = __float_as_uint(u1n);
        break;
    }
    case SEC_ADAPTER: {   // kern_bssrdf.h:91-92, 107
        const SurfaceInteraction pi = frame_interaction(frames + 15);
        BssrdfAdapterBsdf bsdf; bsdf.init(pi, bss.eta);
        const V3 wo(q[0], q[1], q[2]), wi(q[3], q[4], q[5]);
        const int flags = (int)__float_as_uint(q[8]);
        put3(o, bsdf.f(wo, wi, flags));
        o[3] = __float_as_uint(bsdf.pdf(wo, wi, flags));
        V3 sw(0.0f, 0.0f, 0.0f); float spdf = 0.0f; int sampled = 0;   // (pdf = 0 on entry, as in the oracle's hook)
        const RGB sf = bsdf.sample_f(wo, sw, P2(q[6], q[7]), spdf, flags, sampled);
        put3(o + 4, sw); put3(o + 7, sf); o[10] = __float_as_uint(spdf); o[11] = (uint32_t)sampled;
        break;
    }
    default: break;
    }
}

}  // namespace

PROBE_API uint32_t probe_bssrdf_sections() { return SEC_COUNT; }
PROBE_API uint32_t probe_bssrdf_words_in(uint32_t section) { return section < SEC_COUNT ? kWordsIn[section] : 0u; }
PROBE_API uint32_t probe_bssrdf_words(uint32_t section) { return section < SEC_COUNT ? kWordsOut[section] : 0u; }

// n queries of one section (in: kWordsIn[section] words each, host memory; the state section takes none and n == 1) of material `mi` of the scene's device material
// table, with the DevBssrdf in form 0 (entry) or 1 (exit); frames: 30 floats, host memory; out: kWordsOut[section] * n words, host memory.
// The state section runs both forms and returns PROBE_FORMS_DIFFER unless every word has the same bits in both; `form` chooses the one that is written out.
PROBE_API int probe_bssrdf(const pt_scene *sc, uint32_t mi, int section, int form, const float *frames, uint32_t n, const float *in, uint32_t *out) {
    if (!sc || !frames || !out || n == 0 || n > (1u << 20) || section < 0 || section >= SEC_COUNT || (form != 0 && form != 1)) return PROBE_BAD_ARGUMENT;
    if (section == SEC_STATE ? n != 1 : !in) return PROBE_BAD_ARGUMENT;
    if (!sc->ds.materials || mi >= sc->ds.n_materials) return PROBE_BAD_ARGUMENT;
    if (hipSetDevice(sc->device) != hipSuccess) return PROBE_HIP;
    PtMaterial m;
    if (hipMemcpy(&m, sc->ds.materials + mi, sizeof m, hipMemcpyDeviceToHost) != hipSuccess) return PROBE_HIP;
    if (!(m.type == PT_MAT_SUBSURFACE || disney_has_bssrdf(m))) return PROBE_NO_BSSRDF;   // kern_shade.h:214
    if (m.type == PT_MAT_SUBSURFACE && (!sc->ds.bss_tables || m.bssrdf_table >= sc->ds.n_bss_tables)) return PROBE_BAD_ARGUMENT;
    if (section == SEC_CONVERSION && m.type != PT_MAT_SUBSURFACE) return PROBE_BAD_ARGUMENT;
    DevTmp tmp;
    float *d_frames = nullptr, *d_in = nullptr; uint32_t *d_out = nullptr, *d_mi = nullptr;
    const size_t ni = (size_t)n * kWordsIn[section] * sizeof(float), no = (size_t)n * kWordsOut[section] * sizeof(uint32_t);
    if (tmp.alloc(&d_frames, 30 * sizeof(float)) != hipSuccess || tmp.alloc(&d_in, ni) != hipSuccess || tmp.alloc(&d_out, no) != hipSuccess ||
        tmp.alloc(&d_mi, (size_t)n * sizeof(uint32_t)) != hipSuccess) return PROBE_HIP;
    if (hipMemcpy(d_frames, frames, 30 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess || (ni && hipMemcpy(d_in, in, ni, hipMemcpyHostToDevice) != hipSuccess) ||
        hipMemsetD32((hipDeviceptr_t)d_mi, (int)mi, n) != hipSuccess) return PROBE_HIP;   // (mi < n_materials: checked above)
    std::vector<uint32_t> words[2];
    for (int f = (section == SEC_STATE ? 0 : form); f <= (section == SEC_STATE ? 1 : form); ++f) {
        if (hipMemset(d_out, 0xff, no) != hipSuccess) return PROBE_HIP;
        hipLaunchKernelGGL(k_bssrdf_probe, dim3((n + 255u) / 256u), dim3(256), 0, 0, sc->ds.materials, sc->ds.bss_tables, sc->ds.n_textures, d_mi, d_frames, section, f, n, d_in, d_out);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return PROBE_HIP;
        words[f].resize((size_t)n * kWordsOut[section]);
        if (hipMemcpy(words[f].data(), d_out, no, hipMemcpyDeviceToHost) != hipSuccess) return PROBE_HIP;
    }
    if (section == SEC_STATE && words[0] != words[1]) return PROBE_FORMS_DIFFER;
    std::memcpy(out, words[form].data(), no);
    return PROBE_OK;
}
