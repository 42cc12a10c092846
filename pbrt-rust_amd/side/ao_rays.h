// ao_rays.h -- the device side of an ambient-occlusion ray (integrators/ao.rs:77-95), once, for the libraries that spawn such rays: libmi355ao from a camera hit
// (ao/ao_kernels.h) and libmi355bake from a texel's surface point (bake/bake_kernels.h). A chunk of a point's rays (AOChunk), the sampler's array value, and the
// ray and its weight from a frame the caller builds (ao_ray). The kernels stay in their libraries' namespaces. (kInv4Pi is ptd's, dev_medium.h.)
#pragma once
#include "../csrc/kern_decl.h"

namespace ptside {
using namespace ptd;

constexpr uint32_t kAOChunk = 64;                    // AO rays per point per trace launch (the rays of one point are consecutive ray ids)

// One chunk of AO rays: elements k0 .. k0 + kn - 1 of every point's nsamples.
struct AOChunk {
    uint32_t nsamples, cos_sample;
    uint32_t k0, kn;
    float4 *ray;            // [rays][2]: {o.xyz, d.x} {d.yz, -, -} (k_trace's 32-byte ray record)
    float *w;               // [rays]: dot(wi, n) / (pdf * nsamples)
    uint32_t *base;         // [points]: first ray id of the point's chunk, PT_NONE where there is no surface point
    uint32_t *ray_count;    // device count of ray ids handed out
    const uint32_t *occluded;   // [rays]: k_trace's any-hit flags (the accumulate kernels)
};

// The 2-D array value of sample number j (GlobalSampler::start_pixel, sampler.rs:288-302): dimensions ARRAY_START_DIM = 5 and 6.
PT_DEV P2 ao_array_sample(const RenderConst &rc, const SobolTables &tabs, int32_t px, int32_t py, uint64_t j) {
    if (rc.halton.enabled) {
        const uint64_t index = halton_index_for_sample(rc.halton, px, py, j);
        return P2(halton_sample_dimension(tabs, rc.halton, index, 5u), halton_sample_dimension(tabs, rc.halton, index, 6u));
    }
    const uint64_t index = sobol_interval_to_index(tabs, (uint32_t)rc.sobol.log2_resolution, j, (uint32_t)(px - rc.sobol.sb_min[0]), (uint32_t)(py - rc.sobol.sb_min[1]));
    return P2(sobol_sample_float(tabs.m32, index, 5u), sobol_sample_float(tabs.m32, index, 6u));
}

// The frame of ao.rs:77-80: s = normalize(dpdu), t = cross(n, s) from the un-flipped normal (not normalised), and the n the caller chooses -- face-forwarded against
// the camera ray (k_ao_rays) or the interaction's own (the bake: there is no camera ray).
struct AOFrame { V3 n, sv, tv; };

// Sample number `number` of pixel / texel (px, py): origin, direction and weight (ao.rs:82-95)
PT_DEV void ao_ray(const RenderConst &rc, const SobolTables &tabs, const SurfaceInteraction &si, const AOFrame &f, int32_t px, int32_t py, uint64_t number,
                   uint32_t cos_sample, float nsf, V3 &o, V3 &wo, float &w) {
    const P2 u = ao_array_sample(rc, tabs, px, py, number);
    V3 wi; float pdf;
    if (cos_sample) { wi = cosine_sample_hemisphere(u); pdf = fabsf(wi.z) * kInvPi; }   // cosine_hemisphere_pdf (sampling.rs:195-197)
    else {   // uniform_sample_sphere (sampling.rs:212-218), uniform_sphere_pdf
        const float z = 1.0f - 2.0f * u.x;
        const float r = sqrtf(maxf(1.0f - z * z, 0.0f));
        const float phi = 2.0f * kPi * u.y;
        float sn, cs; dm_sincosf(phi, sn, cs);
        wi = V3(r * cs, r * sn, z); pdf = kInv4Pi;
    }
    wo = V3(f.sv.x * wi.x + f.tv.x * wi.y + f.n.x * wi.z, f.sv.y * wi.x + f.tv.y * wi.y + f.n.y * wi.z, f.sv.z * wi.x + f.tv.z * wi.y + f.n.z * wi.z);
    o = offset_ray_origin(si.p, si.p_error, si.n, wo);   // SurfaceInteraction::spawn_ray (interaction.rs:32-36)
    w = dot(wo, f.n) / (pdf * nsf);
}

}  // namespace ptside
