// ao_kernels.h -- the kernels of the ambient-occlusion integrator (integrators/ao.rs:63-110). Camera rays (k_generate), their
// closest hits and the AO rays' any-hit walk (k_trace) and the film (k_film) are libmi355pt's; this file adds the two steps
// between them: k_ao_rays spawns one chunk of a camera hit's AO rays, k_ao_accum adds the unoccluded ones to the path's L.
#pragma once
#include "../csrc/kern_decl.h"
#include "../csrc/kern_film.h"
#include "../side/ao_rays.h"

namespace ptao {
using namespace ptside;

// One chunk of AO rays: elements k0 .. k0 + kn - 1 of every camera hit's nsamples; base: [paths], PT_NONE when the path's camera ray missed.
// (A type of this namespace: the kernels' symbols name ptao::AOJob.)
struct AOJob : AOChunk {};

// Per alive path (the camera-ray queue of k_generate): rebuild the camera hit's interaction and write this chunk's AO rays.
template <bool SPH>
__global__ __launch_bounds__(256) void k_ao_rays(DeviceScene s, RenderConst rc, SobolTables tabs, PathSoA ps, const uint32_t *queue, const uint32_t *count_ptr, AOJob job) {
    const uint32_t count = *count_ptr;
    const uint32_t rounded = (count + 63u) & ~63u;   // whole waves iterate together (one ray-id reservation per wave)
    for (uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x; qi < rounded; qi += gridDim.x * blockDim.x) {
        uint32_t pid = 0;
        bool found = false;
        float4 r0, r1, h0, h1;
        if (qi < count) {
            pid = queue[qi];
            const float4 *rq = reinterpret_cast<const float4 *>(ps.ray) + 2 * (size_t)pid, *hq = reinterpret_cast<const float4 *>(ps.hit) + 2 * (size_t)pid;
            r0 = rq[0]; r1 = rq[1]; h0 = hq[0]; h1 = hq[1];
            found = __float_as_uint(h0.x) != PT_NONE;
        }
        // one atomic per wave: the wave's hit paths take consecutive blocks of kn ray ids, in lane order
        const uint32_t first = wave_reserve(job.ray_count, found, job.kn);
        if (qi >= count) continue;
        if (!found) { job.base[pid] = PT_NONE; continue; }
        job.base[pid] = first;
        const V3 ro(r0.x, r0.y, r0.z), rd(r0.w, r1.x, r1.y);
        SurfaceInteraction si;
        fill_hit_pkt<SPH>(s, __float_as_uint(h1.z), SPH ? __float_as_uint(h1.x) : PT_NONE, ro, rd, h0.y, h0.z, h0.w, si);
        // ao.rs:77-80: the frame of the true geometry (t from the un-flipped normal, not normalised)
        const V3 n = face_forward(si.n, -rd);
        const V3 sv = normalize(si.dpdu);
        const V3 tv = cross(si.n, sv);
        const uint32_t slot = pid % rc.n_pix_slots, sl = pid / rc.n_pix_slots;
        int32_t px, py;
        slot_to_pixel(rc, slot, px, py);   // (an alive path's slot is a pixel: k_generate queued it)
        const uint64_t sample = (uint64_t)rc.s_begin + sl;
        const float nsf = (float)job.nsamples;
        // NOTE: the loop body is ao_ray's (side/ao_rays.h), restated here: called through that inlined helper, in any shape of it, k_ao_rays<false> came out of the compiler
        // with 83 VGPRs for 79 -- five waves per SIMD for six (profiles/r6/NOTES.md section 21) --, so this kernel keeps its body. A fix to either belongs in both.
        for (uint32_t kk = 0; kk < job.kn; ++kk) {
            const P2 u = ao_array_sample(rc, tabs, px, py, sample * job.nsamples + job.k0 + kk);
            V3 wi; float pdf;
            if (job.cos_sample) { wi = cosine_sample_hemisphere(u); pdf = fabsf(wi.z) * kInvPi; }   // cosine_hemisphere_pdf (sampling.rs:195-197)
            else {   // uniform_sample_sphere (sampling.rs:212-218), uniform_sphere_pdf
                const float z = 1.0f - 2.0f * u.x;
                const float r = sqrtf(maxf(1.0f - z * z, 0.0f));
                const float phi = 2.0f * kPi * u.y;
                float sn, cs; dm_sincosf(phi, sn, cs);
                wi = V3(r * cs, r * sn, z); pdf = kInv4Pi;
            }
            const V3 wo(sv.x * wi.x + tv.x * wi.y + n.x * wi.z, sv.y * wi.x + tv.y * wi.y + n.y * wi.z, sv.z * wi.x + tv.z * wi.y + n.z * wi.z);
            const V3 o = offset_ray_origin(si.p, si.p_error, si.n, wo);   // SurfaceInteraction::spawn_ray (interaction.rs:32-36): t_max = infinity
            const uint32_t id = first + kk;
            job.ray[2 * (size_t)id] = make_float4(o.x, o.y, o.z, wo.x);
            job.ray[2 * (size_t)id + 1] = make_float4(wo.y, wo.z, 0.0f, 0.0f);
            job.w[id] = dot(wo, n) / (pdf * nsf);
        }
    }
}

// L += the unoccluded rays' terms, in element order (ao.rs:96-98); all three channels carry the same value (Spectrum::new).
__global__ __launch_bounds__(256) void k_ao_accum(PathSoA ps, const uint32_t *queue, const uint32_t *count_ptr, AOJob job) {
    const uint32_t count = *count_ptr;
    for (uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x; qi < count; qi += gridDim.x * blockDim.x) {
        const uint32_t pid = queue[qi];
        const uint32_t first = job.base[pid];
        if (first == PT_NONE) continue;
        float L = ps.L_r(pid);
        for (uint32_t kk = 0; kk < job.kn; ++kk) if (!job.occluded[first + kk]) L += job.w[first + kk];
        ps.L_r(pid) = L; ps.L_g(pid) = L; ps.L_b(pid) = L;
    }
}

}  // namespace ptao
