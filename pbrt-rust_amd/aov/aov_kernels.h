// aov_kernels.h -- the kernels of the feature buffers (include/mi355aov.h). Camera rays (k_generate) and their closest hits (k_trace) are libmi355pt's; this file adds
// the two steps behind them: k_aov leaves a camera sample's albedo, shading normal and depth in a record of its own -- or sends the ray on behind a surface without a
// material --, k_aov_film splats the records of a pixel slot's samples onto the planes with the film's filter weights, in sample order.
#pragma once
#include "../csrc/kern_decl.h"
#include "../csrc/kern_shade_common.h"
#include "../csrc/kern_film.h"

namespace ptaov {
using namespace ptd;

enum : uint32_t { kAovAlbedo = 1u, kAovNormal = 2u, kAovDepth = 4u };   // the planes the caller wants (AovJob::mask, wave-uniform)
enum : uint32_t { kAovMiss = 0u, kAovSurface = 1u };                    // word 7 of a finished record

// A camera sample's record, two quads per path id. Finished: {albedo.rgb, t} {n.xyz, kAovMiss | kAovSurface}. On its way behind a shell: {the camera ray's origin, the
// segments' t so far} -- the continuation ray overwrites the path's ray record, and the differentials stay the camera ray's (include/mi355aov.h: unlike the path
// integrator, whose spawned ray has none).
struct AovJob {
    float4 *rec;
    uint32_t *next, *next_count;   // the continuation queue: path ids whose ray goes on behind a surface without a material
    uint32_t mask;
    uint32_t first_round;          // the queue holds camera rays (no record yet)
};
struct AovPlanes { float *albedo, *normal, *depth; };   // device; NULL: not wanted

// The albedo of one material that is not a mix (include/mi355aov.h has the table); the parameters evaluated and clamped as build_bsdf_leaf evaluates them (dev_bsdf.h).
template <class ME> PT_DEV RGB leaf_albedo(const PtMaterial &m, const ME &E) {
    switch (m.type) {
    case PT_MAT_MIRROR: case PT_MAT_GLASS: case PT_MAT_SUBSURFACE: return E.spec(m, PT_MP_KR, m.kr).clamps(0.0f, PT_INF);
    case PT_MAT_METAL: return fr_conductor(1.0f, RGB(1.0f), E.spec(m, PT_MP_ETA_RGB, m.eta_rgb), E.spec(m, PT_MP_K_RGB, m.k_rgb)).clamps(0.0f, PT_INF);
    case PT_MAT_UBER: return E.spec(m, PT_MP_OPACITY, m.opacity).clamps(0.0f, PT_INF) * E.spec(m, PT_MP_KD, m.kd).clamps(0.0f, PT_INF);   // uber.rs:62 `kd = op * Kd`
    default: return E.spec(m, PT_MP_KD, m.kd).clamps(0.0f, PT_INF);   // matte, plastic, substrate, translucent: Kd; disney: "color"
    }
}

// One lane per traced ray of the queue (camera rays, or continuations behind shells): the first surface with a material ends the sample.
template <bool SPH>
__global__ __launch_bounds__(256, 1) void k_aov(DeviceScene s, RenderConst rc, SobolTables tabs, PathSoA ps, const uint32_t *queue, const uint32_t *count_ptr, AovJob job) {
    const uint32_t count = *count_ptr;
    const uint32_t rounded = (count + 63u) & ~63u;   // whole waves iterate together (one queue reservation per wave)
    for (uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x; qi < rounded; qi += gridDim.x * blockDim.x) {
        bool go_on = false;
        uint32_t pid = 0;
        if (qi < count) {
            pid = queue[qi];
            float4 *rq = reinterpret_cast<float4 *>(ps.ray) + 2 * (size_t)pid;
            const float4 *hq = reinterpret_cast<const float4 *>(ps.hit) + 2 * (size_t)pid;
            float4 *out = job.rec + 2 * (size_t)pid;
            const float4 r0 = rq[0], r1 = rq[1], h0 = hq[0], h1 = hq[1];
            const V3 ro(r0.x, r0.y, r0.z), rd(r0.w, r1.x, r1.y);
            const float4 way = job.first_round ? make_float4(ro.x, ro.y, ro.z, 0.0f) : out[0];
            const uint32_t hp = __float_as_uint(h0.x);
            if (hp == PT_NONE) out[1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kAovMiss));
            else {
                SurfaceInteraction si;
                const uint32_t pfl = fill_hit_pkt<SPH>(s, __float_as_uint(h1.z), SPH ? __float_as_uint(h1.x) : PT_NONE, ro, rd, h0.y, h0.z, h0.w, si);
                const uint32_t mi = packet_material(s, pfl, hp);
                const float t = way.w + h1.y;
                if (mi == PT_NONE) {   // path.rs:124-129: `ray = isect.spawn_ray(ray.d)`, no bounce counted
                    IData it; it.p = si.p; it.p_error = si.p_error; it.n = si.n;
                    V3 o; spawn_ray(it, rd, o);
                    rq[0] = make_float4(o.x, o.y, o.z, rd.x);
                    out[0] = make_float4(way.x, way.y, way.z, t);
                    go_on = true;
                } else {
                    const PtMaterial &m = s.materials[mi];
                    // compute_scattering_functions -> compute_differentials(ray) (interaction.rs:262-342) of the CAMERA ray, as k_shade's first vertex has them (kern_shade.h)
                    RayDiff rdiff; rdiff.has = false;
                    if (s.n_textures > 0 && (job.mask & (kAovAlbedo | kAovNormal))) {   // (depth alone reads no texture: no lens sample, no differentials)
                        const float4 c2 = reinterpret_cast<const float4 *>(ps.core)[4 * (size_t)pid + 2];   // {sobol index, pfilm}
                        const uint64_t index = (uint64_t)__float_as_uint(c2.x) | ((uint64_t)__float_as_uint(c2.y) << 32);
                        P2 plens_u(0.0f, 0.0f);
                        if (rc.lens_radius > 0.0f) plens_u = rc.halton.enabled ? P2(halton_sample_dimension(tabs, rc.halton, index, 3u), halton_sample_dimension(tabs, rc.halton, index, 4u))
                                                                              : P2(sobol_sample_float(tabs.m32, index, 3u), sobol_sample_float(tabs.m32, index, 4u));
                        rdiff = camera_ray_differentials(rc, c2.z, c2.w, plens_u, V3(way.x, way.y, way.z), rd);
                    }
                    const TexCtx tctx = compute_differentials(si, rdiff);
                    V3 n = si.sh_n;
                    // bump() (core/material.rs:46-87). NOTE: the body is k_shade's (kern_shade.h, `if (mi != PT_NONE && s.materials[mi].tex[PT_MP_BUMP] >= 0)`), restated here: as one
                    // inlined device helper called from both, the textured k_shade forms came out of the compiler with other registers (k_shade<1, 2, 0> 63 -> 64 AGPRs, <1, 2, 1>
                    // 52 -> 54; profiles/r6/NOTES.md section 15), and those kernels' code objects do not move for a tidier source. A fix to either belongs in both.
                    if ((job.mask & kAovNormal) && m.tex[PT_MP_BUMP] >= 0) {
                        const int dtex = m.tex[PT_MP_BUMP];
                        TexCtx e = tctx;
                        float du = 0.5f * (fabsf(tctx.dudx) + fabsf(tctx.dudy));
                        if (du == 0.0f) du = 0.0005f;
                        e.p = si.p + si.sh_dpdu * du; e.uv = P2(si.uv.x + du, si.uv.y + 0.0f);
                        const float udisplace = tex_eval(s, dtex, e).r;
                        float dv = 0.5f * (fabsf(tctx.dvdx) + fabsf(tctx.dvdy));
                        if (dv == 0.0f) dv = 0.0005f;
                        e.p = si.p + si.sh_dpdv * dv; e.uv = P2(si.uv.x + 0.0f, si.uv.y + dv);
                        const float vdisplace = tex_eval(s, dtex, e).r;
                        const float displace = tex_eval(s, dtex, tctx).r;
                        const V3 bdpdu = si.sh_dpdu + si.sh_n * ((udisplace - displace) / du) + si.sh_dndu * displace;
                        const V3 bdpdv = si.sh_dpdv + si.sh_n * ((vdisplace - displace) / dv) + si.sh_dndv * displace;
                        n = normalize(cross(bdpdu, bdpdv));   // set_shading_geometry(.., false), interaction.rs:228-249
                        if (si.has_shape) { if (si.shape_flip) n = -n; n = face_forward(n, si.n); }
                    }
                    n = face_forward(n, -rd);
                    RGB a(0.0f);
                    if (job.mask & kAovAlbedo) {
                        const TexMatEval E{s, tctx};
                        if (m.type == PT_MAT_MIX) {   // mix.rs:25-50: material 1 scaled by "amount", material 2 -- on a fresh interaction, no differentials -- by 1 - amount
                            const RGB s1 = E.spec(m, PT_MP_KD, m.kd).clamps(0.0f, PT_INF);
                            const RGB s2 = RGB(1.0f - s1.r, 1.0f - s1.g, 1.0f - s1.b).clamps(0.0f, PT_INF);
                            a = s1 * leaf_albedo(s.materials[m.mix[0]], E) + s2 * leaf_albedo(s.materials[m.mix[1]], E.plain());
                        } else a = leaf_albedo(m, E);
                    }
                    out[0] = make_float4(a.r, a.g, a.b, t);
                    out[1] = make_float4(n.x, n.y, n.z, __uint_as_float(kAovSurface));
                }
            }
        }
        // one atomic per wave: its continuing lanes take consecutive queue entries, in lane order
        const uint32_t at = wave_reserve(job.next_count, go_on, 1u);
        if (go_on) job.next[at] = pid;
    }
}

// One thread per pixel slot, its s_count samples in sample order: FilmTile::add_sample's footprint and weights (film.rs:292-331) as film_slot applies them (kern_film.h) --
// the thread's own pixel accumulated in registers from the planes' present values and written back once, other pixels by float atomics --, for up to ten sums instead of
// the film's four, with neither sanitising nor a luminance clamp. A sample is one splat per pixel it reaches, whatever the number of planes.
__global__ __launch_bounds__(256) void k_aov_film(RenderConst rc, PathSoA ps, const float4 *rec, const float *filter_table, AovPlanes planes, DevCounters *counters) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long splats = 0;
    int32_t px, py;
    if (slot < rc.n_pix_slots && slot_to_pixel(rc, slot, px, py)) {
        const FilmRect tb = tile_footprint<true>(rc, slot_tile(rc, slot >> 8));
        const float invrx = 1.0f / rc.filter_radius[0], invry = 1.0f / rc.filter_radius[1];
        const bool own_ok = px >= tb.x0 && px < tb.x1 && py >= tb.y0 && py < tb.y1;
        // sums 0-3 albedo, 4-7 normal, 8-9 depth
        auto sum_ptr = [&](int k, int64_t x, int64_t y) -> float * {
            const size_t pix = (size_t)(y - rc.crop[1]) * rc.film_w + (size_t)(x - rc.crop[0]);
            float *base = k < 4 ? planes.albedo : k < 8 ? planes.normal : planes.depth;
            return base ? base + (k < 8 ? 4 * pix + (size_t)(k & 3) : 2 * pix + (size_t)(k - 8)) : nullptr;
        };
        float seed[10], acc[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            float *own = own_ok ? sum_ptr(k, px, py) : nullptr;
            seed[k] = own ? __hip_atomic_load(own, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
            acc[k] = seed[k];
        }
        for (uint32_t sl = 0; sl < rc.s_count; ++sl) {
            const uint32_t pid = sl * rc.n_pix_slots + slot;
            const float4 c2 = reinterpret_cast<const float4 *>(ps.core)[4 * (size_t)pid + 2], v0 = rec[2 * (size_t)pid], v1 = rec[2 * (size_t)pid + 1];
            const bool surface = __float_as_uint(v1.w) == kAovSurface;
            const float dx = c2.z - 0.5f, dy = c2.w - 0.5f;   // pfilm
            const int64_t p0x = max(f2i_sat(ceilf(dx - rc.filter_radius[0])), tb.x0), p0y = max(f2i_sat(ceilf(dy - rc.filter_radius[1])), tb.y0);
            const int64_t p1x = min(f2i_sat(floorf(dx + rc.filter_radius[0])) + 1, tb.x1), p1y = min(f2i_sat(floorf(dy + rc.filter_radius[1])) + 1, tb.y1);
            for (int64_t y = p0y; y < p1y; ++y) {
                const float fy = fabsf(((float)y - dy) * invry * 16.0f);
                const uint32_t iy = min(f2u32_sat(floorf(fy)), 15u);
                for (int64_t x = p0x; x < p1x; ++x) {
                    const float fx = fabsf(((float)x - dx) * invrx * 16.0f);
                    const uint32_t ix = min(f2u32_sat(floorf(fx)), 15u);
                    const float fw = filter_table[iy * 16 + ix];
                    const float v[10] = {v0.x * fw, v0.y * fw, v0.z * fw, fw, v1.x * fw, v1.y * fw, v1.z * fw, fw, v0.w * fw, fw};
                    const bool own = own_ok && x == (int64_t)px && y == (int64_t)py;
#pragma unroll
                    for (int k = 0; k < 10; ++k) {
                        if (k < 4 ? (k < 3 && !surface) : !surface) continue;   // a miss adds its weight to the albedo plane only
                        if (own) acc[k] += v[k];
                        else if (float *dst = sum_ptr(k, x, y)) atomicAdd(dst, v[k]);
                    }
                    splats++;
                }
            }
        }
        if (own_ok) {
#pragma unroll
            for (int k = 0; k < 10; ++k) {
                float *own = sum_ptr(k, px, py);
                if (!own || __float_as_uint(acc[k]) == __float_as_uint(seed[k])) continue;
                const uint32_t old = atomicCAS((uint32_t *)own, __float_as_uint(seed[k]), __float_as_uint(acc[k]));
                if (old != __float_as_uint(seed[k])) atomicAdd(own, acc[k] - seed[k]);
            }
        }
    }
    counter_add(&counters->splats, splats);
}

}  // namespace ptaov
