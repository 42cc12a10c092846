// aov_kernels.h -- the kernels of the feature buffers (include/mi355aov.h). Camera rays (k_generate) and their closest hits (k_trace) are libmi355pt's; this file adds
// the two steps behind them: k_aov leaves a camera sample's albedo, shading normal and depth in a record of its own -- or sends the ray on behind a surface without a
// material --, k_aov_film splats the records of a pixel slot's samples onto the planes with the film's filter weights, in sample order.
// The ID mattes (pt_matte_render) take the same route with k_matte -- the hit's ids, no interaction -- and k_matte_film, which gathers per FILM pixel instead of scattering;
// k_matte_mask extracts the coverage of a list of ids from a layer's tables.
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

// ---- ID mattes (include/mi355aov.h: pt_matte_render) -------------------------------------------------------------------------------------------------------------------

enum : uint32_t { kMatteMaterial = 1u, kMatteInstance = 2u, kMatteGroup = 4u };   // the layers the caller wants (MatteTables::mask, wave-uniform)
constexpr int kMatteSlots = 8;                                                    // PT_MATTE_SLOTS

// A camera sample's ids, one quad per path id: {material, instance, group, kAovMiss | kAovSurface}.
struct MatteJob {
    uint4 *rec;
    uint32_t *next, *next_count;   // the continuation queue, as AovJob's
    const uint32_t *prim_group;    // device, DeviceScene::n_prims entries; NULL: the group layer is not wanted
};
// PtMattePixel as the kernels move it: five quads.
struct MatteTable {
    uint32_t id[kMatteSlots]; float w[kMatteSlots];
    uint32_t n_ids; float w_total, w_other; uint32_t reserved;
};
static_assert(sizeof(MatteTable) == 80, "PtMattePixel is 80 bytes");
struct MatteTables { uint4 *layer[3]; uint32_t mask; };   // device, one table per pixel of the cropped film; NULL: not wanted

PT_DEV void matte_load(const uint4 *q, MatteTable &t) {
    const uint4 a = q[0], b = q[1], c = q[2], d = q[3], e = q[4];
    t.id[0] = a.x; t.id[1] = a.y; t.id[2] = a.z; t.id[3] = a.w; t.id[4] = b.x; t.id[5] = b.y; t.id[6] = b.z; t.id[7] = b.w;
    t.w[0] = __uint_as_float(c.x); t.w[1] = __uint_as_float(c.y); t.w[2] = __uint_as_float(c.z); t.w[3] = __uint_as_float(c.w);
    t.w[4] = __uint_as_float(d.x); t.w[5] = __uint_as_float(d.y); t.w[6] = __uint_as_float(d.z); t.w[7] = __uint_as_float(d.w);
    t.n_ids = e.x; t.w_total = __uint_as_float(e.y); t.w_other = __uint_as_float(e.z); t.reserved = e.w;
}
PT_DEV void matte_store(uint4 *q, const MatteTable &t) {
    q[0] = make_uint4(t.id[0], t.id[1], t.id[2], t.id[3]); q[1] = make_uint4(t.id[4], t.id[5], t.id[6], t.id[7]);
    q[2] = make_uint4(__float_as_uint(t.w[0]), __float_as_uint(t.w[1]), __float_as_uint(t.w[2]), __float_as_uint(t.w[3]));
    q[3] = make_uint4(__float_as_uint(t.w[4]), __float_as_uint(t.w[5]), __float_as_uint(t.w[6]), __float_as_uint(t.w[7]));
    q[4] = make_uint4(t.n_ids, __float_as_uint(t.w_total), __float_as_uint(t.w_other), t.reserved);
}
// One contribution of weight fw with the id `id` (include/mi355aov.h has the three cases). Every index below is a constant once the loops are unrolled: the table stays
// in registers (a dynamically indexed slot would send it to scratch).
PT_DEV void matte_add(MatteTable &t, uint32_t id, float fw) {
    bool found = false;
#pragma unroll
    for (int k = 0; k < kMatteSlots; ++k) {
        const bool here = (uint32_t)k < t.n_ids && t.id[k] == id;
        t.w[k] = here ? t.w[k] + fw : t.w[k];
        found = found || here;
    }
    if (!found) {
        if (t.n_ids < (uint32_t)kMatteSlots) {
#pragma unroll
            for (int k = 0; k < kMatteSlots; ++k) {
                const bool here = (uint32_t)k == t.n_ids;
                t.id[k] = here ? id : t.id[k];
                t.w[k] = here ? fw : t.w[k];
            }
            t.n_ids++;
        } else t.w_other += fw;
    }
}

// k_aov's sibling: one lane per traced ray of the queue, the first surface with a material ends the sample -- with its ids, nothing else. The interaction is rebuilt only
// where a ray goes on behind a surface without a material (its spawn point needs p, p_error and n).
template <bool SPH>
__global__ __launch_bounds__(256, 1) void k_matte(DeviceScene s, PathSoA ps, const uint32_t *queue, const uint32_t *count_ptr, MatteJob job) {
    const uint32_t count = *count_ptr;
    const uint32_t rounded = (count + 63u) & ~63u;   // whole waves iterate together (one queue reservation per wave)
    for (uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x; qi < rounded; qi += gridDim.x * blockDim.x) {
        bool go_on = false;
        uint32_t pid = 0;
        if (qi < count) {
            pid = queue[qi];
            const float4 *hq = reinterpret_cast<const float4 *>(ps.hit) + 2 * (size_t)pid;
            const float4 h0 = hq[0], h1 = hq[1];
            const uint32_t hp = __float_as_uint(h0.x);
            if (hp == PT_NONE) job.rec[pid] = make_uint4(0u, 0u, 0u, kAovMiss);
            else {
                const uint32_t inst = SPH ? __float_as_uint(h1.x) : PT_NONE;
                const uint32_t mi = packet_material(s, __float_as_uint(h1.w), hp);
                if (mi == PT_NONE) {   // path.rs:124-129, as k_aov
                    float4 *rq = reinterpret_cast<float4 *>(ps.ray) + 2 * (size_t)pid;
                    const float4 r0 = rq[0], r1 = rq[1];
                    const V3 ro(r0.x, r0.y, r0.z), rd(r0.w, r1.x, r1.y);
                    SurfaceInteraction si;
                    fill_hit_pkt<SPH>(s, __float_as_uint(h1.z), inst, ro, rd, h0.y, h0.z, h0.w, si);
                    IData it; it.p = si.p; it.p_error = si.p_error; it.n = si.n;
                    V3 o; spawn_ray(it, rd, o);
                    rq[0] = make_float4(o.x, o.y, o.z, rd.x);
                    go_on = true;
                } else job.rec[pid] = make_uint4(mi, inst == PT_NONE ? 0u : 1u + inst, job.prim_group ? job.prim_group[hp] : 0u, kAovSurface);
            }
        }
        const uint32_t at = wave_reserve(job.next_count, go_on, 1u);
        if (go_on) job.next[at] = pid;
    }
}

// One thread per FILM pixel: a gather. The pixel's tables are loaded once, the pass's samples that reach the pixel are added in the contract's order -- sample numbers
// ascending, within one the source pixels in raster order -- and the tables written back once: no atomics, one chain of additions per pixel whatever the filter. The
// candidates are the source pixels within ceil(radius + 0.5) of the pixel (a sample of pixel q has pfilm in [q, q + 1]), clipped to the sample bounds and the integrator's
// pixel_bounds (slot_to_pixel: pixels outside them have no samples); each sample is tested with FilmTile::add_sample's own footprint, as k_aov_film forms it. The tile's
// film footprint that k_aov_film also clips to holds every pixel of the crop window a sample of the tile reaches (kern_film.h: tile_footprint<true> rounds the same sums
// of the tile's edges), so the crop window -- the pixels there are threads for -- is the only clip. Needs every tile's samples: tile_world == 1 and no tile list.
__global__ __launch_bounds__(256) void k_matte_film(RenderConst rc, PathSoA ps, const uint4 *rec, const float *filter_table, MatteTables tabs, DevCounters *counters) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long splats = 0;
    if (pix < rc.film_w * rc.film_h) {
        const int32_t px = rc.crop[0] + (int32_t)(pix % rc.film_w), py = rc.crop[1] + (int32_t)(pix / rc.film_w);
        const float invrx = 1.0f / rc.filter_radius[0], invry = 1.0f / rc.filter_radius[1];
        const int32_t reach_x = (int32_t)min(f2i_sat(ceilf(rc.filter_radius[0] + 0.5f)), (int64_t)(1 << 20)), reach_y = (int32_t)min(f2i_sat(ceilf(rc.filter_radius[1] + 0.5f)), (int64_t)(1 << 20));
        const int32_t qx0 = max(px - reach_x, max(rc.sample_bounds[0], rc.pixel_bounds[0])), qx1 = min(px + reach_x + 1, min(rc.sample_bounds[2], rc.pixel_bounds[2]));
        const int32_t qy0 = max(py - reach_y, max(rc.sample_bounds[1], rc.pixel_bounds[1])), qy1 = min(py + reach_y + 1, min(rc.sample_bounds[3], rc.pixel_bounds[3]));
        MatteTable t[3];
#pragma unroll
        for (int l = 0; l < 3; ++l) if (tabs.mask & (1u << l)) matte_load(tabs.layer[l] + 5 * (size_t)pix, t[l]);
        for (uint32_t sl = 0; sl < rc.s_count; ++sl) {
            for (int32_t qy = qy0; qy < qy1; ++qy) {
                const uint32_t ry = (uint32_t)(qy - rc.sample_bounds[1]);
                for (int32_t qx = qx0; qx < qx1; ++qx) {
                    const uint32_t rx = (uint32_t)(qx - rc.sample_bounds[0]);
                    const uint32_t slot = ((ry >> 4) * rc.ntx + (rx >> 4)) * 256u + (ry & 15u) * 16u + (rx & 15u);   // slot_to_pixel's inverse
                    const size_t pid = (size_t)sl * rc.n_pix_slots + slot;
                    const float4 c2 = reinterpret_cast<const float4 *>(ps.core)[4 * pid + 2];
                    const float dx = c2.z - 0.5f, dy = c2.w - 0.5f;   // pfilm
                    const int64_t p0x = f2i_sat(ceilf(dx - rc.filter_radius[0])), p0y = f2i_sat(ceilf(dy - rc.filter_radius[1]));
                    const int64_t p1x = f2i_sat(floorf(dx + rc.filter_radius[0])) + 1, p1y = f2i_sat(floorf(dy + rc.filter_radius[1])) + 1;
                    if ((int64_t)px < p0x || (int64_t)px >= p1x || (int64_t)py < p0y || (int64_t)py >= p1y) continue;
                    const float fy = fabsf(((float)py - dy) * invry * 16.0f), fx = fabsf(((float)px - dx) * invrx * 16.0f);
                    const uint32_t iy = min(f2u32_sat(floorf(fy)), 15u), ix = min(f2u32_sat(floorf(fx)), 15u);
                    const float fw = filter_table[iy * 16 + ix];
                    const uint4 v = rec[pid];
                    const uint32_t ids[3] = {v.x, v.y, v.z};
#pragma unroll
                    for (int l = 0; l < 3; ++l) {
                        if (!(tabs.mask & (1u << l))) continue;
                        if (v.w == kAovSurface) matte_add(t[l], ids[l], fw);
                        t[l].w_total += fw;
                    }
                    splats++;
                }
            }
        }
#pragma unroll
        for (int l = 0; l < 3; ++l) if (tabs.mask & (1u << l)) matte_store(tabs.layer[l] + 5 * (size_t)pix, t[l]);
    }
    counter_add(&counters->splats, splats);
}

// mask[p] = the sum, in slot order, of the weights of pixel p's slots whose id is in `ids`, over w_total; 0 where w_total == 0. The list sits in LDS (n_ids <= 4096).
constexpr uint32_t kMatteMaskIds = 4096;
__global__ __launch_bounds__(256) void k_matte_mask(const uint4 *table, uint32_t n_pixels, const uint32_t *ids, uint32_t n_ids, float *mask) {
    __shared__ uint32_t list[kMatteMaskIds];
    for (uint32_t i = threadIdx.x; i < n_ids; i += blockDim.x) list[i] = ids[i];
    __syncthreads();
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= n_pixels) return;
    MatteTable t;
    matte_load(table + 5 * (size_t)pix, t);
    uint32_t in = 0;   // bit k: slot k's id is in the list
    for (uint32_t i = 0; i < n_ids; ++i) {
        const uint32_t id = list[i];
#pragma unroll
        for (int k = 0; k < kMatteSlots; ++k) in |= (t.id[k] == id ? 1u : 0u) << k;
    }
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < kMatteSlots; ++k) if ((uint32_t)k < t.n_ids && (in >> k & 1u)) sum += t.w[k];
    mask[pix] = t.w_total != 0.0f ? sum / t.w_total : 0.0f;
}

}  // namespace ptaov
