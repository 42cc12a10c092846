// bake_kernels.h -- the kernels of libmi355bake.so (include/mi355bake.h, where the contract stands operation by operation). The walks of their rays (k_trace, any-hit
// and closest-hit) are libmi355pt's; this file is the front of the pipe and its end. Kernels are thin: what two of them do alike is a force-inlined body, written once.
// Every atlas call:
//   k_bake_top, k_bake_check  the primitives of the top-level accelerator (a primitive of an instanced object is no bake target); why a selected primitive is none
//   k_bake_raster             selected triangles -> atomicMin on the owner map
//   k_bake_points             one thread per texel: the owner's interaction (texel_interaction) -> position and shading normal
//   k_bake_covered, k_bake_dilate<CH>   pt_bake_dilate: the gutter fill, one iteration per launch
// The ray kernels, one item (a texel sample, a point sample) per lane, a wave = an 8 x 8 tile or 64 points of ONE sample number:
//   ao_chunk_rays      the body of k_bake_rays (from the owner's interaction) and k_bake_transfer_rays (from the source hit; ray_surface tells them apart): one
//                      reservation of kn ray ids per wave (wave_reserve), the base, ao_ray (side/ao_rays.h: the rays libmi355ao spawns from a camera hit) per element
//   light_group_rays   the body of k_bake_light_rays<SPH> (light_ray: Light::sample_li, cosine and side test) and k_bake_sh_rays<SPH> (sh_ray: from a point without
//                      surface; the ray's wi is kept): the wave-uniform light index, kLightGroup samples in registers, ONE reservation per group, the id table
// The accumulate kernels, one thread per texel or point, additions in (sample, element) order:
//   k_bake_accum       ao_w += the unoccluded rays' wi and w (the transfer bake's too, with the detail-hit map in the owner map's place)
//   k_bake_light_accum light_w += {E, 1}        k_bake_sh_accum   sh_w += {E * Y_q(wi), 1}, the basis evaluated here
// The transfer bake's projection (`t`: the scene whose atlas is filled, `s`: the scene the rays see):
//   k_bake_project, k_bake_transfer_points   the projection ray of an owned texel; its hit classified -> hit_prim, height, the three vector planes, the hit record
// The probes (pt_bake_*_rays), single queries by the functions the ray kernels call:
//   k_bake_probe, k_bake_transfer_probe, k_bake_light_probe<SPH>, k_bake_sh_probe<SPH>; the two light probes leave one row (store_light_row)
// No atomics other than the owner map's atomicMin and the per-wave ray-id reservations.
#pragma once
#include "../csrc/kern_decl.h"
#include "../side/ao_rays.h"

namespace ptbake {
using namespace ptside;

constexpr uint32_t kLightGroup = 4;                  // k_bake_light_rays: light samples of a texel sample whose rays share one ray-id reservation
constexpr uint32_t kShAhead = 4;                     // k_bake_sh_accum: steps of a point's walk whose loads are in flight together
constexpr uint32_t kRasterOwnTexels = 16;           // k_bake_raster: a triangle whose texel box holds at most this many texels is walked by its own lane

// `slots`: the texel samples of one sample number in the order the ray kernel walks them -- 8 x 8 texel tiles, one per wave, so that the rays of a wave start from a
// square patch of the surface and not from a line of 64 texels (measured against raster order on a 2048^2 bake of a 4.3 M-triangle mesh: the any-hit launch 129.8 ms
// against 139.4 ms, profiles/r6/NOTES.md). The tiles of the last column / row hang over the atlas: those slots have no texel.
struct BakeAtlas { uint32_t width, height, n_texels, tiles_x, slots; };
PT_HD BakeAtlas make_atlas(uint32_t width, uint32_t height) { return BakeAtlas{width, height, width * height, (width + 7u) / 8u, ((width + 7u) / 8u) * ((height + 7u) / 8u) * 64u}; }
PT_DEV uint32_t slot_texel(const BakeAtlas &a, uint32_t slot) {   // PT_NONE: the slot hangs over the atlas
    const uint32_t tile = slot >> 6, lane = slot & 63u;
    const uint32_t x = (tile % a.tiles_x) * 8u + (lane & 7u), y = (tile / a.tiles_x) * 8u + (lane >> 3);
    return (x < a.width && y < a.height) ? y * a.width + x : PT_NONE;
}
PT_DEV uint32_t texel_slot(const BakeAtlas &a, uint32_t texel) {
    const uint32_t x = texel % a.width, y = texel / a.width;
    return (((y >> 3) * a.tiles_x + (x >> 3)) << 6) | ((y & 7u) << 3) | (x & 7u);
}

// One chunk of AO rays of the texel samples [s_begin, s_begin + s_count) of every owned texel; base: [slots * s_count], PT_NONE for a texel without owner
struct BakeJob : AOChunk {
    uint32_t s_begin, s_count;
    const uint32_t *owner;   // [texels]
    float4 *ao_w;            // [texels]
};

// Texel centre (mi355bake.h "Texel centres")
PT_DEV P2 texel_centre(const BakeAtlas &a, uint32_t x, uint32_t y) { return P2(((float)x + 0.5f) / (float)a.width, ((float)y + 0.5f) / (float)a.height); }

// The barycentrics of c in the UV triangle (mi355bake.h "Ownership"); false: the triangle does not contain c
PT_DEV bool uv_barycentrics(P2 uv0, P2 uv1, P2 uv2, P2 c, float &b0, float &b1, float &b2) {
    const float e0x = uv1.x - uv0.x, e0y = uv1.y - uv0.y, e1x = uv2.x - uv0.x, e1y = uv2.y - uv0.y, dx = c.x - uv0.x, dy = c.y - uv0.y;
    const float det = e0x * e1y - e0y * e1x;
    if (det == 0.0f) return false;
    b1 = (dx * e1y - dy * e1x) / det;
    b2 = (e0x * dy - e0y * dx) / det;
    b0 = 1.0f - b1 - b2;
    return b0 >= 0.0f && b1 >= 0.0f && b2 >= 0.0f;
}

PT_DEV void tri_vertex_uvs(const DeviceScene &s, uint32_t tri, P2 &uv0, P2 &uv1, P2 &uv2) {
    const uint32_t i0 = s.indices[3 * tri], i1 = s.indices[3 * tri + 1], i2 = s.indices[3 * tri + 2];
    uv0 = P2(s.UV[2 * i0], s.UV[2 * i0 + 1]); uv1 = P2(s.UV[2 * i1], s.UV[2 * i1 + 1]); uv2 = P2(s.UV[2 * i2], s.UV[2 * i2 + 1]);
}

// The interaction of a texel's owner at the texel's centre (mi355bake.h "The surface point"): Triangle::intersect's, by the function the shade and AO kernels rebuild
// their hits with. The owner contains the centre (k_bake_raster decided so with the same arithmetic), so the barycentrics are the ones it saw.
PT_DEV void texel_interaction(const DeviceScene &s, const BakeAtlas &a, uint32_t texel, uint32_t prim, SurfaceInteraction &si) {
    const uint32_t tri = s.prim_shape[prim] & 0x3fffffffu;
    P2 uv0, uv1, uv2; tri_vertex_uvs(s, tri, uv0, uv1, uv2);
    float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
    uv_barycentrics(uv0, uv1, uv2, texel_centre(a, texel % a.width, texel / a.width), b0, b1, b2);
    tri_fill_interaction(s, tri, V3(0.0f, 0.0f, 0.0f), b0, b1, b2, true, si);
}

// The frame of ao.rs:77-80 without the face-forward (there is no camera ray): s = normalize(dpdu), t = cross(n, s), n
PT_DEV AOFrame bake_frame(const SurfaceInteraction &si) { AOFrame f; f.n = si.n; f.sv = normalize(si.dpdu); f.tv = cross(si.n, f.sv); return f; }

// The packets [0, n_top) are the top-level accelerator's, one per top-level primitive or instance (scene_plan.hip: the packet order of every accelerator)
__global__ __launch_bounds__(256) void k_bake_top(DeviceScene s, uint32_t n_top, uint8_t *top) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_top) return;
    const uint32_t prim = s.leaf[i].prim;
    if (!(s.leaf[i].flags & TP_INSTANCE) && prim < s.n_prims) top[prim] = 1;
}

// Why a selected primitive is no bake target (0: it is one). One thread per selected primitive leaves its code; a block leaves whether any of its 256 has one, so that
// the host reads a word per block and, only when a selection is refused, the codes of one block.
enum { kBakeOk = 0, kBakeQuadric = 1, kBakeInstanced = 2, kBakeNoUV = 3 };
__global__ __launch_bounds__(256) void k_bake_check(DeviceScene s, const uint8_t *top, const uint32_t *selected, uint32_t n_selected, uint8_t *code, uint32_t *block_refused) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c = kBakeOk;
    if (i < n_selected) {
        const uint32_t prim = selected[i], sh = s.prim_shape[prim], tri = sh & 0x3fffffffu;
        if ((sh >> 30) != PT_SHAPE_TRIANGLE) c = kBakeQuadric;
        else if (!top[prim]) c = kBakeInstanced;
        else if (tri >= s.n_triangles || !(s.tri_flags[tri] & PT_TRI_HAS_UV)) c = kBakeNoUV;
        code[i] = (uint8_t)c;
    }
    const int any = __syncthreads_or(c != kBakeOk);
    if (threadIdx.x == 0) block_refused[blockIdx.x] = any ? 1u : 0u;
}

// The texel box of a triangle (mi355bake.h "Ownership": part of the contract, every operation float32 in this order): the texels whose centres the UV bounds can hold,
// with a margin of a sixteenth of a texel plus size * 2.4e-7 -- more than the roundings of the bounds and of the centres amount to, so a centre the barycentrics of a
// well-conditioned triangle contain is never cut off. It is a second condition and not a mere speed-up: the barycentrics of a sliver with a tiny determinant round
// without bound and "contain" centres far from the triangle; the box denies it those. false: the triangle owns nothing.
PT_DEV bool texel_box(const BakeAtlas &a, P2 uv0, P2 uv1, P2 uv2, uint32_t &x0, uint32_t &x1, uint32_t &y0, uint32_t &y1) {
    const float ulo = fminf(uv0.x, fminf(uv1.x, uv2.x)) * (float)a.width, uhi = fmaxf(uv0.x, fmaxf(uv1.x, uv2.x)) * (float)a.width;
    const float vlo = fminf(uv0.y, fminf(uv1.y, uv2.y)) * (float)a.height, vhi = fmaxf(uv0.y, fmaxf(uv1.y, uv2.y)) * (float)a.height;
    // (a NaN, an infinity or a bound of 1e30 texels and more: no box)
    if (!(ulo <= uhi && vlo <= vhi && fabsf(ulo) < 1e30f && fabsf(uhi) < 1e30f && fabsf(vlo) < 1e30f && fabsf(vhi) < 1e30f)) return false;
    const float mx = 0.5625f + (float)a.width * 2.4e-7f, my = 0.5625f + (float)a.height * 2.4e-7f;
    const float fx0 = fmaxf(floorf(ulo - mx), 0.0f), fx1 = fminf(ceilf(uhi - 1.0f + mx), (float)(a.width - 1u));
    const float fy0 = fmaxf(floorf(vlo - my), 0.0f), fy1 = fminf(ceilf(vhi - 1.0f + my), (float)(a.height - 1u));
    if (!(fx0 <= fx1 && fy0 <= fy1)) return false;
    x0 = (uint32_t)fx0; x1 = min((uint32_t)fx1, a.width - 1u); y0 = (uint32_t)fy0; y1 = min((uint32_t)fy1, a.height - 1u);   // ((float)(size - 1) rounds up beyond 2^24)
    return true;
}

// What a lane knows of its triangle: the UVs and its texel box clipped to rows [row0, row1) of the atlas
struct RasterTri { P2 uv0, uv1, uv2; uint32_t prim, x0, y0, nx, ny; };
PT_DEV void raster_texels(const BakeAtlas &a, const RasterTri &t, uint32_t first, uint32_t step, uint32_t *owner) {
    const uint32_t n = t.nx * t.ny;
    for (uint32_t i = first; i < n; i += step) {
        const uint32_t x = t.x0 + i % t.nx, y = t.y0 + i / t.nx;
        float b0, b1, b2;
        if (uv_barycentrics(t.uv0, t.uv1, t.uv2, texel_centre(a, x, y), b0, b1, b2)) atomicMin(&owner[(size_t)y * a.width + x], t.prim);
    }
}
// Selected triangles -> owner map. blockIdx.y is a band of `band_rows` atlas rows: a lane sets its triangle up and clips its box to the band. A small box is walked by
// the lane itself; the large ones of a wave are taken one after the other by all 64 lanes (the set-up travels by __shfl), so that a quad over the whole atlas is
// rastered by every wave of every band and not by one thread. The host gives one band to a selection of many triangles and many bands to a selection of few.
__global__ __launch_bounds__(256) void k_bake_raster(DeviceScene s, BakeAtlas a, const uint32_t *selected, uint32_t n_selected, uint32_t band_rows, uint32_t *owner) {
    const uint32_t row0 = blockIdx.y * band_rows, row1 = min(a.height, row0 + band_rows);
    const uint32_t rounded = (n_selected + 63u) & ~63u;   // whole waves iterate together (the large boxes are shared)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < rounded; i += gridDim.x * blockDim.x) {
        RasterTri t; t.nx = t.ny = 0; t.x0 = t.y0 = 0; t.prim = PT_NONE;
        if (i < n_selected) {
            t.prim = selected[i];
            tri_vertex_uvs(s, s.prim_shape[t.prim] & 0x3fffffffu, t.uv0, t.uv1, t.uv2);
            uint32_t x0, x1, y0, y1;
            if (texel_box(a, t.uv0, t.uv1, t.uv2, x0, x1, y0, y1)) {
                y0 = max(y0, row0); y1 = min(y1, row1 - 1u);
                if (y0 <= y1) { t.x0 = x0; t.y0 = y0; t.nx = x1 - x0 + 1u; t.ny = y1 - y0 + 1u; }
            }
        }
        const uint32_t n = t.nx * t.ny;   // (<= 2^28 texels)
        if (n != 0 && n <= kRasterOwnTexels) raster_texels(a, t, 0u, 1u, owner);
        unsigned long long large = __ballot(n > kRasterOwnTexels);
        while (large) {
            const int src = __ffsll((long long)large) - 1;
            large &= large - 1ull;
            RasterTri g;
            g.uv0 = P2(__shfl(t.uv0.x, src), __shfl(t.uv0.y, src)); g.uv1 = P2(__shfl(t.uv1.x, src), __shfl(t.uv1.y, src)); g.uv2 = P2(__shfl(t.uv2.x, src), __shfl(t.uv2.y, src));
            g.prim = __shfl(t.prim, src); g.x0 = __shfl(t.x0, src); g.y0 = __shfl(t.y0, src); g.nx = __shfl(t.nx, src); g.ny = __shfl(t.ny, src);
            raster_texels(a, g, lane_id(), 64u, owner);
        }
    }
}

// position = p, normal = the normalised shading normal of the owner's interaction; zeros where the texel has no owner
__global__ __launch_bounds__(256) void k_bake_points(DeviceScene s, BakeAtlas a, const uint32_t *owner, float *position, float *normal) {
    const uint32_t texel = blockIdx.x * blockDim.x + threadIdx.x;
    if (texel >= a.n_texels) return;
    const uint32_t prim = owner[texel];
    V3 p(0.0f, 0.0f, 0.0f), n(0.0f, 0.0f, 0.0f);
    if (prim != PT_NONE) {
        SurfaceInteraction si;
        texel_interaction(s, a, texel, prim, si);
        p = si.p; n = normalize(si.sh_n);
    }
    if (position) { position[3 * (size_t)texel] = p.x; position[3 * (size_t)texel + 1] = p.y; position[3 * (size_t)texel + 2] = p.z; }
    if (normal) { normal[3 * (size_t)texel] = n.x; normal[3 * (size_t)texel + 1] = n.y; normal[3 * (size_t)texel + 2] = n.z; }
}

// Where a texel's AO rays leave: the owner's interaction at the texel's centre
PT_DEV AOFrame ray_surface(const DeviceScene &s, const BakeAtlas &a, const BakeJob &, uint32_t texel, uint32_t prim, SurfaceInteraction &si) { texel_interaction(s, a, texel, prim, si); return bake_frame(si); }

// The body of k_bake_rays and k_bake_transfer_rays, per texel sample of the pass (item = sample-in-pass * slots + slot: the lanes of a wave are neighbouring texels of
// one sample; the kernels round the items up to whole waves, since there is one ray-id reservation per wave): this chunk's AO rays of sample `sl` of `texel`, whose
// job.owner entry `mark` is PT_NONE where it has no surface point. ray_surface(s, a, job, texel, mark, si) -- the job type's -- fills the interaction the rays leave
// and returns their frame. (The item loop stays in the kernels: under a kernel's launch bounds the index arithmetic compiles as it did.)
template <class Job>
PT_DEV void ao_chunk_rays(const DeviceScene &s, const RenderConst &rc, const SobolTables &tabs, const BakeAtlas &a, const Job &job, uint32_t total, uint32_t item, uint32_t texel, uint32_t sl, uint32_t mark) {
    const bool found = mark != PT_NONE;
    // one atomic per wave: the wave's owned texels take consecutive blocks of kn ray ids, in lane order
    const uint32_t first = wave_reserve(job.ray_count, found, job.kn);
    if (item >= total) return;
    if (!found) { job.base[item] = PT_NONE; return; }
    job.base[item] = first;
    SurfaceInteraction si;
    const AOFrame f = ray_surface(s, a, job, texel, mark, si);
    const int32_t px = (int32_t)(texel % a.width), py = (int32_t)(texel / a.width);
    const uint64_t sample = (uint64_t)job.s_begin + sl;
    const float nsf = (float)job.nsamples;
    for (uint32_t kk = 0; kk < job.kn; ++kk) {
        V3 o, wo; float w;
        ao_ray(rc, tabs, si, f, px, py, sample * job.nsamples + job.k0 + kk, job.cos_sample, nsf, o, wo, w);
        const uint32_t id = first + kk;
        job.ray[2 * (size_t)id] = make_float4(o.x, o.y, o.z, wo.x);
        job.ray[2 * (size_t)id + 1] = make_float4(wo.y, wo.z, 0.0f, 0.0f);
        job.w[id] = w;
    }
}

__global__ __launch_bounds__(256) void k_bake_rays(DeviceScene s, RenderConst rc, SobolTables tabs, BakeAtlas a, BakeJob job) {
    const uint32_t total = a.slots * job.s_count;
    const uint32_t rounded = (total + 63u) & ~63u;
    for (uint32_t item = blockIdx.x * blockDim.x + threadIdx.x; item < rounded; item += gridDim.x * blockDim.x) {
        uint32_t texel = PT_NONE, sl = 0, prim = PT_NONE;
        if (item < total) { texel = slot_texel(a, item % a.slots); sl = item / a.slots; if (texel != PT_NONE) prim = job.owner[texel]; }
        ao_chunk_rays(s, rc, tabs, a, job, total, item, texel, sl, prim);
    }
}

// ao_w += the unoccluded rays' wi and w, in (sample, element) order (ao.rs:96-98): one thread per texel walks the pass's samples in order and, in each, this chunk's
// elements. (A pass of more than one sample has ONE chunk -- the host sees to it --, so the chain of additions of a texel is (s, k) ascending however the job is cut.)
__global__ __launch_bounds__(256) void k_bake_accum(BakeAtlas a, BakeJob job) {
    const uint32_t texel = blockIdx.x * blockDim.x + threadIdx.x;
    if (texel >= a.n_texels) return;
    if (job.owner[texel] == PT_NONE) return;
    const uint32_t slot = texel_slot(a, texel);
    float4 acc = job.ao_w[texel];
    for (uint32_t sl = 0; sl < job.s_count; ++sl) {
        const uint32_t first = job.base[(size_t)sl * a.slots + slot];
        for (uint32_t kk = 0; kk < job.kn; ++kk) {
            const uint32_t id = first + kk;
            if (job.occluded[id]) continue;
            const float4 r0 = job.ray[2 * (size_t)id], r1 = job.ray[2 * (size_t)id + 1];
            acc.x += r0.w; acc.y += r1.x; acc.z += r1.y; acc.w += job.w[id];
        }
    }
    job.ao_w[texel] = acc;
}

// One iteration of pt_bake_dilate (mi355bake.h): src / covered -> dst / covered_next
template <int CH>
__global__ __launch_bounds__(256) void k_bake_dilate(BakeAtlas a, const float *src, const uint8_t *covered, float *dst, uint8_t *covered_next) {
    const uint32_t texel = blockIdx.x * blockDim.x + threadIdx.x;
    if (texel >= a.n_texels) return;
    const int32_t x = (int32_t)(texel % a.width), y = (int32_t)(texel / a.width);
    float sum[CH]; uint32_t n = 0;
    for (int c = 0; c < CH; ++c) sum[c] = 0.0f;
    const bool own = covered[texel] != 0;
    if (!own) {
        for (int32_t dy = -1; dy <= 1; ++dy) for (int32_t dx = -1; dx <= 1; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const int32_t nx = x + dx, ny = y + dy;
            if (nx < 0 || ny < 0 || nx >= (int32_t)a.width || ny >= (int32_t)a.height) continue;
            const size_t q = (size_t)ny * a.width + (size_t)nx;
            if (!covered[q]) continue;
            for (int c = 0; c < CH; ++c) sum[c] += src[q * CH + c];
            ++n;
        }
    }
    const bool fill = !own && n > 0;
    const float nf = (float)n;
    for (int c = 0; c < CH; ++c) dst[(size_t)texel * CH + c] = fill ? sum[c] / nf : src[(size_t)texel * CH + c];
    covered_next[texel] = (own || fill) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_bake_covered(BakeAtlas a, const uint32_t *owner, uint8_t *covered) {
    const uint32_t texel = blockIdx.x * blockDim.x + threadIdx.x;
    if (texel < a.n_texels) covered[texel] = owner[texel] != PT_NONE ? 1 : 0;
}

// pt_bake_rays: ray i = element[i] of sample[i] of texel[i], by ao_ray
__global__ __launch_bounds__(256) void k_bake_probe(DeviceScene s, RenderConst rc, SobolTables tabs, BakeAtlas a, const uint32_t *owner, uint32_t nsamples, uint32_t cos_sample, uint32_t n,
                                                    const uint32_t *texel, const uint32_t *sample, const uint32_t *element, float *out_o, float *out_d, float *out_w, uint8_t *found) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t tx = texel[i];
    const uint32_t prim = tx < a.n_texels ? owner[tx] : PT_NONE;
    V3 o(0.0f, 0.0f, 0.0f), wo(0.0f, 0.0f, 0.0f); float w = 0.0f;
    if (prim != PT_NONE) {
        SurfaceInteraction si;
        texel_interaction(s, a, tx, prim, si);
        ao_ray(rc, tabs, si, bake_frame(si), (int32_t)(tx % a.width), (int32_t)(tx / a.width), (uint64_t)sample[i] * nsamples + element[i], cos_sample, (float)nsamples, o, wo, w);
    }
    out_o[3 * (size_t)i] = o.x; out_o[3 * (size_t)i + 1] = o.y; out_o[3 * (size_t)i + 2] = o.z;
    out_d[3 * (size_t)i] = wo.x; out_d[3 * (size_t)i + 1] = wo.y; out_d[3 * (size_t)i + 2] = wo.z;
    out_w[i] = w; found[i] = prim != PT_NONE ? 1 : 0;
}

// ---- the transfer bake (mi355bake.h "Transfer"): `t` is the scene whose atlas is filled, `s` the scene the rays see

// The projection ray of an owned texel (contract step 2): from `front` above the target's surface along its normalised shading normal, straight down
PT_DEV void projection_ray(const SurfaceInteraction &si, float front, V3 &ns, V3 &o, V3 &d) { ns = normalize(si.sh_n); d = -ns; o = si.p + ns * front; }

// The tangent frame of a target texel (step 4): dpdu made orthogonal to ns, its partner on dpdv's side (a mirrored island keeps its handedness)
PT_DEV void tangent_frame(const SurfaceInteraction &si, V3 ns, V3 &sv, V3 &tv) {
    sv = si.dpdu - ns * dot(ns, si.dpdu);
    if (dot(sv, sv) > 0.0f) {
        sv = normalize(sv); tv = cross(ns, sv);
        if (dot(tv, si.dpdv) < 0.0f) tv = -tv;
    } else coordinate_system(ns, sv, tv);
}

// The interaction of a detail hit and the frame of its AO rays (step 5): ao.rs:77-80 with the projection ray as the camera ray. `flip`: face_forward(hs.n, -d) turned n round
PT_DEV AOFrame transfer_hit(const DeviceScene &s, float4 rec, bool flip, SurfaceInteraction &hs) {
    tri_fill_interaction(s, s.prim_shape[__float_as_uint(rec.x)] & 0x3fffffffu, V3(0.0f, 0.0f, 0.0f), rec.y, rec.z, rec.w, true, hs);
    AOFrame f; f.n = flip ? -hs.n : hs.n; f.sv = normalize(hs.dpdu); f.tv = cross(hs.n, f.sv); return f;
}

// Slots [slot0, slot0 + n_slots) of the tile order (slot0 a multiple of 64: a wave is a tile): ray ids in lane order, base[slot - slot0] = the texel's ray id or PT_NONE
__global__ __launch_bounds__(256) void k_bake_project(DeviceScene t, BakeAtlas a, const uint32_t *owner, uint32_t slot0, uint32_t n_slots, float front, float t_max, float4 *ray, uint32_t *base,
                                                      uint32_t *ray_count) {
    const uint32_t rounded = (n_slots + 63u) & ~63u;   // whole waves iterate together (one ray-id reservation per wave)
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < rounded; i += gridDim.x * blockDim.x) {
        uint32_t texel = PT_NONE, prim = PT_NONE;
        if (i < n_slots) { texel = slot_texel(a, slot0 + i); if (texel != PT_NONE) prim = owner[texel]; }
        const bool found = prim != PT_NONE;
        const uint32_t id = wave_reserve(ray_count, found, 1u);
        if (i >= n_slots) continue;
        if (!found) { base[i] = PT_NONE; continue; }
        base[i] = id;
        SurfaceInteraction si;
        texel_interaction(t, a, texel, prim, si);
        V3 ns, o, d; projection_ray(si, front, ns, o, d);
        ray[2 * (size_t)id] = make_float4(o.x, o.y, o.z, d.x);
        ray[2 * (size_t)id + 1] = make_float4(d.y, d.z, t_max, 0.0f);   // (per-ray t_max: k_trace reads it from the record)
    }
}

// The planes pt_bake_transfer writes (NULL: not wanted) and what the AO passes read: detail[texel] = PT_NONE, or -- a detail hit -- whether n was turned round;
// rec[texel] = {source primitive, b0, b1, b2} of a detail hit (both NULL when no AO is wanted)
struct TransferOut { uint32_t *hit_prim; float *height, *src_position, *src_normal, *tangent_normal; uint32_t *detail; float4 *rec; };
PT_DEV void store3(float *plane, uint32_t texel, V3 v) { if (plane) { plane[3 * (size_t)texel] = v.x; plane[3 * (size_t)texel + 1] = v.y; plane[3 * (size_t)texel + 2] = v.z; } }

// One thread per slot of the slice: the hit of the texel's projection ray (hit: {prim, b0, b1, b2}, hit_t, by ray id), classified (steps 3 and 4). `top`: k_bake_top's
// marks of the source scene
__global__ __launch_bounds__(256) void k_bake_transfer_points(DeviceScene t, DeviceScene s, BakeAtlas a, const uint32_t *owner, const uint8_t *top, uint32_t slot0, uint32_t n_slots,
                                                              const uint32_t *base, const float4 *hit, const float *hit_t, float front, TransferOut out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    const uint32_t texel = slot_texel(a, slot0 + i);
    if (texel == PT_NONE) return;
    uint32_t hit_prim = PT_NONE, detail = PT_NONE;
    float height = 0.0f;
    V3 p(0.0f, 0.0f, 0.0f), nh(0.0f, 0.0f, 0.0f), tn(0.0f, 0.0f, 0.0f);
    float4 rec = make_float4(__uint_as_float(PT_NONE), 0.0f, 0.0f, 0.0f);
    const uint32_t id = base[i];
    if (id != PT_NONE) {
        const float4 h = hit[id];
        hit_prim = __float_as_uint(h.x);
        if (hit_prim != PT_NONE) {
            height = front - hit_t[id];
            if ((s.prim_shape[hit_prim] >> 30) == PT_SHAPE_TRIANGLE && top[hit_prim]) {
                V3 ns, sv, tv;
                {   // the target texel: its normal and tangent frame
                    SurfaceInteraction si;
                    texel_interaction(t, a, texel, owner[texel], si);
                    ns = normalize(si.sh_n);
                    tangent_frame(si, ns, sv, tv);
                }
                SurfaceInteraction hs;
                tri_fill_interaction(s, s.prim_shape[hit_prim] & 0x3fffffffu, -ns, h.y, h.z, h.w, true, hs);
                p = hs.p;
                nh = normalize(hs.sh_n);
                if (dot(nh, -ns) > 0.0f) nh = -nh;
                tn = V3(dot(nh, sv), dot(nh, tv), dot(nh, ns));
                detail = dot(hs.n, ns) < 0.0f ? 1u : 0u;   // face_forward(hs.n, -d)
                rec = h;
            }
        }
    }
    if (out.hit_prim) out.hit_prim[texel] = hit_prim;
    if (out.height) out.height[texel] = height;
    store3(out.src_position, texel, p); store3(out.src_normal, texel, nh); store3(out.tangent_normal, texel, tn);
    if (out.detail) { out.detail[texel] = detail; out.rec[texel] = rec; }
}

// k_bake_rays from the source hits: job.owner is the detail-hit map, rec the hits
struct TransferJob : BakeJob { const float4 *rec; };
PT_DEV AOFrame ray_surface(const DeviceScene &s, const BakeAtlas &, const TransferJob &job, uint32_t texel, uint32_t detail, SurfaceInteraction &hs) { return transfer_hit(s, job.rec[texel], detail != 0u, hs); }
__global__ __launch_bounds__(256) void k_bake_transfer_rays(DeviceScene s, RenderConst rc, SobolTables tabs, BakeAtlas a, TransferJob job) {
    const uint32_t total = a.slots * job.s_count;
    const uint32_t rounded = (total + 63u) & ~63u;
    for (uint32_t item = blockIdx.x * blockDim.x + threadIdx.x; item < rounded; item += gridDim.x * blockDim.x) {
        uint32_t texel = PT_NONE, sl = 0, detail = PT_NONE;
        if (item < total) { texel = slot_texel(a, item % a.slots); sl = item / a.slots; if (texel != PT_NONE) detail = job.owner[texel]; }
        ao_chunk_rays(s, rc, tabs, a, job, total, item, texel, sl, detail);
    }
}

// pt_bake_transfer_rays: the projection ray of texel[i] and the AO ray (sample[i], element[i]) from its detail hit. found[i]: bit 0 the texel has an owner, bit 1 a detail hit
__global__ __launch_bounds__(256) void k_bake_transfer_probe(DeviceScene t, DeviceScene s, RenderConst rc, SobolTables tabs, BakeAtlas a, const uint32_t *owner, const uint32_t *detail,
                                                             const float4 *rec, float front, float t_max, uint32_t nsamples, uint32_t cos_sample, uint32_t n, const uint32_t *texel,
                                                             const uint32_t *sample, const uint32_t *element, float *out, uint8_t *found) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t tx = texel[i];
    const uint32_t prim = tx < a.n_texels ? owner[tx] : PT_NONE;
    V3 po(0.0f, 0.0f, 0.0f), pd(0.0f, 0.0f, 0.0f), o(0.0f, 0.0f, 0.0f), wo(0.0f, 0.0f, 0.0f);
    float pt = 0.0f, w = 0.0f;
    uint32_t bits = 0;
    if (prim != PT_NONE) {
        bits = 1u; pt = t_max;
        {
            SurfaceInteraction si;
            texel_interaction(t, a, tx, prim, si);
            V3 ns; projection_ray(si, front, ns, po, pd);
        }
        const uint32_t dt = detail[tx];
        if (dt != PT_NONE) {
            bits = 3u;
            SurfaceInteraction hs;
            const AOFrame f = transfer_hit(s, rec[tx], dt != 0u, hs);
            ao_ray(rc, tabs, hs, f, (int32_t)(tx % a.width), (int32_t)(tx / a.width), (uint64_t)sample[i] * nsamples + element[i], cos_sample, (float)nsamples, o, wo, w);
        }
    }
    float *r = out + 14 * (size_t)i;   // {projection o, d, t_max, AO o, d, w}
    r[0] = po.x; r[1] = po.y; r[2] = po.z; r[3] = pd.x; r[4] = pd.y; r[5] = pd.z; r[6] = pt;
    r[7] = o.x; r[8] = o.y; r[9] = o.z; r[10] = wo.x; r[11] = wo.y; r[12] = wo.z; r[13] = w;
    found[i] = (uint8_t)bits;
}

// ---- the lightmap (mi355bake.h "Lightmap")

// One chunk of light samples of the samples [s_begin, s_begin + s_count) of every item (a texel, a point): AOChunk's ray records and flags (w is not used), and per
// ray what it adds when it arrives. Not every sample spawns a ray: id[kk * items + item] is the ray id of element k0 + kk of the item, PT_NONE for a sample that
// contributes nothing. `LightSamples light` is what the lightmap's and the SH points' jobs hold alike: a member, since as a base ahead of the other fields it moved the
// kernel arguments and with them k_bake_light_rays' register traffic (profiles/r6/NOTES.md section 23).
struct LightSamples {
    const uint32_t *sel;     // [n_sel]: the selected lights, ascending
    uint32_t n_sel;
    float scale;             // (float)n_sel / (float)nsamples
    uint32_t *id;            // [kn][items]
    float4 *e;               // [rays]: {E.rgb, 1}
};
struct LightJob : AOChunk {
    uint32_t s_begin, s_count;
    const uint32_t *owner;   // [texels]
    float4 *light_w;         // [texels]
    LightSamples light;
};

// The reference point of a texel's light samples (contract step 1) and the normalised shading normal
PT_DEV IData light_ref(const SurfaceInteraction &si, V3 &ns) { IData ref; ref.p = si.p; ref.p_error = si.p_error; ref.n = si.n; ns = normalize(si.sh_n); return ref; }

// Sample number j of texel (px, py) on light li (contract steps 3 to 5): Light::sample_li, the contribution test, E and the shadow ray. false: the sample adds
// nothing and spawns no ray (E, o and d are zeros then).
template <bool SPH>
PT_DEV bool light_ray(const DeviceScene &s, const RenderConst &rc, const SobolTables &tabs, const IData &ref, V3 ns, int32_t px, int32_t py, uint64_t j, uint32_t li, float scale,
                      V3 &wi, float &pdf, RGB &Li, RGB &E, V3 &o, V3 &d) {
    const P2 u = ao_array_sample(rc, tabs, px, py, j);
    wi = V3(0.0f, 0.0f, 0.0f); pdf = 0.0f;
    IData p1;
    Li = light_sample_li<SPH>(s, li, ref, u, wi, pdf, p1);
    E = RGB(0.0f); o = V3(0.0f, 0.0f, 0.0f); d = V3(0.0f, 0.0f, 0.0f);
    const float c = dot(wi, ns);
    if (!(pdf > 0.0f) || (Li.r == 0.0f && Li.g == 0.0f && Li.b == 0.0f) || !(c > 0.0f) || !(dot(wi, ref.n) > 0.0f)) return false;
    const float w = (c * scale) / pdf;
    E = Li * w;
    spawn_ray_to(ref, p1, o, d);
    return true;
}

// The body of k_bake_light_rays and k_bake_sh_rays: this chunk's light samples of item `item` of `total`, sample `sl` of the pass. A wave is 64 items (an 8 x 8 tile,
// 64 consecutive points) of ONE sample number, so the sample number j of an element, and with it the light sel[j mod n_sel], is the same for all 64 lanes: the index
// goes through readfirstlane and the light's record and PtLight are fetched by scalar loads, once per wave. Every lane of the wave is here; one without surface or
// point (`found` false) takes part in the ballots and spawns nothing. `sample(j, li, wi, E, o, d)` is sample number j of the item on light li (light_ray, sh_ray);
// `store(id, wi)` writes what the caller keeps of ray `id` besides the records here (the SH points: wi; the lightmap: nothing, and its wi registers are dead).
// kLightGroup elements at a time: their rays wait in registers for ONE reservation of the wave, for the lanes whose samples contribute -- a single counter sustains
// ~88 returning atomics per microsecond (MI355X_MICROARCH.md), and one per element made the kernel wait for the counter (2048^2 x 16 x 3 samples: 30.3 ms;
// k_bake_rays, one per item, 13.2 ms)
template <class Job, class Sample, class Store>
PT_DEV void light_group_rays(const Job &job, uint32_t total, uint32_t item, uint32_t sl, bool found, const Sample &sample, const Store &store) {
    const uint64_t j0 = ((uint64_t)job.s_begin + sl) * job.nsamples + job.k0;
    uint32_t r = (uint32_t)(j0 % job.light.n_sel);
    for (uint32_t kk = 0; kk < job.kn; kk += kLightGroup) {
        V3 o[kLightGroup], d[kLightGroup], wi[kLightGroup]; RGB E[kLightGroup];
        unsigned long long rays[kLightGroup];   // per element: the lanes whose sample contributes
        uint32_t n_rays = 0;
#pragma unroll
        for (uint32_t g = 0; g < kLightGroup; ++g) {
            bool ray = false;
            if (kk + g < job.kn) {
                const uint32_t li = (uint32_t)__builtin_amdgcn_readfirstlane((int)job.light.sel[r]);
                r = r + 1u == job.light.n_sel ? 0u : r + 1u;
                if (found) ray = sample(j0 + kk + g, li, wi[g], E[g], o[g], d[g]);
            }
            rays[g] = __ballot(ray);
            n_rays += (uint32_t)__popcll(rays[g]);
        }
        // ids: the group's elements one after the other, each in lane order (lane 0 asks)
        uint32_t base = 0;
        if (n_rays != 0u) {
            if (lane_id() == 0u) base = atomicAdd(job.ray_count, n_rays);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        }
        const unsigned long long below = (1ull << lane_id()) - 1ull;
#pragma unroll
        for (uint32_t g = 0; g < kLightGroup; ++g) {
            if (kk + g >= job.kn) break;
            const bool ray = ((rays[g] >> lane_id()) & 1ull) != 0ull;
            const uint32_t id = base + (uint32_t)__popcll(rays[g] & below);
            base += (uint32_t)__popcll(rays[g]);
            job.light.id[(size_t)(kk + g) * total + item] = ray ? id : PT_NONE;
            if (!ray) continue;
            job.ray[2 * (size_t)id] = make_float4(o[g].x, o[g].y, o[g].z, d[g].x);
            job.ray[2 * (size_t)id + 1] = make_float4(d[g].y, d[g].z, 0.0f, 0.0f);
            job.light.e[id] = make_float4(E[g].r, E[g].g, E[g].b, 1.0f);
            store(id, wi[g]);
        }
    }
}

// Per texel sample of the pass (item = sample-in-pass * slots + slot, as k_bake_rays): this chunk's light samples from the owner's interaction at the texel's centre
template <bool SPH>
__global__ __launch_bounds__(256) void k_bake_light_rays(DeviceScene s, RenderConst rc, SobolTables tabs, BakeAtlas a, LightJob job) {
    const uint32_t total = a.slots * job.s_count;   // (a multiple of 64: whole waves)
    for (uint32_t item = blockIdx.x * blockDim.x + threadIdx.x; item < total; item += gridDim.x * blockDim.x) {
        const uint32_t texel = slot_texel(a, item % a.slots);
        const uint32_t sl = (uint32_t)__builtin_amdgcn_readfirstlane((int)(item / a.slots));
        const uint32_t prim = texel != PT_NONE ? job.owner[texel] : PT_NONE;
        const bool found = prim != PT_NONE;
        IData ref; V3 ns(0.0f, 0.0f, 0.0f);
        ref.p = ref.p_error = ref.n = V3(0.0f, 0.0f, 0.0f);
        if (found) {
            SurfaceInteraction si;
            texel_interaction(s, a, texel, prim, si);
            ref = light_ref(si, ns);
        }
        const int32_t px = found ? (int32_t)(texel % a.width) : 0, py = found ? (int32_t)(texel / a.width) : 0;
        light_group_rays(job, total, item, sl, found,
                         [&](uint64_t j, uint32_t li, V3 &wi, RGB &E, V3 &o, V3 &d) { float pdf; RGB Li; return light_ray<SPH>(s, rc, tabs, ref, ns, px, py, j, li, job.light.scale, wi, pdf, Li, E, o, d); },
                         [](uint32_t, V3) {});
    }
}

// light_w += {E, 1} of the unoccluded contributing samples, in (sample, element) order: k_bake_accum's walk over the id table (a pass of more than one sample has ONE chunk)
__global__ __launch_bounds__(256) void k_bake_light_accum(BakeAtlas a, LightJob job) {
    const uint32_t texel = blockIdx.x * blockDim.x + threadIdx.x;
    if (texel >= a.n_texels) return;
    if (job.owner[texel] == PT_NONE) return;
    const uint32_t slot = texel_slot(a, texel), total = a.slots * job.s_count;
    float4 acc = job.light_w[texel];
    for (uint32_t sl = 0; sl < job.s_count; ++sl) {
        for (uint32_t kk = 0; kk < job.kn; ++kk) {
            const uint32_t id = job.light.id[(size_t)kk * total + (size_t)sl * a.slots + slot];
            if (id == PT_NONE || job.occluded[id]) continue;
            const float4 e = job.light.e[id];
            acc.x += e.x; acc.y += e.y; acc.z += e.z; acc.w += e.w;
        }
    }
    job.light_w[texel] = acc;
}

// What a light probe leaves of query i: 16 floats {wi, pdf, Li, E, o, d}, the light, and found -- bit 0 the item exists, bit 1 the sample contributes (its shadow ray is {o, d})
PT_DEV void store_light_row(uint32_t i, uint32_t li, uint32_t bits, V3 wi, float pdf, RGB Li, RGB E, V3 o, V3 d, uint32_t *out_light, float *out, uint8_t *found) {
    float *r = out + 16 * (size_t)i;
    r[0] = wi.x; r[1] = wi.y; r[2] = wi.z; r[3] = pdf; r[4] = Li.r; r[5] = Li.g; r[6] = Li.b; r[7] = E.r; r[8] = E.g; r[9] = E.b;
    r[10] = o.x; r[11] = o.y; r[12] = o.z; r[13] = d.x; r[14] = d.y; r[15] = d.z;
    out_light[i] = li; found[i] = (uint8_t)bits;
}

// pt_bake_light_rays: query i = element[i] of sample[i] of texel[i], by light_ray (store_light_row; bit 0: the texel has an owner)
template <bool SPH>
__global__ __launch_bounds__(256) void k_bake_light_probe(DeviceScene s, RenderConst rc, SobolTables tabs, BakeAtlas a, const uint32_t *owner, uint32_t nsamples, const uint32_t *sel, uint32_t n_sel,
                                                          float scale, uint32_t n, const uint32_t *texel, const uint32_t *sample, const uint32_t *element, uint32_t *out_light, float *out, uint8_t *found) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t tx = texel[i];
    const uint32_t prim = tx < a.n_texels ? owner[tx] : PT_NONE;
    const uint64_t j = (uint64_t)sample[i] * nsamples + element[i];
    const uint32_t li = sel[j % n_sel];
    V3 wi(0.0f, 0.0f, 0.0f), o(0.0f, 0.0f, 0.0f), d(0.0f, 0.0f, 0.0f); float pdf = 0.0f; RGB Li(0.0f), E(0.0f);
    uint32_t bits = 0;
    if (prim != PT_NONE) {
        SurfaceInteraction si;
        texel_interaction(s, a, tx, prim, si);
        V3 ns; const IData ref = light_ref(si, ns);
        bits = light_ray<SPH>(s, rc, tabs, ref, ns, (int32_t)(tx % a.width), (int32_t)(tx / a.width), j, li, scale, wi, pdf, Li, E, o, d) ? 3u : 1u;
    }
    store_light_row(i, li, bits, wi, pdf, Li, E, o, d, out_light, out, found);
}

// ---- the SH points (mi355bake.h "SH points")

// One chunk of light samples of the point samples [s_begin, s_begin + s_count) of n_points points. A sample number's items are the points padded to whole waves
// (`padded`, a multiple of 64): item = sample-in-pass * padded + point. LightSamples' records, and per ray the wi its basis is evaluated with where the sums are made.
struct ShJob : AOChunk {
    uint32_t s_begin, s_count;
    uint32_t n_points, padded, row;
    const float *points;     // [n_points][3]
    float4 *sh_w;            // [n_points][7]: 27 sums (coefficient q, channel c at 3 q + c) and the count of arrived samples
    LightSamples light;
    float4 *wi;              // [rays]: {wi.xyz, -}
};

// Sample number j of point p, pixel (px, py), on light li (contract steps 1 and 3 to 5): light_ray from a reference point without surface -- a medium interaction's,
// p_error = n = 0, so the shadow ray starts at p exactly --, without cosine and side test. false: the sample adds nothing and spawns no ray (E, o and d are zeros then).
// (Two functions on purpose. They share ao_array_sample, light_sample_li and spawn_ray_to; one light_sample<SPH, SURFACE> with the cosine ahead of the same || chain
// was tried and left the four lightmap kernels as they are, but changed the code of all four SH kernels -- k_bake_sh_rays<false> 147 -> 149 VGPRs, the <true> probe
// 79 -> 83 --, which the rule of profiles/r6/NOTES.md section 23 does not allow without timing them anew.)
template <bool SPH>
PT_DEV bool sh_ray(const DeviceScene &s, const RenderConst &rc, const SobolTables &tabs, V3 p, int32_t px, int32_t py, uint64_t j, uint32_t li, float scale,
                   V3 &wi, float &pdf, RGB &Li, RGB &E, V3 &o, V3 &d) {
    IData ref; ref.p = p; ref.p_error = ref.n = V3(0.0f, 0.0f, 0.0f);
    const P2 u = ao_array_sample(rc, tabs, px, py, j);
    wi = V3(0.0f, 0.0f, 0.0f); pdf = 0.0f;
    IData p1;
    Li = light_sample_li<SPH>(s, li, ref, u, wi, pdf, p1);
    E = RGB(0.0f); o = V3(0.0f, 0.0f, 0.0f); d = V3(0.0f, 0.0f, 0.0f);
    if (!(pdf > 0.0f) || (Li.r == 0.0f && Li.g == 0.0f && Li.b == 0.0f)) return false;
    const float w = scale / pdf;
    E = Li * w;
    spawn_ray_to(ref, p1, o, d);
    return true;
}

// The nine real SH basis functions of orders 0 to 2 at (x, y, z) (contract step 6)
PT_HD void sh_basis(float x, float y, float z, float Y[9]) {
    Y[0] = 0.282095f;
    Y[1] = 0.488603f * y;
    Y[2] = 0.488603f * z;
    Y[3] = 0.488603f * x;
    Y[4] = 1.092548f * (x * y);
    Y[5] = 1.092548f * (y * z);
    Y[6] = 0.315392f * ((3.0f * (z * z)) - 1.0f);
    Y[7] = 1.092548f * (x * z);
    Y[8] = 0.546274f * ((x * x) - (y * y));
}

// Per point sample of the pass: this chunk's light samples, with a wave of 64 consecutive points of ONE sample number in the tile's place; a ray's wi is kept beside
// what it adds. Lanes beyond n_points have no point.
template <bool SPH>
__global__ __launch_bounds__(256) void k_bake_sh_rays(DeviceScene s, RenderConst rc, SobolTables tabs, ShJob job) {
    const uint32_t total = job.padded * job.s_count;   // (a multiple of 64: whole waves)
    for (uint32_t item = blockIdx.x * blockDim.x + threadIdx.x; item < total; item += gridDim.x * blockDim.x) {
        const uint32_t point = item % job.padded;
        const uint32_t sl = (uint32_t)__builtin_amdgcn_readfirstlane((int)(item / job.padded));
        const bool found = point < job.n_points;
        V3 p(0.0f, 0.0f, 0.0f);
        if (found) p = V3(job.points[3 * (size_t)point], job.points[3 * (size_t)point + 1], job.points[3 * (size_t)point + 2]);
        const int32_t px = found ? (int32_t)(point % job.row) : 0, py = found ? (int32_t)(point / job.row) : 0;
        light_group_rays(job, total, item, sl, found,
                         [&](uint64_t j, uint32_t li, V3 &wi, RGB &E, V3 &o, V3 &d) { float pdf; RGB Li; return sh_ray<SPH>(s, rc, tabs, p, px, py, j, li, job.light.scale, wi, pdf, Li, E, o, d); },
                         [&](uint32_t id, V3 wi) { job.wi[id] = make_float4(wi.x, wi.y, wi.z, 0.0f); });
    }
}

// sh_w += {E * Y_q(wi), 1} of the unoccluded contributing samples, in (sample, element) order through the id table: one lane per point, its 28 sums in registers, the
// basis evaluated here from the ray's wi. (One lane per float4 of a point's seven was measured beside it and lost: DESIGN section 5, "SH points".)
__global__ __launch_bounds__(256) void k_bake_sh_accum(ShJob job) {
    const uint32_t point = blockIdx.x * blockDim.x + threadIdx.x;
    if (point >= job.n_points) return;
    const uint32_t total = job.padded * job.s_count;
    float4 *out = job.sh_w + 7 * (size_t)point;
    float acc[28];
#pragma unroll
    for (uint32_t g = 0; g < 7; ++g) { const float4 v = out[g]; acc[4 * g] = v.x; acc[4 * g + 1] = v.y; acc[4 * g + 2] = v.z; acc[4 * g + 3] = v.w; }
    // The walk is a chain of dependent loads per step (id, flag, records), and a point's additions have one order: kShAhead steps' loads are issued together, stage by
    // stage, and their sums are added one after the other (step = sl * kn + kk)
    const uint32_t steps = job.s_count * job.kn;
    uint32_t sl = 0, kk = 0;
    for (uint32_t t0 = 0; t0 < steps; t0 += kShAhead) {
        uint32_t id[kShAhead]; bool arrived[kShAhead]; float4 e[kShAhead], w[kShAhead];
#pragma unroll
        for (uint32_t g = 0; g < kShAhead; ++g) {
            id[g] = t0 + g < steps ? job.light.id[(size_t)kk * total + (size_t)sl * job.padded + point] : PT_NONE;
            if (++kk == job.kn) { kk = 0; ++sl; }
        }
#pragma unroll
        for (uint32_t g = 0; g < kShAhead; ++g) arrived[g] = id[g] != PT_NONE && job.occluded[id[g]] == 0u;
#pragma unroll
        for (uint32_t g = 0; g < kShAhead; ++g) {
            e[g] = w[g] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (arrived[g]) { e[g] = job.light.e[id[g]]; w[g] = job.wi[id[g]]; }
        }
#pragma unroll
        for (uint32_t g = 0; g < kShAhead; ++g) {
            if (!arrived[g]) continue;
            float Y[9]; sh_basis(w[g].x, w[g].y, w[g].z, Y);
#pragma unroll
            for (uint32_t k = 0; k < 9; ++k) { acc[3 * k] += e[g].x * Y[k]; acc[3 * k + 1] += e[g].y * Y[k]; acc[3 * k + 2] += e[g].z * Y[k]; }
            acc[27] += 1.0f;
        }
    }
#pragma unroll
    for (uint32_t g = 0; g < 7; ++g) out[g] = make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
}

// pt_bake_sh_rays: query i = element[i] of sample[i] of point[i], by sh_ray (store_light_row; bit 0: the point index is below n_points)
template <bool SPH>
__global__ __launch_bounds__(256) void k_bake_sh_probe(DeviceScene s, RenderConst rc, SobolTables tabs, const float *points, uint32_t n_points, uint32_t row, uint32_t nsamples,
                                                       const uint32_t *sel, uint32_t n_sel, float scale, uint32_t n, const uint32_t *point, const uint32_t *sample, const uint32_t *element,
                                                       uint32_t *out_light, float *out, uint8_t *found) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t pt = point[i];
    const uint64_t j = (uint64_t)sample[i] * nsamples + element[i];
    const uint32_t li = sel[j % n_sel];
    V3 wi(0.0f, 0.0f, 0.0f), o(0.0f, 0.0f, 0.0f), d(0.0f, 0.0f, 0.0f); float pdf = 0.0f; RGB Li(0.0f), E(0.0f);
    uint32_t bits = 0;
    if (pt < n_points) {
        const V3 p(points[3 * (size_t)pt], points[3 * (size_t)pt + 1], points[3 * (size_t)pt + 2]);
        bits = sh_ray<SPH>(s, rc, tabs, p, (int32_t)(pt % row), (int32_t)(pt / row), j, li, scale, wi, pdf, Li, E, o, d) ? 3u : 1u;
    }
    store_light_row(i, li, bits, wi, pdf, Li, E, o, d, out_light, out, found);
}

}  // namespace ptbake
