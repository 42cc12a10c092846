// kern_film.h -- the film kernel's body, shared by k_film (kern_misc.h) and k_film_final (kern_aux.h).
#pragma once
#include "kern_common.h"
// The tile of a tile slot: the rank's share of the grid, tile_rank + tile_slot * tile_world, or -- a render of listed tiles (pt_render_tiles) -- the list's entry.
// tile_slot < rc.n_tile_slots, which is then the list's length.
PT_DEV uint32_t slot_tile(const RenderConst &rc, uint32_t tile_slot) { return rc.tile_list ? rc.tile_list[tile_slot] : rc.tile_rank + tile_slot * rc.tile_world; }
// A tile's film footprint: the pixels [x0, x1) x [y0, y1) its samples splat onto, clipped to the crop window; empty (x0 >= x1 or y0 >= y1) for a tile of the sample bounds
// that lies wholly outside the crop's reach. EDGE = true is Film::get_film_tile (film.rs:125-140), the bounds film_slot clips its splats to: it counts the pixels whose filter
// support merely TOUCHES the tile, which only a sample exactly on the tile's edge reaches (the box filter of radius 0.5: a rim of one pixel around the tile). EDGE = false
// leaves those out -- the pixels whose support overlaps the tile's area, where all but a vanishing share of its samples land: what pt_tiles_select asks about, so that under
// the box filter a tile's footprint is the tile. The two differ only where tile edge -/+ radius falls on a pixel centre (radii 0.5, 1.5, ...).
struct FilmRect { int64_t x0, y0, x1, y1; };
template <bool EDGE> PT_DEV FilmRect tile_footprint(const RenderConst &rc, uint32_t tile) {
    int32_t tx0 = rc.sample_bounds[0] + (int32_t)((tile % rc.ntx) * 16u), ty0 = rc.sample_bounds[1] + (int32_t)((tile / rc.ntx) * 16u);
    int32_t tx1 = min(tx0 + 16, rc.sample_bounds[2]), ty1 = min(ty0 + 16, rc.sample_bounds[3]);
    const float lx = (float)tx0 - 0.5f - rc.filter_radius[0], ly = (float)ty0 - 0.5f - rc.filter_radius[1];
    const float hx = (float)tx1 - 0.5f + rc.filter_radius[0], hy = (float)ty1 - 0.5f + rc.filter_radius[1];
    FilmRect r;
    r.x0 = max(EDGE ? f2i_sat(ceilf(lx)) : f2i_sat(floorf(lx)) + 1, (int64_t)rc.crop[0]);
    r.y0 = max(EDGE ? f2i_sat(ceilf(ly)) : f2i_sat(floorf(ly)) + 1, (int64_t)rc.crop[1]);
    r.x1 = min(EDGE ? f2i_sat(floorf(hx)) + 1 : f2i_sat(ceilf(hx)), (int64_t)rc.crop[2]);
    r.y1 = min(EDGE ? f2i_sat(floorf(hy)) + 1 : f2i_sat(ceilf(hy)), (int64_t)rc.crop[3]);
    return r;
}
// pixel slot -> pixel: slot = tile_slot*256 + ty*16 + tx, tile index = slot_tile(tile_slot)
PT_DEV bool slot_to_pixel(const RenderConst &rc, uint32_t slot, int32_t &px, int32_t &py) {
    uint32_t tile_slot = slot >> 8, in_tile = slot & 255u;
    uint32_t tile = slot_tile(rc, tile_slot);
    uint32_t tx = tile % rc.ntx, ty = tile / rc.ntx;
    px = rc.sample_bounds[0] + (int32_t)(tx * 16u + (in_tile & 15u));
    py = rc.sample_bounds[1] + (int32_t)(ty * 16u + (in_tile >> 4));
    if (ty >= rc.nty || px >= rc.sample_bounds[2] || py >= rc.sample_bounds[3]) return false;
    // integrator.rs:328: pixels outside the integrator's pixel_bounds are skipped
    return px >= rc.pixel_bounds[0] && px < rc.pixel_bounds[2] && py >= rc.pixel_bounds[1] && py < rc.pixel_bounds[3];
}


// ---- film ----------------------------------------------------------------------------------------------------
// One thread per pixel slot; its s_count samples are added in sample order (integrator.rs:331-376), FilmTile::add_sample (film.rs:292-331) with
// the tile's pixel bounds == footprint clipped to the crop window. Splats onto the thread's own pixel are accumulated in registers, seeded with the pixel's current value, and
// written back once: the additions happen in sample order exactly as FilmTile::add_sample makes them, without one L2 atomic per channel per sample. Splats onto other pixels
// (wide filters; for the box filter only the pfilm == pixel-corner case) are float atomics; should one of them land on this pixel meanwhile, the final compare-and-swap fails
// and the delta is added atomically instead (contribution preserved, order then unspecified as for any such splat).
// (Several lanes per pixel slot, round 6: slower at 2 / 4 / 8 / 16 lanes -- profiles/r6/NOTES.md section 4; the code is profiles/r6/experiments/settled_ab_hooks.patch.)
// `fin(pid, L)`: called for every sample before it is sanitised and splatted (k_film: nothing; k_film_final, kern_aux.h: the path's last step -- its pending
// next-event estimate, the environment's Le -- where the plain path integrator has no k_shade_miss pass any more).
template <class Fin> PT_DEV void film_slot(const RenderConst &rc, const PathSoA &ps, const float *filter_table, float *film_rgbw, DevCounters *counters, Fin fin) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long nan_c = 0, neg_c = 0, inf_c = 0, splats = 0;
    int32_t px, py;
    if (slot < rc.n_pix_slots && slot_to_pixel(rc, slot, px, py)) {
        // tile pixel bounds (Film::get_film_tile, film.rs:125-140)
        const FilmRect tb = tile_footprint<true>(rc, slot_tile(rc, slot >> 8));
        const int64_t tb0 = tb.x0, tb1 = tb.y0, tb2 = tb.x1, tb3 = tb.y1;
        const float invrx = 1.0f / rc.filter_radius[0], invry = 1.0f / rc.filter_radius[1];
        // Splats onto this thread's own pixel are accumulated in registers, seeded with the pixel's current value, and written
        // back once: the additions happen in sample order exactly as before (and as FilmTile::add_sample does), without one
        // L2 atomic per channel per sample. Splats onto other pixels (wide filters; for the box filter only the pfilm == px
        // edge case) still use atomics; should one of them land on this pixel meanwhile, the final compare-and-swap fails
        // and the delta is added atomically instead (contribution preserved, order then unspecified as for any such splat).
        const bool own_ok = px >= tb0 && px < tb2 && py >= tb1 && py < tb3;
        float *own = film_rgbw + 4 * ((size_t)(py - rc.crop[1]) * rc.film_w + (size_t)(px - rc.crop[0]));
        float seed[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (own_ok) for (int k = 0; k < 4; ++k) { seed[k] = __hip_atomic_load(own + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); acc[k] = seed[k]; }
        for (uint32_t sl = 0; sl < rc.s_count; ++sl) {
            const uint32_t pid = sl * rc.n_pix_slots + slot;
            const float4 c0 = reinterpret_cast<const float4 *>(ps.core)[4 * (size_t)pid], c2 = reinterpret_cast<const float4 *>(ps.core)[4 * (size_t)pid + 2];
            RGB L(c0.x, c0.y, c0.z);
            fin(pid, L);
            // integrator.rs:350-368
            if (L.has_nans()) { L = RGB(0.0f); nan_c++; }
            else if (L.y() < -1.0e-5f) { L = RGB(0.0f); neg_c++; }
            else if (__builtin_isinf(L.y())) { L = RGB(0.0f); inf_c++; }
            if (L.y() > rc.max_sample_luminance) L = L * RGB(rc.max_sample_luminance / L.y());
            const float dx = c2.z - 0.5f, dy = c2.w - 0.5f;   // pfilm
            int64_t p0x = max(f2i_sat(ceilf(dx - rc.filter_radius[0])), tb0), p0y = max(f2i_sat(ceilf(dy - rc.filter_radius[1])), tb1);
            int64_t p1x = min(f2i_sat(floorf(dx + rc.filter_radius[0])) + 1, tb2), p1y = min(f2i_sat(floorf(dy + rc.filter_radius[1])) + 1, tb3);
            for (int64_t y = p0y; y < p1y; ++y) {
                const float fy = fabsf(((float)y - dy) * invry * 16.0f);
                const uint32_t iy = min(f2u32_sat(floorf(fy)), 15u);
                for (int64_t x = p0x; x < p1x; ++x) {
                    const float fx = fabsf(((float)x - dx) * invrx * 16.0f);
                    const uint32_t ix = min(f2u32_sat(floorf(fx)), 15u);
                    const float fw = filter_table[iy * 16 + ix];
                    const RGB c = L * RGB(1.0f) * RGB(fw);
                    if (own_ok && x == (int64_t)px && y == (int64_t)py) { acc[0] += c.r; acc[1] += c.g; acc[2] += c.b; acc[3] += fw; }
                    else {
                        float *dst = film_rgbw + 4 * ((size_t)(y - rc.crop[1]) * rc.film_w + (size_t)(x - rc.crop[0]));
                        atomicAdd(dst + 0, c.r); atomicAdd(dst + 1, c.g); atomicAdd(dst + 2, c.b); atomicAdd(dst + 3, fw);
                    }
                    splats++;
                }
            }
        }
        if (own_ok) for (int k = 0; k < 4; ++k) {
            if (__float_as_uint(acc[k]) == __float_as_uint(seed[k])) continue;
            const uint32_t old = atomicCAS((uint32_t *)(own + k), __float_as_uint(seed[k]), __float_as_uint(acc[k]));
            if (old != __float_as_uint(seed[k])) atomicAdd(own + k, acc[k] - seed[k]);
        }
    }
    counter_add(&counters->san_nan, nan_c); counter_add(&counters->san_neg, neg_c);
    counter_add(&counters->san_inf, inf_c); counter_add(&counters->splats, splats);
}
