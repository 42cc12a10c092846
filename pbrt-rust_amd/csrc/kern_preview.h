// kern_preview.h -- the device film tools (pt_film_resolve_device, pt_film_halves_error): a host that renders in ranges (pt_render_samples) looks at its film, and at how far
// it has converged, without reading the film back -- and picks the tiles that have not (pt_tiles_select), for a render of listed tiles (pt_render_tiles).
#pragma once
#include "kern_common.h"
#include "kern_film.h"   // tile_footprint

// write_image_png_tga (imageio.rs:365-366): clamp(255 * gamma_correct(v) + 0.5, 0, 255) as u8, gamma_correct (pbrt.rs:210-216); `as u8` truncates and takes NaN to 0
PT_DEV uint32_t srgb8_code(float v) {
    const float g = v <= 0.0031308f ? 12.92f * v : 1.055f * powf(v, 1.0f / 2.4f) - 0.055f;
    const float s = 255.0f * g + 0.5f;
    return (uint32_t)(s != s ? 0.0f : fminf(fmaxf(s, 0.0f), 255.0f));
}

// One pixel per lane: a 16-byte load of its XYZW sums, film_resolve_pixel (dev_math.h: pt_film_resolve's arithmetic, bit for bit), three floats out and / or three 8-bit codes.
// packed != 0 (srgb8 is 4-byte aligned): the twelve bytes of four neighbouring pixels leave as three dwords, lanes 4g .. 4g + 2 storing one each from the codes the group
// exchanges with __shfl; the last, ragged group of the film stores bytes. Every lane of a wave reaches the shuffles (no early return).
__global__ __launch_bounds__(256) void k_film_resolve(const float4 *film_xyzw, uint32_t n_pixels, float scale, float *rgb, uint8_t *srgb8, int packed) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = i < n_pixels;
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (live) {
        const float4 p = film_xyzw[i];
        const float xyzw[4] = {p.x, p.y, p.z, p.w};
        film_resolve_pixel(xyzw, scale, c);
        if (rgb) { rgb[3 * i] = c[0]; rgb[3 * i + 1] = c[1]; rgb[3 * i + 2] = c[2]; }
    }
    if (!srgb8) return;   // (uniform)
    const uint32_t code = srgb8_code(c[0]) | srgb8_code(c[1]) << 8 | srgb8_code(c[2]) << 16;
    const int sub = (int)(threadIdx.x & 3u), l0 = (int)(lane_id() & ~3u);
    const uint32_t p0 = (uint32_t)__shfl((int)code, l0), p1 = (uint32_t)__shfl((int)code, l0 + 1), p2 = (uint32_t)__shfl((int)code, l0 + 2), p3 = (uint32_t)__shfl((int)code, l0 + 3);
    if (packed && (i | 3u) < n_pixels) {   // bytes: p0.rgb p1.rgb p2.rgb p3.rgb
        const uint32_t word = sub == 0 ? (p0 | p1 << 24) : sub == 1 ? (p1 >> 8 | p2 << 16) : (p2 >> 16 | p3 << 8);
        if (sub < 3) reinterpret_cast<uint32_t *>(srgb8)[3 * (i >> 2) + (size_t)sub] = word;
    } else if (live) {
        srgb8[3 * i] = (uint8_t)(code & 255u); srgb8[3 * i + 1] = (uint8_t)(code >> 8 & 255u); srgb8[3 * i + 2] = (uint8_t)(code >> 16);
    }
}

// Sum over the 256 lanes of a block in a FIXED order: within a wave the halving tree of __shfl_down (lane l takes l + 32, then + 16, ... + 1), then wave 0 + wave 1 + wave 2 +
// wave 3 from LDS, left to right. `red` holds 4 floats. The result is valid in thread 0.
PT_DEV float block_sum_256(float v, float *red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
PT_DEV float block_max_256(float v, float *red) {
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off));
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// The two-half-buffer convergence estimate: films A and B hold disjoint sample ranges of one job (A + B is the film). Per pixel, with rA / rB the resolved rgb at scale 1,
//   e = (|rA.r - rB.r| + |rA.g - rB.g| + |rA.b - rB.b|) / sqrt(1e-4 + m),  m = the three channels of (rA + rB) / 2 summed r + g + b;  e = 0 where either weight is 0.
// One block per 16x16 tile of the film's tile grid (edge tiles ragged), lane t = pixel (t & 15, t >> 4) of the tile; lanes outside the film add 0. tile_sum = block_sum_256 of
// e (the order fixed there), tile_err = tile_sum / the tile's pixel count. No atomics: the result is a function of the inputs alone.
__global__ __launch_bounds__(256) void k_film_halves_error(const float4 *film_a, const float4 *film_b, uint32_t width, uint32_t height, uint32_t ntx, float *tile_sum, float *tile_err) {
    __shared__ float red[4];
    const uint32_t tile = blockIdx.x, x0 = (tile % ntx) * 16u, y0 = (tile / ntx) * 16u;
    const uint32_t x = x0 + (threadIdx.x & 15u), y = y0 + (threadIdx.x >> 4);
    float e = 0.0f;
    if (x < width && y < height) {
        const size_t i = (size_t)y * width + x;
        const float4 a = film_a[i], b = film_b[i];
        if (a.w != 0.0f && b.w != 0.0f) {
            const float fa[4] = {a.x, a.y, a.z, a.w}, fb[4] = {b.x, b.y, b.z, b.w};
            float ra[3], rb[3];
            film_resolve_pixel(fa, 1.0f, ra); film_resolve_pixel(fb, 1.0f, rb);
            const float m = ((ra[0] + rb[0]) * 0.5f + (ra[1] + rb[1]) * 0.5f) + (ra[2] + rb[2]) * 0.5f;
            e = ((fabsf(ra[0] - rb[0]) + fabsf(ra[1] - rb[1])) + fabsf(ra[2] - rb[2])) / sqrtf(1.0e-4f + m);
        }
    }
    const float sum = block_sum_256(e, red);
    if (threadIdx.x == 0u) {
        const uint32_t tw = min(16u, width - x0), th = min(16u, height - y0);
        tile_sum[tile] = sum; tile_err[tile] = sum / (float)(tw * th);
    }
}

// The film's mean and largest tile error from the tile array, ONE block: lane t adds / compares tiles t, t + 256, ... in that order, then block_sum_256 / block_max_256.
// out[0] = (sum of the tile sums) / n_pixels, out[1] = max tile error.
__global__ __launch_bounds__(256) void k_film_error_reduce(const float *tile_sum, const float *tile_err, uint32_t n_tiles, float n_pixels, float *out) {
    __shared__ float red_s[4], red_m[4];
    float s = 0.0f, m = 0.0f;
    for (uint32_t t = threadIdx.x; t < n_tiles; t += 256u) { s += tile_sum[t]; m = fmaxf(m, tile_err[t]); }
    s = block_sum_256(s, red_s); m = block_max_256(m, red_m);
    if (threadIdx.x == 0u) { out[0] = s / n_pixels; out[1] = m; }
}

// The tiles of a candidate list that go on rendering: those whose film footprint (tile_footprint<false>, kern_film.h: without the rim only edge samples reach) meets a film-grid tile with tile_err > threshold. The two
// grids differ: a candidate is a 16x16 tile of the SAMPLE bounds, tile_err is indexed by the 16x16 tiles of the cropped FILM (k_film_halves_error), and a tile's samples
// splat onto its whole footprint -- up to 3x3 film tiles for filter radii <= 16. Selected iff !(e <= threshold) for any film tile e of the footprint, i.e. for their largest
// with a NaN among them kept (the job's spp ends the host's loop); an empty footprint is never selected. candidates == NULL: every tile 0 .. n_candidates - 1.
// ONE block of 256 lanes walks the list in chunks of 256. Compaction keeps the list's order and uses no atomics: per wave a ballot and the popcount of the lanes below, the
// four wave totals through LDS, and a base carried from chunk to chunk -- two calls write the same list. out[0] = the count, out[1 ..] = the tiles.
__global__ __launch_bounds__(256) void k_tiles_select(RenderConst rc, const float *tile_err, float threshold, const uint32_t *candidates, uint32_t n_candidates, uint32_t *out) {
    __shared__ uint32_t wave_n[4];
    const uint32_t fntx = (rc.film_w + 15u) / 16u, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t base = 0;   // (uniform: every lane adds the same four totals)
    for (uint32_t c0 = 0; c0 < n_candidates; c0 += 256u) {
        const uint32_t i = c0 + threadIdx.x;
        uint32_t tile = 0; bool keep = false;
        if (i < n_candidates) {
            tile = candidates ? candidates[i] : i;
            const FilmRect r = tile_footprint<false>(rc, tile);
            if (r.x0 < r.x1 && r.y0 < r.y1) {   // inside the crop, so inside the film's tile grid
                const uint32_t fx0 = (uint32_t)(r.x0 - rc.crop[0]) >> 4, fx1 = (uint32_t)(r.x1 - 1 - rc.crop[0]) >> 4;
                const uint32_t fy0 = (uint32_t)(r.y0 - rc.crop[1]) >> 4, fy1 = (uint32_t)(r.y1 - 1 - rc.crop[1]) >> 4;
                for (uint32_t fy = fy0; fy <= fy1; ++fy) for (uint32_t fx = fx0; fx <= fx1; ++fx) keep = keep || !(tile_err[(size_t)fy * fntx + fx] <= threshold);
            }
        }
        const unsigned long long kept = __ballot(keep);
        if (lane == 0u) wave_n[wave] = (uint32_t)__popcll(kept);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < 4u; ++w) { const uint32_t n = wave_n[w]; before += w < wave ? n : 0u; total += n; }
        if (keep) out[1u + base + before + (uint32_t)__popcll(kept & ((1ull << lane) - 1ull))] = tile;
        base += total;
        __syncthreads();   // (wave_n is rewritten by the next chunk)
    }
    if (threadIdx.x == 0u) out[0] = base;
}
