// dn_kernels.h -- the kernels of the denoiser (include/mi355dn.h; DESIGN.md section 5 states the filter operation by operation). All arithmetic is float32 in the order
// written here (-ffp-contract=off, IEEE division and square root); tests/denoise_reference.py is the same arithmetic in numpy. No atomics.
//   k_dn_prepare     one lane per pixel: the two half films and the feature sums -> the demodulated colour and its variance estimate {d.rgb, v} and the pixel's guide
//                    record {n.xyz, z} {depth slope, flags, 0, 0}; the output of the pixels no level will write.
//   k_dn_noise       before every level: the pixel's noise estimate, the square root of the 3 x 3 mean of its neighbours' variances.
//   k_dn_atrous<S>   one level of stride S: {d, v} of image `src` -> `dst`; the last level writes the re-modulated image instead.
#pragma once
#include "../csrc/kern_common.h"

namespace ptdn {
using namespace ptd;

enum : uint32_t { kDnValid = 1u, kDnHit = 2u, kDnInside = 4u };   // a guide record's flags; kDnInside only in LDS: the halo cell is a pixel of the image

struct DnImage { uint32_t w, h; };
struct DnParams { float sigma_l, sigma_z, sigma_n2, albedo_floor, scale; };   // sigma_n2 = sigma_n * sigma_n
struct DnSums { const float4 *albedo, *normal; const float2 *depth; };

PT_DEV float dn_lum(float r, float g, float b) { return (0.212671f * r + 0.715160f * g) + 0.072169f * b; }

// The demodulation factor of a pixel: its mean albedo, the part of it that sees the background counted as albedo 1, bounded below.
PT_DEV void dn_demod(const float4 aw, float normal_weight, float floor, float m[3]) {
    float alb[3] = {0.0f, 0.0f, 0.0f}, cov = 0.0f;
    if (aw.w != 0.0f) { alb[0] = aw.x / aw.w; alb[1] = aw.y / aw.w; alb[2] = aw.z / aw.w; cov = fminf(normal_weight / aw.w, 1.0f); }
    const float open = 1.0f - cov;
    for (int k = 0; k < 3; ++k) m[k] = fmaxf(alb[k] + open, floor);
}

// |z(q) - z(p)| along one axis for the depth slope: the forward neighbour when both are hits, else the backward one, else 0. `q` < 0 or >= n: outside the image.
PT_DEV float dn_slope(const DnSums &s, size_t row, int64_t p, int64_t step, int64_t n, float z) {
    for (int side = 0; side < 2; ++side) {
        const int64_t q = side == 0 ? p + 1 : p - 1;
        if (q < 0 || q >= n) continue;
        const size_t i = row + (size_t)(q * step);
        if (!(s.normal[i].w > 0.0f)) continue;
        const float2 dq = s.depth[i];
        return side == 0 ? fabsf(dq.x / dq.y - z) : fabsf(z - dq.x / dq.y);
    }
    return 0.0f;
}

__global__ __launch_bounds__(256) void k_dn_prepare(DnImage im, DnParams p, const float4 *film_a, const float4 *film_b, DnSums s, uint32_t iterations, float4 *img, float4 *img_b, float4 *guide, float *rgb_out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x, n_pix = (size_t)im.w * im.h;
    if (i >= n_pix) return;   // (no barrier in this kernel)
    const int64_t x = (int64_t)(i % im.w), y = (int64_t)(i / im.w);
    const float4 a = film_a[i], b = film_b[i], aw = s.albedo[i], nw = s.normal[i];
    const float fa[4] = {a.x, a.y, a.z, a.w}, fb[4] = {b.x, b.y, b.z, b.w}, fc[4] = {a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
    const bool valid = a.w != 0.0f && b.w != 0.0f, hit = nw.w > 0.0f;
    float c[3];
    if (!valid) {   // resolved as the film, feeds nobody: the levels stage its records (flags: not valid) and never write them, so both images get a value here
        film_resolve_pixel(fc, p.scale, c);
        rgb_out[3 * i] = c[0]; rgb_out[3 * i + 1] = c[1]; rgb_out[3 * i + 2] = c[2];
        img[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); img_b[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        guide[2 * i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); guide[2 * i + 1] = make_float4(0.0f, __uint_as_float(hit ? kDnHit : 0u), 0.0f, 0.0f);
        return;
    }
    float ra[3], rb[3], m[3];
    film_resolve_pixel(fa, 1.0f, ra); film_resolve_pixel(fb, 1.0f, rb); film_resolve_pixel(fc, 1.0f, c);
    dn_demod(aw, nw.w, p.albedo_floor, m);
    const float d[3] = {c[0] / m[0], c[1] / m[1], c[2] / m[2]};
    const float dl = dn_lum(ra[0] / m[0], ra[1] / m[1], ra[2] / m[2]) - dn_lum(rb[0] / m[0], rb[1] / m[1], rb[2] / m[2]);
    const float v = 0.25f * (dl * dl);
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, z = 0.0f, fw = 0.0f;
    const float len = sqrtf((nw.x * nw.x + nw.y * nw.y) + nw.z * nw.z);
    if (len != 0.0f) { nx = nw.x / len; ny = nw.y / len; nz = nw.z / len; }
    if (hit) {
        const float2 dw = s.depth[i];
        z = dw.x / dw.y;
        fw = dn_slope(s, (size_t)y * im.w, x, 1, im.w, z) + dn_slope(s, (size_t)x, y, im.w, im.h, z);
    }
    img[i] = make_float4(d[0], d[1], d[2], v);
    guide[2 * i] = make_float4(nx, ny, nz, z);
    guide[2 * i + 1] = make_float4(fw, __uint_as_float(kDnValid | (hit ? kDnHit : 0u)), 0.0f, 0.0f);
    if (iterations == 0u) {
        for (int k = 0; k < 3; ++k) rgb_out[3 * i + k] = fmaxf(d[k] * m[k], 0.0f) * p.scale;
    }
}

// The noise estimate a level's luminance edge stop is scaled by: sd = sqrt(max(0, V)), V the 3 x 3 binomial mean of the variance over the pixel's valid neighbours inside
// the image, rows outer, normalised by the weights used. One lane per pixel, before every level (the variance is the previous level's): in pixel order the nine reads of
// a lane are its neighbours' in the wave, where a lane of k_dn_atrous<S> would gather them from lines S pixels apart (measured at 1080p: 1.93 ms for five levels against 1.00).
__global__ __launch_bounds__(256) void k_dn_noise(DnImage im, const float4 *src, const float4 *guide, float *noise) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x, n_pix = (size_t)im.w * im.h;
    if (i >= n_pix) return;   // (no barrier in this kernel)
    float sd = 0.0f;
    if ((__float_as_uint(guide[2 * i + 1].y) & kDnValid) != 0u) {
        constexpr float kBin[3] = {0.25f, 0.5f, 0.25f};
        const int64_t x = (int64_t)(i % im.w), y = (int64_t)(i / im.w);
        float vs = 0.0f, vw = 0.0f;
#pragma unroll
        for (int j = -1; j <= 1; ++j) {
#pragma unroll
            for (int k = -1; k <= 1; ++k) {
                const int64_t qx = x + k, qy = y + j;
                if (qx < 0 || qy < 0 || qx >= (int64_t)im.w || qy >= (int64_t)im.h) continue;
                const size_t q = (size_t)qy * im.w + (size_t)qx;
                if ((__float_as_uint(guide[2 * q + 1].y) & kDnValid) == 0u) continue;
                const float wk = kBin[j + 1] * kBin[k + 1];
                vs += wk * src[q].w; vw += wk;
            }
        }
        sd = sqrtf(fmaxf(0.0f, vs / vw));
    }
    noise[i] = sd;
}

// One level. At stride S the 25 taps of a pixel are pixels of its own residue class (x mod S, y mod S), so a block owns a 16 x 16 tile of ONE sub-lattice: lane t is lattice
// cell (t & 15, t >> 4) of tile (tx, ty) of class (rx, ry), pixel ((16 tx + cx) S + rx, (16 ty + cy) S + ry). The block stages the tile with a rim of two cells -- 20 x 20
// records, 16 KB of LDS at every stride -- and the 25 taps are LDS reads. (A pixel-space tile would need a rim of 2 S pixels: 80 x 80 records at stride 16.) The pixel's
// noise is k_dn_noise's: its 3 x 3 is of the pixel's NEIGHBOURS at every level, pixels of other classes at S > 1.
// Tiles are numbered with the class innermost, so the S tiles that share a run of cache lines are worked on side by side; a block takes tiles blockIdx.x, + gridDim.x, ...
// (the grid is capped, kDnMaxBlocks: a thin image of 2^31 pixels has 2^27 tiles, mostly of empty lanes). Every global load is a whole quad; cells outside the image are staged with flags 0; edge
// tiles are ragged and the tiles of a class the image is too small for are empty; no lane leaves before a barrier.
constexpr int kDnTile = 16, kDnRim = 2, kDnHalo = kDnTile + 2 * kDnRim, kDnCells = kDnHalo * kDnHalo;
constexpr uint32_t kDnMaxBlocks = 1u << 14;   // eight times the 2048 blocks 256 CUs hold at once: enough to even out ragged tiles, far below any launch limit (1080p has 8.6 k tiles)

template <uint32_t S>
__global__ __launch_bounds__(256) void k_dn_atrous(DnImage im, DnParams p, const float4 *src, const float4 *guide, float4 *dst, const float *noise, uint32_t nbx, uint32_t nrx, uint32_t nry, uint32_t n_tiles,
                                                    const float4 *albedo_w, const float4 *normal_w, float *rgb_out) {
    __shared__ float4 s_img[kDnCells], s_g0[kDnCells];
    __shared__ float2 s_g1[kDnCells];   // {depth slope, flags}
    constexpr float kTap[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    constexpr float kRoot[9] = {0.0f, 1.0f, 1.4142135623730951f, 0.0f, 2.0f, 2.23606797749979f, 0.0f, 0.0f, 2.8284271247461903f};   // sqrt(i * i + j * j)
    constexpr uint32_t kLive = kDnInside | kDnValid;
    const int cx = (int)(threadIdx.x & 15u) + kDnRim, cy = (int)(threadIdx.x >> 4) + kDnRim, me = cy * kDnHalo + cx;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // (uniform in the block)
        const uint32_t bx = tile % nbx, by = tile / nbx;
        const uint32_t rx = bx % nrx, tx = bx / nrx, ry = by % nry, ty = by / nry;
        const int64_t mx = ((int64_t)tx * kDnTile + (cx - kDnRim)) * S + rx, my = ((int64_t)ty * kDnTile + (cy - kDnRim)) * S + ry;   // the lane's own pixel
        const bool inside = mx < (int64_t)im.w && my < (int64_t)im.h;
        const float sd = inside ? noise[(size_t)my * im.w + (size_t)mx] : 0.0f;   // (in flight while the tile is staged)
        for (int k = (int)threadIdx.x; k < kDnCells; k += 256) {
            const int hx = k % kDnHalo, hy = k / kDnHalo;
            const int64_t lx = (int64_t)tx * kDnTile + hx - kDnRim, ly = (int64_t)ty * kDnTile + hy - kDnRim;
            const int64_t px = lx * S + rx, py = ly * S + ry;
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g0 = c;
            float2 g1 = make_float2(0.0f, __uint_as_float(0u));
            if (lx >= 0 && ly >= 0 && px < (int64_t)im.w && py < (int64_t)im.h) {
                const size_t i = (size_t)py * im.w + (size_t)px;
                c = src[i]; g0 = guide[2 * i];
                const float4 q = guide[2 * i + 1];
                g1 = make_float2(q.x, __uint_as_float(__float_as_uint(q.y) | kDnInside));
            }
            s_img[k] = c; s_g0[k] = g0; s_g1[k] = g1;
        }
        __syncthreads();
        const uint32_t flags = __float_as_uint(s_g1[me].y);
        if ((flags & kLive) == kLive) {
            const float4 cp = s_img[me], gp = s_g0[me];
            const float fw = s_g1[me].x;
            const bool hit = (flags & kDnHit) != 0u;
            const float den_l = p.sigma_l * sd + 1.0e-6f, lum_p = dn_lum(cp.x, cp.y, cp.z);
            float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
            for (int j = -2; j <= 2; ++j) {
#pragma unroll
                for (int i = -2; i <= 2; ++i) {
                    const int q = me + j * kDnHalo + i;
                    const uint32_t fq = __float_as_uint(s_g1[q].y);
                    if ((fq & kLive) != kLive || ((fq ^ flags) & kDnHit) != 0u) continue;
                    const float4 cq = s_img[q], gq = s_g0[q];
                    float e_n = 0.0f, e_z = 0.0f;
                    if (hit) {
                        const float r = (float)S * kRoot[i * i + j * j];
                        e_n = fmaxf(0.0f, 2.0f - 2.0f * ((gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z)) / p.sigma_n2;
                        e_z = fabsf(gp.w - gq.w) / ((p.sigma_z * fw) * r + 1.0e-4f);
                    }
                    const float e_l = fabsf(lum_p - dn_lum(cq.x, cq.y, cq.z)) / den_l;
                    const float w = (kTap[j + 2] * kTap[i + 2]) * expf(-((e_n + e_z) + e_l));
                    sw += w; sr += w * cq.x; sg += w * cq.y; sb += w * cq.z; sv += (w * w) * cq.w;
                }
            }
            const float d[3] = {sr / sw, sg / sw, sb / sw};
            const size_t at = (size_t)my * im.w + (size_t)mx;
            if (rgb_out) {   // the last level: re-modulated, as the film is resolved
                float m[3];
                dn_demod(albedo_w[at], normal_w[at].w, p.albedo_floor, m);
                for (int k = 0; k < 3; ++k) rgb_out[3 * at + k] = fmaxf(d[k] * m[k], 0.0f) * p.scale;
            } else {
                dst[at] = make_float4(d[0], d[1], d[2], sv / (sw * sw));
            }
        }
        __syncthreads();   // (the next tile's records replace these)
    }
}

}  // namespace ptdn
