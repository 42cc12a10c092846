// film_tools.hip -- pt_film_resolve_device / pt_film_halves_error / pt_tiles_select: the device film tools (kern_preview.h) behind the C ABI (host_common.h has the map).
// They run on the scene's stream through the render's begin() / launch() / end() bookkeeping and ADD their launch kinds ("film_resolve", "film_halves_error",
// "film_error_reduce", "tiles_select") to the kernel statistics of the last render; the counters are not touched.
#include "host_common.h"

namespace {
int film_tool_begin(pt_scene *sc) {
    if (sc->device != g_device) { if (int st = bind_device(sc->device)) return st; }
    if (!sc->stream) HIP_TRY(hipStreamCreate(&sc->stream));
    sc->drop_timings();   // (event pairs a failed call left behind)
    return PT_OK;
}
int film_tool_end(pt_scene *sc) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(sc->stream));
    sc->resolve_timings();
    return PT_OK;
}
}  // namespace

extern "C" {

int pt_film_resolve_device(pt_scene *sc, const float *film_xyzw_dev, uint32_t n_pixels, float scale, float *rgb_dev, uint8_t *srgb8_dev) {
    if (!sc || !film_xyzw_dev) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (!rgb_dev && !srgb8_dev) return fail(PT_ERR_INVALID_ARG, "pt_film_resolve_device: neither rgb nor srgb8 asked for");
    if (n_pixels == 0) return PT_OK;
    if (int st = film_tool_begin(sc)) return st;
    sc->begin("film_resolve", n_pixels);
    launch(sc, "k_film_resolve", k_film_resolve, dim3((unsigned)(((size_t)n_pixels + 255) / 256)), dim3(256), (const float4 *)film_xyzw_dev, n_pixels, scale, rgb_dev, srgb8_dev,
           ((uintptr_t)srgb8_dev & 3u) == 0 ? 1 : 0);
    sc->end();
    return film_tool_end(sc);
}

int pt_film_halves_error(pt_scene *sc, const float *film_a_dev, const float *film_b_dev, uint32_t width, uint32_t height, float *tile_error_dev, float *mean_error_host, float *max_tile_error_host) {
    if (!sc || !film_a_dev || !film_b_dev) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (width == 0 || height == 0) return fail(PT_ERR_INVALID_ARG, "empty film");
    const uint64_t ntx = ((uint64_t)width + 15) / 16, nty = ((uint64_t)height + 15) / 16, n_tiles = ntx * nty;
    if (n_tiles > (1ull << 31)) return fail(PT_ERR_INVALID_ARG, "pt_film_halves_error: more than 2^31 tiles");
    if (int st = film_tool_begin(sc)) return st;
    DevTmp tmp; float *tile_sum = nullptr, *tile_err = tile_error_dev, *out = nullptr;
    if (tmp.alloc(&tile_sum, n_tiles * 4) != hipSuccess || tmp.alloc(&out, 8) != hipSuccess || (!tile_err && tmp.alloc(&tile_err, n_tiles * 4) != hipSuccess)) {
        (void)hipGetLastError(); return fail(PT_ERR_OUT_OF_MEMORY, "pt_film_halves_error: tile array");
    }
    sc->begin("film_halves_error", (uint64_t)width * height);
    launch(sc, "k_film_halves_error", k_film_halves_error, dim3((unsigned)n_tiles), dim3(256), (const float4 *)film_a_dev, (const float4 *)film_b_dev, width, height, (uint32_t)ntx, tile_sum, tile_err);
    sc->end();
    sc->begin("film_error_reduce", n_tiles);
    launch(sc, "k_film_error_reduce", k_film_error_reduce, dim3(1), dim3(256), (const float *)tile_sum, (const float *)tile_err, (uint32_t)n_tiles, (float)((double)width * height), out);
    sc->end();
    float h[2] = {0.0f, 0.0f};
    HIP_TRY(hipMemcpyAsync(h, out, 8, hipMemcpyDeviceToHost, sc->stream));
    if (int st = film_tool_end(sc)) return st;
    if (mean_error_host) *mean_error_host = h[0];
    if (max_tile_error_host) *max_tile_error_host = h[1];
    return PT_OK;
}

// The candidates whose film footprint meets a film tile with error > threshold (k_tiles_select), in the candidates' order. The count and the list come back in one copy.
int pt_tiles_select(pt_scene *sc, const PtRenderParams *rp, const float *tile_error_dev, float threshold, const uint32_t *candidates, uint32_t n_candidates, uint32_t *tiles_out, uint32_t *n_out) {
    if (!sc || !rp || !tile_error_dev || !tiles_out || !n_out) return fail(PT_ERR_INVALID_ARG, "null argument");
    uint32_t ntx = 0, nty = 0; tile_grid(rp, &ntx, &nty);
    const uint64_t n_grid = (uint64_t)ntx * nty;
    if (n_grid > (1ull << 31)) return fail(PT_ERR_INVALID_ARG, "pt_tiles_select: more than 2^31 tiles");
    if (candidates) { if (int lst = check_tile_list(candidates, n_candidates, n_grid, "pt_tiles_select")) return lst; }   // (before the device is touched)
    const uint32_t n = candidates ? n_candidates : (uint32_t)n_grid;
    RenderConst rc;
    if (int st = frame_geometry(sc, rp, rc)) return st;
    *n_out = 0;
    if (n == 0) return PT_OK;
    if (int st = film_tool_begin(sc)) return st;
    DevTmp tmp; uint32_t *cand = nullptr, *out = nullptr;
    if ((candidates && tmp.alloc(&cand, (size_t)n * 4) != hipSuccess) || tmp.alloc(&out, ((size_t)n + 1) * 4) != hipSuccess) { (void)hipGetLastError(); return fail(PT_ERR_OUT_OF_MEMORY, "pt_tiles_select: tile lists"); }
    if (candidates) HIP_TRY(hipMemcpyAsync(cand, candidates, (size_t)n * 4, hipMemcpyHostToDevice, sc->stream));
    sc->begin("tiles_select", n);
    launch(sc, "k_tiles_select", k_tiles_select, dim3(1), dim3(256), rc, tile_error_dev, threshold, (const uint32_t *)cand, n, out);
    sc->end();
    std::vector<uint32_t> h((size_t)n + 1, 0u);
    HIP_TRY(hipMemcpyAsync(h.data(), out, h.size() * 4, hipMemcpyDeviceToHost, sc->stream));
    if (int st = film_tool_end(sc)) return st;
    if (h[0] > n) return fail(PT_ERR_HIP, "internal: pt_tiles_select selected more tiles than it was given");
    std::copy(h.begin() + 1, h.begin() + 1 + h[0], tiles_out);
    *n_out = h[0];
    return PT_OK;
}

}  // extern "C"
