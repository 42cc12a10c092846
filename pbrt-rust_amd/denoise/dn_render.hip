// dn_render.hip -- pt_denoise / pt_denoise_default_params (include/mi355dn.h): the a-trous filter over two half films and their feature sums.
//   k_dn_prepare                   the halves and the sums -> demodulated colour + variance, one guide record per pixel; the output of invalid pixels (and of every pixel
//                                  when there is no level)
//   k_dn_noise                     before every level: the pixel's noise estimate from its neighbours' variances
//   k_dn_atrous<1, 2, 4, 8, 16>    one launch per level, ping-pong between the two colour images; the last one writes the image
// The call runs on the scene's stream through the render's begin() / launch() / end() bookkeeping, as the film tools of libmi355pt do (film_tools.hip: dn_begin / dn_end
// restate its film_tool_begin / film_tool_end), and ADDS the launch kinds "denoise_prepare", "denoise_variance" and "denoise_atrous" to the kernel statistics of the last render; the
// counters are not touched. The workspace lives for the call.
#include "../csrc/host_common.h"
#include "../side/side_host.h"
#include "../../include/mi355dn.h"
#include "dn_kernels.h"
#include <cmath>

using namespace ptdn;

namespace {

constexpr uint32_t kDnMaxIterations = 5;

int dn_begin(pt_scene *sc) {
    if (sc->device != g_device) { if (int st = bind_device(sc->device)) return st; }
    if (!sc->stream) HIP_TRY(hipStreamCreate(&sc->stream));
    sc->drop_timings();   // (event pairs a failed call left behind)
    return PT_OK;
}
int dn_end(pt_scene *sc) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(sc->stream));
    sc->resolve_timings();
    return PT_OK;
}

bool positive_finite(float v) { return v > 0.0f && std::isfinite(v); }

template <uint32_t S> void launch_level(pt_scene *sc, DnImage im, const DnParams &p, const float4 *src, const float4 *guide, const float *noise, float4 *dst, const DnSums &s, float *rgb_out) {
    // residue classes the image has pixels of, and the 16 x 16 lattice tiles of the largest class
    const uint32_t nrx = std::min(S, im.w), nry = std::min(S, im.h);
    const uint32_t tiles_x = ((im.w + S - 1) / S + kDnTile - 1) / kDnTile, tiles_y = ((im.h + S - 1) / S + kDnTile - 1) / kDnTile;
    const uint32_t nbx = tiles_x * nrx, nby = tiles_y * nry, n_tiles = nbx * nby;   // (at most 2^27 + 16 each, and 2^28 together: width * height <= 2^31)
    launch(sc, "ptdn::k_dn_atrous<" + std::to_string(S) + ">", k_dn_atrous<S>, dim3(std::min(n_tiles, kDnMaxBlocks)), dim3(256), im, p, src, guide, dst, noise, nbx, nrx, nry, n_tiles, s.albedo, s.normal, rgb_out);
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) void pt_denoise_default_params(PtDenoiseParams *p) {
    if (!p) return;
    p->iterations = 5; p->sigma_l = 4.0f; p->sigma_z = 1.0f; p->sigma_n = 0.25f; p->albedo_floor = 0.01f; p->scale = 1.0f;
}

__attribute__((visibility("default"))) int pt_denoise(pt_scene *sc, const PtDenoiseParams *dp, const float *film_a, const float *film_b, const PtAOVBuffers *sums, uint32_t width, uint32_t height,
                                                       float *rgb_out, int buffers_are_device) {
    if (!sc || !dp || !film_a || !film_b || !sums || !rgb_out) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (!sums->albedo_w || !sums->normal_w || !sums->depth_w) return fail(PT_ERR_INVALID_ARG, "pt_denoise: all three planes of the feature sums are needed");
    if (width == 0 || height == 0) return fail(PT_ERR_INVALID_ARG, "empty image");
    if ((uint64_t)width * height > (1ull << 31)) return fail(PT_ERR_INVALID_ARG, "pt_denoise: more than 2^31 pixels");
    if (dp->iterations > kDnMaxIterations) return fail(PT_ERR_INVALID_ARG, "pt_denoise: iterations > 5");
    if (!positive_finite(dp->sigma_l) || !positive_finite(dp->sigma_z) || !positive_finite(dp->sigma_n) || !positive_finite(dp->albedo_floor) || !positive_finite(dp->scale))
        return fail(PT_ERR_INVALID_ARG, "pt_denoise: sigma_l, sigma_z, sigma_n, albedo_floor and scale must be positive and finite");
    if (int st = dn_begin(sc)) return st;   // (all of the above before the device is touched)
    const size_t n_pix = (size_t)width * height;
    const DnImage im{width, height};
    const DnParams p{dp->sigma_l, dp->sigma_z, dp->sigma_n * dp->sigma_n, dp->albedo_floor, dp->scale};
    DevTmp tmp;
    float4 *img[2] = {nullptr, nullptr}, *guide = nullptr;
    float *noise = nullptr;
    for (float4 *&q : img) SIDE_ALLOC(tmp, q, n_pix * 16, "pt_denoise");
    SIDE_ALLOC(tmp, guide, n_pix * 32, "pt_denoise");
    SIDE_ALLOC(tmp, noise, n_pix * 4, "pt_denoise");
    const float *in[5] = {film_a, film_b, sums->albedo_w, sums->normal_w, sums->depth_w};
    float *out = rgb_out;
    if (!buffers_are_device) {
        const size_t bytes[5] = {n_pix * 16, n_pix * 16, n_pix * 16, n_pix * 16, n_pix * 8};
        for (int k = 0; k < 5; ++k) {
            float *d = nullptr;
            SIDE_ALLOC(tmp, d, bytes[k], "pt_denoise");
            HIP_TRY(hipMemcpyAsync(d, in[k], bytes[k], hipMemcpyHostToDevice, sc->stream));
            in[k] = d;
        }
        SIDE_ALLOC(tmp, out, n_pix * 12, "pt_denoise");
    }
    const DnSums s{(const float4 *)in[2], (const float4 *)in[3], (const float2 *)in[4]};
    sc->begin("denoise_prepare", n_pix);
    launch(sc, "ptdn::k_dn_prepare", k_dn_prepare, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), im, p, (const float4 *)in[0], (const float4 *)in[1], s, dp->iterations, img[0], img[1], guide, out);
    sc->end();
    for (uint32_t level = 0; level < dp->iterations; ++level) {
        const float4 *src = img[level & 1u];
        float4 *dst = img[1u - (level & 1u)];
        float *rgb = level + 1 == dp->iterations ? out : nullptr;
        sc->begin("denoise_variance", n_pix);
        launch(sc, "ptdn::k_dn_noise", k_dn_noise, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), im, src, (const float4 *)guide, noise);
        sc->end();
        sc->begin("denoise_atrous", n_pix);
        switch (level) {
        case 0: launch_level<1>(sc, im, p, src, guide, noise, dst, s, rgb); break;
        case 1: launch_level<2>(sc, im, p, src, guide, noise, dst, s, rgb); break;
        case 2: launch_level<4>(sc, im, p, src, guide, noise, dst, s, rgb); break;
        case 3: launch_level<8>(sc, im, p, src, guide, noise, dst, s, rgb); break;
        default: launch_level<16>(sc, im, p, src, guide, noise, dst, s, rgb); break;
        }
        sc->end();
    }
    if (int st = dn_end(sc)) return st;
    if (!buffers_are_device) HIP_TRY(hipMemcpy(rgb_out, out, n_pix * 12, hipMemcpyDeviceToHost));
    return PT_OK;
}

}  // extern "C"
