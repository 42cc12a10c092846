/* mi355dn.h -- C ABI of libmi355dn.so: the denoiser the feature buffers of libmi355aov.so were made for. An edge-avoiding a-trous
 * wavelet filter (Dammertz et al. 2010) with the variance guidance of SVGF's spatial pass (Schied et al. 2017), run on the MI355X on
 * albedo-demodulated radiance; it stops at normal and depth edges. Deterministic, no learned weights, no atomics: the result is a
 * function of the inputs alone, and DESIGN.md section 5 states every operation in its order.
 *
 * A fourth library beside libmi355pt.so, libmi355ao.so and libmi355aov.so. It takes what the other three render:
 *   film_a, film_b  the XYZW sums of two DISJOINT sample ranges of one job (pt_render_samples into two films): A + B is the film,
 *                   and the difference of the two resolved halves is the noise estimate (as pt_film_halves_error reads them);
 *   sums            the un-normalised feature sums of the samples of A + B (pt_aov_render / pt_aov_render_samples).
 * A pixel whose half A or half B holds no weight is INVALID: it is resolved as pt_film_resolve resolves it and feeds no neighbour.
 *
 * The call runs on the scene's stream. Its launch kinds are added to the kernel statistics of the scene's last render
 * (pt_get_kernel_stats): "denoise_prepare" once, "denoise_variance" and "denoise_atrous" once per level each. The counters are not touched. */
#ifndef MI355DN_H
#define MI355DN_H
#include <stdint.h>
#include "mi355aov.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct PtDenoiseParams {
    uint32_t iterations;   /* 0..5; level i uses stride 2^i. 0: the resolved film */
    float sigma_l;         /* luminance edge stop, in standard deviations of the pixel's estimated noise */
    float sigma_z;         /* depth edge stop, in units of the pixel's depth slope times the tap's distance */
    float sigma_n;         /* normal edge stop: a tap's weight falls as exp(-(2 - 2 cos angle) / sigma_n^2) */
    float albedo_floor;    /* lower bound of the demodulation factor */
    float scale;           /* as pt_film_resolve's */
} PtDenoiseParams;

/* iterations 5, sigma_l 4, sigma_z 1, sigma_n 0.25, albedo_floor 0.01, scale 1. A NULL argument is ignored. */
void pt_denoise_default_params(PtDenoiseParams *p);

/* The denoised image of A + B: rgb_out holds 3 floats per pixel, as pt_film_resolve's output. film_a and film_b hold 4 floats per
 * pixel, `sums` ALL THREE planes for width x height pixels. buffers_are_device: every buffer (rgb_out too) is device memory the
 * scene's stream may read; otherwise the inputs are copied up and rgb_out is copied back, on success only. The inputs are not changed.
 * The workspace (68 bytes per pixel) is allocated for the call.
 * Errors: PT_ERR_INVALID_ARG, before the device is touched, for a NULL argument, a NULL plane, width or height 0, width * height >
 * 2^31, iterations > 5, a sigma, floor or scale that is not positive and finite; PT_ERR_OUT_OF_MEMORY when the workspace cannot be
 * allocated (the scene stays usable); PT_ERR_HIP otherwise. */
int pt_denoise(pt_scene *scene, const PtDenoiseParams *params, const float *film_a, const float *film_b, const PtAOVBuffers *sums,
               uint32_t width, uint32_t height, float *rgb_out, int buffers_are_device);

#ifdef __cplusplus
}
#endif
#endif
