/* mi355ao.h -- C ABI of libmi355ao.so: the reference's "ambientocclusion" integrator (integrators/ao.rs) on the MI355X.
 *
 * A second library beside libmi355pt.so. It renders scenes created with pt_scene_create (include/mi355pt.h) and reaches the
 * traversal through libmi355pt's driver: one closest-hit camera ray per pixel sample, then `nsamples` any-hit rays from the hit
 * point (AOIntegrator::li, ao.rs:63-110), in the render loop of SamplerIntegrator::render (integrator.rs:263-403).
 *
 * Sampler arrays: the AO directions of pixel sample s come from the sampler's one 2-D array (request_2d_array(nsamples),
 * sampler.rs:100-160): element k is sample number s * nsamples + k of the same pixel, dimensions 5 (x) and 6 (y)
 * (GlobalSampler::start_pixel, sampler.rs:265-306). The camera sample keeps dimensions 0-4.
 *
 * Counters (pt_get_counters) and kernel statistics (pt_get_kernel_stats) of the last pt_ao_render are read through libmi355pt:
 * camera_rays, intersect_tests (= camera rays), shadow_tests (= AO rays), bvh_nodes_visited, triangle_tests, sphere_tests,
 * film_splats and sanitized_*. path_length_hist and zero_radiance_* stay 0.
 *
 * Known limitation: pt_render given integrator == PT_INTEGRATOR_AO renders the path integrator. Call pt_ao_render. */
#ifndef MI355AO_H
#define MI355AO_H
#include <stdint.h>
#include "mi355pt.h"
#ifdef __cplusplus
extern "C" {
#endif

/* PtRenderParams.integrator as a front end reports an `Integrator "ambientocclusion"` scene (mi355front.h: ptf_ao_params). */
#define PT_INTEGRATOR_AO 2

/* create_ao_integrator (ao.rs:113-141): "nsamples" (default 64) and "cossample" (default true). round_count is the identity
 * for the Sobol' and Halton samplers (sampler.rs:34), so nsamples is used as given. */
typedef struct PtAOParams {
    uint32_t nsamples;    /* AO rays per camera hit, > 0 */
    uint32_t cos_sample;  /* != 0: cosine-weighted hemisphere (pdf |cos| / pi); 0: uniform sphere (pdf 1 / (4 pi)) */
} PtAOParams;

/* Renders params->spp samples per pixel with the AO integrator and ADDS the film (XYZ sums + weight sum per pixel of the
 * cropped film, as pt_render) to film_xyzw (device memory when film_is_device). Honours tile_rank / tile_world sharding,
 * spp_per_pass (0: the library chooses from the free memory) and profile. params->integrator is not read.
 * Errors: PT_ERR_INVALID_ARG for a NULL argument, nsamples == 0, or more sample numbers per pixel (spp * nsamples) than the
 * sampler's tables serve; otherwise pt_render's statuses. Text: pt_last_error(). */
int pt_ao_render(pt_scene *scene, const PtRenderParams *params, const PtAOParams *ao, float *film_xyzw, int film_is_device);
/* pt_render_samples for the AO integrator: samples [first_sample, first_sample + n_samples) of every pixel, ADDED to film_xyzw. params->spp stays the job's sample
 * count: element k of sample s is sample number s * nsamples + k of the job, and the table-size check is the job's. n_samples == 0 or first_sample + n_samples > spp
 * (in 64 bits): PT_ERR_INVALID_ARG before the device is touched. pt_ao_render is the call (0, spp). */
int pt_ao_render_samples(pt_scene *scene, const PtRenderParams *params, const PtAOParams *ao, uint32_t first_sample, uint32_t n_samples, float *film_xyzw, int film_is_device);
/* Samples per pixel per pass pt_ao_render would use. The workspace grows with paths x nsamples: the AO rays of a pass are
 * traced in chunks of at most 64 per path, accumulated in order. */
int pt_ao_pass_size(pt_scene *scene, const PtRenderParams *params, const PtAOParams *ao, uint32_t *spp_per_pass);

#ifdef __cplusplus
}
#endif
#endif
