/* mi355aov.h -- C ABI of libmi355aov.so: the per-pixel feature buffers a denoiser takes beside the noisy film -- first-hit albedo,
 * shading normal and depth -- rendered on the MI355X for the same camera samples as the film.
 *
 * A third library beside libmi355pt.so and libmi355ao.so. It renders scenes created with pt_scene_create (include/mi355pt.h) through
 * libmi355pt's driver: the camera rays of pt_render_samples (sampler dimensions 0-4, either sampler), their closest hits, and one
 * kernel of its own that rebuilds the hit's interaction, evaluates the material's parameters through the scene's texture system with
 * the camera ray's differentials, and leaves the sample's three values; a second kernel splats them with the film's filter weights.
 *
 * The surface of a sample is the first intersection that carries a material. An intersection without one (a medium-interface shell)
 * is passed through as the path integrator passes it: a ray spawned in the same direction, its parameter added to the depth. A ray
 * that leaves the scene is a miss. One difference on purpose: the surface behind a shell is still textured with the CAMERA ray's
 * differentials (the path integrator's spawned ray has none and point-samples there), so the planes do not change where a shell
 * happens to stand in front of a surface.
 *   depth   t of the camera ray (its direction is normalised); the segments' sum where shells were passed.
 *   normal  the world-space shading normal the BSDF is built on -- after bump mapping; of a mix material: material 1's --, flipped so
 *           that dot(n, wo) >= 0. Not normalised per pixel: pt_aov_resolve normalises the mean.
 *   albedo  from the material's parameters (textures evaluated as a first path vertex evaluates them; the job's spp scales the
 *           differentials), clamped to >= 0:
 *             matte, plastic, substrate, translucent  Kd            uber    opacity * Kd
 *             disney                                  color         metal   fr_conductor(1, 1, eta, k)
 *             mirror, glass                           Kr            mix     amount * albedo(1) + (1 - amount) * albedo(2)
 *             subsurface, kdsubsurface                Kr  (the diffuse look of a BSSRDF is not a surface parameter)
 * There is no max_sample_luminance clamp and no sanitising of the values.
 *
 * Counters (pt_get_counters) and kernel statistics (pt_get_kernel_stats) of the last call are read through libmi355pt: camera_rays,
 * intersect_tests (camera rays + the continuations behind shells), bvh_nodes_visited, triangle_tests, sphere_tests, and film_splats,
 * counted once per sample and pixel whatever the number of planes. The rest are 0. */
#ifndef MI355AOV_H
#define MI355AOV_H
#include <stdint.h>
#include "mi355pt.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Sums over a pixel's filter footprint, one entry per pixel of the cropped film (as pt_render's film). A NULL plane is not wanted:
 * nothing is evaluated for it (no albedo textures without albedo_w, no bump map without normal_w, no ray differentials for depth_w
 * alone; the hit's interaction is rebuilt in any case). w is the film's filter weight of the sample at the pixel (FilmTile::add_sample's table lookup). */
typedef struct PtAOVBuffers {
    float *albedo_w;   /* 4 per pixel: sum w * albedo.rgb, sum w over ALL camera samples (a miss adds w only) */
    float *normal_w;   /* 4 per pixel: sum w * n.xyz,      sum w over the samples that reach a surface        */
    float *depth_w;    /* 2 per pixel: sum w * t,          the same sum of w                                  */
} PtAOVBuffers;

/* Renders the planes for params->spp samples per pixel and ADDS them to the buffers (device memory when buffers_are_device). A pixel's
 * own samples are added to what the buffer holds in sample order, so that disjoint sample ranges rendered one after the other INTO THE
 * SAME buffers leave what the whole range leaves. Honours tile_rank / tile_world, spp_per_pass (0: the library chooses from the free
 * memory) and profile; params->integrator and max_depth are not read.
 * Errors: PT_ERR_INVALID_ARG for a NULL scene, params or buffers, or when all three planes are NULL; otherwise pt_render's statuses. */
int pt_aov_render(pt_scene *scene, const PtRenderParams *params, const PtAOVBuffers *buffers, int buffers_are_device);
/* Samples [first_sample, first_sample + n_samples) of every pixel: the camera samples of pt_render_samples for the same arguments.
 * params->spp stays the job's sample count (the differentials' scale). n_samples == 0 or first_sample + n_samples > spp (in 64 bits):
 * PT_ERR_INVALID_ARG before the device is touched. pt_aov_render is the call (0, spp). */
int pt_aov_render_samples(pt_scene *scene, const PtRenderParams *params, uint32_t first_sample, uint32_t n_samples, const PtAOVBuffers *buffers, int buffers_are_device);
/* Samples per pixel per pass pt_aov_render would use. */
int pt_aov_pass_size(pt_scene *scene, const PtRenderParams *params, uint32_t *spp_per_pass);
/* Host arithmetic: albedo_rgb[3 n] = sum / w over all samples, normal_xyz[3 n] = normalize(sum), depth[n] = sum / w over the hits;
 * 0 where the weight (the normal sum's length) is 0. A NULL plane of `sums` or a NULL output is skipped. */
int pt_aov_resolve(const PtAOVBuffers *sums, uint32_t n_pixels, float *albedo_rgb, float *normal_xyz, float *depth);

#ifdef __cplusplus
}
#endif
#endif
