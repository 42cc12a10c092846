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
 * counted once per sample and pixel whatever the number of planes. The rest are 0.
 *
 * The same library renders ID mattes (pt_matte_*, below the feature buffers): per pixel, which material, instance or caller-defined
 * group covers it and with what share of the filter weight -- the same camera samples, surfaces and weights, gathered per film pixel
 * in a stated order so that the tables are deterministic to the bit. Their contract stands above their declarations. */
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

/* ---- ID mattes: which material, object instance or caller-defined group covers a pixel, and by how much -------------------------------
 *
 * A first-hit render like the feature buffers, for the same camera samples, with the film's own filter weights: a matte's edges are
 * the beauty image's edges. Per pixel and layer a table of up to PT_MATTE_SLOTS ids with the sum of the filter weights of the samples
 * that carry each id (what Cryptomatte stores as ranked id / coverage pairs; pt_matte_resolve ranks, pt_matte_mask extracts).
 *
 * A sample's ids. Its surface is pt_aov_render's: the first intersection that carries a material, surfaces without one passed through
 * in the same way.
 *   PT_MATTE_MATERIAL  the surface's material index (PtSceneDesc::prim_material; of a mix material: the mix's own index)
 *   PT_MATTE_INSTANCE  1 + the index of the instance the hit went through; 0 for top-level geometry
 *   PT_MATTE_GROUP     prim_group[prim], prim as pt_trace_closest reports it
 * A sample that reaches no surface adds its weight to w_total of every wanted layer and to nothing else: the coverage missing from 1
 * is the background.
 *
 * Weights and footprint are FilmTile::add_sample's, as pt_aov_render computes them: the pixels ceil(pfilm - 0.5 - radius) ..
 * floor(pfilm - 0.5 + radius) clipped to the crop window, the filter table's entry as it stands (negative lobes included), neither
 * sanitised nor clamped. Pixels outside the integrator's pixel_bounds have no samples.
 *
 * Order -- part of the contract: the first-seen slot order, the overflow and the float sums depend on it. The contributions to a film
 * pixel p are taken with sample numbers ascending; within one sample number, the source pixels q of the sample bounds in raster order
 * (y outer, x inner); the sample (q, s) contributes when p lies in its footprint. A contribution of weight fw looks its id up in slots
 * [0, n_ids):
 *   found                        w[k] += fw
 *   not found, n_ids < 8         id[n_ids] = id, w[n_ids] = fw, n_ids += 1
 *   not found, all slots taken   w_other += fw
 * and w_total += fw in every case. A render CONTINUES the tables it finds in the buffers: disjoint sample ranges rendered in ascending
 * order into the same buffers leave what the whole range leaves, bit for bit, however the job is cut into calls and passes; so do two
 * renders of the same arguments (one thread per film pixel gathers the pixel's samples: no atomics).
 *
 * Counters and kernel statistics are read as for pt_aov_render: film_splats counts every (sample, pixel) contribution once, whatever
 * the number of layers; the launch kinds are "matte" and "matte_film" ("matte_mask" for pt_matte_mask). */
#define PT_MATTE_SLOTS 8u
typedef enum PtMatteLayer { PT_MATTE_MATERIAL = 0, PT_MATTE_INSTANCE = 1, PT_MATTE_GROUP = 2 } PtMatteLayer;   /* 3 layers */
typedef struct PtMattePixel {          /* 80 bytes; all zero = the empty table */
    uint32_t id[PT_MATTE_SLOTS];       /* slots [0, n_ids) in the order their ids were first seen */
    float    w[PT_MATTE_SLOTS];        /* sum of filter weights of the samples with that id */
    uint32_t n_ids;
    float    w_total;                  /* sum of w over ALL contributing samples, misses included */
    float    w_other;                  /* weight of the samples whose id found all eight slots taken */
    uint32_t reserved;                 /* 0 */
} PtMattePixel;
typedef struct PtMatteBuffers {
    PtMattePixel *layer[3];            /* by PtMatteLayer; one entry per pixel of the cropped film, 16-byte aligned; NULL: layer not wanted */
    const uint32_t *prim_group;        /* HOST memory, n_prims entries: the caller's id of each primitive; read for layer[PT_MATTE_GROUP] only */
    uint32_t n_prims;
} PtMatteBuffers;
/* Renders params->spp samples per pixel into the tables (device memory when buffers_are_device; host tables are copied up, continued
 * and copied back once every pass has succeeded). Honours spp_per_pass and profile; params->integrator and max_depth are not read.
 * Errors: PT_ERR_INVALID_ARG, before the device is touched, for a NULL scene, params or buffers, all three layers NULL, or the group
 * layer without prim_group; then for n_prims != the scene's primitive count. PT_ERR_UNSUPPORTED for tile_world > 1: a pixel gathers
 * the samples of its neighbour pixels in the order above, and another rank owns those across a tile edge. Otherwise pt_render's. */
int pt_matte_render(pt_scene *scene, const PtRenderParams *params, const PtMatteBuffers *buffers, int buffers_are_device);
/* Samples [first_sample, first_sample + n_samples) of every pixel, continuing the tables. The range is checked as pt_aov_render_samples checks it. */
int pt_matte_render_samples(pt_scene *scene, const PtRenderParams *params, uint32_t first_sample, uint32_t n_samples, const PtMatteBuffers *buffers, int buffers_are_device);
/* Samples per pixel per pass pt_matte_render would use. */
int pt_matte_pass_size(pt_scene *scene, const PtRenderParams *params, uint32_t *spp_per_pass);
/* Host arithmetic: per pixel the n_ranks (1 .. 8) heaviest slots, by w descending, ties to the lower id: ids[n_pixels * n_ranks] and
 * coverage = w / w_total. Ranks without a slot are id 0, coverage 0; everything is 0 where w_total == 0. PT_ERR_INVALID_ARG for a NULL
 * argument or n_ranks outside 1 .. 8. */
int pt_matte_resolve(const PtMattePixel *table, uint32_t n_pixels, uint32_t n_ranks, uint32_t *ids, float *coverage);
/* On the device: mask[p] = the sum, in slot order, of w[k] of the slots whose id is in ids[0, n_ids) (host memory), over w_total; 0 where
 * w_total == 0. 1 <= n_ids <= 4096, else PT_ERR_INVALID_ARG. Adds the launch kind "matte_mask" to the last render's kernel statistics. */
int pt_matte_mask(pt_scene *scene, const PtMattePixel *table, int table_is_device, uint32_t n_pixels, const uint32_t *ids, uint32_t n_ids, float *mask, int mask_is_device);

#ifdef __cplusplus
}
#endif
#endif
