/* mi355bake.h -- C ABI of libmi355bake.so: ambient occlusion, bent normals, positions and shading normals of a UV-mapped mesh baked
 * into its own texture space (a UV atlas) on the MI355X.
 *
 * A fifth library beside libmi355pt.so. It bakes scenes created with pt_scene_create (include/mi355pt.h) and reaches the any-hit
 * traversal, the samplers' arrays and the pass budget through libmi355pt's driver. There is no camera, no path state and no film:
 * the front of the pipe is its own -- which triangle owns which texel (k_bake_raster), the surface point there (k_bake_points), the
 * AO rays from it (k_bake_rays), their any-hit walk (libmi355pt's k_trace, launch kind "shadow") and the sums (k_bake_accum).
 * pt_bake_transfer (below, "Transfer") fills the atlas of one scene's mesh with what rays from its surface hit in ANOTHER scene: the
 * height, position, world- and tangent-space normal of a detailed mesh, and the AO there. pt_bake_light (below, "Lightmap") bakes the
 * scene's lights into the atlas: the irradiance every texel receives directly from them.
 *
 * ---- the contract -----------------------------------------------------------------------------------------------------------------
 *
 * Texel centres. Texel (x, y) of a width x height atlas has index y * width + x and centre c = (u, v), u = (x + 0.5) / width,
 * v = (y + 0.5) / height, in float32: ((float)x + 0.5f) / (float)width. Row 0 is at v = 0. Every sample of a texel starts at its
 * centre: antialiasing in texture space is done by baking larger.
 *
 * Ownership. For a selected triangle with vertex UVs uv0, uv1, uv2 (TriangleMesh "uv", by the triangle's three indices), every
 * operation in float32, unfused, in this order:
 *     e0 = uv1 - uv0, e1 = uv2 - uv0, d = c - uv0
 *     det = e0.x * e1.y - e0.y * e1.x
 *     b1 = (d.x * e1.y - d.y * e1.x) / det,  b2 = (e0.x * d.y - e0.y * d.x) / det,  b0 = 1 - b1 - b2      ((1 - b1) - b2)
 * A triangle with det == 0 owns nothing. It contains the centre when b0 >= 0, b1 >= 0 and b2 >= 0 (a NaN fails) AND the texel lies in
 * the triangle's texel box, x0 <= x <= x1 and y0 <= y <= y1, in float32 (fminf / fmaxf: a NaN operand loses):
 *     ulo = min(uv0.x, min(uv1.x, uv2.x)) * (float)width,   uhi = max(uv0.x, max(uv1.x, uv2.x)) * (float)width    (vlo, vhi alike with .y, height)
 *     no box -- the triangle owns nothing -- unless ulo <= uhi, vlo <= vhi and all four are below 1e30 in magnitude
 *     mx = 0.5625f + (float)width * 2.4e-7f                                                                       (my alike with height)
 *     x0 = max(floor(ulo - mx), 0),   x1 = min(ceil((uhi - 1) + mx), width - 1);   no box when x0 > x1            (y0, y1 alike)
 * The box holds every texel whose centre the UV bounds can hold, with a margin beyond what the roundings of the bounds and of the centres
 * amount to: a well-conditioned triangle loses nothing to it. It is there for slivers: with a determinant of a few 1e-9 the rounded
 * barycentrics of a nearly collinear triangle are >= 0 at centres far along its line, and without the box a low-numbered sliver would own
 * texels anywhere on the atlas. The owner of a texel
 * is the LOWEST-NUMBERED selected primitive that contains its centre (primitive numbers are PtSceneDesc's, as pt_trace_closest reports
 * them): ownership is deterministic on shared edges and overlapping islands and does not depend on launch geometry. UVs outside
 * [0, 1] are not wrapped: the part of a triangle outside the unit square owns nothing.
 *
 * The surface point. The interaction Triangle::intersect (shapes/triangle.rs:236-392) builds for the barycentrics (b0, b1, b2) of the
 * owner: p = b0 p0 + b1 p1 + b2 p2 and its error bound p_error, the geometric normal n (flipped by ReverseOrientation xor a
 * handedness-swapping transform, then faced toward the shading normal when the mesh has N or S), dpdu, and the shading normal from
 * per-vertex N -- by the device function the shade and AO kernels use (tri_fill_interaction). `position` is p, `normal` the
 * normalised shading normal. A triangle with area in UV space and none in space has no normal: its texels get NaN normals, rays and
 * sums, as the interaction's arithmetic leaves them; leave such triangles out of the selection.
 *
 * AO rays, as AOIntegrator::li (integrators/ao.rs:77-98) with the surface point in place of the camera hit:
 *     frame        s = normalize(dpdu), t = cross(n, s), and n itself: with no camera ray there is nothing to face n toward
 *     sample       element k of sample s of a texel is the 2-D array value of sample number s * nsamples + k of pixel (x, y),
 *                  dimensions 5 and 6, of a sampler set up for sample bounds [0, width) x [0, height) (sampler.rs:265-306)
 *     direction    cos_sample != 0: cosine_sample_hemisphere(u), pdf = |wi.z| / pi;
 *                  else uniform_sample_sphere(u), pdf = 1 / (4 pi); wi = s * wi.x + t * wi.y + n * wi.z
 *     origin       offset_ray_origin(p, p_error, n, wi) (SurfaceInteraction::spawn_ray)
 *     weight       w = dot(wi, n) / (pdf * nsamples);  t_max = max_distance
 * The rays see the whole scene through libmi355pt's any-hit walk: spheres, instances, alpha masks and the baked mesh itself.
 * ao_w of a texel gains, per unoccluded ray, wi.xyz and w, added in ascending (s, k) order to what the buffer holds. Disjoint sample
 * ranges baked in ascending order into the same buffers leave what the whole range leaves, bit for bit; so do different pass sizes
 * and repeated calls. spp * nsamples is limited as pt_ao_render limits it (the Sobol' tables' 52 columns, Halton's 64-bit index).
 *
 * Counters and kernel statistics of the last call are read through libmi355pt (pt_get_counters, pt_get_kernel_stats): shadow_tests
 * = the AO rays, bvh_nodes_visited, triangle_tests, sphere_tests; the launch kinds are "bake_select", "bake_raster", "bake_points",
 * "bake_rays", "shadow", "bake_accum" and "bake_dilate" ("bake_probe" for pt_bake_rays). */
#ifndef MI355BAKE_H
#define MI355BAKE_H
#include <stdint.h>
#include "mi355pt.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct PtBakeParams {
    uint32_t width, height;      /* the atlas, texels; width * height <= 2^28                         */
    uint32_t spp;                /* the job's samples per texel, > 0                                  */
    uint32_t nsamples;           /* AO rays per sample (ao.rs "nsamples"), > 0                        */
    uint32_t cos_sample;         /* ao.rs "cossample"                                                 */
    float    max_distance;       /* t_max of the AO rays, > 0; INFINITY is ao.rs                      */
    uint32_t sampler_type;       /* PtSamplerType                                                     */
    uint32_t spp_per_pass;       /* 0: the library chooses from the free memory                       */
    uint32_t profile;            /* != 0: time every launch kind (pt_get_kernel_stats)                */
} PtBakeParams;

typedef struct PtBakeBuffers {   /* width * height entries, row-major; NULL = not wanted */
    uint32_t *owner;             /* primitive that owns the texel, PT_NONE for none -- written        */
    float *position;             /* 3 per texel: p; 0 where the texel has no owner -- written         */
    float *normal;               /* 3 per texel: the normalised shading normal; 0 likewise -- written */
    float *ao_w;                 /* 4 per texel: sum of unoccluded wi.xyz, sum of w -- ADDED to       */
} PtBakeBuffers;

/* Bakes params->spp samples per texel of the primitives selected by prim_select -- HOST memory, n_prims bytes, non-zero = a bake
 * target -- into the wanted planes (device memory when buffers_are_device). Without ao_w no ray is traced.
 * Errors. PT_ERR_INVALID_ARG, before the device is touched, for a NULL scene, params, prim_select or buffers; width or height 0 or
 * more than 2^28 texels; spp or nsamples 0; all planes NULL; max_distance not positive, or NaN; a bad sample range; nothing selected;
 * n_prims different from the scene's primitive count (the handle's host side). Then, with the device bound, for more sample numbers per
 * texel than the sampler's tables serve.
 * PT_ERR_UNSUPPORTED, the message naming the primitive, for a selected sphere or disk, a selected primitive that belongs to an
 * instanced object, or a selected triangle of a mesh without UVs. Otherwise pt_render's statuses. Text: pt_last_error(). */
int pt_bake_render(pt_scene *scene, const PtBakeParams *params, const uint8_t *prim_select, uint32_t n_prims, const PtBakeBuffers *buffers, int buffers_are_device);
/* Samples [first_sample, first_sample + n_samples) of every texel; params->spp stays the job's sample count. n_samples == 0 or
 * first_sample + n_samples > spp (in 64 bits): PT_ERR_INVALID_ARG before the device is touched. pt_bake_render is the call (0, spp). */
int pt_bake_render_samples(pt_scene *scene, const PtBakeParams *params, const uint8_t *prim_select, uint32_t n_prims, uint32_t first_sample, uint32_t n_samples,
                           const PtBakeBuffers *buffers, int buffers_are_device);
/* Samples per texel per pass pt_bake_render would use: a pass holds width * height * spp_per_pass texel samples and their rays, traced
 * in chunks of at most 64 per texel sample. With nsamples > 64 a pass is one sample, whatever spp_per_pass asks for: the additions to a
 * texel stay in (s, k) order. */
int pt_bake_pass_size(pt_scene *scene, const PtBakeParams *params, uint32_t *spp_per_pass);
/* Host arithmetic: ao[n] = sum w / (spp * pi) -- sum w / spp is ao.rs's radiance, pi where nothing occludes under cosine sampling, so the
 * map is 1 for an open surface --, bent_xyz[3 n] = normalize(sum wi); 0 where nothing was added (all four sums 0; the bent normal also
 * where the sum's length is 0). A NULL output is skipped. PT_ERR_INVALID_ARG for a NULL ao_w, both outputs NULL, or spp == 0. */
int pt_bake_resolve(const float *ao_w, uint32_t n_texels, uint32_t spp, float *ao, float *bent_xyz);
/* Fills the gutter round the islands of a plane of `channels` (1 .. 4) floats per texel, in place. Per iteration every texel that is
 * not covered and has at least one covered 8-neighbour inside the atlas gets the mean of its covered neighbours: per channel the sum
 * in the order (-1,-1), (0,-1), (1,-1), (-1,0), (1,0), (-1,1), (0,1), (1,1) of (dx, dy), divided by their count as a float; it counts
 * as covered from the next iteration on. Covered at the start: owner[texel] != PT_NONE. `owner` is not modified. Ping-pong buffers, no
 * atomics: the result does not depend on launch geometry. iterations == 0 leaves the plane as it is. PT_ERR_INVALID_ARG for a NULL
 * argument, width or height 0, more than 2^28 texels, or channels outside 1 .. 4. Unlike pt_bake_render, which starts the scene's kernel
 * statistics afresh, this call ADDS its launches to the kind "bake_dilate" of the statistics it finds (timed when the last bake was
 * profiled): the dilations that follow a bake are read with it, and their counts add up over calls until the next bake. */
int pt_bake_dilate(pt_scene *scene, const uint32_t *owner, float *plane, uint32_t channels, uint32_t width, uint32_t height, uint32_t iterations, int buffers_are_device);
/* Parity entry, in the style of pt_camera_rays: for n triples (texel index, sample number s, element k) -- host arrays -- the origin,
 * direction and weight of that AO ray, by the device function the render uses; found[i] = 0 and zeros where the texel has no owner.
 * The parameters, the selection and their checks are pt_bake_render's (spp_per_pass and profile are not read). */
int pt_bake_rays(pt_scene *scene, const PtBakeParams *params, const uint8_t *prim_select, uint32_t n_prims, uint32_t n, const uint32_t *texel, const uint32_t *sample,
                 const uint32_t *element, float *out_o, float *out_d, float *out_w, uint8_t *found);

/* ---- Transfer: another scene projected onto the atlas ------------------------------------------------------------------------------
 *
 * The other half of a baker's job: a low-polygon mesh with UVs (the TARGET scene, whose atlas is filled) and a detailed mesh without
 * them (the SOURCE scene, which the rays see). Per owned texel one projection ray goes from above the target's surface straight down
 * through the source; what it hits first leaves a height, a position, a world-space and a tangent-space normal, and the ambient
 * occlusion of the source at that point. The two handles may be the same: the target is then part of what the rays see and every
 * projection ray hits it at t = front or sooner -- rarely what one wants. Both must live on the same device. The target is only read:
 * every launch runs on the source scene's stream, and the counters and kernel statistics of the call are the SOURCE scene's.
 *
 * Every operation float32, unfused, in this order; cross, dot, normalize, coordinate_system and face_forward are dev_math.h's
 * (vector.rs): cross in float64 products rounded once, normalize(a) = a * (1 / sqrt(dot(a, a))).
 *
 * 1. Texel and owner. As above: texel centres, ownership with the texel box, and the owner's interaction si at the centre -- on the
 *    target scene. ns = normalize(si.sh_n).
 * 2. Projection ray. d = -ns, o = si.p + ns * front (no error-bound offset), t_max = front + back. A closest-hit query, Scene::intersect,
 *    through the source scene (libmi355pt's k_trace, launch kind "extend"; intersect_tests counts them). It is the same ray for every
 *    sample of the texel: one ray per owned texel per call.
 * 3. Hit. hit_prim = the source primitive (as pt_trace_closest reports it) or PT_NONE; height = front - t. A DETAIL HIT is a hit on a
 *    top-level triangle of the source: hs = the interaction Triangle::intersect builds for the hit's primitive and barycentrics, as
 *    pt_trace_closest reports them (tri_fill_interaction); src_position = hs.p; src_normal = nh = normalize(hs.sh_n), negated when
 *    dot(nh, d) > 0. A hit on a sphere, a disk or a primitive of an instanced object writes hit_prim and height only: the other planes
 *    are 0 there and no AO ray starts. A miss or a texel without owner: 0 everywhere, PT_NONE in hit_prim.
 * 4. Tangent frame of the target texel. sv = si.dpdu - ns * dot(ns, si.dpdu). If dot(sv, sv) > 0: sv = normalize(sv), tv = cross(ns, sv),
 *    and tv = -tv when dot(tv, si.dpdv) < 0 -- a mirrored UV island keeps its handedness; else (sv, tv) = coordinate_system(ns).
 *    dpdu and dpdv are Triangle::intersect's (triangle.rs:236-265; for degenerate UVs coordinate_system of the geometric normal).
 *    tangent_normal = (dot(nh, sv), dot(nh, tv), dot(nh, ns)).
 * 5. AO at a detail hit: AOIntegrator::li (ao.rs:78-107) with the projection ray as its camera ray. Frame n = face_forward(hs.n, -d),
 *    s = normalize(hs.dpdu), t = cross(hs.n, s). Element k of sample s of texel (x, y): the array value of sample number
 *    s * nsamples + k, dimensions 5 and 6, sample bounds [0, width) x [0, height); direction, origin (offset_ray_origin(hs.p, hs.p_error,
 *    hs.n, wi)) and weight as under "AO rays" above, by the same device function. The any-hit walk goes through the source scene with
 *    t_max = max_distance. ao_w gains the unoccluded rays' wi and w in ascending (s, k) order, onto what the buffer holds: sample
 *    ranges baked in ascending order, any spp_per_pass and repeated calls leave the same bytes. pt_bake_resolve and pt_bake_dilate
 *    serve the planes unchanged; hit_prim is a valid coverage map for pt_bake_dilate.
 *
 * Launch kinds (the source scene's pt_get_kernel_stats): "bake_select", "bake_raster", "bake_project" (the projection rays), "extend"
 * (their closest-hit walk), "bake_transfer_points", and with ao_w "bake_transfer_rays", "shadow", "bake_accum" ("bake_probe" for
 * pt_bake_transfer_rays). The projection rays are traced in slices of 8 x 8-texel tiles sized by the pass budget. */
typedef struct PtBakeTransferParams {
    uint32_t width, height;      /* the target's atlas; width * height <= 2^28                                            */
    float    front, back;        /* the projection ray starts `front` above the target's surface along its shading normal */
                                 /* and ends `back` below it; both >= 0 and finite, front + back > 0                      */
    uint32_t spp;                /* the AO at the source hit: PtBakeParams' meaning. spp, nsamples, max_distance and       */
    uint32_t nsamples;           /* sampler_type are read -- and checked -- only when ao_w is wanted                      */
    uint32_t cos_sample;
    float    max_distance;
    uint32_t sampler_type;
    uint32_t spp_per_pass;       /* 0: the library chooses from the free memory                                           */
    uint32_t profile;            /* != 0: time every launch kind                                                          */
} PtBakeTransferParams;

typedef struct PtBakeTransferBuffers {   /* width * height entries, row-major; NULL = not wanted */
    uint32_t *owner;             /* target primitive that owns the texel (pt_bake_render's owner map) -- written          */
    uint32_t *hit_prim;          /* source primitive the projection ray hits first, PT_NONE for none -- written           */
    float *height;               /* 1: front - t of that hit, 0 without one -- written                                    */
    float *src_position;         /* 3: the source hit point -- written                                                    */
    float *src_normal;           /* 3: the source's normalised shading normal there, world space -- written               */
    float *tangent_normal;       /* 3: the same vector in the target texel's tangent frame -- written                     */
    float *ao_w;                 /* 4: sums of the unoccluded AO directions and weights at the source hit -- ADDED to     */
} PtBakeTransferBuffers;

/* Projects the source scene onto the atlas of the target's primitives selected by prim_select (HOST memory, n_prims bytes: the TARGET's
 * primitives) and bakes params->spp AO samples per detail hit. Without ao_w no AO ray is traced and no sample number is drawn.
 * Errors. PT_ERR_INVALID_ARG, before the device is touched and in this order, for a NULL target, source, params, prim_select or buffers;
 * width or height 0 or more than 2^28 texels; front or back negative, infinite or NaN, or front + back == 0; all seven planes NULL; with
 * ao_w wanted: spp or nsamples 0, max_distance not positive, an unknown sampler_type, a bad sample range; nothing selected; n_prims
 * different from the target's primitive count. Then, with the source's device bound: the two scenes on different devices; more sample
 * numbers per texel than the sampler's tables serve. PT_ERR_UNSUPPORTED as pt_bake_render, for the selection. Host planes are written
 * only after everything has succeeded. */
int pt_bake_transfer(pt_scene *target, pt_scene *source, const PtBakeTransferParams *params, const uint8_t *prim_select, uint32_t n_prims,
                     const PtBakeTransferBuffers *buffers, int buffers_are_device);
/* AO samples [first_sample, first_sample + n_samples) of every detail hit (the range is read only when ao_w is wanted); the written planes
 * are written again, the same. pt_bake_transfer is the call (0, spp). */
int pt_bake_transfer_samples(pt_scene *target, pt_scene *source, const PtBakeTransferParams *params, const uint8_t *prim_select, uint32_t n_prims,
                             uint32_t first_sample, uint32_t n_samples, const PtBakeTransferBuffers *buffers, int buffers_are_device);
/* AO samples per texel per pass pt_bake_transfer would use (pt_bake_pass_size's rule, on the source scene); spp and nsamples are checked. */
int pt_bake_transfer_pass_size(pt_scene *target, pt_scene *source, const PtBakeTransferParams *params, uint32_t *spp_per_pass);
/* Parity entry, in the style of pt_bake_rays: for n triples (texel index, sample number s, element k) -- host arrays -- the texel's
 * projection ray (proj_o, proj_d, proj_tmax) and the AO ray (ao_o, ao_d, ao_w) from its detail hit, by the device functions the bake
 * uses. found[i]: bit 0 = the texel has an owner (else the projection ray is zeros), bit 1 = its ray made a detail hit (else the AO ray
 * is zeros). The parameters, the selection and their checks are pt_bake_transfer's with ao_w wanted (spp_per_pass and profile are not read). */
int pt_bake_transfer_rays(pt_scene *target, pt_scene *source, const PtBakeTransferParams *params, const uint8_t *prim_select, uint32_t n_prims, uint32_t n,
                          const uint32_t *texel, const uint32_t *sample, const uint32_t *element, float *proj_o, float *proj_d, float *proj_tmax,
                          float *ao_o, float *ao_d, float *ao_w, uint8_t *found);

/* ---- Lightmap: the scene's lights baked into the atlas -------------------------------------------------------------------------------
 *
 * The irradiance every owned texel receives DIRECTLY from the scene's lights, on the side its normal faces: the direct-lighting estimate
 * of integrators/directlighting.rs with the surface's BSDF left out (a lightmap is multiplied with the albedo where it is used), no
 * indirect light, no emission of the baked surface itself. Every light type the renderer knows is served, by the device function the
 * render samples its lights with. Every operation float32, unfused, in this order:
 *
 * 1. Texel, owner, surface point. The atlas bake's, unchanged: texel centres, ownership with the texel box, the owner's interaction si at
 *    the centre. The reference point of the light samples is ref = {si.p, si.p_error, si.n}; ns = normalize(si.sh_n).
 * 2. Which light. sel[0 .. n_sel) are the selected lights in ascending index (light_select; NULL: all of the scene's). Sample number
 *    j = s * nsamples + k of a texel -- element k of sample s -- samples light sel[j mod n_sel], in 64-bit arithmetic. spp * nsamples
 *    must be a multiple of n_sel, so that every light gets exactly spp * nsamples / n_sel samples per texel. nsamples == n_sel is
 *    directlighting.rs's "all lights, one sample each"; a smaller nsamples serves scenes with many emissive triangles. The light of a
 *    sample does NOT depend on the texel: the 64 texels a wave works on sample the same light (see k_bake_light_rays).
 * 3. Light sample. u = the 2-D array value of sample number j of pixel (x, y), dimensions 5 and 6, of a sampler set up for sample bounds
 *    [0, width) x [0, height), as under "AO rays". (Li, wi, pdf, p1) = Light::sample_li(ref, u) (lights/point.rs, spot.rs, distant.rs,
 *    diffuse.rs with Triangle / Sphere / Disk::sample, infinite.rs), p1 being the far end of its visibility segment: the light's
 *    position, the sampled point of an area light with its error bound and normal, or ref.p + wi * (2 * world radius).
 * 4. Contribution. A sample contributes only if pdf > 0, Li is not black (all three channels 0), c = dot(wi, ns) > 0 and
 *    dot(wi, si.n) > 0 (a NaN fails each): a lightmap is one-sided, light from behind the surface adds nothing. Then
 *        w = (c * ((float)n_sel / (float)nsamples)) / pdf,      E = Li * w   per channel.
 * 5. Shadow ray. VisibilityTester::unoccluded's ray: Interaction::spawn_ray_to(ref, p1) (interaction.rs:45-52) --
 *        o = offset_ray_origin(ref.p, ref.p_error, ref.n, p1.p - ref.p),  d = offset_ray_origin(p1.p, p1.p_error, p1.n, o - p1.p) - o
 *    -- an any-hit query through the whole scene (spheres, instances, alpha masks, the baked mesh itself) with t_max = 1 - 0.0001f: the
 *    render's shadow ray. A sample that does not contribute spawns no ray. Media are NOT consulted: there is no transmittance along the
 *    segment, as under Integrator "path" -- a scene's participating media do not dim its lightmap.
 * 6. Sums. light_w[texel] += (E.r, E.g, E.b, 1.0f) for every unoccluded contributing sample, in ascending (s, k), onto what the buffer
 *    holds. Sample ranges baked in ascending order, any spp_per_pass, repeated calls and device or host buffers leave the same bytes.
 * 7. Resolve (pt_bake_light_resolve). irradiance = rgb / (float)spp; reached = w / ((float)spp * (float)nsamples), the fraction of
 *    the light samples that arrived; both 0 where nothing was added (all four sums 0).
 *
 * spp * nsamples is limited as under "AO rays". PtCounters.shadow_tests = the shadow rays traced = the contributing samples. Launch
 * kinds: "bake_select", "bake_raster", "bake_points", "bake_light_rays", "shadow", "bake_light_accum" ("bake_probe" for
 * pt_bake_light_rays). The samples of a pass are taken in chunks of at most 64 elements per texel sample; with nsamples > 64 a pass is one
 * sample, as for the AO bake. */
typedef struct PtBakeLightParams {
    uint32_t width, height;      /* the atlas, texels; width * height <= 2^28                         */
    uint32_t spp;                /* the job's samples per texel, > 0                                  */
    uint32_t nsamples;           /* light samples per sample, > 0; spp * nsamples a multiple of n_sel */
    uint32_t sampler_type;       /* PtSamplerType                                                     */
    uint32_t spp_per_pass;       /* 0: the library chooses from the free memory                       */
    uint32_t profile;            /* != 0: time every launch kind (pt_get_kernel_stats)                */
} PtBakeLightParams;

typedef struct PtBakeLightBuffers {   /* width * height entries, row-major; NULL = not wanted */
    uint32_t *owner;             /* primitive that owns the texel, PT_NONE for none -- written        */
    float *position;             /* 3 per texel: p; 0 where the texel has no owner -- written         */
    float *normal;               /* 3 per texel: the normalised shading normal; 0 likewise -- written */
    float *light_w;              /* 4 per texel: sum of E.rgb, count of arrived samples -- ADDED to   */
} PtBakeLightBuffers;

/* Bakes params->spp samples of params->nsamples light samples each per texel of the primitives selected by prim_select (pt_bake_render's)
 * under the lights selected by light_select -- HOST memory, n_lights bytes in PtSceneDesc's light order, non-zero = the light is baked;
 * NULL = all n_lights lights: static lights only, or one map per light. Without light_w no ray is traced.
 * Errors. PT_ERR_INVALID_ARG, before the device is touched and in this order, for a NULL scene, params, prim_select or buffers; width or
 * height 0 or more than 2^28 texels; spp or nsamples 0; an unknown sampler_type; all four planes NULL; a bad sample range; no primitive
 * selected; no light selected (n_lights == 0 included); spp * nsamples no multiple of the number of selected lights (the message names both
 * numbers); n_prims different from the scene's primitive count; n_lights different from the scene's light count. Then as pt_bake_render:
 * the sampler's limits, PT_ERR_UNSUPPORTED for the selection. Host planes are written only after everything has succeeded. */
int pt_bake_light(pt_scene *scene, const PtBakeLightParams *params, const uint8_t *prim_select, uint32_t n_prims, const uint8_t *light_select, uint32_t n_lights,
                  const PtBakeLightBuffers *buffers, int buffers_are_device);
/* Samples [first_sample, first_sample + n_samples) of every texel; params->spp stays the job's sample count. pt_bake_light is the call (0, spp). */
int pt_bake_light_samples(pt_scene *scene, const PtBakeLightParams *params, const uint8_t *prim_select, uint32_t n_prims, const uint8_t *light_select, uint32_t n_lights,
                          uint32_t first_sample, uint32_t n_samples, const PtBakeLightBuffers *buffers, int buffers_are_device);
/* Samples per texel per pass pt_bake_light would use: pt_bake_pass_size's rule with 20 more bytes per ray (what it adds, its id). */
int pt_bake_light_pass_size(pt_scene *scene, const PtBakeLightParams *params, const uint8_t *light_select, uint32_t n_lights, uint32_t *spp_per_pass);
/* Host arithmetic: step 7. A NULL output is skipped. PT_ERR_INVALID_ARG for a NULL light_w, both outputs NULL, spp or nsamples 0. */
int pt_bake_light_resolve(const float *light_w, uint32_t n_texels, uint32_t spp, uint32_t nsamples, float *irradiance_rgb, float *reached);
/* Parity entry, in the style of pt_bake_rays: for n triples (texel index, sample number s, element k) -- host arrays -- the light that
 * sample is taken on, Light::sample_li's wi, pdf and Li, E and the shadow ray (out_o, out_d), by the device function the bake uses.
 * found[i]: bit 0 = the texel has an owner (else everything but out_light is zeros), bit 1 = the sample contributes (else E and the ray are
 * zeros). The parameters, the selections and their checks are pt_bake_light's (spp_per_pass and profile are not read). */
int pt_bake_light_rays(pt_scene *scene, const PtBakeLightParams *params, const uint8_t *prim_select, uint32_t n_prims, const uint8_t *light_select, uint32_t n_lights,
                       uint32_t n, const uint32_t *texel, const uint32_t *sample, const uint32_t *element, uint32_t *out_light, float *out_wi, float *out_pdf,
                       float *out_li, float *out_e, float *out_o, float *out_d, uint8_t *found);

/* ---- SH points: the scene's lights baked at free points into order-2 spherical harmonics ("light probes") -----------------------------
 *
 * What has no UV atlas -- a character, a prop, a particle, a point in the air -- gets its direct light from points in space: the incident
 * radiance at a point, projected onto the nine real spherical harmonics of orders 0 to 2, per colour channel. A dynamic object evaluates
 * them with its own normal (pt_bake_sh_irradiance). The light samples, the shadow rays and the sums are the lightmap's; the reference point
 * has no surface and an SH projection stands where the cosine stood. Every operation float32, unfused, in this order:
 *
 * 1. Points. n_points points p_i, HOST memory, three floats each, all finite. Point i is pixel (x, y) = (i mod row, i / row) of a sampler
 *    set up for sample bounds [0, row) x [0, rows), rows = ceil(n_points / row). The reference point of its light samples is
 *    ref = {p_i, p_error = 0, n = 0}: a medium interaction's, as estimate_direct gets one from integrators/volpath.rs. With n = 0
 *    offset_ray_origin adds nothing: every shadow ray starts at p_i exactly.
 * 2. Which light. The lightmap's step 2: sel[] ascending, sample number j = s * nsamples + k samples light sel[j mod n_sel] in 64-bit
 *    arithmetic, spp * nsamples a multiple of n_sel. The light of a sample does NOT depend on the point (see k_bake_sh_rays).
 * 3. Light sample. The lightmap's step 3: u = the 2-D array value of sample number j of pixel (x, y), dimensions 5 and 6;
 *    (Li, wi, pdf, p1) = Light::sample_li(ref, u), by the device function the render samples its lights with.
 * 4. Contribution. A sample contributes if pdf > 0 (a NaN fails) and Li is not black. There is no cosine and no side test: a point
 *    receives light from the whole sphere. Then
 *        w = ((float)n_sel / (float)nsamples) / pdf,      E = Li * w   per channel.
 * 5. Shadow ray. The lightmap's step 5: Interaction::spawn_ray_to(ref, p1), an any-hit query through the whole scene with
 *    t_max = 1 - 0.0001f. Media are NOT consulted. A sample that does not contribute spawns no ray.
 * 6. Basis. With (x, y, z) = wi -- sample_li's wi, not the normalised ray direction -- and float32 literals:
 *        Y0 = 0.282095f                  Y1 = 0.488603f * y              Y2 = 0.488603f * z
 *        Y3 = 0.488603f * x              Y4 = 1.092548f * (x * y)        Y5 = 1.092548f * (y * z)
 *        Y6 = 0.315392f * ((3.0f * (z * z)) - 1.0f)                      Y7 = 1.092548f * (x * z)
 *        Y8 = 0.546274f * ((x * x) - (y * y))
 * 7. Sums. sh_w holds 28 floats per point. For every unoccluded contributing sample sh_w[28 i + 3 q + c] += E.c * Y_q for q in 0 .. 8 and
 *    c in r, g, b, and sh_w[28 i + 27] += 1.0f, in ascending (s, k), onto what the buffer holds. Sample ranges baked in ascending order,
 *    any spp_per_pass, repeated calls and device or host buffers leave the same bytes.
 * 8. Resolve (pt_bake_sh_resolve). sh[27 i + m] = sh_w[28 i + m] / (float)spp: the SH coefficients of the direct incident radiance;
 *    reached[i] = sh_w[28 i + 27] / ((float)spp * (float)nsamples). Both 0 where all 28 sums are 0.
 * 9. Irradiance (pt_bake_sh_irradiance). For a unit normal nrm, E_c = the sum over q ascending, from 0.0f, of (A_q * sh[3 q + c]) *
 *    Y_q(nrm), with A_0 = 3.141593f, A_1..3 = 2.094395f, A_4..8 = 0.785398f: Ramamoorthi and Hanrahan's cosine-lobe factors. The sum is
 *    NOT clamped: an order-2 fit can go slightly negative, and the caller decides what to do with that.
 *
 * Where the arithmetic produces NaN or infinity the sums hold what it leaves: a point on a point light's position (wi = 0 / 0, pdf = 1
 * contributes), or in an emissive triangle's plane. Keep points off the lights. spp * nsamples is limited as under "AO rays"; under Sobol'
 * row and rows are limited to the 2^25 pixel grid. PtCounters.shadow_tests = the shadow rays traced = the contributing samples. Launch
 * kinds: "bake_sh_rays", "shadow", "bake_sh_accum" ("bake_probe" for pt_bake_sh_rays). Chunks and passes as for the lightmap. */
typedef struct PtBakeShParams {
    uint32_t n_points;           /* 1 .. 2^28                                                          */
    uint32_t row;                /* points per sampler row, 1 .. 2^28                                  */
    uint32_t spp;                /* the job's samples per point, > 0                                   */
    uint32_t nsamples;           /* light samples per sample, > 0; spp * nsamples a multiple of n_sel  */
    uint32_t sampler_type;       /* PtSamplerType                                                      */
    uint32_t spp_per_pass;       /* 0: the library chooses from the free memory                        */
    uint32_t profile;            /* != 0: time every launch kind (pt_get_kernel_stats)                 */
} PtBakeShParams;

/* Bakes params->spp samples of params->nsamples light samples each at every point under the lights selected by light_select
 * (pt_bake_light's). points and light_select are HOST memory; sh_w -- 28 floats per point, device or host memory -- is ADDED to.
 * Errors. PT_ERR_INVALID_ARG, before the device is touched and before the scene handle is read, in this order: a NULL scene, params, points
 * or sh_w; n_points 0 or above 2^28; row 0 or above 2^28; spp or nsamples 0; an unknown sampler_type; a bad sample range; a point with a
 * coordinate that is not finite (the message names the point); no light selected (n_lights == 0 included); spp * nsamples no multiple of
 * the number of selected lights (the message names both numbers). Then, reading the handle's host side: n_lights different from the
 * scene's light count. Then, with the device bound: the sampler's limits. A host sh_w is written only after everything has succeeded. */
int pt_bake_sh(pt_scene *scene, const PtBakeShParams *params, const float *points, const uint8_t *light_select, uint32_t n_lights, float *sh_w, int buffers_are_device);
/* Samples [first_sample, first_sample + n_samples) of every point; params->spp stays the job's sample count. pt_bake_sh is the call (0, spp). */
int pt_bake_sh_samples(pt_scene *scene, const PtBakeShParams *params, const float *points, const uint8_t *light_select, uint32_t n_lights, uint32_t first_sample,
                       uint32_t n_samples, float *sh_w, int buffers_are_device);
/* Samples per point per pass pt_bake_sh would use: pt_bake_light_pass_size's rule over the points padded to a multiple of 64, with 36 more
 * bytes per ray (what it adds, its wi, its id). */
int pt_bake_sh_pass_size(pt_scene *scene, const PtBakeShParams *params, const uint8_t *light_select, uint32_t n_lights, uint32_t *spp_per_pass);
/* Host arithmetic: step 8. sh: 27 floats per point (coefficient q, channel c at 3 q + c). A NULL output is skipped. PT_ERR_INVALID_ARG for
 * a NULL sh_w, both outputs NULL, spp or nsamples 0. */
int pt_bake_sh_resolve(const float *sh_w, uint32_t n_points, uint32_t spp, uint32_t nsamples, float *sh, float *reached);
/* Host arithmetic: step 9 for n pairs -- entry i of sh (27 floats) goes with normal i (3 floats, unit length; not checked).
 * PT_ERR_INVALID_ARG for a NULL argument. */
int pt_bake_sh_irradiance(const float *sh, const float *normals, uint32_t n, float *irradiance_rgb);
/* Parity entry, in the style of pt_bake_light_rays: for n triples (point index, sample number s, element k) -- host arrays -- the light
 * that sample is taken on, Light::sample_li's wi, pdf and Li, E and the shadow ray (out_o, out_d), by the device function the bake uses.
 * found[i]: bit 0 = the point index is below n_points (else everything but out_light is zeros), bit 1 = the sample contributes (else E and
 * the ray are zeros). The parameters, the points, the selection and their checks are pt_bake_sh's (spp_per_pass and profile are not read);
 * a sample or element outside the job is refused after them. */
int pt_bake_sh_rays(pt_scene *scene, const PtBakeShParams *params, const float *points, const uint8_t *light_select, uint32_t n_lights, uint32_t n, const uint32_t *point,
                    const uint32_t *sample, const uint32_t *element, uint32_t *out_light, float *out_wi, float *out_pdf, float *out_li, float *out_e, float *out_o,
                    float *out_d, uint8_t *found);

#ifdef __cplusplus
}
#endif
#endif
