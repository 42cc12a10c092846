// bake_render.hip -- the entry points of include/mi355bake.h: four bakes (pt_bake_render: AO and bent normals, pt_bake_transfer: another scene projected onto the atlas,
// pt_bake_light: the lightmap, pt_bake_sh: the lights at free points in order-2 spherical harmonics), each with its _samples, _pass_size and _rays (probe) forms, the
// resolves and pt_bake_dilate. There is no camera, no path state and no film, so a bake does not go through render_frame: the scene's stream, counters and traversal spill
// area come from ensure_workspace with no paths and no film, the sampler from fill_render_const for a width x height image (bake_geometry), the traversal goes through
// trace_job / trace_sub / traced as libmi355ao's AO rays do. Every call is made of the same steps, each written once:
//   the refusals          check_*: before the device or a handle is touched, in the header's order; then bake_geometry (bind_device, sampler, pass size), begin_call
//   Staging               a plane on the device: the caller's device pointer, or a temporary that is uploaded where it is added to (the *_w sums) and copied home by
//                         finish() -- after end_call, so a call that fails midway writes no host plane; the temporaries go when the call returns
//   atlas_frame           upload_selection (k_bake_top, k_bake_check: why a selected primitive is no bake target), the owner map (k_bake_raster), the position / normal
//                         planes where wanted (k_bake_points). It takes the scene that is read and the scene the launches run on: a transfer's are target and source.
//                         The SH points have no atlas: their points are uploaded instead (upload_points)
//   for_passes            samples [first, first + n) in passes of S; a pass of several samples has ONE chunk (bake_geometry), so a texel's additions are in (s, k) order
//   pass_chunks           one pass through ao_chunks (side_host.h), <= 64 rays per item and chunk: the bake's ray kernel, k_trace<any> ("shadow", libmi355pt's), the
//                         bake's accumulate kernel -- bake_pass, transfer_pass, light_pass and sh_pass fill in their job and their two launches
//   light_samples         the light-sample fields of the lightmap's and the SH points' jobs: selection, scale, id table, E records
//   launch_sph            the <true> / <false> pair of the kernels that sample lights, SPH as the render chooses it
//   upload_queries, check_queries, LightRows    a probe's three index arrays, their range check, and the 16-float row the two light probes leave
// What is a bake's own:
//   AO         k_bake_rays (dimensions 5 and 6 of sample numbers s * nsamples + k), t_max = max_distance, k_bake_accum: ao_w += the unoccluded rays' wi and w
//   transfer   project(): k_bake_top of the source, then per slice of 8 x 8-texel tiles sized by the pass budget k_bake_project, k_trace<closest> ("extend", per-ray t_max =
//              front + back), k_bake_transfer_points (hit_prim, height, source position, world- and tangent-space normal, the hit records); its slice records are freed
//              before the AO passes allocate theirs. Then k_bake_transfer_rays and k_bake_accum over the detail-hit map. Counters and statistics are the source's
//   lightmap   k_bake_light_rays<SPH> (Light::sample_li, the contribution test, the shadow rays of the samples that contribute and what each adds), t_max = 1 - 0.0001 as the
//              render's shadow rays, k_bake_light_accum: light_w += {E, 1}. The budget is ao_ray_budget's plus 20 bytes per ray
//   SH points  k_bake_sh_rays<SPH> (those samples from a point without surface, and each ray's wi), k_bake_sh_accum: sh_w += {E * Y_q(wi), 1}. A sample number's items are
//              the points padded to whole waves; the budget is ao_ray_budget's plus 36 bytes per ray
#include "../csrc/host_common.h"
#include "../side/side_host.h"
#include "../../include/mi355bake.h"
#include "bake_kernels.h"

using namespace ptbake;

namespace {

constexpr size_t kBakeMaxTexels = (size_t)1 << 28;
constexpr uint32_t kRasterFewTriangles = 16384;    // a selection of fewer triangles is rastered in row bands (k_bake_raster)

struct Geometry { RenderConst rc; BakeAtlas atlas; uint32_t S; uint32_t K; };

// ---- what is checked before the device is touched
int check_atlas(uint32_t width, uint32_t height) {
    if (width == 0 || height == 0) return fail(PT_ERR_INVALID_ARG, "bake: width and height must be > 0");
    if ((size_t)width * height > kBakeMaxTexels) return fail(PT_ERR_INVALID_ARG, "bake: the atlas holds more than 2^28 texels");
    return PT_OK;
}
int check_spp(uint32_t spp) { return spp == 0 ? fail(PT_ERR_INVALID_ARG, "bake: spp must be > 0") : PT_OK; }
int check_nsamples(uint32_t nsamples) { return nsamples == 0 ? fail(PT_ERR_INVALID_ARG, "bake: nsamples must be > 0") : PT_OK; }
int check_sampler(uint32_t type) {
    if (type != PT_SAMPLER_SOBOL && type != PT_SAMPLER_HALTON) return fail(PT_ERR_INVALID_ARG, "bake: sampler_type must be PT_SAMPLER_SOBOL or PT_SAMPLER_HALTON");
    return PT_OK;
}
int check_params(const PtBakeParams *bp) {
    if (int st = check_atlas(bp->width, bp->height)) return st;
    if (int st = check_spp(bp->spp)) return st;
    if (int st = check_nsamples(bp->nsamples)) return st;
    if (!(bp->max_distance > 0.0f)) return fail(PT_ERR_INVALID_ARG, "bake: max_distance must be > 0 (INFINITY: unbounded)");
    return check_sampler(bp->sampler_type);
}
int check_range(const PtBakeParams *bp, uint32_t first, uint32_t n) {
    if (n == 0) return fail(PT_ERR_INVALID_ARG, "bake: n_samples must be > 0");
    if ((uint64_t)first + n > bp->spp) return fail(PT_ERR_INVALID_ARG, "bake: sample range [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + n) + ") exceeds the job's spp = " + std::to_string(bp->spp));
    return PT_OK;
}
// The queries of a probe: every one names a sample and an element of the job
int check_queries(uint32_t n, const uint32_t *sample, const uint32_t *element, uint32_t spp, uint32_t nsamples) {
    for (uint32_t i = 0; i < n; ++i)
        if (sample[i] >= spp || element[i] >= nsamples) return fail(PT_ERR_INVALID_ARG, "bake: ray " + std::to_string(i) + " names a sample or element outside the job");
    return PT_OK;
}
int check_selection(const uint8_t *prim_select, uint32_t n_prims) {
    for (uint32_t i = 0; i < n_prims; ++i) if (prim_select[i]) return PT_OK;
    return fail(PT_ERR_INVALID_ARG, "bake: no primitive is selected");
}

// (the scene's primitive count is the handle's host side)
int check_prim_count(const pt_scene *sc, uint32_t n_prims) {
    if (n_prims != sc->ds.n_prims) return fail(PT_ERR_INVALID_ARG, "bake: prim_select has " + std::to_string(n_prims) + " entries, the scene " + std::to_string(sc->ds.n_prims) + " primitives");
    return PT_OK;
}

// The sampler of a width x height image (fill_render_const), the checks on its sample numbers and the pass size
// (`slots`: the items of one sample number, 0: the atlas's tile slots; the SH points have no atlas and pass their padded point count)
int bake_geometry(pt_scene *sc, const PtBakeParams *bp, uint32_t n_samples, Geometry &g, size_t extra_bytes_per_ray = 0, uint32_t slots = 0) {
    if (sc->device != g_device) { if (int st = bind_device(sc->device)) return st; }
    PtRenderParams rp{};
    rp.sample_bounds[2] = rp.pixel_bounds[2] = rp.cropped_pixel_bounds[2] = (int32_t)bp->width;
    rp.sample_bounds[3] = rp.pixel_bounds[3] = rp.cropped_pixel_bounds[3] = (int32_t)bp->height;
    rp.full_resolution[0] = (int32_t)bp->width; rp.full_resolution[1] = (int32_t)bp->height;
    for (int i = 0; i < 4; ++i) rp.raster_to_camera[5 * i] = rp.camera_to_world[5 * i] = 1.0f;   // (not read: there is no camera)
    rp.spp = bp->spp; rp.sampler_type = bp->sampler_type; rp.filter_radius[0] = rp.filter_radius[1] = 1.0f; rp.tile_world = 1;
    RenderConst &rc = g.rc;
    fill_render_const(&rp, rc);
    if (rc.sobol.log2_resolution > 25) return fail(PT_ERR_INVALID_ARG, "bake: the atlas exceeds the 2^25 Sobol' pixel grid");
    g.atlas = make_atlas(bp->width, bp->height);
    if (slots == 0) slots = g.atlas.slots;
    if (int st = check_ao_sample_numbers(rc, bp->spp, bp->nsamples, "bake", "texel")) return st;
    g.K = std::min<uint32_t>(bp->nsamples, kAOChunk);
    uint32_t S = bp->spp_per_pass;
    // (per texel sample: the ray id base and the chunk's rays. The rule counts libmi355pt's path workspace too, which the bake does not allocate: the choice errs small)
    PassBudget budget = ao_ray_budget(g.K);
    budget.extra_bytes_per_path += (size_t)g.K * extra_bytes_per_ray;   // (the lightmap: what a ray adds and its entry of the id table)
    if (S == 0) S = choose_pass_size(sc, slots, n_samples, 1, false, budget);
    S = std::min(S, n_samples);
    // The additions to a texel are in (sample, element) order: a pass of several samples is accumulated sample by sample within ONE chunk; with more than one chunk
    // per sample a pass is one sample
    if (bp->nsamples > kAOChunk) S = 1;
    if ((size_t)slots * S * g.K > kAOMaxRays) return fail(PT_ERR_INVALID_ARG, "bake: pass too large: texels x samples per pass x min(nsamples, 64) AO rays per launch > 2^31 (lower spp_per_pass)");
    g.S = S;
    return PT_OK;
}

// The scene's stream, counters and traversal spill area (no paths, no film), and a clean slate for the call's statistics
int begin_call(pt_scene *sc, bool profile) {
    if (int st = ensure_workspace(sc, 0, 0)) return st;
    sc->profile = profile;
    sc->drop_timings();
    sc->stats.clear();
    sc->counters = PtCounters{};
    HIP_TRY(hipMemsetAsync(sc->dc, 0, sizeof(DevCounters), sc->stream));
    HIP_TRY(hipMemsetAsync(sc->qc, 0, sizeof(QCounters), sc->stream));
    return PT_OK;
}

dim3 texel_grid(const BakeAtlas &a) { return dim3((unsigned)(((size_t)a.n_texels + 255) / 256)); }

// In the three functions below `of` is the scene whose primitives are read and `sc` the scene whose stream and statistics the launches run under (pt_bake_render: the
// same scene; pt_bake_transfer: the target and the source). `of` is only read.
// The marks of the top-level accelerator's primitives (d_top: zeroed, of->ds.n_prims bytes), inside the launch kind the caller has opened
void launch_top(pt_scene *sc, const pt_scene *of, uint8_t *d_top) {
    const uint32_t n_top = (uint32_t)of->ordered.size();
    if (n_top > 0 && of->ds.n_nodes > 0) launch(sc, "ptbake::k_bake_top", k_bake_top, dim3((n_top + 255) / 256), dim3(256), of->ds, n_top, d_top);
}

// The selection on the device: the ascending list of selected primitives, every one of which must be a top-level triangle of a mesh with UVs. The check runs on the
// device (k_bake_top, k_bake_check); what comes back is one word per 256 selected primitives and, for a refused selection, the codes of the first refused block.
// (prim_select itself is walked on the host, a byte per primitive, and the list uploaded, 4 bytes per selected primitive: on every call, a continuation's included.)
int upload_selection(pt_scene *sc, const pt_scene *of, const uint8_t *prim_select, uint32_t n_prims, DevTmp &tmp, uint32_t *&d_selected, uint32_t &n_selected) {
    const DeviceScene &ds = of->ds;
    std::vector<uint32_t> selected;
    for (uint32_t p = 0; p < n_prims; ++p) if (prim_select[p]) selected.push_back(p);
    n_selected = (uint32_t)selected.size();
    const uint32_t n_top = (uint32_t)of->ordered.size(), n_blocks = (n_selected + 255) / 256;
    uint8_t *d_top = nullptr, *d_code = nullptr; uint32_t *d_refused = nullptr;
    SIDE_ALLOC(tmp, d_top, n_prims, "bake selection"); SIDE_ALLOC(tmp, d_selected, (size_t)n_selected * 4, "bake selection");
    SIDE_ALLOC(tmp, d_code, n_selected, "bake selection"); SIDE_ALLOC(tmp, d_refused, (size_t)n_blocks * 4, "bake selection");
    HIP_TRY(hipMemsetAsync(d_top, 0, n_prims, sc->stream));
    HIP_TRY(hipMemcpyAsync(d_selected, selected.data(), (size_t)n_selected * 4, hipMemcpyHostToDevice, sc->stream));
    sc->begin("bake_select", (uint64_t)n_top + n_selected);
    launch_top(sc, of, d_top);
    launch(sc, "ptbake::k_bake_check", k_bake_check, dim3(n_blocks), dim3(256), ds, (const uint8_t *)d_top, (const uint32_t *)d_selected, n_selected, d_code, d_refused);
    sc->end();
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> refused(n_blocks);
    HIP_TRY(hipMemcpyAsync(refused.data(), d_refused, (size_t)n_blocks * 4, hipMemcpyDeviceToHost, sc->stream));
    HIP_TRY(hipStreamSynchronize(sc->stream));   // (`selected` is on the device by now, too)
    for (uint32_t blk = 0; blk < n_blocks; ++blk) {
        if (!refused[blk]) continue;
        const uint32_t first = blk * 256u, n = std::min(256u, n_selected - first);
        uint8_t code[256];
        HIP_TRY(hipMemcpy(code, d_code + first, n, hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < n; ++k) {
            const std::string who = "bake: selected primitive " + std::to_string(selected[first + k]);
            if (code[k] == kBakeQuadric) return fail(PT_ERR_UNSUPPORTED, who + " is a sphere or disk: only triangles have a UV atlas here");
            if (code[k] == kBakeInstanced) return fail(PT_ERR_UNSUPPORTED, who + " belongs to an instanced object: instanced geometry is not baked");
            if (code[k] == kBakeNoUV) return fail(PT_ERR_UNSUPPORTED, who + " is a triangle of a mesh without UVs");
        }
    }
    return PT_OK;
}

// Owner map of the selection. Few triangles: row bands, so that a large triangle's box is shared among the waves of many blocks; many: one band, a triangle per lane.
int raster(pt_scene *sc, const pt_scene *of, const BakeAtlas &a, const uint32_t *d_selected, uint32_t n_selected, uint32_t *d_owner) {
    HIP_TRY(hipMemsetAsync(d_owner, 0xff, (size_t)a.n_texels * 4, sc->stream));
    // (a two-triangle quad over a 4096^2 atlas: one thread per triangle 3806 ms, one wave sharing each box 107.9 ms, bands of 64 rows 1.71 ms, of 16 rows 0.44 ms, of 8
    // rows 0.24 ms; 4.3 M sub-texel triangles on 2048^2 in one band: 0.15 ms -- profiles/r6/NOTES.md)
    const uint32_t band_rows = std::min(a.height, n_selected >= kRasterFewTriangles ? a.height : std::max<uint32_t>(4, (a.height + 511) / 512));
    const uint32_t bands = (a.height + band_rows - 1) / band_rows;
    const uint32_t blocks = std::max(1u, std::min<uint32_t>((n_selected + 255) / 256, (uint32_t)g_num_cus * 8u));
    sc->begin("bake_raster", n_selected);
    launch(sc, "ptbake::k_bake_raster", k_bake_raster, dim3(blocks, bands), dim3(256), of->ds, a, d_selected, n_selected, band_rows, d_owner);
    sc->end();
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

int end_call(pt_scene *sc) {
    QCounters h;
    if (int st = sync_queue_counters(sc, h)) return st;   // (a status a kernel raised fails the call here)
    sc->resolve_timings();
    read_counters(sc);
    return PT_OK;
}

// ---- the call frame: what every bake and every probe is made of

// The planes of a call on the device. A plane the caller did not ask for is NULL; one of a call with device buffers is the caller's pointer; one of a call with host
// buffers is a temporary of `tmp` (freed when the call returns, however it ends: a bake leaves the device's free memory as it found it, apart from the scene's
// workspace) that finish() copies home -- after end_call has succeeded, so a call that fails midway writes no host plane.
struct Staging {
    DevTmp &tmp; hipStream_t stream; bool dev;
    struct Home { void *host; const void *device; size_t bytes; };
    std::vector<Home> home;
    // `upload`: the plane is added to (the *_w sums), so the temporary starts from what the caller's array holds
    template <class D, class T> int plane(T *user, size_t bytes, const char *what, bool upload, D *&d) {
        d = dev ? reinterpret_cast<D *>(user) : nullptr;
        if (!user || dev) return PT_OK;
        SIDE_ALLOC(tmp, d, bytes, what);
        if (upload) HIP_TRY(hipMemcpyAsync(d, user, bytes, hipMemcpyHostToDevice, stream));
        home.push_back(Home{user, d, bytes});
        return PT_OK;
    }
    int finish(pt_scene *sc) {
        if (int st = end_call(sc)) return st;
        for (const Home &h : home) HIP_TRY(hipMemcpy(h.host, h.device, h.bytes, hipMemcpyDeviceToHost));
        return PT_OK;
    }
};

// The atlas part of a call: the selection of `of`'s primitives on the device, their owner map -- the caller's plane (Staging) or a temporary nobody reads back -- and,
// where asked for, the position and normal planes. `of` is the scene that is read, `sc` the scene the launches run on (upload_selection).
int atlas_frame(pt_scene *sc, const pt_scene *of, const BakeAtlas &a, const uint8_t *prim_select, uint32_t n_prims, Staging &out, uint32_t *owner, float *position, float *normal, uint32_t *&d_owner) {
    const size_t n = a.n_texels;
    uint32_t *d_selected = nullptr, n_selected = 0;
    if (int st = upload_selection(sc, of, prim_select, n_prims, out.tmp, d_selected, n_selected)) return st;
    if (int st = out.plane(owner, n * 4, "bake owner map", false, d_owner)) return st;
    if (!d_owner) SIDE_ALLOC(out.tmp, d_owner, n * 4, "bake owner map");
    if (int st = raster(sc, of, a, d_selected, n_selected, d_owner)) return st;
    if (!position && !normal) return PT_OK;
    float *d_pos = nullptr, *d_nrm = nullptr;
    if (int st = out.plane(position, n * 12, "bake position plane", false, d_pos)) return st;
    if (int st = out.plane(normal, n * 12, "bake normal plane", false, d_nrm)) return st;
    sc->begin("bake_points", n);
    launch(sc, "ptbake::k_bake_points", k_bake_points, texel_grid(a), dim3(256), of->ds, a, d_owner, d_pos, d_nrm);
    sc->end();
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

// The ray buffers of the largest pass (`slots` items per sample number), and the passes of the samples [first, first + n_samples): pass(s_begin, s_count)
int alloc_pass_rays(const Geometry &g, uint32_t slots, const char *what, AORayBuffers &b, size_t &rays) {
    const size_t items = (size_t)slots * g.S;
    rays = items * g.K;
    return b.alloc(items, rays, what);
}
template <class Pass> int for_passes(const Geometry &g, uint32_t first, uint32_t n_samples, const Pass &pass) {
    for (uint32_t s0 = first, end = first + n_samples; s0 < end; s0 += g.S)
        if (int st = pass(s0, std::min(g.S, end - s0))) return st;
    return PT_OK;
}

// One pass chunk by chunk (ao_chunks): `job` comes with what its bake adds and gets the samples here; spawn(job, blocks) and accum(job) launch under their launch kinds
template <class Job, class Spawn, class Accum>
int pass_chunks(pt_scene *sc, const Geometry &g, Job job, uint32_t nsamples, uint32_t cos_sample, uint32_t s_begin, uint32_t s_count, uint32_t items, float t_max, const AORayBuffers &b,
                const char *spawn_kind, const Spawn &spawn, const char *accum_kind, const Accum &accum) {
    job.nsamples = nsamples; job.cos_sample = cos_sample ? 1u : 0u; job.s_begin = s_begin; job.s_count = s_count;
    const dim3 blocks = blocks_for(items, 16u);
    return ao_chunks<Job>(sc, job, g.K, items, t_max, b,
                          [&](const Job &j) { sc->begin(spawn_kind, (uint64_t)items * j.kn); spawn(j, blocks); sc->end(); },
                          [&](const Job &j) { sc->begin(accum_kind, items); accum(j); sc->end(); });
}

// A kernel's <true> / <false> pair under the launch kind the caller has opened: SPH as the render chooses it (light_sample_li<SPH>)
template <class K, class... A> void launch_sph(pt_scene *sc, const char *name_true, K k_true, const char *name_false, K k_false, dim3 blocks, const A &...args) {
    if (general_geometry(sc)) launch(sc, name_true, k_true, blocks, dim3(256), args...);
    else launch(sc, name_false, k_false, blocks, dim3(256), args...);
}

// The queries of a probe on the device: three index arrays in one allocation
struct Queries { const uint32_t *item, *sample, *element; };
int upload_queries(pt_scene *sc, uint32_t n, const uint32_t *item, const uint32_t *sample, const uint32_t *element, const char *what, DevTmp &tmp, Queries &q) {
    uint32_t *d = nullptr;
    SIDE_ALLOC(tmp, d, (size_t)n * 12, what);
    const uint32_t *from[3] = {item, sample, element};
    for (size_t k = 0; k < 3; ++k) HIP_TRY(hipMemcpyAsync(d + k * n, from[k], (size_t)n * 4, hipMemcpyHostToDevice, sc->stream));
    q = Queries{d, d + n, d + 2 * (size_t)n};
    return PT_OK;
}

// The rays of one pass: samples [s_begin, s_begin + s_count) of every texel (t_max = max_distance)
int bake_pass(pt_scene *sc, const Geometry &g, const PtBakeParams *bp, uint32_t s_begin, uint32_t s_count, const uint32_t *d_owner, float4 *d_ao, const AORayBuffers &b) {
    BakeJob job{};
    job.owner = d_owner; job.ao_w = d_ao;
    return pass_chunks(sc, g, job, bp->nsamples, bp->cos_sample, s_begin, s_count, g.atlas.slots * s_count, bp->max_distance, b,
                       "bake_rays", [&](const BakeJob &j, dim3 blocks) { launch(sc, "ptbake::k_bake_rays", k_bake_rays, blocks, dim3(256), sc->ds, g.rc, g_tabs, g.atlas, j); },
                       "bake_accum", [&](const BakeJob &j) { launch(sc, "ptbake::k_bake_accum", k_bake_accum, texel_grid(g.atlas), dim3(256), g.atlas, j); });
}

// ---- the transfer bake: `target` is the scene whose atlas is filled and is only read, `source` the scene the rays see -- every launch runs on its stream, under its
// statistics and counters
int check_transfer(const PtBakeTransferParams *tp) {
    if (int st = check_atlas(tp->width, tp->height)) return st;
    if (!(tp->front >= 0.0f && tp->back >= 0.0f && std::isfinite(tp->front) && std::isfinite(tp->back) && tp->front + tp->back > 0.0f))
        return fail(PT_ERR_INVALID_ARG, "bake transfer: front and back must be >= 0 and finite, front + back > 0");
    return PT_OK;
}
// The AO at the source hit as a bake's parameters. Without ao_w no sample number is drawn: spp and nsamples are not read (and not checked)
PtBakeParams ao_params(const PtBakeTransferParams *tp, bool want_ao) {
    PtBakeParams bp{};
    bp.width = tp->width; bp.height = tp->height; bp.spp = want_ao ? tp->spp : 1u; bp.nsamples = want_ao ? tp->nsamples : 1u; bp.cos_sample = tp->cos_sample;
    bp.max_distance = want_ao ? tp->max_distance : INFINITY; bp.sampler_type = want_ao ? tp->sampler_type : (uint32_t)PT_SAMPLER_SOBOL; bp.spp_per_pass = tp->spp_per_pass; bp.profile = tp->profile;
    return bp;
}
int same_device(pt_scene *target, pt_scene *source) {
    if (source->device != g_device) { if (int st = bind_device(source->device)) return st; }
    if (target->device != source->device) return fail(PT_ERR_INVALID_ARG, "bake transfer: the target scene lives on device " + std::to_string(target->device) + ", the source scene on device " + std::to_string(source->device));
    return PT_OK;
}

// Steps 1 to 4 of the contract over the whole atlas: the projection rays of the owned texels through the source scene, in slices of whole tiles sized by the pass budget
// (per slot the ray id, the ray record, the hit quad and t: a 2^28-texel atlas does not hold them all at once), and what each hit leaves in the planes
int project(pt_scene *target, pt_scene *source, const PtBakeTransferParams *tp, const BakeAtlas &a, const uint32_t *d_owner, const TransferOut &out) {
    DevTmp tmp;   // (the slices' records: freed before the AO passes allocate theirs)
    uint8_t *d_top = nullptr;
    SIDE_ALLOC(tmp, d_top, source->ds.n_prims, "bake transfer marks");
    HIP_TRY(hipMemsetAsync(d_top, 0, source->ds.n_prims, source->stream));
    source->begin("bake_select", source->ordered.size());
    launch_top(source, source, d_top);
    source->end();
    const uint32_t n_tiles = a.slots / 64u;
    const uint32_t tiles = choose_pass_size(source, 64u, n_tiles, 1, false, PassBudget{4 + 32 + 16 + 4, 0.5, kAOMaxRays});
    const uint32_t cap = tiles * 64u;
    float4 *d_ray = nullptr, *d_hit = nullptr; float *d_t = nullptr; uint32_t *d_base = nullptr, *d_count = nullptr;
    SIDE_ALLOC(tmp, d_ray, (size_t)cap * 32, "bake transfer rays"); SIDE_ALLOC(tmp, d_hit, (size_t)cap * 16, "bake transfer rays"); SIDE_ALLOC(tmp, d_t, (size_t)cap * 4, "bake transfer rays");
    SIDE_ALLOC(tmp, d_base, (size_t)cap * 4, "bake transfer rays"); SIDE_ALLOC(tmp, d_count, 4, "bake transfer rays");
    const float t_max = tp->front + tp->back;
    for (uint32_t slot0 = 0; slot0 < a.slots; slot0 += cap) {
        const uint32_t n_slots = std::min(cap, a.slots - slot0);
        HIP_TRY(hipMemsetAsync(d_count, 0, 4, source->stream));
        HIP_TRY(hipMemsetAsync(source->qc->head, 0, sizeof source->qc->head, source->stream));
        source->begin("bake_project", n_slots);
        launch(source, "ptbake::k_bake_project", k_bake_project, blocks_for(n_slots, 16u), dim3(256), target->ds, a, d_owner, slot0, n_slots, tp->front, t_max, d_ray, d_base, d_count);
        source->end();
        HIP_TRY(hipGetLastError());
        TraceJob tj = trace_job(source, 0);   // ray ids, no queue
        tj.sub[0] = trace_sub(nullptr, d_count, (const float *)d_ray, 8, t_max, 0);
        tj.sub[0].per_ray_tmax = 1; tj.sub[0].out_hit = d_hit; tj.sub[0].out_hit_stride = 1; tj.sub[0].out_t = d_t; tj.sub[0].out_t_stride = 1;
        if (int st = traced(source, "extend", 0, tj, n_slots)) return st;   // (an upper bound: the launch reads the count of rays spawned)
        source->begin("bake_transfer_points", n_slots);
        launch(source, "ptbake::k_bake_transfer_points", k_bake_transfer_points, dim3((n_slots + 255) / 256), dim3(256), target->ds, source->ds, a, d_owner, (const uint8_t *)d_top, slot0, n_slots,
               (const uint32_t *)d_base, (const float4 *)d_hit, (const float *)d_t, tp->front, out);
        source->end();
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(source->stream));   // (the records are freed on return)
    return PT_OK;
}

// The AO rays of one pass from the detail hits (bake_pass with the source hits in the owners' place)
int transfer_pass(pt_scene *sc, const Geometry &g, const PtBakeParams *bp, uint32_t s_begin, uint32_t s_count, const uint32_t *d_detail, const float4 *d_rec, float4 *d_ao, const AORayBuffers &b) {
    TransferJob job{};
    job.owner = d_detail; job.ao_w = d_ao; job.rec = d_rec;
    return pass_chunks(sc, g, job, bp->nsamples, bp->cos_sample, s_begin, s_count, g.atlas.slots * s_count, bp->max_distance, b,
                       "bake_transfer_rays", [&](const TransferJob &j, dim3 blocks) { launch(sc, "ptbake::k_bake_transfer_rays", k_bake_transfer_rays, blocks, dim3(256), sc->ds, g.rc, g_tabs, g.atlas, j); },
                       "bake_accum", [&](const TransferJob &j) { launch(sc, "ptbake::k_bake_accum", k_bake_accum, texel_grid(g.atlas), dim3(256), g.atlas, static_cast<const BakeJob &>(j)); });
}

// ---- the lightmap (mi355bake.h "Lightmap")
constexpr float kShadowTMax = 1.0f - 0.0001f;     // the render's shadow ray (render_loop.hip: the scalar t_max of its "shadow" launches)
constexpr size_t kLightBytesPerRay = 16 + 4;      // besides ao_ray_budget's: the E record and the id table's entry

// A lightmap job as a bake's parameters: the sampler, the atlas and the checks on them are the AO bake's (cos_sample and max_distance are not read)
PtBakeParams light_params(const PtBakeLightParams *lp) {
    PtBakeParams bp{};
    bp.width = lp->width; bp.height = lp->height; bp.spp = lp->spp; bp.nsamples = lp->nsamples; bp.cos_sample = 0; bp.max_distance = INFINITY;
    bp.sampler_type = lp->sampler_type; bp.spp_per_pass = lp->spp_per_pass; bp.profile = lp->profile;
    return bp;
}
// The selected lights in ascending order (light_select NULL: all n_lights), and the rule that gives every light the same number of samples
int check_lights(uint32_t spp, uint32_t nsamples, const uint8_t *light_select, uint32_t n_lights, std::vector<uint32_t> &sel, const char *per = "texel") {
    sel.clear();
    for (uint32_t i = 0; i < n_lights; ++i) if (!light_select || light_select[i]) sel.push_back(i);
    if (sel.empty()) return fail(PT_ERR_INVALID_ARG, "bake light: no light is selected");
    const uint64_t numbers = (uint64_t)spp * nsamples;
    if (numbers % sel.size() != 0)
        return fail(PT_ERR_INVALID_ARG, "bake light: spp x nsamples = " + std::to_string(numbers) + " light samples per " + per + " are no multiple of the " + std::to_string(sel.size()) + " selected lights");
    return PT_OK;
}
int check_light_count(const pt_scene *sc, uint32_t n_lights) {
    if (n_lights != sc->n_lights) return fail(PT_ERR_INVALID_ARG, "bake light: light_select has " + std::to_string(n_lights) + " entries, the scene " + std::to_string(sc->n_lights) + " lights");
    return PT_OK;
}
// The light-sample fields of a lightmap or SH job: the selection on the device (`sel` outlives the call's last synchronisation), the rule's scale and, for `rays`
// rays in flight at the most (a probe: none), the id table and the E records
int light_samples(pt_scene *sc, const std::vector<uint32_t> &sel, uint32_t nsamples, size_t rays, const char *what, DevTmp &tmp, LightSamples &ls) {
    uint32_t *d_sel = nullptr;
    SIDE_ALLOC(tmp, d_sel, sel.size() * 4, "bake light selection");
    HIP_TRY(hipMemcpyAsync(d_sel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, sc->stream));
    ls = LightSamples{};
    ls.sel = d_sel; ls.n_sel = (uint32_t)sel.size(); ls.scale = (float)ls.n_sel / (float)nsamples;
    if (rays) { SIDE_ALLOC(tmp, ls.id, rays * 4, what); SIDE_ALLOC(tmp, ls.e, rays * 16, what); }
    return PT_OK;
}

// The light samples of one pass: samples [s_begin, s_begin + s_count) of every texel (the shadow ray's t_max)
int light_pass(pt_scene *sc, const Geometry &g, uint32_t nsamples, uint32_t s_begin, uint32_t s_count, const uint32_t *d_owner, float4 *d_light, const LightSamples &ls, const AORayBuffers &b) {
    LightJob job{};
    job.owner = d_owner; job.light_w = d_light; job.light = ls;
    return pass_chunks(sc, g, job, nsamples, 0, s_begin, s_count, g.atlas.slots * s_count, kShadowTMax, b,
                       "bake_light_rays", [&](const LightJob &j, dim3 blocks) {
                           launch_sph(sc, "ptbake::k_bake_light_rays<true>", k_bake_light_rays<true>, "ptbake::k_bake_light_rays<false>", k_bake_light_rays<false>, blocks, sc->ds, g.rc, g_tabs, g.atlas, j);
                       },
                       "bake_light_accum", [&](const LightJob &j) { launch(sc, "ptbake::k_bake_light_accum", k_bake_light_accum, texel_grid(g.atlas), dim3(256), g.atlas, j); });
}

// What a light probe leaves per query on the device (store_light_row), and its way into the caller's arrays
struct LightRows {
    float *d_out = nullptr; uint32_t *d_light = nullptr; uint8_t *d_found = nullptr;
    int alloc(DevTmp &tmp, uint32_t n, const char *what) {
        SIDE_ALLOC(tmp, d_out, (size_t)n * 64, what); SIDE_ALLOC(tmp, d_light, (size_t)n * 4, what); SIDE_ALLOC(tmp, d_found, n, what);
        return PT_OK;
    }
    int read(uint32_t n, uint32_t *out_light, float *out_wi, float *out_pdf, float *out_li, float *out_e, float *out_o, float *out_d, uint8_t *found) const {
        std::vector<float> rows((size_t)n * 16);
        HIP_TRY(hipMemcpy(rows.data(), d_out, rows.size() * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out_light, d_light, (size_t)n * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(found, d_found, n, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            const float *r = rows.data() + 16 * i;
            for (int k = 0; k < 3; ++k) { out_wi[3 * i + k] = r[k]; out_li[3 * i + k] = r[4 + k]; out_e[3 * i + k] = r[7 + k]; out_o[3 * i + k] = r[10 + k]; out_d[3 * i + k] = r[13 + k]; }
            out_pdf[i] = r[3];
        }
        return PT_OK;
    }
};

// What the light and SH resolves share: per item `width` sums, the last of them the count of arrived samples -- the others / spp, the count / (spp * nsamples), zeros
// where nothing arrived and nothing was added
int resolve_light_sums(const float *sums, size_t n, size_t width, uint32_t spp, uint32_t nsamples, float *mean, float *reached) {
    if (!sums || (!mean && !reached)) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_spp(spp)) return st;
    if (int st = check_nsamples(nsamples)) return st;
    const float sf = (float)spp, nf = (float)spp * (float)nsamples;
    for (size_t i = 0; i < n; ++i) {
        const float *w = sums + width * i;
        bool any = false;
        for (size_t m = 0; m < width; ++m) any = any || w[m] != 0.0f;
        if (mean) for (size_t m = 0; m + 1 < width; ++m) mean[(width - 1) * i + m] = any ? w[m] / sf : 0.0f;
        if (reached) reached[i] = any ? w[width - 1] / nf : 0.0f;
    }
    return PT_OK;
}

// ---- the SH points (mi355bake.h "SH points")
constexpr uint32_t kShMaxPoints = 1u << 28;
constexpr size_t kShBytesPerRay = 16 + 16 + 4;    // besides ao_ray_budget's: the E record, wi and the id table's entry

uint32_t sh_rows(const PtBakeShParams *hp) { return (hp->n_points + hp->row - 1) / hp->row; }
uint32_t sh_padded(const PtBakeShParams *hp) { return (hp->n_points + 63u) / 64u * 64u; }
// An SH job as a bake's parameters: the sampler is that of a row x rows image (cos_sample and max_distance are not read)
PtBakeParams sh_params(const PtBakeShParams *hp) {
    PtBakeParams bp{};
    bp.width = hp->row; bp.height = sh_rows(hp); bp.spp = hp->spp; bp.nsamples = hp->nsamples; bp.cos_sample = 0; bp.max_distance = INFINITY;
    bp.sampler_type = hp->sampler_type; bp.spp_per_pass = hp->spp_per_pass; bp.profile = hp->profile;
    return bp;
}
// Errors 2 to 5 of the header's list
int check_sh(const PtBakeShParams *hp) {
    if (hp->n_points == 0) return fail(PT_ERR_INVALID_ARG, "bake sh: n_points must be > 0");
    if (hp->n_points > kShMaxPoints) return fail(PT_ERR_INVALID_ARG, "bake sh: more than 2^28 points");
    if (hp->row == 0) return fail(PT_ERR_INVALID_ARG, "bake sh: row must be > 0");
    if (hp->row > kShMaxPoints) return fail(PT_ERR_INVALID_ARG, "bake sh: row exceeds 2^28");
    if (int st = check_spp(hp->spp)) return st;
    if (int st = check_nsamples(hp->nsamples)) return st;
    return check_sampler(hp->sampler_type);
}
// Errors 7 to 9
int check_sh_points_and_lights(const PtBakeShParams *hp, const float *points, const uint8_t *light_select, uint32_t n_lights, std::vector<uint32_t> &sel) {
    for (size_t i = 0; i < (size_t)hp->n_points * 3; ++i)
        if (!std::isfinite(points[i])) return fail(PT_ERR_INVALID_ARG, "bake sh: point " + std::to_string(i / 3) + " has a coordinate that is not finite");
    return check_lights(hp->spp, hp->nsamples, light_select, n_lights, sel, "point");
}
int sh_geometry(pt_scene *sc, const PtBakeShParams *hp, uint32_t n_samples, Geometry &g) {
    const PtBakeParams bp = sh_params(hp);
    return bake_geometry(sc, &bp, n_samples, g, kShBytesPerRay, sh_padded(hp));
}
int upload_points(pt_scene *sc, const PtBakeShParams *hp, const float *points, DevTmp &tmp, float *&d_points) {
    SIDE_ALLOC(tmp, d_points, (size_t)hp->n_points * 12, "bake sh points");
    HIP_TRY(hipMemcpyAsync(d_points, points, (size_t)hp->n_points * 12, hipMemcpyHostToDevice, sc->stream));   // (the caller's array outlives the call's last synchronisation)
    return PT_OK;
}

// The light samples of one pass: samples [s_begin, s_begin + s_count) of every point (light_pass without atlas)
int sh_pass(pt_scene *sc, const Geometry &g, const PtBakeShParams *hp, uint32_t s_begin, uint32_t s_count, const float *d_points, float4 *d_sh, const LightSamples &ls, float4 *d_wi,
            const AORayBuffers &b) {
    ShJob job{};
    job.n_points = hp->n_points; job.padded = sh_padded(hp); job.row = hp->row; job.points = d_points; job.sh_w = d_sh; job.light = ls; job.wi = d_wi;
    return pass_chunks(sc, g, job, hp->nsamples, 0, s_begin, s_count, job.padded * s_count, kShadowTMax, b,
                       "bake_sh_rays", [&](const ShJob &j, dim3 blocks) {
                           launch_sph(sc, "ptbake::k_bake_sh_rays<true>", k_bake_sh_rays<true>, "ptbake::k_bake_sh_rays<false>", k_bake_sh_rays<false>, blocks, sc->ds, g.rc, g_tabs, j);
                       },
                       "bake_sh_accum", [&](const ShJob &j) { launch(sc, "ptbake::k_bake_sh_accum", k_bake_sh_accum, dim3((hp->n_points + 255) / 256), dim3(256), j); });
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int pt_bake_pass_size(pt_scene *sc, const PtBakeParams *bp, uint32_t *spp_per_pass) {
    if (!sc || !bp || !spp_per_pass) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_params(bp)) return st;
    Geometry g;
    if (int st = bake_geometry(sc, bp, bp->spp, g)) return st;
    *spp_per_pass = g.S;
    return PT_OK;
}

__attribute__((visibility("default"))) int pt_bake_render(pt_scene *sc, const PtBakeParams *bp, const uint8_t *prim_select, uint32_t n_prims, const PtBakeBuffers *buffers, int buffers_are_device) {
    if (!sc || !bp || !prim_select || !buffers) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_params(bp)) return st;
    return pt_bake_render_samples(sc, bp, prim_select, n_prims, 0, bp->spp, buffers, buffers_are_device);
}

__attribute__((visibility("default"))) int pt_bake_render_samples(pt_scene *sc, const PtBakeParams *bp, const uint8_t *prim_select, uint32_t n_prims, uint32_t first, uint32_t n_samples,
                                                                  const PtBakeBuffers *buffers, int buffers_are_device) {
    if (!sc || !bp || !prim_select || !buffers) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_params(bp)) return st;
    if (!buffers->owner && !buffers->position && !buffers->normal && !buffers->ao_w) return fail(PT_ERR_INVALID_ARG, "bake: all four planes are NULL");
    if (int st = check_range(bp, first, n_samples)) return st;
    if (int st = check_selection(prim_select, n_prims)) return st;
    if (int st = check_prim_count(sc, n_prims)) return st;   // (all of the above before the device is touched)
    Geometry g;
    if (int st = bake_geometry(sc, bp, n_samples, g)) return st;
    if (int st = begin_call(sc, bp->profile != 0)) return st;
    DevTmp tmp;
    Staging out{tmp, sc->stream, buffers_are_device != 0};
    uint32_t *d_owner = nullptr; float4 *d_ao = nullptr;
    if (int st = atlas_frame(sc, sc, g.atlas, prim_select, n_prims, out, buffers->owner, buffers->position, buffers->normal, d_owner)) return st;
    if (int st = out.plane(buffers->ao_w, (size_t)g.atlas.n_texels * 16, "bake ao plane", true, d_ao)) return st;
    if (d_ao) {
        AORayBuffers b; size_t rays;
        if (int st = alloc_pass_rays(g, g.atlas.slots, "bake rays", b, rays)) return st;
        if (int st = for_passes(g, first, n_samples, [&](uint32_t s0, uint32_t sn) { return bake_pass(sc, g, bp, s0, sn, d_owner, d_ao, b); })) return st;
    }
    return out.finish(sc);
}

__attribute__((visibility("default"))) int pt_bake_resolve(const float *ao_w, uint32_t n_texels, uint32_t spp, float *ao, float *bent_xyz) {
    if (!ao_w || (!ao && !bent_xyz)) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_spp(spp)) return st;
    // (sum w / spp is ao.rs's radiance of the texel: pi where nothing occludes under cosine sampling. The map is that over pi: 1 for an open surface)
    const float sf = (float)spp * ptd::kPi;
    for (size_t i = 0; i < n_texels; ++i) {
        const float x = ao_w[4 * i], y = ao_w[4 * i + 1], z = ao_w[4 * i + 2], w = ao_w[4 * i + 3];
        const bool any = x != 0.0f || y != 0.0f || z != 0.0f || w != 0.0f;
        if (ao) ao[i] = any ? w / sf : 0.0f;
        if (bent_xyz) {
            const float len = std::sqrt(x * x + y * y + z * z);
            const bool ok = any && len > 0.0f;
            const float inv = ok ? 1.0f / len : 0.0f;
            bent_xyz[3 * i] = ok ? x * inv : 0.0f; bent_xyz[3 * i + 1] = ok ? y * inv : 0.0f; bent_xyz[3 * i + 2] = ok ? z * inv : 0.0f;
        }
    }
    return PT_OK;
}

__attribute__((visibility("default"))) int pt_bake_dilate(pt_scene *sc, const uint32_t *owner, float *plane, uint32_t channels, uint32_t width, uint32_t height, uint32_t iterations, int buffers_are_device) {
    if (!sc || !owner || !plane) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_atlas(width, height)) return st;
    if (channels < 1 || channels > 4) return fail(PT_ERR_INVALID_ARG, "bake: a plane has 1 .. 4 channels");
    if (iterations == 0) return PT_OK;   // (all of the above before the device is touched)
    if (sc->device != g_device) { if (int st = bind_device(sc->device)) return st; }
    if (int st = ensure_workspace(sc, 0, 0)) return st;   // (the scene's stream; no paths, no film)
    sc->drop_timings();
    const BakeAtlas a = make_atlas(width, height);
    const size_t n = a.n_texels, bytes = n * channels * 4;
    DevTmp tmp;
    const bool dev = buffers_are_device != 0;
    const uint32_t *d_owner = owner;
    float *buf[2] = {plane, nullptr};
    uint8_t *cov[2] = {nullptr, nullptr};
    if (!dev) {
        uint32_t *up = nullptr;
        SIDE_ALLOC(tmp, up, n * 4, "bake dilation"); SIDE_ALLOC(tmp, buf[0], bytes, "bake dilation");
        HIP_TRY(hipMemcpyAsync(up, owner, n * 4, hipMemcpyHostToDevice, sc->stream));
        HIP_TRY(hipMemcpyAsync(buf[0], plane, bytes, hipMemcpyHostToDevice, sc->stream));
        d_owner = up;
    }
    SIDE_ALLOC(tmp, buf[1], bytes, "bake dilation"); SIDE_ALLOC(tmp, cov[0], n, "bake dilation"); SIDE_ALLOC(tmp, cov[1], n, "bake dilation");
    sc->begin("bake_dilate", n);
    launch(sc, "ptbake::k_bake_covered", k_bake_covered, texel_grid(a), dim3(256), a, d_owner, cov[0]);
    sc->end();
    int cur = 0;
    for (uint32_t it = 0; it < iterations; ++it, cur ^= 1) {
        sc->begin("bake_dilate", n);
        const float *src = buf[cur]; const uint8_t *cs = cov[cur];
        switch (channels) {
        case 1: launch(sc, "ptbake::k_bake_dilate<1>", k_bake_dilate<1>, texel_grid(a), dim3(256), a, src, cs, buf[cur ^ 1], cov[cur ^ 1]); break;
        case 2: launch(sc, "ptbake::k_bake_dilate<2>", k_bake_dilate<2>, texel_grid(a), dim3(256), a, src, cs, buf[cur ^ 1], cov[cur ^ 1]); break;
        case 3: launch(sc, "ptbake::k_bake_dilate<3>", k_bake_dilate<3>, texel_grid(a), dim3(256), a, src, cs, buf[cur ^ 1], cov[cur ^ 1]); break;
        default: launch(sc, "ptbake::k_bake_dilate<4>", k_bake_dilate<4>, texel_grid(a), dim3(256), a, src, cs, buf[cur ^ 1], cov[cur ^ 1]); break;
        }
        sc->end();
    }
    HIP_TRY(hipGetLastError());
    if (dev) { if (buf[cur] != plane) HIP_TRY(hipMemcpyAsync(plane, buf[cur], bytes, hipMemcpyDeviceToDevice, sc->stream)); }
    else HIP_TRY(hipMemcpyAsync(plane, buf[cur], bytes, hipMemcpyDeviceToHost, sc->stream));
    HIP_TRY(hipStreamSynchronize(sc->stream));
    sc->resolve_timings();
    return PT_OK;
}

__attribute__((visibility("default"))) int pt_bake_rays(pt_scene *sc, const PtBakeParams *bp, const uint8_t *prim_select, uint32_t n_prims, uint32_t n, const uint32_t *texel, const uint32_t *sample,
                                                        const uint32_t *element, float *out_o, float *out_d, float *out_w, uint8_t *found) {
    if (!sc || !bp || !prim_select || !texel || !sample || !element || !out_o || !out_d || !out_w || !found) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_params(bp)) return st;
    if (int st = check_selection(prim_select, n_prims)) return st;
    if (int st = check_queries(n, sample, element, bp->spp, bp->nsamples)) return st;
    if (int st = check_prim_count(sc, n_prims)) return st;
    Geometry g;
    PtBakeParams one = *bp; one.spp_per_pass = 1;
    if (int st = bake_geometry(sc, &one, bp->spp, g)) return st;
    if (n == 0) return PT_OK;
    if (int st = begin_call(sc, false)) return st;
    DevTmp tmp;
    Staging none{tmp, sc->stream, false};
    uint32_t *d_owner = nullptr; float *d_out = nullptr; uint8_t *d_found = nullptr; Queries q;
    if (int st = atlas_frame(sc, sc, g.atlas, prim_select, n_prims, none, nullptr, nullptr, nullptr, d_owner)) return st;
    if (int st = upload_queries(sc, n, texel, sample, element, "bake rays", tmp, q)) return st;
    SIDE_ALLOC(tmp, d_out, (size_t)n * 28, "bake rays"); SIDE_ALLOC(tmp, d_found, n, "bake rays");
    sc->begin("bake_probe", n);
    launch(sc, "ptbake::k_bake_probe", k_bake_probe, dim3((n + 255) / 256), dim3(256), sc->ds, g.rc, g_tabs, g.atlas, d_owner, bp->nsamples, bp->cos_sample ? 1u : 0u, n, q.item, q.sample, q.element,
           d_out, d_out + 3 * (size_t)n, d_out + 6 * (size_t)n, d_found);
    sc->end();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(sc->stream));
    sc->resolve_timings();
    HIP_TRY(hipMemcpy(out_o, d_out, (size_t)n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_d, d_out + 3 * (size_t)n, (size_t)n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_w, d_out + 6 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(found, d_found, n, hipMemcpyDeviceToHost));
    return PT_OK;
}

__attribute__((visibility("default"))) int pt_bake_transfer_pass_size(pt_scene *target, pt_scene *source, const PtBakeTransferParams *tp, uint32_t *spp_per_pass) {
    if (!target || !source || !tp || !spp_per_pass) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_transfer(tp)) return st;
    const PtBakeParams bp = ao_params(tp, true);
    if (int st = check_params(&bp)) return st;
    if (int st = same_device(target, source)) return st;
    Geometry g;
    if (int st = bake_geometry(source, &bp, bp.spp, g)) return st;
    *spp_per_pass = g.S;
    return PT_OK;
}

__attribute__((visibility("default"))) int pt_bake_transfer(pt_scene *target, pt_scene *source, const PtBakeTransferParams *tp, const uint8_t *prim_select, uint32_t n_prims,
                                                            const PtBakeTransferBuffers *buffers, int buffers_are_device) {
    if (!target || !source || !tp || !prim_select || !buffers) return fail(PT_ERR_INVALID_ARG, "null argument");
    return pt_bake_transfer_samples(target, source, tp, prim_select, n_prims, 0, tp->spp, buffers, buffers_are_device);
}

__attribute__((visibility("default"))) int pt_bake_transfer_samples(pt_scene *target, pt_scene *source, const PtBakeTransferParams *tp, const uint8_t *prim_select, uint32_t n_prims, uint32_t first,
                                                                    uint32_t n_samples, const PtBakeTransferBuffers *buffers, int buffers_are_device) {
    if (!target || !source || !tp || !prim_select || !buffers) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_transfer(tp)) return st;
    const PtBakeTransferBuffers &B = *buffers;
    if (!B.owner && !B.hit_prim && !B.height && !B.src_position && !B.src_normal && !B.tangent_normal && !B.ao_w) return fail(PT_ERR_INVALID_ARG, "bake transfer: all seven planes are NULL");
    const bool want_ao = B.ao_w != nullptr;
    const PtBakeParams bp = ao_params(tp, want_ao);
    if (want_ao) {   // (without ao_w the sample range is not read either)
        if (int st = check_params(&bp)) return st;
        if (int st = check_range(&bp, first, n_samples)) return st;
    } else { first = 0; n_samples = 1; }
    if (int st = check_selection(prim_select, n_prims)) return st;
    if (int st = check_prim_count(target, n_prims)) return st;   // (all of the above before the device is touched)
    if (int st = same_device(target, source)) return st;
    Geometry g;
    if (int st = bake_geometry(source, &bp, n_samples, g)) return st;
    if (int st = begin_call(source, tp->profile != 0)) return st;   // (counters and statistics of a transfer are the source's)
    const BakeAtlas &a = g.atlas;
    const size_t n = a.n_texels;
    DevTmp tmp;
    Staging planes{tmp, source->stream, buffers_are_device != 0};
    uint32_t *d_owner = nullptr; float4 *d_ao = nullptr;
    if (int st = atlas_frame(source, target, a, prim_select, n_prims, planes, B.owner, nullptr, nullptr, d_owner)) return st;
    TransferOut out{};
    if (int st = planes.plane(B.hit_prim, n * 4, "bake transfer planes", false, out.hit_prim)) return st;
    if (int st = planes.plane(B.height, n * 4, "bake transfer planes", false, out.height)) return st;
    if (int st = planes.plane(B.src_position, n * 12, "bake transfer planes", false, out.src_position)) return st;
    if (int st = planes.plane(B.src_normal, n * 12, "bake transfer planes", false, out.src_normal)) return st;
    if (int st = planes.plane(B.tangent_normal, n * 12, "bake transfer planes", false, out.tangent_normal)) return st;
    if (want_ao) { SIDE_ALLOC(tmp, out.detail, n * 4, "bake transfer hits"); SIDE_ALLOC(tmp, out.rec, n * 16, "bake transfer hits"); }
    if (out.hit_prim || out.height || out.src_position || out.src_normal || out.tangent_normal || want_ao)
        if (int st = project(target, source, tp, a, d_owner, out)) return st;
    if (int st = planes.plane(B.ao_w, n * 16, "bake ao plane", true, d_ao)) return st;
    if (want_ao) {
        AORayBuffers b; size_t rays;
        if (int st = alloc_pass_rays(g, a.slots, "bake rays", b, rays)) return st;
        if (int st = for_passes(g, first, n_samples, [&](uint32_t s0, uint32_t sn) { return transfer_pass(source, g, &bp, s0, sn, out.detail, out.rec, d_ao, b); })) return st;
    }
    return planes.finish(source);
}

__attribute__((visibility("default"))) int pt_bake_transfer_rays(pt_scene *target, pt_scene *source, const PtBakeTransferParams *tp, const uint8_t *prim_select, uint32_t n_prims, uint32_t n,
                                                                 const uint32_t *texel, const uint32_t *sample, const uint32_t *element, float *proj_o, float *proj_d, float *proj_tmax, float *ao_o,
                                                                 float *ao_d, float *ao_w, uint8_t *found) {
    if (!target || !source || !tp || !prim_select || !texel || !sample || !element || !proj_o || !proj_d || !proj_tmax || !ao_o || !ao_d || !ao_w || !found) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_transfer(tp)) return st;
    PtBakeParams bp = ao_params(tp, true);
    if (int st = check_params(&bp)) return st;
    if (int st = check_selection(prim_select, n_prims)) return st;
    if (int st = check_queries(n, sample, element, bp.spp, bp.nsamples)) return st;
    if (int st = check_prim_count(target, n_prims)) return st;
    if (int st = same_device(target, source)) return st;
    Geometry g;
    bp.spp_per_pass = 1;
    if (int st = bake_geometry(source, &bp, bp.spp, g)) return st;
    if (n == 0) return PT_OK;
    if (int st = begin_call(source, false)) return st;
    const BakeAtlas &a = g.atlas;
    DevTmp tmp;
    Staging none{tmp, source->stream, false};
    uint32_t *d_owner = nullptr; float *d_out = nullptr; uint8_t *d_found = nullptr; Queries q;
    if (int st = atlas_frame(source, target, a, prim_select, n_prims, none, nullptr, nullptr, nullptr, d_owner)) return st;
    TransferOut out{};
    SIDE_ALLOC(tmp, out.detail, (size_t)a.n_texels * 4, "bake transfer hits"); SIDE_ALLOC(tmp, out.rec, (size_t)a.n_texels * 16, "bake transfer hits");
    if (int st = project(target, source, tp, a, d_owner, out)) return st;
    if (int st = upload_queries(source, n, texel, sample, element, "bake rays", tmp, q)) return st;
    SIDE_ALLOC(tmp, d_out, (size_t)n * 56, "bake rays"); SIDE_ALLOC(tmp, d_found, n, "bake rays");
    source->begin("bake_probe", n);
    launch(source, "ptbake::k_bake_transfer_probe", k_bake_transfer_probe, dim3((n + 255) / 256), dim3(256), target->ds, source->ds, g.rc, g_tabs, a, d_owner, out.detail, out.rec, tp->front,
           tp->front + tp->back, bp.nsamples, bp.cos_sample ? 1u : 0u, n, q.item, q.sample, q.element, d_out, d_found);
    source->end();
    HIP_TRY(hipGetLastError());
    if (int st = end_call(source)) return st;
    std::vector<float> rows((size_t)n * 14);
    HIP_TRY(hipMemcpy(rows.data(), d_out, rows.size() * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(found, d_found, n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) {
        const float *r = rows.data() + 14 * i;
        for (int k = 0; k < 3; ++k) { proj_o[3 * i + k] = r[k]; proj_d[3 * i + k] = r[3 + k]; ao_o[3 * i + k] = r[7 + k]; ao_d[3 * i + k] = r[10 + k]; }
        proj_tmax[i] = r[6]; ao_w[i] = r[13];
    }
    return PT_OK;
}

// ---- the lightmap
__attribute__((visibility("default"))) int pt_bake_light_pass_size(pt_scene *sc, const PtBakeLightParams *lp, const uint8_t *light_select, uint32_t n_lights, uint32_t *spp_per_pass) {
    if (!sc || !lp || !spp_per_pass) return fail(PT_ERR_INVALID_ARG, "null argument");
    const PtBakeParams bp = light_params(lp);
    if (int st = check_params(&bp)) return st;
    std::vector<uint32_t> sel;
    if (int st = check_lights(lp->spp, lp->nsamples, light_select, n_lights, sel)) return st;
    if (int st = check_light_count(sc, n_lights)) return st;
    Geometry g;
    if (int st = bake_geometry(sc, &bp, bp.spp, g, kLightBytesPerRay)) return st;
    *spp_per_pass = g.S;
    return PT_OK;
}

__attribute__((visibility("default"))) int pt_bake_light(pt_scene *sc, const PtBakeLightParams *lp, const uint8_t *prim_select, uint32_t n_prims, const uint8_t *light_select, uint32_t n_lights,
                                                         const PtBakeLightBuffers *buffers, int buffers_are_device) {
    if (!sc || !lp || !prim_select || !buffers) return fail(PT_ERR_INVALID_ARG, "null argument");
    return pt_bake_light_samples(sc, lp, prim_select, n_prims, light_select, n_lights, 0, lp->spp, buffers, buffers_are_device);
}

__attribute__((visibility("default"))) int pt_bake_light_samples(pt_scene *sc, const PtBakeLightParams *lp, const uint8_t *prim_select, uint32_t n_prims, const uint8_t *light_select, uint32_t n_lights,
                                                                 uint32_t first, uint32_t n_samples, const PtBakeLightBuffers *buffers, int buffers_are_device) {
    if (!sc || !lp || !prim_select || !buffers) return fail(PT_ERR_INVALID_ARG, "null argument");
    const PtBakeParams bp = light_params(lp);
    if (int st = check_params(&bp)) return st;
    if (!buffers->owner && !buffers->position && !buffers->normal && !buffers->light_w) return fail(PT_ERR_INVALID_ARG, "bake: all four planes are NULL");
    if (int st = check_range(&bp, first, n_samples)) return st;
    if (int st = check_selection(prim_select, n_prims)) return st;
    std::vector<uint32_t> sel;
    if (int st = check_lights(lp->spp, lp->nsamples, light_select, n_lights, sel)) return st;
    if (int st = check_prim_count(sc, n_prims)) return st;
    if (int st = check_light_count(sc, n_lights)) return st;   // (all of the above before the device is touched)
    Geometry g;
    if (int st = bake_geometry(sc, &bp, n_samples, g, kLightBytesPerRay)) return st;
    if (int st = begin_call(sc, bp.profile != 0)) return st;
    DevTmp tmp;
    Staging out{tmp, sc->stream, buffers_are_device != 0};
    uint32_t *d_owner = nullptr; float4 *d_light = nullptr;
    if (int st = atlas_frame(sc, sc, g.atlas, prim_select, n_prims, out, buffers->owner, buffers->position, buffers->normal, d_owner)) return st;
    if (int st = out.plane(buffers->light_w, (size_t)g.atlas.n_texels * 16, "bake light plane", true, d_light)) return st;
    if (d_light) {
        AORayBuffers b; size_t rays; LightSamples ls;
        if (int st = alloc_pass_rays(g, g.atlas.slots, "bake light rays", b, rays)) return st;
        if (int st = light_samples(sc, sel, bp.nsamples, rays, "bake light rays", tmp, ls)) return st;
        if (int st = for_passes(g, first, n_samples, [&](uint32_t s0, uint32_t sn) { return light_pass(sc, g, bp.nsamples, s0, sn, d_owner, d_light, ls, b); })) return st;
    }
    return out.finish(sc);
}

__attribute__((visibility("default"))) int pt_bake_light_resolve(const float *light_w, uint32_t n_texels, uint32_t spp, uint32_t nsamples, float *irradiance_rgb, float *reached) {
    return resolve_light_sums(light_w, n_texels, 4, spp, nsamples, irradiance_rgb, reached);
}

__attribute__((visibility("default"))) int pt_bake_light_rays(pt_scene *sc, const PtBakeLightParams *lp, const uint8_t *prim_select, uint32_t n_prims, const uint8_t *light_select, uint32_t n_lights,
                                                              uint32_t n, const uint32_t *texel, const uint32_t *sample, const uint32_t *element, uint32_t *out_light, float *out_wi, float *out_pdf,
                                                              float *out_li, float *out_e, float *out_o, float *out_d, uint8_t *found) {
    if (!sc || !lp || !prim_select || !texel || !sample || !element || !out_light || !out_wi || !out_pdf || !out_li || !out_e || !out_o || !out_d || !found) return fail(PT_ERR_INVALID_ARG, "null argument");
    PtBakeParams bp = light_params(lp);
    if (int st = check_params(&bp)) return st;
    if (int st = check_selection(prim_select, n_prims)) return st;
    std::vector<uint32_t> sel;
    if (int st = check_lights(lp->spp, lp->nsamples, light_select, n_lights, sel)) return st;
    if (int st = check_queries(n, sample, element, bp.spp, bp.nsamples)) return st;
    if (int st = check_prim_count(sc, n_prims)) return st;
    if (int st = check_light_count(sc, n_lights)) return st;
    Geometry g;
    bp.spp_per_pass = 1;
    if (int st = bake_geometry(sc, &bp, bp.spp, g, kLightBytesPerRay)) return st;
    if (n == 0) return PT_OK;
    if (int st = begin_call(sc, false)) return st;
    DevTmp tmp;
    Staging none{tmp, sc->stream, false};
    uint32_t *d_owner = nullptr; LightSamples ls; Queries q; LightRows rows;
    if (int st = atlas_frame(sc, sc, g.atlas, prim_select, n_prims, none, nullptr, nullptr, nullptr, d_owner)) return st;
    if (int st = light_samples(sc, sel, bp.nsamples, 0, "bake light rays", tmp, ls)) return st;
    if (int st = upload_queries(sc, n, texel, sample, element, "bake light rays", tmp, q)) return st;
    if (int st = rows.alloc(tmp, n, "bake light rays")) return st;
    sc->begin("bake_probe", n);
    launch_sph(sc, "ptbake::k_bake_light_probe<true>", k_bake_light_probe<true>, "ptbake::k_bake_light_probe<false>", k_bake_light_probe<false>, dim3((n + 255) / 256), sc->ds, g.rc, g_tabs, g.atlas,
               d_owner, bp.nsamples, ls.sel, ls.n_sel, ls.scale, n, q.item, q.sample, q.element, rows.d_light, rows.d_out, rows.d_found);
    sc->end();
    HIP_TRY(hipGetLastError());
    if (int st = end_call(sc)) return st;
    return rows.read(n, out_light, out_wi, out_pdf, out_li, out_e, out_o, out_d, found);
}

// ---- the SH points
__attribute__((visibility("default"))) int pt_bake_sh_pass_size(pt_scene *sc, const PtBakeShParams *hp, const uint8_t *light_select, uint32_t n_lights, uint32_t *spp_per_pass) {
    if (!sc || !hp || !spp_per_pass) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_sh(hp)) return st;
    std::vector<uint32_t> sel;
    if (int st = check_lights(hp->spp, hp->nsamples, light_select, n_lights, sel, "point")) return st;
    if (int st = check_light_count(sc, n_lights)) return st;
    Geometry g;
    if (int st = sh_geometry(sc, hp, hp->spp, g)) return st;
    *spp_per_pass = g.S;
    return PT_OK;
}

__attribute__((visibility("default"))) int pt_bake_sh(pt_scene *sc, const PtBakeShParams *hp, const float *points, const uint8_t *light_select, uint32_t n_lights, float *sh_w, int buffers_are_device) {
    if (!sc || !hp || !points || !sh_w) return fail(PT_ERR_INVALID_ARG, "null argument");
    return pt_bake_sh_samples(sc, hp, points, light_select, n_lights, 0, hp->spp, sh_w, buffers_are_device);
}

__attribute__((visibility("default"))) int pt_bake_sh_samples(pt_scene *sc, const PtBakeShParams *hp, const float *points, const uint8_t *light_select, uint32_t n_lights, uint32_t first,
                                                              uint32_t n_samples, float *sh_w, int buffers_are_device) {
    if (!sc || !hp || !points || !sh_w) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_sh(hp)) return st;
    const PtBakeParams bp = sh_params(hp);
    if (int st = check_range(&bp, first, n_samples)) return st;
    std::vector<uint32_t> sel;
    if (int st = check_sh_points_and_lights(hp, points, light_select, n_lights, sel)) return st;
    if (int st = check_light_count(sc, n_lights)) return st;   // (all of the above before the device is touched)
    Geometry g;
    if (int st = sh_geometry(sc, hp, n_samples, g)) return st;
    if (int st = begin_call(sc, hp->profile != 0)) return st;
    DevTmp tmp;
    Staging out{tmp, sc->stream, buffers_are_device != 0};
    float4 *d_sh = nullptr, *d_wi = nullptr; float *d_points = nullptr;
    if (int st = out.plane(sh_w, (size_t)hp->n_points * 112, "bake sh sums", true, d_sh)) return st;
    if (int st = upload_points(sc, hp, points, tmp, d_points)) return st;
    AORayBuffers b; size_t rays; LightSamples ls;
    if (int st = alloc_pass_rays(g, sh_padded(hp), "bake sh rays", b, rays)) return st;
    if (int st = light_samples(sc, sel, hp->nsamples, rays, "bake sh rays", tmp, ls)) return st;
    SIDE_ALLOC(tmp, d_wi, rays * 16, "bake sh rays");
    if (int st = for_passes(g, first, n_samples, [&](uint32_t s0, uint32_t sn) { return sh_pass(sc, g, hp, s0, sn, d_points, d_sh, ls, d_wi, b); })) return st;
    return out.finish(sc);
}

__attribute__((visibility("default"))) int pt_bake_sh_resolve(const float *sh_w, uint32_t n_points, uint32_t spp, uint32_t nsamples, float *sh, float *reached) {
    return resolve_light_sums(sh_w, n_points, 28, spp, nsamples, sh, reached);
}

__attribute__((visibility("default"))) int pt_bake_sh_irradiance(const float *sh, const float *normals, uint32_t n, float *irradiance_rgb) {
    if (!sh || !normals || !irradiance_rgb) return fail(PT_ERR_INVALID_ARG, "null argument");
    // (Ramamoorthi and Hanrahan's cosine-lobe factors: pi, 2 pi / 3, pi / 4)
    const float A[9] = {3.141593f, 2.094395f, 2.094395f, 2.094395f, 0.785398f, 0.785398f, 0.785398f, 0.785398f, 0.785398f};
    for (size_t i = 0; i < n; ++i) {
        float Y[9]; sh_basis(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], Y);
        for (int c = 0; c < 3; ++c) {
            float e = 0.0f;
            for (int q = 0; q < 9; ++q) e += (A[q] * sh[27 * i + 3 * q + c]) * Y[q];
            irradiance_rgb[3 * i + c] = e;
        }
    }
    return PT_OK;
}

__attribute__((visibility("default"))) int pt_bake_sh_rays(pt_scene *sc, const PtBakeShParams *hp, const float *points, const uint8_t *light_select, uint32_t n_lights, uint32_t n, const uint32_t *point,
                                                           const uint32_t *sample, const uint32_t *element, uint32_t *out_light, float *out_wi, float *out_pdf, float *out_li, float *out_e,
                                                           float *out_o, float *out_d, uint8_t *found) {
    if (!sc || !hp || !points || !point || !sample || !element || !out_light || !out_wi || !out_pdf || !out_li || !out_e || !out_o || !out_d || !found) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_sh(hp)) return st;
    std::vector<uint32_t> sel;
    if (int st = check_sh_points_and_lights(hp, points, light_select, n_lights, sel)) return st;
    if (int st = check_queries(n, sample, element, hp->spp, hp->nsamples)) return st;
    if (int st = check_light_count(sc, n_lights)) return st;
    Geometry g;
    PtBakeShParams one = *hp; one.spp_per_pass = 1;
    if (int st = sh_geometry(sc, &one, hp->spp, g)) return st;
    if (n == 0) return PT_OK;
    if (int st = begin_call(sc, false)) return st;
    DevTmp tmp;
    float *d_points = nullptr; LightSamples ls; Queries q; LightRows rows;
    if (int st = upload_points(sc, hp, points, tmp, d_points)) return st;
    if (int st = light_samples(sc, sel, hp->nsamples, 0, "bake sh rays", tmp, ls)) return st;
    if (int st = upload_queries(sc, n, point, sample, element, "bake sh rays", tmp, q)) return st;
    if (int st = rows.alloc(tmp, n, "bake sh rays")) return st;
    sc->begin("bake_probe", n);
    launch_sph(sc, "ptbake::k_bake_sh_probe<true>", k_bake_sh_probe<true>, "ptbake::k_bake_sh_probe<false>", k_bake_sh_probe<false>, dim3((n + 255) / 256), sc->ds, g.rc, g_tabs, d_points, hp->n_points,
               hp->row, hp->nsamples, ls.sel, ls.n_sel, ls.scale, n, q.item, q.sample, q.element, rows.d_light, rows.d_out, rows.d_found);
    sc->end();
    HIP_TRY(hipGetLastError());
    if (int st = end_call(sc)) return st;
    return rows.read(n, out_light, out_wi, out_pdf, out_li, out_e, out_o, out_d, found);
}

}  // extern "C"
