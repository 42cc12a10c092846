// aov_render.hip -- pt_aov_render / pt_aov_render_samples / pt_aov_pass_size / pt_aov_resolve (include/mi355aov.h): first-hit albedo, shading normal and depth for the
// camera samples of pt_render_samples. Per pass of s_count samples of every pixel slot:
//   k_generate                     camera rays (libmi355pt's render_frame; dimensions 0-4 of the sample)
//   k_trace<closest>               their hits ("extend_camera")
//   k_aov                          the hit's record: albedo, normal, depth -- or the ray goes on behind a surface without a material
//   while rays go on (scenes with material-less shells only):
//     k_trace<closest>             the continuations' hits ("extend")
//     k_aov                        their records
//   k_aov_film                     the records' splats onto the planes, a pixel's own samples in sample order
// The scene, its workspace, the device counters, the traversal, the render frame and the steps a pass shares with the path integrator's -- the pass size the library chooses
// (choose_pass_size: one budget rule, given the record's bytes per path), the traversal set-up (extend_sub / trace_job / traced) and the launch geometry (blocks_for, film_grid,
// general_geometry) -- are libmi355pt's (host_common.h), as for libmi355ao: this library adds its checks and budget (aov_geometry), one pass (aov_pass), the kernels of
// aov_kernels.h, the records and the planes. The planes are the CALLER's while a call runs: device buffers
// are added to in place; host buffers are copied up, added to and copied back when every pass has succeeded -- so the additions onto a pixel are one chain in sample order
// however the job is cut into calls and passes. The frame's own film stays empty and is delivered to a scratch buffer.
// pt_matte_render / pt_matte_render_samples / pt_matte_pass_size / pt_matte_resolve / pt_matte_mask (the ID mattes) follow below the feature buffers: the same pass with
// k_matte and k_matte_film, the same geometry function with the mattes' record size.
#include "../csrc/host_common.h"
#include "../side/side_host.h"
#include "../../include/mi355aov.h"
#include "aov_kernels.h"
#include <algorithm>

using namespace ptaov;

namespace {

constexpr double kAovMemFraction = 0.5;   // of the device's free memory, for a pass the caller leaves to the library
constexpr size_t kAovRecBytes = 32;       // the sample's record (aov_kernels.h: AovJob): what a path costs besides libmi355pt's workspace

struct Geometry { RenderConst rc; uint32_t S; };

int check_buffers(const PtAOVBuffers *b) {
    if (!b->albedo_w && !b->normal_w && !b->depth_w) return fail(PT_ERR_INVALID_ARG, "feature buffers: all three planes are NULL");
    return PT_OK;
}

// The frame's checks (frame_geometry, libmi355pt) and the pass size. `n_samples`: how many of the job's rp->spp samples per pixel the call renders: it caps and divides
// the pass size only. `rec_bytes`: the sample's record of the render -- the feature buffers' or the mattes'.
int aov_geometry(pt_scene *sc, const PtRenderParams *rp, uint32_t n_samples, Geometry &g, size_t rec_bytes = kAovRecBytes) {
    RenderConst &rc = g.rc;
    PtRenderParams p = *rp;
    p.integrator = PT_INTEGRATOR_PATH;   // (not read: no medium, no volpath state)
    if (int st = frame_geometry(sc, &p, rc)) return st;
    uint32_t S = rp->spp_per_pass;
    // (the most paths of a pass: what the workspace's ray queue addresses, kernels.h)
    if (S == 0 && rc.n_pix_slots > 0) S = choose_pass_size(sc, rc.n_pix_slots, n_samples, 1, false, PassBudget{rec_bytes, kAovMemFraction, kMaxRayQueuePaths});
    return frame_pass_size(rc, S, n_samples, &g.S);
}

// What lives for one call (freed on every exit path): the records, the frame's scratch film, and the device side of host planes.
struct AovCall {
    DevTmp tmp;
    float4 *rec = nullptr;
    float *scratch_film = nullptr;
    AovPlanes planes{nullptr, nullptr, nullptr};
    uint32_t mask = 0;
    float *host[3] = {nullptr, nullptr, nullptr};   // the caller's host planes (buffers_are_device == 0)
    size_t bytes[3] = {0, 0, 0};
    float **dev(int k) { return k == 0 ? &planes.albedo : k == 1 ? &planes.normal : &planes.depth; }
};

int aov_prepare(pt_scene *sc, const Geometry &g, const PtAOVBuffers *b, int on_device, AovCall &c) {
    const size_t film_px = (size_t)g.rc.film_w * g.rc.film_h, paths = (size_t)g.rc.n_pix_slots * g.S;
    float *const given[3] = {b->albedo_w, b->normal_w, b->depth_w};
    SIDE_ALLOC(c.tmp, c.rec, paths * kAovRecBytes, "feature buffers");
    for (int k = 0; k < 3; ++k) {
        if (!given[k]) continue;
        c.mask |= 1u << k;
        c.bytes[k] = film_px * (k < 2 ? 16 : 8);
        if (on_device) { *c.dev(k) = given[k]; continue; }
        c.host[k] = given[k];
        SIDE_ALLOC(c.tmp, *c.dev(k), c.bytes[k], "feature buffers");
        HIP_TRY(hipMemcpyAsync(*c.dev(k), given[k], c.bytes[k], hipMemcpyHostToDevice, sc->stream));
    }
    return PT_OK;
}

int aov_pass(pt_scene *sc, const RenderConst &rc, AovCall &c) {
    const uint32_t total = rc.n_pix_slots * rc.s_count;
    QCounters *qc = sc->qc;
    const bool sph = general_geometry(sc);
    auto record = [&](int cur, bool first_round, uint32_t n) {
        AovJob job{};
        job.rec = c.rec; job.next = sc->q.ext[1 - cur]; job.next_count = &qc->ext[1 - cur]; job.mask = c.mask; job.first_round = first_round ? 1u : 0u;
        const dim3 grid = blocks_for(n, 16u);
        sc->begin("aov", n);
        if (sph) launch(sc, "ptaov::k_aov<true>", k_aov<true>, grid, dim3(256), sc->ds, rc, g_tabs, sc->ps, sc->q.ext[cur], &qc->ext[cur], job);
        else launch(sc, "ptaov::k_aov<false>", k_aov<false>, grid, dim3(256), sc->ds, rc, g_tabs, sc->ps, sc->q.ext[cur], &qc->ext[cur], job);
        sc->end();
    };
    if (int st = first_hit_chase(sc, total, "feature buffers", record)) return st;
    sc->begin("film", total);
    launch(sc, "ptaov::k_aov_film", k_aov_film, film_grid(rc), dim3(256), rc, sc->ps, c.rec, sc->d_filter, c.planes, sc->dc);
    sc->end();
    HIP_TRY(hipGetLastError());
    QCounters h;
    return sync_queue_counters(sc, h);   // (a status a kernel raised fails the call here)
}

// The host planes' way back, once every pass has succeeded
int aov_finish(pt_scene *sc, AovCall &c) {
    HIP_TRY(hipStreamSynchronize(sc->stream));
    for (int k = 0; k < 3; ++k) if (c.host[k]) HIP_TRY(hipMemcpy(c.host[k], *c.dev(k), c.bytes[k], hipMemcpyDeviceToHost));
    return PT_OK;
}

// ---- ID mattes: pt_matte_render / pt_matte_render_samples / pt_matte_pass_size / pt_matte_mask (pt_matte_resolve is host arithmetic) ----
// The pass is aov_pass's with k_matte for k_aov and k_matte_film -- one thread per film pixel, a gather -- for k_aov_film. The tables are the CALLER's while a call
// runs, as the planes are: device tables are continued in place, host tables copied up, continued and copied back when every pass has succeeded.

constexpr size_t kMatteRecBytes = 16;   // the sample's ids (aov_kernels.h: MatteJob)

int check_matte_buffers(const PtMatteBuffers *b) {
    if (!b->layer[0] && !b->layer[1] && !b->layer[2]) return fail(PT_ERR_INVALID_ARG, "mattes: all three layers are NULL");
    if (b->layer[PT_MATTE_GROUP] && !b->prim_group) return fail(PT_ERR_INVALID_ARG, "mattes: the group layer needs prim_group");
    return PT_OK;
}

// What the scene decides, read from the handle's host side
int check_matte_scene(const pt_scene *sc, const PtRenderParams *rp, const PtMatteBuffers *b) {
    if (b->layer[PT_MATTE_GROUP] && b->n_prims != sc->ds.n_prims)
        return fail(PT_ERR_INVALID_ARG, "mattes: prim_group has " + std::to_string(b->n_prims) + " entries, the scene " + std::to_string(sc->ds.n_prims) + " primitives");
    if (rp->tile_world > 1)
        return fail(PT_ERR_UNSUPPORTED, "mattes: tile_world > 1 -- a pixel's table gathers the samples of its neighbour pixels in a fixed order, and another rank owns the neighbours across a tile edge");
    if (rp->tile_rank != 0) return fail(PT_ERR_INVALID_ARG, "mattes: tile_rank must be 0 (the render owns every tile)");   // (k_matte_film's pixel -> slot map is the whole grid's)
    return PT_OK;
}

struct MatteCall {
    DevTmp tmp;
    uint4 *rec = nullptr;
    float *scratch_film = nullptr;
    uint32_t *prim_group = nullptr;
    MatteTables tabs{{nullptr, nullptr, nullptr}, 0};
    PtMattePixel *host[3] = {nullptr, nullptr, nullptr};   // the caller's host tables (buffers_are_device == 0)
    size_t bytes = 0;
};

int matte_prepare(pt_scene *sc, const Geometry &g, const PtMatteBuffers *b, int on_device, MatteCall &c) {
    const size_t film_px = (size_t)g.rc.film_w * g.rc.film_h, paths = (size_t)g.rc.n_pix_slots * g.S;
    SIDE_ALLOC(c.tmp, c.rec, paths * kMatteRecBytes, "mattes");
    c.bytes = film_px * sizeof(PtMattePixel);
    for (int k = 0; k < 3; ++k) {
        if (!b->layer[k]) continue;
        c.tabs.mask |= 1u << k;
        if (on_device) { c.tabs.layer[k] = reinterpret_cast<uint4 *>(b->layer[k]); continue; }
        c.host[k] = b->layer[k];
        SIDE_ALLOC(c.tmp, c.tabs.layer[k], c.bytes, "mattes");
        HIP_TRY(hipMemcpyAsync(c.tabs.layer[k], b->layer[k], c.bytes, hipMemcpyHostToDevice, sc->stream));
    }
    if (b->layer[PT_MATTE_GROUP]) {   // once per call
        SIDE_ALLOC(c.tmp, c.prim_group, (size_t)b->n_prims * 4, "mattes");
        HIP_TRY(hipMemcpyAsync(c.prim_group, b->prim_group, (size_t)b->n_prims * 4, hipMemcpyHostToDevice, sc->stream));
    }
    return PT_OK;
}

int matte_pass(pt_scene *sc, const RenderConst &rc, MatteCall &c) {
    const uint32_t total = rc.n_pix_slots * rc.s_count;
    QCounters *qc = sc->qc;
    const bool sph = general_geometry(sc);
    auto record = [&](int cur, bool, uint32_t n) {
        MatteJob job{c.rec, sc->q.ext[1 - cur], &qc->ext[1 - cur], c.prim_group};
        const dim3 grid = blocks_for(n, 16u);
        sc->begin("matte", n);
        if (sph) launch(sc, "ptaov::k_matte<true>", k_matte<true>, grid, dim3(256), sc->ds, sc->ps, sc->q.ext[cur], &qc->ext[cur], job);
        else launch(sc, "ptaov::k_matte<false>", k_matte<false>, grid, dim3(256), sc->ds, sc->ps, sc->q.ext[cur], &qc->ext[cur], job);
        sc->end();
    };
    if (int st = first_hit_chase(sc, total, "mattes", record)) return st;
    const size_t film_px = (size_t)rc.film_w * rc.film_h;
    sc->begin("matte_film", total);
    launch(sc, "ptaov::k_matte_film", k_matte_film, dim3((unsigned)((film_px + 255) / 256)), dim3(256), rc, sc->ps, c.rec, sc->d_filter, c.tabs, sc->dc);
    sc->end();
    HIP_TRY(hipGetLastError());
    QCounters h;
    return sync_queue_counters(sc, h);
}

int matte_finish(pt_scene *sc, MatteCall &c) {
    HIP_TRY(hipStreamSynchronize(sc->stream));
    for (int k = 0; k < 3; ++k) if (c.host[k]) HIP_TRY(hipMemcpy(c.host[k], c.tabs.layer[k], c.bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int pt_matte_pass_size(pt_scene *sc, const PtRenderParams *rp, uint32_t *spp_per_pass) {
    if (!sc || !rp || !spp_per_pass) return fail(PT_ERR_INVALID_ARG, "null argument");
    Geometry g;
    if (int st = aov_geometry(sc, rp, rp->spp, g, kMatteRecBytes)) return st;
    *spp_per_pass = reported_pass_size(g.S, rp);
    return PT_OK;
}

__attribute__((visibility("default"))) int pt_matte_render(pt_scene *sc, const PtRenderParams *rp, const PtMatteBuffers *buffers, int buffers_are_device) {   // the whole job: [0, spp)
    if (!sc || !rp || !buffers) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_matte_buffers(buffers)) return st;
    if (int st = check_spp(rp)) return st;
    return pt_matte_render_samples(sc, rp, 0, rp->spp, buffers, buffers_are_device);
}

__attribute__((visibility("default"))) int pt_matte_render_samples(pt_scene *sc, const PtRenderParams *rp, uint32_t first, uint32_t n_samples, const PtMatteBuffers *buffers, int buffers_are_device) {
    if (!sc || !rp || !buffers) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_matte_buffers(buffers)) return st;
    if (int rst = check_sample_range(rp, first, n_samples)) return rst;   // (all of this before the device is touched, and before the scene is looked at)
    if (int st = check_matte_scene(sc, rp, buffers)) return st;
    Geometry g;
    if (int gst = aov_geometry(sc, rp, n_samples, g, kMatteRecBytes)) return gst;
    if ((uint64_t)g.rc.film_w * g.rc.film_h > (1ull << 31)) return fail(PT_ERR_INVALID_ARG, "mattes: more than 2^31 film pixels");
    MatteCall c;   // (freed when the call returns, however it ends)
    if (g.rc.n_pix_slots > 0) SIDE_ALLOC(c.tmp, c.scratch_film, (size_t)g.rc.film_w * g.rc.film_h * 16, "mattes");
    return render_frame(sc, rp, g.rc, g.S, first, n_samples, c.scratch_film, 1,
                        [&]() { return matte_prepare(sc, g, buffers, buffers_are_device, c); }, [&]() { return matte_pass(sc, g.rc, c); }, [&]() { return matte_finish(sc, c); });
}

__attribute__((visibility("default"))) int pt_matte_resolve(const PtMattePixel *table, uint32_t n_pixels, uint32_t n_ranks, uint32_t *ids, float *coverage) {
    if (!table || !ids || !coverage) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (n_ranks == 0 || n_ranks > PT_MATTE_SLOTS) return fail(PT_ERR_INVALID_ARG, "mattes: n_ranks must be 1 .. 8");
    for (size_t i = 0; i < n_pixels; ++i) {
        const PtMattePixel &t = table[i];
        const uint32_t n = std::min(t.n_ids, (uint32_t)PT_MATTE_SLOTS);
        uint32_t order[PT_MATTE_SLOTS];
        for (uint32_t k = 0; k < n; ++k) order[k] = k;
        std::sort(order, order + n, [&](uint32_t a, uint32_t b) { return t.w[a] != t.w[b] ? t.w[a] > t.w[b] : t.id[a] < t.id[b]; });
        for (uint32_t r = 0; r < n_ranks; ++r) {
            const bool there = r < n && t.w_total != 0.0f;
            ids[i * n_ranks + r] = there ? t.id[order[r]] : 0u;
            coverage[i * n_ranks + r] = there ? t.w[order[r]] / t.w_total : 0.0f;
        }
    }
    return PT_OK;
}

__attribute__((visibility("default"))) int pt_matte_mask(pt_scene *sc, const PtMattePixel *table, int table_is_device, uint32_t n_pixels, const uint32_t *ids, uint32_t n_ids, float *mask, int mask_is_device) {
    if (!sc || !table || !ids || !mask) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (n_ids == 0 || n_ids > kMatteMaskIds) return fail(PT_ERR_INVALID_ARG, "mattes: a mask takes 1 .. 4096 ids");
    if (n_pixels == 0) return PT_OK;
    if (n_pixels > (1u << 31)) return fail(PT_ERR_INVALID_ARG, "mattes: more than 2^31 pixels");   // (all of the above before the device is touched)
    if (sc->device != g_device) { if (int st = bind_device(sc->device)) return st; }
    if (!sc->stream) HIP_TRY(hipStreamCreate(&sc->stream));
    sc->drop_timings();
    DevTmp tmp;
    const uint4 *d_table = reinterpret_cast<const uint4 *>(table);
    uint32_t *d_ids = nullptr;
    float *d_mask = mask;
    SIDE_ALLOC(tmp, d_ids, (size_t)n_ids * 4, "mattes");
    HIP_TRY(hipMemcpyAsync(d_ids, ids, (size_t)n_ids * 4, hipMemcpyHostToDevice, sc->stream));
    if (!table_is_device) {
        uint4 *up = nullptr;
        SIDE_ALLOC(tmp, up, (size_t)n_pixels * sizeof(PtMattePixel), "mattes");
        HIP_TRY(hipMemcpyAsync(up, table, (size_t)n_pixels * sizeof(PtMattePixel), hipMemcpyHostToDevice, sc->stream));
        d_table = up;
    }
    if (!mask_is_device) SIDE_ALLOC(tmp, d_mask, (size_t)n_pixels * 4, "mattes");
    sc->begin("matte_mask", n_pixels);
    launch(sc, "ptaov::k_matte_mask", k_matte_mask, dim3((unsigned)(((size_t)n_pixels + 255) / 256)), dim3(256), d_table, n_pixels, (const uint32_t *)d_ids, n_ids, d_mask);
    sc->end();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(sc->stream));
    sc->resolve_timings();
    if (!mask_is_device) HIP_TRY(hipMemcpy(mask, d_mask, (size_t)n_pixels * 4, hipMemcpyDeviceToHost));
    return PT_OK;
}

__attribute__((visibility("default"))) int pt_aov_pass_size(pt_scene *sc, const PtRenderParams *rp, uint32_t *spp_per_pass) {
    if (!sc || !rp || !spp_per_pass) return fail(PT_ERR_INVALID_ARG, "null argument");
    Geometry g;
    if (int st = aov_geometry(sc, rp, rp->spp, g)) return st;
    *spp_per_pass = reported_pass_size(g.S, rp);
    return PT_OK;
}

__attribute__((visibility("default"))) int pt_aov_render(pt_scene *sc, const PtRenderParams *rp, const PtAOVBuffers *buffers, int buffers_are_device) {   // the whole job: [0, spp)
    if (!sc || !rp || !buffers) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_buffers(buffers)) return st;
    if (int st = check_spp(rp)) return st;
    return pt_aov_render_samples(sc, rp, 0, rp->spp, buffers, buffers_are_device);
}

__attribute__((visibility("default"))) int pt_aov_render_samples(pt_scene *sc, const PtRenderParams *rp, uint32_t first, uint32_t n_samples, const PtAOVBuffers *buffers, int buffers_are_device) {
    if (!sc || !rp || !buffers) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_buffers(buffers)) return st;
    if (int rst = check_sample_range(rp, first, n_samples)) return rst;   // (all of this before the device is touched)
    Geometry g;
    if (int gst = aov_geometry(sc, rp, n_samples, g)) return gst;
    AovCall c;   // (freed when the call returns, however it ends)
    // the frame's film: nothing is splatted onto it, and a rank that owns no tile never delivers it
    if (g.rc.n_pix_slots > 0) SIDE_ALLOC(c.tmp, c.scratch_film, (size_t)g.rc.film_w * g.rc.film_h * 16, "feature buffers");
    return render_frame(sc, rp, g.rc, g.S, first, n_samples, c.scratch_film, 1,
                        [&]() { return aov_prepare(sc, g, buffers, buffers_are_device, c); }, [&]() { return aov_pass(sc, g.rc, c); }, [&]() { return aov_finish(sc, c); });
}

__attribute__((visibility("default"))) int pt_aov_resolve(const PtAOVBuffers *sums, uint32_t n_pixels, float *albedo_rgb, float *normal_xyz, float *depth) {
    if (!sums) return fail(PT_ERR_INVALID_ARG, "null argument");
    for (size_t i = 0; i < n_pixels; ++i) {
        if (sums->albedo_w && albedo_rgb) {
            const float *a = sums->albedo_w + 4 * i;
            for (int k = 0; k < 3; ++k) albedo_rgb[3 * i + k] = a[3] != 0.0f ? a[k] / a[3] : 0.0f;
        }
        if (sums->normal_w && normal_xyz) {
            const float *n = sums->normal_w + 4 * i;
            const float len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            for (int k = 0; k < 3; ++k) normal_xyz[3 * i + k] = (n[3] != 0.0f && len > 0.0f) ? n[k] / len : 0.0f;
        }
        if (sums->depth_w && depth) {
            const float *d = sums->depth_w + 2 * i;
            depth[i] = d[1] != 0.0f ? d[0] / d[1] : 0.0f;
        }
    }
    return PT_OK;
}

}  // extern "C"
