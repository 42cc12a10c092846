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
#include "../csrc/host_common.h"
#include "../../include/mi355aov.h"
#include "aov_kernels.h"

using namespace ptaov;

namespace {

constexpr double kAovMemFraction = 0.5;   // of the device's free memory, for a pass the caller leaves to the library
constexpr size_t kAovRecBytes = 32;       // the sample's record (aov_kernels.h: AovJob): what a path costs besides libmi355pt's workspace
constexpr int kAovMaxRounds = 1 << 16;    // continuations of one camera ray: a scene's shells are finitely many

struct Geometry { RenderConst rc; uint32_t S; };

int check_buffers(const PtAOVBuffers *b) {
    if (!b->albedo_w && !b->normal_w && !b->depth_w) return fail(PT_ERR_INVALID_ARG, "feature buffers: all three planes are NULL");
    return PT_OK;
}

// The frame's checks (frame_geometry, libmi355pt) and the pass size. `n_samples`: how many of the job's rp->spp samples per pixel the call renders: it caps and divides
// the pass size only.
int aov_geometry(pt_scene *sc, const PtRenderParams *rp, uint32_t n_samples, Geometry &g) {
    RenderConst &rc = g.rc;
    PtRenderParams p = *rp;
    p.integrator = PT_INTEGRATOR_PATH;   // (not read: no medium, no volpath state)
    if (int st = frame_geometry(sc, &p, rc)) return st;
    uint32_t S = rp->spp_per_pass;
    // (the most paths of a pass: what the workspace's ray queue addresses, kernels.h)
    if (S == 0 && rc.n_pix_slots > 0) S = choose_pass_size(sc, rc.n_pix_slots, n_samples, 1, false, PassBudget{kAovRecBytes, kAovMemFraction, kMaxRayQueuePaths});
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
    auto oom = [](hipError_t e) { (void)hipGetLastError(); return fail(PT_ERR_OUT_OF_MEMORY, std::string("feature buffers: ") + hipGetErrorString(e)); };
    if (hipError_t e = c.tmp.alloc(&c.rec, paths * kAovRecBytes); e != hipSuccess) return oom(e);
    for (int k = 0; k < 3; ++k) {
        if (!given[k]) continue;
        c.mask |= 1u << k;
        c.bytes[k] = film_px * (k < 2 ? 16 : 8);
        if (on_device) { *c.dev(k) = given[k]; continue; }
        c.host[k] = given[k];
        if (hipError_t e = c.tmp.alloc(c.dev(k), c.bytes[k]); e != hipSuccess) return oom(e);
        HIP_TRY(hipMemcpyAsync(*c.dev(k), given[k], c.bytes[k], hipMemcpyHostToDevice, sc->stream));
    }
    return PT_OK;
}

int aov_pass(pt_scene *sc, const RenderConst &rc, AovCall &c) {
    const uint32_t total = rc.n_pix_slots * rc.s_count;
    QCounters *qc = sc->qc;
    const bool sph = general_geometry(sc);
    uint32_t n = total;   // rays of the round (round 0: an upper bound, the launches read the count of camera rays)
    for (int round = 0, cur = 0; n > 0; ++round, cur = 1 - cur) {
        if (round == kAovMaxRounds) return fail(PT_ERR_PROBE_CHAIN, "feature buffers: camera rays still going on behind material-less surfaces after " + std::to_string(round) + " continuations");
        TraceJob tj = trace_job(sc, 0);   // Scene::intersect of the camera rays, then of the rays spawned behind shells
        tj.sub[0] = extend_sub(sc, cur, round == 0);
        if (round > 0) HIP_TRY(hipMemsetAsync(qc->head, 0, sizeof qc->head, sc->stream));
        int st;
        if ((st = traced(sc, round == 0 ? "extend_camera" : "extend", 0, tj, n))) return st;
        AovJob job{};
        job.rec = c.rec; job.next = sc->q.ext[1 - cur]; job.next_count = &qc->ext[1 - cur]; job.mask = c.mask; job.first_round = round == 0 ? 1u : 0u;
        HIP_TRY(hipMemsetAsync(&qc->ext[1 - cur], 0, 4, sc->stream));
        const dim3 grid = blocks_for(n, 16u);
        sc->begin("aov", n);
        if (sph) launch(sc, "ptaov::k_aov<true>", k_aov<true>, grid, dim3(256), sc->ds, rc, g_tabs, sc->ps, sc->q.ext[cur], &qc->ext[cur], job);
        else launch(sc, "ptaov::k_aov<false>", k_aov<false>, grid, dim3(256), sc->ds, rc, g_tabs, sc->ps, sc->q.ext[cur], &qc->ext[cur], job);
        sc->end();
        HIP_TRY(hipGetLastError());
        if (!sc->has_null_material) break;   // every hit carries a material: nothing goes on, no count to wait for
        QCounters h;
        if ((st = sync_queue_counters(sc, h))) return st;
        n = h.ext[1 - cur];
    }
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

}  // namespace

extern "C" {

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
    if (g.rc.n_pix_slots > 0) if (hipError_t e = c.tmp.alloc(&c.scratch_film, (size_t)g.rc.film_w * g.rc.film_h * 16); e != hipSuccess) { (void)hipGetLastError(); return fail(PT_ERR_OUT_OF_MEMORY, std::string("feature buffers: ") + hipGetErrorString(e)); }
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
