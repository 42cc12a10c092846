// ao_render.hip -- pt_ao_render / pt_ao_render_samples / pt_ao_pass_size (include/mi355ao.h): the ambient-occlusion integrator (integrators/ao.rs) in the
// render loop of SamplerIntegrator::render (integrator.rs:263-403). Per pass of s_count samples of every pixel slot:
//   k_generate                     camera rays (libmi355pt's render_frame; dimensions 0-4 of the sample)
//   k_trace<closest>               their hits ("extend_camera")
//   per chunk of <= 64 AO rays per path:
//     k_ao_rays                    the chunk's rays from each hit (dimensions 5 and 6 of sample numbers s * nsamples + k)
//     k_trace<any>                 the rays' any-hit walk ("shadow": Scene::intersect_p, t_max = infinity)
//     k_ao_accum                   L += the unoccluded rays' terms, in order
//   k_film                         sanitise + splat (libmi355pt)
// The scene, its workspace, the device counters, the traversal and the render frame -- the shared checks, the pass loop, the film's way out, the counters
// (frame_geometry / render_frame, render_loop.hip) -- are libmi355pt's (host_common.h), and so are the steps a pass shares with the path integrator's: the pass size the
// library chooses (choose_pass_size: one budget rule, given AO's bytes per path), the camera-ray traversal set-up (extend_sub / trace_job / traced), the launch geometry
// (blocks_for, general_geometry) and the k_film step (film_pass). This library adds AO's own checks and budget (ao_geometry), one pass (ao_pass), the kernels of
// ao_kernels.h and the buffers of the AO rays, which live for one call.
#include "../csrc/host_common.h"
#include "../side/side_host.h"
#include "../../include/mi355ao.h"
#include "ao_kernels.h"

using namespace ptao;

namespace {

struct Geometry { RenderConst rc; uint32_t S; uint32_t K; };

// The frame's checks (frame_geometry, libmi355pt) around AO's own: its parameters, the sample numbers its arrays use, its pass size and the rays of one launch.
// `n_samples`: how many of the job's rp->spp samples per pixel the call renders (pt_ao_render_samples): it caps and divides the pass size only -- the array numbering
// s * nsamples + k and its table-size check are the job's.
int ao_geometry(pt_scene *sc, const PtRenderParams *rp, const PtAOParams *ao, uint32_t n_samples, Geometry &g) {
    if (!sc || !rp || !ao) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (ao->nsamples == 0) return fail(PT_ERR_INVALID_ARG, "ambientocclusion: nsamples must be > 0");
    RenderConst &rc = g.rc;
    PtRenderParams p = *rp;
    p.integrator = PT_INTEGRATOR_PATH;   // (no medium, no volpath state)
    if (int st = frame_geometry(sc, &p, rc)) return st;
    if (int st = check_ao_sample_numbers(rc, rp->spp, ao->nsamples, "ambientocclusion", "pixel")) return st;
    g.K = std::min<uint32_t>(ao->nsamples, kAOChunk);
    uint32_t S = rp->spp_per_pass;
    // (per path besides libmi355pt's workspace: the ray id base and the chunk's rays)
    if (S == 0 && rc.n_pix_slots > 0) S = choose_pass_size(sc, rc.n_pix_slots, n_samples, 1, false, ao_ray_budget(g.K));
    if (int st = frame_pass_size(rc, S, n_samples, &g.S)) return st;
    if ((size_t)rc.n_pix_slots * g.S * g.K > kAOMaxRays) return fail(PT_ERR_INVALID_ARG, "pass too large: paths x min(nsamples, 64) AO rays per launch > 2^31 (lower spp_per_pass)");
    return PT_OK;
}

int ao_pass(pt_scene *sc, const RenderConst &rc, const PtAOParams *ao, uint32_t K, const AORayBuffers &b) {
    const uint32_t total = rc.n_pix_slots * rc.s_count;
    QCounters *qc = sc->qc;
    TraceJob cam = trace_job(sc, 0);   // camera rays -> hit records (Scene::intersect, ao.rs:72)
    cam.sub[0] = extend_sub(sc, 0, true);
    int st;
    if ((st = traced(sc, "extend_camera", 0, cam, total))) return st;
    const bool sph = general_geometry(sc);
    const dim3 qblocks = blocks_for(total, 16u);
    auto spawn = [&](const AOJob &job) {
        sc->begin("ao_rays", (uint64_t)total * job.kn);
        if (sph) launch(sc, "ptao::k_ao_rays<true>", k_ao_rays<true>, qblocks, dim3(256), sc->ds, rc, g_tabs, sc->ps, sc->q.ext[0], &qc->ext[0], job);
        else launch(sc, "ptao::k_ao_rays<false>", k_ao_rays<false>, qblocks, dim3(256), sc->ds, rc, g_tabs, sc->ps, sc->q.ext[0], &qc->ext[0], job);
        sc->end();
    };
    auto accum = [&](const AOJob &job) {
        sc->begin("ao_accum", total);
        launch(sc, "ptao::k_ao_accum", k_ao_accum, qblocks, dim3(256), sc->ps, sc->q.ext[0], &qc->ext[0], job);
        sc->end();
    };
    AOJob job{};
    job.nsamples = ao->nsamples; job.cos_sample = ao->cos_sample ? 1u : 0u;
    if ((st = ao_chunks<AOJob>(sc, job, K, total, INFINITY, b, spawn, accum))) return st;   // (Scene::intersect_p of spawn_ray(wi): t_max = infinity)
    if ((st = film_pass(sc, rc))) return st;
    QCounters h;
    return sync_queue_counters(sc, h);   // (a status a kernel raised fails the call here)
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int pt_ao_pass_size(pt_scene *sc, const PtRenderParams *rp, const PtAOParams *ao, uint32_t *spp_per_pass) {
    if (!spp_per_pass) return fail(PT_ERR_INVALID_ARG, "null argument");
    Geometry g;
    if (int st = ao_geometry(sc, rp, ao, rp ? rp->spp : 0, g)) return st;
    *spp_per_pass = reported_pass_size(g.S, rp);
    return PT_OK;
}

__attribute__((visibility("default"))) int pt_ao_render(pt_scene *sc, const PtRenderParams *rp, const PtAOParams *ao, float *film_xyzw, int film_is_device) {   // the whole job: [0, spp)
    if (!sc || !rp || !ao || !film_xyzw) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (ao->nsamples == 0) return fail(PT_ERR_INVALID_ARG, "ambientocclusion: nsamples must be > 0");
    if (int st = check_spp(rp)) return st;
    return pt_ao_render_samples(sc, rp, ao, 0, rp->spp, film_xyzw, film_is_device);
}

// Sample numbers [first, first + n) of every pixel: element k of sample s stays sample number s * nsamples + k of the JOB (k_ao_rays: rc.s_begin + sl)
__attribute__((visibility("default"))) int pt_ao_render_samples(pt_scene *sc, const PtRenderParams *rp, const PtAOParams *ao, uint32_t first, uint32_t n_samples, float *film_xyzw, int film_is_device) {
    if (!sc || !rp || !ao || !film_xyzw) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int rst = check_sample_range(rp, first, n_samples)) return rst;   // (before the device is touched)
    Geometry g;
    if (int gst = ao_geometry(sc, rp, ao, n_samples, g)) return gst;
    AORayBuffers b;   // (freed when the call returns, however it ends)
    // (the steps cross as std::function, FrameStep: render_frame launches libmi355pt's k_generate / k_film_finish, so it is one function there, not a header template compiled here too)
    auto prepare = [&]() { const size_t paths = (size_t)g.rc.n_pix_slots * g.S; return b.alloc(paths, paths * g.K, "ambientocclusion rays"); };
    return render_frame(sc, rp, g.rc, g.S, first, n_samples, film_xyzw, film_is_device, prepare, [&]() { return ao_pass(sc, g.rc, ao, g.K, b); });
}

}  // extern "C"
