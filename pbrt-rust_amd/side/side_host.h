// side_host.h -- the host side of what the libraries beside libmi355pt.so share among themselves (ao/, aov/, bake/, denoise/), once. Included after
// csrc/host_common.h, whose declarations it is written in; header-only, since every side library is a shared object of its own with hidden visibility.
// Its place would be host_common.h; it stands here because the profile record is taken of csrc/ as hashed (tools/code_hash.py).
#pragma once

namespace ptside {

inline int oom(const char *what, hipError_t e) { (void)hipGetLastError(); return fail(PT_ERR_OUT_OF_MEMORY, std::string(what) + ": " + hipGetErrorString(e)); }
#define SIDE_ALLOC(tmp, ptr, bytes, what) do { if (hipError_t _a = (tmp).alloc(&(ptr), (bytes)); _a != hipSuccess) return oom(what, _a); } while (0)

// The array values of a pixel / texel are sample numbers 0 .. spp * nsamples - 1 (sampler.rs:288-302). Sobol': the global index of sample number j is j << 2m plus the
// pixel's bits, and the generator matrices have 52 columns (lowdiscrepancy.rs:512-569). Halton: index = offset + j * stride must fit in 64 bits (halton.rs:122-155).
// `who` / `per`: "ambientocclusion" / "pixel", "bake" / "texel".
inline int check_ao_sample_numbers(const RenderConst &rc, uint32_t spp, uint32_t nsamples, const char *who, const char *per) {
    const uint64_t numbers = (uint64_t)spp * nsamples;
    if (rc.halton.enabled) {
        if (numbers > ~0ull / rc.halton.stride - 1) return fail(PT_ERR_INVALID_ARG, std::string(who) + ": spp x nsamples sample numbers per " + per + " exceed the Halton sampler's 64-bit index");
    } else if (numbers - 1 >= (1ull << (52 - 2 * rc.sobol.log2_resolution))) {
        return fail(PT_ERR_INVALID_ARG, std::string(who) + ": spp x nsamples = " + std::to_string(numbers) + " sample numbers per " + per + " exceed the 2^" +
                                         std::to_string(52 - 2 * rc.sobol.log2_resolution) + " the Sobol' tables serve at this resolution");
    }
    return PT_OK;
}

// What a point (a path, a texel sample) costs besides libmi355pt's workspace when K AO rays of it are in flight: the ray id base and, per ray, the ray record, the
// weight and the any-hit flag -- of half the device's free memory, for a pass the caller leaves to the library. kAOMaxRays: ray ids per chunk (32-bit ids, k_trace's queue index).
constexpr size_t kAOMaxRays = (size_t)1 << 31;
inline PassBudget ao_ray_budget(uint32_t K) { return PassBudget{4 + (size_t)K * (32 + 4 + 4), 0.5, kAOMaxRays / K}; }

// Per-call buffers of the AO rays (freed on every exit path: a call leaves the device's free memory as it found it, apart from the scene's workspace).
struct AORayBuffers {
    DevTmp tmp;
    float4 *ray = nullptr; float *w = nullptr; uint32_t *occ = nullptr, *base = nullptr, *count = nullptr;
    int alloc(size_t items, size_t rays, const char *what) {
        SIDE_ALLOC(tmp, ray, rays * 32, what); SIDE_ALLOC(tmp, w, rays * 4, what); SIDE_ALLOC(tmp, occ, rays * 4, what);
        SIDE_ALLOC(tmp, base, items * 4, what); SIDE_ALLOC(tmp, count, 4, what);
        return PT_OK;
    }
};

// The chunk loop over the job.nsamples AO rays of `items` points, K at a time. `job` (side/ao_rays.h: AOChunk, or a struct that begins with one) comes with nsamples,
// cos_sample and what its library adds; the loop gives it the chunk and the buffers. The caller's spawn step writes the chunk's rays (ray ids from b.count), the any-hit
// walk (Scene::intersect_p of the spawned rays, ao.rs:94, with t_max) leaves b.occ, the caller's accumulate step adds the unoccluded ones. Each step opens its own launch kind.
template <class Job> using ChunkStep = std::function<void(const Job &)>;
template <class Job> int ao_chunks(pt_scene *sc, Job job, uint32_t K, uint32_t items, float t_max, const AORayBuffers &b, const ChunkStep<Job> &spawn, const ChunkStep<Job> &accum) {
    job.ray = b.ray; job.w = b.w; job.base = b.base; job.ray_count = b.count; job.occluded = b.occ;
    for (job.k0 = 0; job.k0 < job.nsamples; job.k0 += K) {
        job.kn = std::min(K, job.nsamples - job.k0);
        HIP_TRY(hipMemsetAsync(b.count, 0, 4, sc->stream));
        HIP_TRY(hipMemsetAsync(sc->qc->head, 0, sizeof sc->qc->head, sc->stream));
        spawn(job);
        HIP_TRY(hipGetLastError());
        TraceJob tj = trace_job(sc, 2);   // ray ids, no queue
        tj.sub[0] = trace_sub(nullptr, b.count, (const float *)b.ray, 8, t_max, 2);
        tj.sub[0].out_word = b.occ; tj.sub[0].out_word_stride = 1; tj.sub[0].any = 1;
        if (int st = traced(sc, "shadow", 1, tj, items * job.kn)) return st;   // (an upper bound: the launch reads the count of rays spawned)
        accum(job);
        HIP_TRY(hipGetLastError());
    }
    return PT_OK;
}

// The first-hit chase of `total` camera rays: Scene::intersect of the camera rays, the caller's record kernel over queue set `cur`, then -- in scenes with material-less
// shells only -- of the rays the record kernel spawned behind such shells into queue set 1 - cur, round by round until none goes on. `n`: rays of the round (round 0: an
// upper bound, the launches read the count of camera rays). `noun`: the caller's, in the error text.
constexpr int kAovMaxRounds = 1 << 16;    // continuations of one camera ray: a scene's shells are finitely many
using RecordStep = std::function<void(int cur, bool first_round, uint32_t n)>;
inline int first_hit_chase(pt_scene *sc, uint32_t total, const char *noun, const RecordStep &record) {
    QCounters *qc = sc->qc;
    uint32_t n = total;
    for (int round = 0, cur = 0; n > 0; ++round, cur = 1 - cur) {
        if (round == kAovMaxRounds) return fail(PT_ERR_PROBE_CHAIN, std::string(noun) + ": camera rays still going on behind material-less surfaces after " + std::to_string(round) + " continuations");
        TraceJob tj = trace_job(sc, 0);
        tj.sub[0] = extend_sub(sc, cur, round == 0);
        if (round > 0) HIP_TRY(hipMemsetAsync(qc->head, 0, sizeof qc->head, sc->stream));
        if (int st = traced(sc, round == 0 ? "extend_camera" : "extend", 0, tj, n)) return st;
        HIP_TRY(hipMemsetAsync(&qc->ext[1 - cur], 0, 4, sc->stream));
        record(cur, round == 0, n);
        HIP_TRY(hipGetLastError());
        if (!sc->has_null_material) break;   // every hit carries a material: nothing goes on, no count to wait for
        QCounters h;
        if (int st = sync_queue_counters(sc, h)) return st;
        n = h.ext[1 - cur];
    }
    return PT_OK;
}

}  // namespace ptside
using namespace ptside;
