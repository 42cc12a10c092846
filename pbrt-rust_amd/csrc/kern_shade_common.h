// kern_shade_common.h -- what the kernels that finish a path vertex share (kern_shade.h, kern_bssrdf.h, kern_aux.h): region timers, resolve_pending / vol_chain_step / nee_vertex,
// the vertex frame (LDS queue set, roulette, meta word, escaped-ray Le, histogram + epilogue), textured material parameters, camera-ray differentials.
#pragma once
#include "kern_common.h"
// ---- shading ---------------------------------------------------------------------------------------------

// ---- optional region timers (build with -DPT_REGION_PROFILE): wave time between markers is charged to the region of the
// previous marker; one lane per wave updates three LDS words. Printed by the host when the scene is destroyed.
// PT_PROF_BEGIN: a kernel's timer state (`prof`, handed on to the helpers with PT_PROF_PASS); PT_PROF_END(counters): the block's sums go to counters->regions
// (k_shade only: the region table is k_shade's, the other kernels keep their timers to themselves).
#ifdef PT_REGION_PROFILE
struct Prof { long long *t; int *r; unsigned long long *acc; };
#define PT_PROF_BEGIN __shared__ long long s_pt[4]; __shared__ int s_pr[4]; __shared__ unsigned long long s_pacc[64]; \
    if (threadIdx.x < 64) s_pacc[threadIdx.x] = 0; \
    if (threadIdx.x < 4) { s_pt[threadIdx.x] = clock64(); s_pr[threadIdx.x] = 15; } \
    Prof prof{s_pt, s_pr, s_pacc};
#define PT_PROF_END(counters) do { PT_T(14); __syncthreads(); \
    if (threadIdx.x < 16) atomicAdd(&(counters)->regions[threadIdx.x], prof.acc[threadIdx.x] + prof.acc[16 + threadIdx.x] + prof.acc[32 + threadIdx.x] + prof.acc[48 + threadIdx.x]); } while (0)
#define PT_T(k) do { if ((int)__lane_id() == __ffsll((unsigned long long)__ballot(1)) - 1) { const long long _n = clock64(); const int _w = threadIdx.x >> 6; \
    prof.acc[_w * 16 + prof.r[_w]] += (unsigned long long)(_n - prof.t[_w]); prof.t[_w] = _n; prof.r[_w] = (k); } } while (0)
#define PT_PROF_ARG , Prof prof
#define PT_PROF_PASS , prof
#else
#define PT_T(k) do {} while (0)
#define PT_PROF_BEGIN
#define PT_PROF_END(counters) do {} while (0)
#define PT_PROF_ARG
#define PT_PROF_PASS
#endif

// Resolve the pending next-event estimation of the previous vertex once its shadow / MIS rays are traced
// (integrator.rs:150-171,199-233): L += beta_at_nee * Ld / choice_pdf.
// Grid media (VOL, DeviceScene::has_grid): the transmittance of the shadow ray and of the MIS ray is a ratio-tracking estimate that
// draws sampler dimensions (grid.rs:113-147), in the reference right after the vertex's light / scattering samples and before its
// continuation sample. Such vertices are therefore resolved in a second stage of the SAME vertex (PF_STAGE_B, kern_shade.h) and pass
// their sampler here; `smp` is NULL everywhere else.
// n_assert: the reference's `assert!(Ld.y() >= 0.0)` (path.rs:143) on the regular vertices' estimate, counted instead of panicking.
// EARLY (k_film_final): the MIS record is requested together with the NEE record, before either is used -- one round trip instead of two in a kernel whose threads walk
// their samples one after the other (the shade kernels keep the later request: batching their front cost registers and time, profiles/r4/NOTES.md).
template <bool SPH, bool VOL = false, bool EARLY = false> PT_DEV void resolve_pending(const DeviceScene &s, const PathSoA &ps, uint32_t pid, uint32_t &flags, RGB &L,
                                                unsigned long long &zero_num, uint32_t &n_assert, unsigned long long &n_bytes PT_PROF_ARG, Sampler *smp = nullptr) {
    if (!(flags & (PF_PEND_SHADOW | PF_PEND_MIS))) return;
    PT_T(1);
    // the pending records as whole quads: nee {sh_d.yz, occluded | sh_prim, nee_light} {A, choice_pdf} {nb, shadow grid medium}; mis {o, d.x} {d.yz, w, spdf} {prim, b} {f, t}
    const float4 *nq = reinterpret_cast<const float4 *>(ps.nee) + 4 * (size_t)pid;
    const float4 n1 = nq[1], n2 = nq[2], n3 = nq[3];
    float4 e0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), e1 = e0, e2 = e0, e3 = e0;
    if constexpr (EARLY) {
        if (flags & PF_PEND_MIS) { const float4 *mq = reinterpret_cast<const float4 *>(ps.mis) + 4 * (size_t)pid; e0 = mq[0]; e1 = mq[1]; e2 = mq[2]; e3 = mq[3]; }
        asm volatile("" :: "v"(n1.x), "v"(n2.x), "v"(n3.x), "v"(e0.x), "v"(e1.x), "v"(e2.x), "v"(e3.x));
    }
    n_bytes += 48 + ((flags & PF_PEND_MIS) ? 64 : 0);
    RGB Ld(0.0f);
    const uint32_t li = __float_as_uint(n1.w);
    // volpath: VisibilityTester::tr intersects (closest hit) and every surface is opaque; the segment's transmittance is already in A
    if ((flags & PF_PEND_SHADOW) && (VOL ? __float_as_uint(n1.z) == PT_NONE : __float_as_uint(n1.z) == 0u)) {
        RGB A(n2.x, n2.y, n2.z);
        if (VOL) {   // VisibilityTester::tr (light.rs:125-150) through a grid medium: estimated now (homogeneous media were folded into A at the vertex)
            const uint32_t sm = __float_as_uint(n3.w);
            if (sm != PT_NONE && s.media[sm].type == PT_MEDIUM_GRID) {
                const float4 n0 = nq[0];
                if (smp) A = A * grid_tr(s.media[sm], s.grid_aux[sm], V3(n0.x, n0.y, n0.z), V3(n0.w, n1.x, n1.y), 1.0f - kShadowEps, *smp);
                else A = RGB(0.0f);
            }
        }
        Ld = Ld + A;
    }
    if (flags & PF_PEND_MIS) {
        const float4 *mq = reinterpret_cast<const float4 *>(ps.mis) + 4 * (size_t)pid;
        const float4 m0 = EARLY ? e0 : mq[0], m1 = EARLY ? e1 : mq[1], m2 = EARLY ? e2 : mq[2], m3 = EARLY ? e3 : mq[3];
        V3 wi(m0.w, m1.x, m1.y);
        RGB lrad(0.0f);
        const uint32_t mp = __float_as_uint(m2.x);
        if (mp != PT_NONE) {
            if (s.prim_light[mp] == li) {  // Arc::ptr_eq(light), integrator.rs:222-228
                SurfaceInteraction lsi;
                fill_hit<SPH>(s, mp, PT_NONE, V3(m0.x, m0.y, m0.z), wi, m2.y, m2.z, m2.w, lsi);  // lights are never inside instances (api.rs:1605-1608)
                lrad = area_l_rec(s, li, lsi.n, -wi);   // Lemit / two_sided from the light's record, not from a PtLight gather
            }
        } else { PT_T(2); lrad = light_le(s, li, wi); PT_T(1); }
        RGB Tr(1.0f);
        bool tr_done = false;
        if (VOL) {   // Scene::intersect_tr (scene.rs:68-87) always evaluates the medium's tr -- a grid medium draws its dimensions whether or not the light is seen
            const uint32_t mm = ps.mis_medium(pid);
            if (mm != PT_NONE && s.media[mm].type == PT_MEDIUM_GRID) {
                Tr = smp ? RGB(grid_tr(s.media[mm], s.grid_aux[mm], V3(m0.x, m0.y, m0.z), wi, mp != PT_NONE ? m3.w : PT_INF, *smp)) : RGB(0.0f);
                tr_done = true;
            }
        }
        if (!lrad.is_black()) {
            RGB f(m3.x, m3.y, m3.z);
            if (VOL && !tr_done) {   // homogeneous: analytic transmittance of the MIS ray's medium up to its hit (or to infinity)
                const uint32_t mm = ps.mis_medium(pid);
                if (mm != PT_NONE) Tr = Tr * medium_tr(s.media[mm], mp != PT_NONE ? m3.w : PT_INF, wi);
            }
            Ld = Ld + f * lrad * Tr * m1.z / m1.w;
        }
    }
    RGB nb(n3.x, n3.y, n3.z);
    RGB Ldb = nb * (Ld / n2.w);
    if (!VOL && Ldb.is_black() && !(flags & PF_NEE_UNCOUNTED)) zero_num++;   // path.rs:142 counts only the regular vertices' NEE
    if (!VOL && !(flags & PF_NEE_UNCOUNTED) && !(Ldb.y() >= 0.0f)) n_assert++;   // path.rs:143 (a NaN estimate fails it too)
    L = L + Ldb;
    flags &= ~(PF_PEND_SHADOW | PF_PEND_MIS | PF_NEE_UNCOUNTED);
}

// Volpath in a scene with material-less shells (`Material "none"` + MediumInterface: how a .pbrt file bounds a medium, api.rs:597). The
// transmittance of a shadow ray is VisibilityTester::tr (light.rs:125-150) and that of a MIS ray Scene::intersect_tr (scene.rs:68-87): LOOPS
// that intersect, multiply the segment's medium transmittance in, and go on behind every surface that has no material. A wavefront
// vertex walks them one traced segment per iteration while it waits in stage B: first the whole shadow chain, then the MIS chain -- the
// order in which the reference draws the ratio-tracking dimensions of grid media (integrator.rs:150-156 before :207-216). The traced
// segment's full hit record is in the path's ext record; a shell hit spawns the next segment (push_shadow / push_mis: the caller keeps
// the path in stage B). Returns true while a chain goes on. When both have ended the nee / mis records are left as a plain, fully
// attenuated estimate (media NONE, the final MIS hit in the mis record) for resolve_pending to sum.
template <bool SPH> PT_DEV bool vol_chain_step(const DeviceScene &s, const PathSoA &ps, uint32_t pid, uint32_t flags, Sampler &smp, bool &push_shadow, bool &push_mis,
                                              unsigned long long &n_bytes) {
    float4 *nq = reinterpret_cast<float4 *>(ps.nee) + 4 * (size_t)pid;
    float4 *mq = reinterpret_cast<float4 *>(ps.mis) + 4 * (size_t)pid;
    float4 *xq = reinterpret_cast<float4 *>(ps.ext) + 8 * (size_t)pid;
    if ((flags & PF_PEND_SHADOW) && __float_as_uint(nq[1].z) != 1u) {   // nee word 6: 1 = the shadow chain has ended (A is final); the traced prim lives in ext
        const float4 n0 = nq[0], n1 = nq[1], n2 = nq[2], n3 = nq[3], h0 = xq[4], h1 = xq[5];
        n_bytes += 64 + 32;
        const uint32_t prim = __float_as_uint(h0.x), sm = __float_as_uint(n3.w);
        const bool hit = prim != PT_NONE;
        const V3 so(n0.x, n0.y, n0.z), sd(n0.w, n1.x, n1.y);
        RGB A(n2.x, n2.y, n2.z);
        bool ended = true;
        if (hit && s.prim_material[prim] != PT_NONE) A = RGB(0.0f);   // light.rs:136-138: an opaque surface, `return Spectrum::new(0.0)` -- before the segment's medium is asked
        else {
            if (sm != PT_NONE) {   // light.rs:141-143: Tr *= ray.medium.tr(ray, sampler), the segment ends at its hit (ray.t_max)
                const float t_seg = hit ? h1.y : 1.0f - kShadowEps;
                A = A * (s.media[sm].type == PT_MEDIUM_GRID ? RGB(grid_tr(s.media[sm], s.grid_aux[sm], so, sd, t_seg, smp)) : medium_tr(s.media[sm], t_seg, sd));
            }
            if (hit) {   // light.rs:146-147: ray = isect.spawn_rayto_interaction(p1)
                SurfaceInteraction hs;
                fill_hit_pkt<SPH>(s, __float_as_uint(h1.z), SPH ? __float_as_uint(h1.x) : PT_NONE, so, sd, h0.y, h0.z, h0.w, hs);
                IData a; a.p = hs.p; a.p_error = hs.p_error; a.n = hs.n;
                IData b; { const float4 x0 = xq[0], x1 = xq[1], x2 = xq[2]; b.p = V3(x0.x, x0.y, x0.z); b.p_error = V3(x1.x, x1.y, x1.z); b.n = V3(x2.x, x2.y, x2.z); }
                V3 o2, d2; spawn_ray_to(a, b, o2, d2);
                const uint32_t sm2 = medium_toward(surface_iface(s, prim, sm), hs.n, d2);   // interaction.rs:54-66 get_medium(d) of the shell's MediumInterface (primitive.rs:139-145)
                nq[0] = make_float4(o2.x, o2.y, o2.z, d2.x); nq[1] = make_float4(d2.y, d2.z, 0.0f, n1.w); nq[3] = make_float4(n3.x, n3.y, n3.z, __uint_as_float(sm2));
                push_shadow = true; ended = false; n_bytes += 48 + 4;
            }
        }
        nq[2] = make_float4(A.r, A.g, A.b, n2.w);
        if (!ended) return true;
        nq[1] = make_float4(n1.x, n1.y, __uint_as_float(1u), n1.w);
    }
    if (flags & PF_PEND_MIS) {
        const float4 m0 = mq[0], m1 = mq[1], m3 = mq[3], h0 = xq[6], h1 = xq[7];
        n_bytes += 64 + 32;
        const uint32_t prim = __float_as_uint(h0.x), mm = ps.mis_medium(pid);
        const bool hit = prim != PT_NONE;
        const V3 mo(m0.x, m0.y, m0.z), wi(m0.w, m1.x, m1.y);
        RGB f(m3.x, m3.y, m3.z);
        // scene.rs:76-79: *tr *= ray.medium.tr(ray, sampler) -- always, whatever the segment ends at
        if (mm != PT_NONE) f = f * (s.media[mm].type == PT_MEDIUM_GRID ? RGB(grid_tr(s.media[mm], s.grid_aux[mm], mo, wi, hit ? h1.y : PT_INF, smp)) : medium_tr(s.media[mm], hit ? h1.y : PT_INF, wi));
        if (hit && s.prim_material[prim] == PT_NONE) {   // scene.rs:84: ray = isect.spawn_ray(ray.d)
            SurfaceInteraction hs;
            fill_hit_pkt<SPH>(s, __float_as_uint(h1.z), SPH ? __float_as_uint(h1.x) : PT_NONE, mo, wi, h0.y, h0.z, h0.w, hs);
            IData a; a.p = hs.p; a.p_error = hs.p_error; a.n = hs.n;
            V3 o2; spawn_ray(a, wi, o2);
            ps.mis_medium(pid) = medium_toward(surface_iface(s, prim, mm), hs.n, wi);
            mq[0] = make_float4(o2.x, o2.y, o2.z, wi.x); mq[3] = make_float4(f.r, f.g, f.b, m3.w);
            push_mis = true; n_bytes += 32 + 4;
            return true;
        }
        // the chain has ended at an opaque surface or escaped: leave the record as resolve_pending reads it
        mq[2] = h0; mq[3] = make_float4(f.r, f.g, f.b, hit ? h1.y : 0.0f);
        ps.mis_medium(pid) = PT_NONE;
    }
    if (flags & PF_PEND_SHADOW) {   // the summed form: "unoccluded" with the fully attenuated (or zeroed) term, no medium left to ask
        const float4 n1 = nq[1], n3 = nq[3];
        nq[1] = make_float4(n1.x, n1.y, __uint_as_float(PT_NONE), n1.w); nq[3] = make_float4(n3.x, n3.y, n3.z, __uint_as_float(PT_NONE));
    }
    return false;
}

// ---- the vertex frame: what k_shade, k_bssrdf (kern_bssrdf.h) and k_shade_medium (kern_aux.h) share around the vertex itself -- a surface hit, a subsurface exit point,
// a medium event. Each keeps its persistent loop and its record loads / stores written out (k_shade moves the core record as whole quads, the other two by field), and
// the steps that moved a kernel's register count when they were shared (profiles/r6/NOTES.md section 12): "resolve the pending estimate, or walk a shell segment in stage B" and
// "the path ends: dead with an estimate pending, or finished" in all three, the roulette in k_shade.

// The block's LDS queues (kern_common.h: LdsQueue) in front of the job's global ones: continuation rays (what k_route reads), resolve-only paths (to the miss class), the ray
// queue (kernels.h: kRayKindShift -- every ray of the vertex, tagged with its kind, the continuation ray once more: what the mixed trace launch reads), and where the kernel
// has them (one-entry stubs where not) probe chains (PROBE) and vertices waiting for stage B (SELF). Written against the field names ShadeJob and BssrdfJob share.
template <int QCAP, bool PROBE, bool SELF> struct VertexQueues {
    // `rays` lives in the LDS bytes the separate shadow and MIS queues took; it holds at least one round's worth, three entries per thread (the QCAP = 256 form: 768)
    static constexpr int kRayCap = 2 * QCAP > 768 ? 2 * QCAP : 768;
    LdsQueue<QCAP> ext, res;
    LdsQueue<kRayCap> rays;
    LdsQueue<PROBE ? QCAP : 1> probe;
    LdsQueue<SELF ? QCAP : 1> self;
    PT_DEV void init() { lq_init(ext); lq_init(res); lq_init(rays); lq_init(probe); lq_init(self); }
    // A lane's 0-3 rays as CONSECUTIVE entries in kind order (continuation, MIS, shadow) at the lane's prefix: three ballots, one LDS atomic of the wave's leader.
    PT_DEV void push_rays(uint32_t pid, bool to_ext, bool to_mis, bool to_shadow) {
        const unsigned long long m_e = __ballot(to_ext), m_m = __ballot(to_mis), m_s = __ballot(to_shadow), any = m_e | m_m | m_s;
        if (any == 0ull) return;
        const uint32_t lane = lane_id(), leader = (uint32_t)__ffsll((long long)any) - 1u;
        const unsigned long long below = (1ull << lane) - 1ull;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&rays.count, (uint32_t)(__popcll(m_e) + __popcll(m_m) + __popcll(m_s)));
        base = __shfl(base, (int)leader);
        uint32_t at = base + (uint32_t)(__popcll(m_e & below) + __popcll(m_m & below) + __popcll(m_s & below));
        if (to_ext) rays.buf[at++] = pid;
        if (to_mis) rays.buf[at++] = pid | (1u << kRayKindShift);
        if (to_shadow) rays.buf[at] = pid | (2u << kRayKindShift);
    }
    // where a finished vertex goes next (the kernels keep these flags as plain bools: as members of one struct they cost several k_shade forms a register)
    template <class Job> PT_DEV void push(const Job &job, uint32_t pid, bool to_ext, bool to_resolve, bool to_shadow, bool to_mis, bool to_self = false, bool to_probe = false) {
        lq_push(ext, pid, to_ext);   // (grouped by the new ray's direction octant: trace no faster -- profiles/HISTORY.md; profiles/r6/experiments/settled_ab_hooks.patch)
        lq_push(res, pid, to_resolve && job.shade_next0 != nullptr);   // (no miss pass: the film kernel ends the dead paths, k_film_final; k_shade_medium pushed without this test: volpath always has the miss pass)
        push_rays(pid, to_ext, to_mis, to_shadow);
        if constexpr (PROBE) if (job.probe_next) lq_push(probe, pid, to_probe);
        if constexpr (SELF) lq_push(self, pid, to_self);
    }
    // One flush round, all threads of the block together: a barrier makes the pushes visible, every queue with fewer than `reserve` free slots (or any entry, `force`) goes to
    // its global queue, a barrier closes the round. In the loop: (256, false) after each round's pushes; after it: (0, true). `reserve` counts threads: the ray queue
    // keeps three entries for each.
    template <class Job> PT_DEV void flush(const Job &job, uint32_t reserve, bool force) {
        __syncthreads();
        lq_flush_nosync(ext, job.ext_next_count, job.ext_next, reserve, force);
        lq_flush_nosync(res, job.shade_next0_count, job.shade_next0, reserve, force);
        lq_flush_nosync(rays, job.rays_count, job.rays, 3u * reserve, force);
        if constexpr (PROBE) if (job.probe_next) lq_flush_nosync(probe, job.probe_next_count, job.probe_next, reserve, force);
        if constexpr (SELF) lq_flush_nosync(self, job.self_next_count, job.self_next, reserve, force);
        __syncthreads();
    }
};

// Russian roulette (path.rs:206-214, volpath.rs:171-176, 223): true when the path is killed, else beta is rescaled.
PT_DEV bool russian_roulette(const RenderConst &rc, Sampler &smp, RGB &beta, float etascale, uint32_t bounces, uint32_t &n_assert) {
    const RGB rrbeta = beta * etascale;
    if (rrbeta.max_component_value() < rc.rr_threshold && bounces > 3) {
        const float q = maxf(1.0f - rrbeta.max_component_value(), 0.05f);
        if (smp.get_1d() < q) return true;
        beta = beta / (1.0f - q); if (__builtin_isinf(beta.y())) n_assert++;   // path.rs:213, volpath.rs:223
    }
    return false;
}

// The meta word a vertex leaves: the sampler's next dimension, the bounce count, the path flags; and the Sobol' table's end, reported once per job.
PT_DEV uint32_t vertex_meta(const Sampler &smp, uint32_t bounces, uint32_t flags, uint32_t *error) {
    if (smp.overflow) atomicMax(error, (uint32_t)PT_ERR_SOBOL_DIMENSIONS);
    return (smp.dim & 0xffffu) | ((bounces & 0xffu) << 16) | (flags << 24);
}
// ... with L and beta, field by field (k_bssrdf, k_shade_medium)
PT_DEV void store_vertex(const PathSoA &ps, uint32_t pid, RGB L, RGB beta, const Sampler &smp, uint32_t bounces, uint32_t flags, uint32_t *error) {
    const uint32_t meta = vertex_meta(smp, bounces, flags, error);
    ps.L_r(pid) = L.r; ps.L_g(pid) = L.g; ps.L_b(pid) = L.b;
    ps.beta_r(pid) = beta.r; ps.beta_g(pid) = beta.g; ps.beta_b(pid) = beta.b;
    ps.meta(pid) = meta;
}

// path.rs:106-117, the ray escaped: the infinite lights' Le along it.
PT_DEV void add_escaped_le(const DeviceScene &s, V3 rd, RGB beta, RGB &L) {
    for (uint32_t k = 0; k < s.n_infinite; ++k) L = L + light_le_infinite(s, s.infinite_lights[k], rd) * beta;
}

// The block's path-length histogram (path.rs:219) in LDS, and the end of a kernel that finishes vertices: histogram and the thread's tallies to the job's counters. `items` /
// `bytes`: the launch kind's work counters (zero_num / zero_den: the kernels that count them add them beside the call). Call block-convergent, after the barrier that follows the last hist_add.
PT_DEV void hist_init(uint32_t *s_hist) { if (threadIdx.x < 16) s_hist[threadIdx.x] = 0; }
PT_DEV void hist_add(uint32_t *s_hist, uint32_t bounces) { atomicAdd(&s_hist[bounces > 15u ? 15u : bounces], 1u); }
PT_DEV void vertex_epilogue(const uint32_t *s_hist, DevCounters *c, unsigned long long *items, unsigned long long *bytes, unsigned long long n_valid, unsigned long long n_bytes,
                            uint32_t n_assert) {
    if (threadIdx.x < 16 && s_hist[threadIdx.x]) atomicAdd(&c->path_len[threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
    counter_add(&c->ref_asserts, (unsigned long long)n_assert);
    counter_add(&c->stages, n_valid);
    counter_add(items, n_valid);
    counter_add(bytes, n_bytes);
}

// uniform_sample_onelight + estimate_direct (integrator.rs:81-237) at one vertex: samples the light and the BSDF,
// records the shadow / MIS rays and their weights in the path state; the estimate is summed by resolve_pending once
// both rays are traced. Returns whether anything is pending (false: Ld is black).
// VOL: estimate_direct with handle_media (integrator.rs:150-156,207-216) -- `mif` is the vertex's MediumInterface; MEDIUM: the
// vertex is a MediumInteraction (f = phase value, no cosine; si carries only p and wo).
template <bool SPH, class B, bool VOL = false, bool MEDIUM = false>
PT_DEV bool nee_vertex(const DeviceScene &s, const LightGrid &grid, const PathSoA &ps, uint32_t pid, Sampler &smp,
                                          const SurfaceInteraction &si, const IData &it, const B &bsdf, RGB beta, uint32_t &flags,
                                          bool &push_shadow, bool &push_mis, unsigned long long &n_bytes PT_PROF_ARG, MedIface mif = MedIface{PT_NONE, PT_NONE}) {
    bool nee_pending = false;
    if (s.n_lights > 0) {
        PT_T(5);
        Dist1D distrib = light_distribution_lookup(grid, s, si.p);
        float choice_pdf = 0.0f;
        const uint32_t li = (uint32_t)dist_sample_discrete(distrib, smp.get_1d(), choice_pdf);
        if (choice_pdf != 0.0f) {
            const P2 ulight = smp.get_2d();
            const P2 uscatt = smp.get_2d();
            // estimate_direct (integrator.rs:109-237), flags = All & !Specular
            const int bf = BSDF_ALL & ~BSDF_SPECULAR;
            V3 wi; float lightpdf = 0.0f, scattpdf = 0.0f; IData p1;
            RGB A(0.0f); V3 sh_o(0.0f, 0.0f, 0.0f), sh_d(0.0f, 0.0f, 0.0f);   // the shadow ray and its term, stored with the rest of the nee record below
            uint32_t sh_medium = PT_NONE;                                       // VOL: a grid medium the shadow ray travels in
            PT_T(6);
            uint32_t lhead;   // the light's record header: its delta bit comes with the record light_sample_li reads anyway
            RGB Li = light_sample_li_rec<SPH>(s, li, it, ulight, wi, lightpdf, p1, lhead);
            PT_T(7);
            const bool delta = head_is_delta(lhead);
            if (lightpdf > 0.0f && !Li.is_black()) {
                RGB f = bsdf.f_pdf(si.wo, wi, bf, scattpdf);
                if (!MEDIUM) f = f * abs_dot(wi, si.sh_n);
                if (!f.is_black()) {
                    V3 so, sd; spawn_ray_to(it, p1, so, sd);
                    if (VOL) {   // Li *= visibility.tr(): the unoccluded segment's transmittance (light.rs:125-150)
                        const uint32_t sm = medium_toward(mif, it.n, sd);
                        if (s.has_shells) {   // the segment may end at a shell: every segment's transmittance is taken when it has been traced (vol_chain_step)
                            sh_medium = sm;
                            float4 *xq = reinterpret_cast<float4 *>(ps.ext) + 8 * (size_t)pid;
                            xq[0] = make_float4(p1.p.x, p1.p.y, p1.p.z, 0.0f); xq[1] = make_float4(p1.p_error.x, p1.p_error.y, p1.p_error.z, 0.0f); xq[2] = make_float4(p1.n.x, p1.n.y, p1.n.z, 0.0f);
                            n_bytes += 48;
                        }
                        else if (sm != PT_NONE && s.media[sm].type == PT_MEDIUM_GRID) sh_medium = sm;   // estimated when the shadow ray has been traced (resolve_pending)
                        else if (sm != PT_NONE) Li = Li * medium_tr(s.media[sm], 1.0f - kShadowEps, sd);
                    }
                    A = delta ? f * Li / lightpdf : f * Li * power_heuristic(lightpdf, scattpdf) / lightpdf;
                    sh_o = so; sh_d = sd;
                    flags |= PF_PEND_SHADOW; push_shadow = true; nee_pending = true; n_bytes += 16 + 4;   // first quad of the nee record + the shadow queue entry
                }
            }
            if (!delta) {
                PT_T(8);
                int sampled_type = 0;
                RGB f = bsdf.sample_f(si.wo, wi, uscatt, scattpdf, bf, sampled_type);
                if (!MEDIUM) f = f * abs_dot(wi, si.sh_n);
                const bool sampled_specular = (sampled_type & BSDF_SPECULAR) != 0;
                if (!f.is_black() && scattpdf > 0.0f) {
                    float weight = 1.0f;
                    bool skip = false;
                    if (!sampled_specular) {
                        PT_T(9);
                        lightpdf = light_pdf_li<SPH>(s, li, it, wi);
                        PT_T(8);
                        if (lightpdf == 0.0f) skip = true;  // `return Ld` (integrator.rs:204)
                        else weight = power_heuristic(scattpdf, lightpdf);
                    }
                    if (!skip) {
                        V3 mo; spawn_ray(it, wi, mo);
                        float4 *mq = reinterpret_cast<float4 *>(ps.mis) + 4 * (size_t)pid;   // {o, d.x} {d.yz, w, spdf} . {f, -}; the third quad is the MIS ray's hit (k_trace)
                        mq[0] = make_float4(mo.x, mo.y, mo.z, wi.x); mq[1] = make_float4(wi.y, wi.z, weight, scattpdf); mq[3] = make_float4(f.r, f.g, f.b, 0.0f);
                        if (VOL) ps.mis_medium(pid) = medium_toward(mif, it.n, wi);
                        flags |= PF_PEND_MIS; push_mis = true; nee_pending = true; n_bytes += 48 + 4;
                    }
                }
            }
            if (nee_pending) {   // the nee record {sh_o, sh_d.x} {sh_d.yz, occluded (k_trace), nee_light} {A, choice_pdf} {nb, -}
                float4 *nq = reinterpret_cast<float4 *>(ps.nee) + 4 * (size_t)pid;
                if (flags & PF_PEND_SHADOW) nq[0] = make_float4(sh_o.x, sh_o.y, sh_o.z, sh_d.x);
                nq[1] = make_float4(sh_d.y, sh_d.z, 0.0f, __uint_as_float(li)); nq[2] = make_float4(A.r, A.g, A.b, choice_pdf); nq[3] = make_float4(beta.r, beta.g, beta.b, __uint_as_float(sh_medium));
                n_bytes += 48;
            }
        }
    }
    return nee_pending;
}

// ---- textured material parameters (8f-1) ---------------------------------------------------------------------
struct TexMatEval {
    const DeviceScene &s; const TexCtx &c;
    // MixMaterial evaluates its second material on a fresh SurfaceInteraction (mix.rs:31-36): same p / uv, no differentials
    struct Plain {
        const DeviceScene &s; TexCtx c;
        PT_DEV bool bound(const PtMaterial &m, int slot) const { return m.tex[slot] >= 0; }
        PT_DEV RGB spec(const PtMaterial &m, int slot, const float *field) const { return m.tex[slot] >= 0 ? tex_eval(s, m.tex[slot], c) : RGB(field[0], field[1], field[2]); }
        PT_DEV float flt(const PtMaterial &m, int slot, float field) const { return m.tex[slot] >= 0 ? tex_eval(s, m.tex[slot], c).r : field; }
    };
    PT_DEV Plain plain() const { Plain q{s, c}; q.c.dpdx = V3(0.0f, 0.0f, 0.0f); q.c.dpdy = V3(0.0f, 0.0f, 0.0f); q.c.dudx = q.c.dvdx = q.c.dudy = q.c.dvdy = 0.0f; return q; }
    PT_DEV bool bound(const PtMaterial &m, int slot) const { return m.tex[slot] >= 0; }
    PT_DEV RGB spec(const PtMaterial &m, int slot, const float *field) const { return m.tex[slot] >= 0 ? tex_eval(s, m.tex[slot], c) : RGB(field[0], field[1], field[2]); }
    PT_DEV float flt(const PtMaterial &m, int slot, float field) const { return m.tex[slot] >= 0 ? tex_eval(s, m.tex[slot], c).r : field; }
};
// The auxiliary rays of the camera's generate_ray_differential after transform_ray (transform.rs:565-575: no error offset on the auxiliary
// origins) and Ray::scale_differential(1 / sqrt(spp)) (ray.rs:34-41, integrator.rs:340), recomputed from the film position (and the lens
// sample, dimensions 3 and 4) instead of being carried in the path state. rc.camera_type is uniform over the launch; the code runs in the
// textured variants only, on camera rays.
//   perspective (perspective.rs:143-176)   as before
//   orthographic (orthographic.rs:123-152) no lens: both auxiliary origins are the main one shifted by dx_camera / dy_camera, both directions the main one.
//       With a lens both origins are the lens point and the directions aim at pcamera + d{x,y}_camera + (0,0,z) * ft, where ft is taken from the ALREADY
//       lens-modified direction's z (:130) and z is 1 for x but 0.1 for y (:135, as written there). Reproduced, not corrected.
//   environment   none: EnvironmentCamera has no generate_ray_differential; the trait's default (core/camera.rs:43-97) writes into rd.diff only when
//       generate_ray left one there, and it leaves None. has = false: the first vertex filters its textures as every later one does.
PT_DEV RayDiff camera_ray_differentials(const RenderConst &rc, float pfx, float pfy, P2 plens_u, V3 ray_o, V3 ray_d) {
    RayDiff d; d.has = true;
    if (rc.camera_type == PT_CAMERA_ENVIRONMENT) {
        d.has = false;
        d.rx_o = d.rx_d = d.ry_o = d.ry_d = V3(0.0f, 0.0f, 0.0f);
        return d;
    }
    const V3 pcamera = xf_point(rc.raster_to_camera, V3(pfx, pfy, 0.0f));
    const V3 dxc(rc.dx_camera[0], rc.dx_camera[1], rc.dx_camera[2]), dyc(rc.dy_camera[0], rc.dy_camera[1], rc.dy_camera[2]);
    if (rc.camera_type == PT_CAMERA_ORTHOGRAPHIC) {
        if (rc.lens_radius > 0.0f) {
            const P2 dk = concentric_sample_disk(plens_u);
            const V3 plens(dk.x * rc.lens_radius, dk.y * rc.lens_radius, 0.0f);
            // the main ray's direction as generate_ray_differential has it by then (orthographic.rs:109-121)
            const V3 pf0 = pcamera + V3(0.0f, 0.0f, 1.0f) * (rc.focal_distance / 1.0f);
            const V3 dmain = normalize(pf0 - plens);
            const float ft = rc.focal_distance / dmain.z;                          // orthographic.rs:130
            V3 pfocus = pcamera + dxc + V3(0.0f, 0.0f, 1.0f) * ft;                 // orthographic.rs:131
            d.rx_o = plens; d.rx_d = normalize(pfocus - plens);
            pfocus = pcamera + dyc + V3(0.0f, 0.0f, 0.1f) * ft;                    // orthographic.rs:135
            d.ry_o = plens; d.ry_d = normalize(pfocus - plens);
        } else {
            d.rx_o = pcamera + dxc; d.ry_o = pcamera + dyc;                        // orthographic.rs:140-143
            d.rx_d = V3(0.0f, 0.0f, 1.0f); d.ry_d = V3(0.0f, 0.0f, 1.0f);
        }
    } else if (rc.lens_radius > 0.0f) {
        const P2 dk = concentric_sample_disk(plens_u);
        const float lx = dk.x * rc.lens_radius, ly = dk.y * rc.lens_radius;
        const V3 dx = normalize(pcamera + dxc);
        float ft = rc.focal_distance / dx.z;
        V3 pfocus = V3(0.0f, 0.0f, 0.0f) + (dx * ft);
        d.rx_o = V3(lx, ly, 0.0f); d.rx_d = normalize(pfocus - d.rx_o);
        const V3 dy = normalize(pcamera + dyc);
        ft = rc.focal_distance / dy.z;
        pfocus = V3(0.0f, 0.0f, 0.0f) + (dy * ft);
        d.ry_o = V3(lx, ly, 0.0f); d.ry_d = normalize(pfocus - d.ry_o);
    } else {
        d.rx_o = V3(0.0f, 0.0f, 0.0f); d.ry_o = V3(0.0f, 0.0f, 0.0f);
        d.rx_d = normalize(pcamera + dxc); d.ry_d = normalize(pcamera + dyc);
    }
    d.rx_o = xf_point(rc.camera_to_world, d.rx_o); d.ry_o = xf_point(rc.camera_to_world, d.ry_o);
    d.rx_d = xf_vector(rc.camera_to_world, d.rx_d); d.ry_d = xf_vector(rc.camera_to_world, d.ry_d);
    const float sc = rc.inv_sqrt_spp;
    d.rx_o = ray_o + (d.rx_o - ray_o) * sc; d.ry_o = ray_o + (d.ry_o - ray_o) * sc;
    d.rx_d = ray_d + (d.rx_d - ray_d) * sc; d.ry_d = ray_d + (d.ry_d - ray_d) * sc;
    return d;
}
