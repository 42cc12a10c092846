// render_loop.hip -- the wavefront scheduler behind pt_render: workspace, light grids, launches, one pass, counters (host_common.h has the map).
#include "host_common.h"
#include <utility>

// Blocks per CU of the persistent grids (knobs.h: PT_*_BLOCKS_PER_CU).
//   k_shade 24: each block walks a fixed stride of the queue: 24 a CU (2, 3 or 4 resident at a time) even out the per-vertex cost differences; 8 left the matte kernel's third round two-thirds full (80.1 -> 76.3 ms on C2)
//   k_generate 40: 16 -> 40: k_generate 12.2 -> 11.7 ms on C2; the miss kernel does not care
//   k_route 3: what a CU's LDS holds of k_route (six 8 KB staging queues per block)

namespace pth {
#ifdef PT_TRACE_UTIL
__global__ void k_trace_util_fold(DevCounters *dc, uint32_t kind, uint32_t waves, int reset) {   // per launch: span x waves, then re-arm min / max
    if (!reset) dc->tail[5 + 2 * kind] += (dc->tail[1] - dc->tail[0]) * waves;
    dc->tail[0] = ~0ull; dc->tail[1] = 0ull;
}
#endif

// ---- kernel variants. A Variant is one instantiation of a kernel template and the symbol rocprofv3 prints for it, both made from the SAME template arguments (the
// symbol is a key: bench.py looks the kernel's PMC record up by it, tests assert it). The run-time conditions pick a variant once; launch() takes function and name from it.
template <class... P> struct Variant { void (*fn)(P...); std::string name; };
static std::string targ(bool b) { return b ? "true" : "false"; }
static std::string targ(int v) { return std::to_string(v); }
template <class... T> std::string symbol(const char *kernel, T... args) { std::string s = std::string(kernel) + "<", sep; ((s += sep + targ(args), sep = ", "), ...); return s + ">"; }

// (launch(sc, name, fn, ...): host_common.h)
template <class... P, class... A> void launch(pt_scene *sc, const Variant<P...> &v, dim3 blocks, dim3 threads, const A &...args) { launch(sc, v.name, v.fn, blocks, threads, args...); }
// TEST HOOK (env PT_TEST_MAX_BLOCKS, read at every render call like PT_TEST_MAX_ITERATIONS, by the thread that launches): a cap on the persistent grids. A persistent kernel's
// result may not depend on its grid, and under a cap of 1 the one block makes many rounds on a tiny render -- the mid-loop queue flushes (kern_shade_common.h: VertexQueues::flush) at test size.
static thread_local uint32_t t_max_blocks = ~0u;
dim3 blocks_for(uint32_t n_upper, uint32_t per_cu) { return dim3(std::min(std::min<uint32_t>((n_upper + 255) / 256, (uint32_t)g_num_cus * per_cu), t_max_blocks)); }   // persistent blocks of 256 threads
bool general_geometry(const pt_scene *sc) { return sc->ds.n_spheres > 0 || sc->ds.n_instances > 0; }   // the SPH forms: spheres or instances besides world-space triangles

// k_trace (tu_trace.hip): ANY 0..2 x MODE 0..3 x QUADK 0..2, and the probe walk (closest hit, PROBE) in the same MODE x QUADK -- row 3 of the table
using TraceVariant = Variant<DeviceScene, TraceJob>;
template <int ANY, int MODE, bool PROBE, int QUADK> TraceVariant trace_inst() { return {k_trace<ANY, MODE, PROBE, QUADK>, symbol("k_trace", ANY, MODE, PROBE, QUADK)}; }
template <int... I> const TraceVariant &trace_table(int i, std::integer_sequence<int, I...>) { static const TraceVariant t[] = {trace_inst<I / 12 % 3, I / 3 % 4, I / 12 == 3, I % 3>()...}; return t[i]; }
static const TraceVariant &trace_variant(int any, int mode, bool probe, int quadk) { return trace_table((probe ? 3 : any) * 12 + mode * 3 + quadk, std::make_integer_sequence<int, 48>()); }

// k_shade (tu_shade.hip). The forms that are not compiled fall back to the general kernel of the same lobe budget (DIFF 0), here and nowhere else: volpath (MODE 3) has
// no DIFF >= 2 form -- its router folds the specular and the lobe-set classes back (shaded_in below) --, and the smooth-subsurface form (DIFF 6) is untextured only (MODE < 2)
using ShadeVariant = Variant<DeviceScene, RenderConst, SobolTables, LightGrid, PathSoA, ShadeJob>;
template <int MAXL, int MODE, int DIFF> const ShadeVariant &shade_inst() {
    constexpr int D = ((MODE == 3 && DIFF >= 2) || (MODE == 2 && DIFF == 6)) ? 0 : DIFF;
    static const ShadeVariant v{k_shade<MAXL, MODE, D>, symbol("k_shade", MAXL, MODE, D)};
    return v;
}
template <int MAXL, int DIFF> const ShadeVariant &shade_variant(int mode) { return mode == 3 ? shade_inst<MAXL, 3, DIFF>() : mode == 2 ? shade_inst<MAXL, 2, DIFF>() : mode == 1 ? shade_inst<MAXL, 1, DIFF>() : shade_inst<MAXL, 0, DIFF>(); }

// k_shade_miss (tu_aux.hip) and k_bssrdf (tu_bssrdf.hip): <SPH, VOL> = <false, false>, <true, false>, <true, true> (volpath runs the general-geometry form, like all its kernels)
using MissVariant = Variant<DeviceScene, RenderConst, PathSoA, ShadeJob>;
using BssrdfVariant = Variant<DeviceScene, RenderConst, SobolTables, LightGrid, PathSoA, BssrdfJob>;
template <bool SPH, bool VOL> MissVariant miss_inst() { return {k_shade_miss<SPH, VOL>, symbol("k_shade_miss", SPH, VOL)}; }
template <bool SPH, bool VOL> BssrdfVariant bssrdf_inst() { return {k_bssrdf<SPH, VOL>, symbol("k_bssrdf", SPH, VOL)}; }
static const MissVariant &miss_variant(bool sph, bool vol) { static const MissVariant t[3] = {miss_inst<false, false>(), miss_inst<true, false>(), miss_inst<true, true>()}; return t[vol ? 2 : sph ? 1 : 0]; }
static const BssrdfVariant &bssrdf_variant(bool sph, bool vol) { static const BssrdfVariant t[3] = {bssrdf_inst<false, false>(), bssrdf_inst<true, false>(), bssrdf_inst<true, true>()}; return t[vol ? 2 : sph ? 1 : 0]; }

// k_film_final<SPH> (tu_aux.hip), k_light_touch<SPH> and k_route<NQ, CAP> (tu_misc.hip: six staging queues of 2048 entries or twelve of 1024)
using FilmFinalVariant = Variant<DeviceScene, RenderConst, PathSoA, const float *, float *, DevCounters *>;
using TouchVariant = Variant<DeviceScene, LightGrid, PathSoA, const uint32_t *, const uint32_t *, uint32_t, uint32_t, uint32_t *, uint32_t *, uint32_t *>;
using RouteVariant = Variant<DeviceScene, const uint32_t *, const uint32_t *, PathSoA, uint32_t *, RouteJob>;
template <bool SPH> FilmFinalVariant film_final_inst() { return {k_film_final<SPH>, symbol("k_film_final", SPH)}; }
template <bool SPH> TouchVariant touch_inst() { return {k_light_touch<SPH>, symbol("k_light_touch", SPH)}; }
template <int NQ, int CAP> RouteVariant route_inst() { return {k_route<NQ, CAP>, symbol("k_route", NQ, CAP)}; }
static const FilmFinalVariant &film_final_variant(bool sph) { static const FilmFinalVariant t[2] = {film_final_inst<false>(), film_final_inst<true>()}; return t[sph]; }
static const TouchVariant &touch_variant(bool sph) { static const TouchVariant t[2] = {touch_inst<false>(), touch_inst<true>()}; return t[sph]; }
static const RouteVariant &route_variant(uint32_t n_slots) { static const RouteVariant t[2] = {route_inst<6, 2048>(), route_inst<12, 1024>()}; return t[n_slots > 6]; }

// k_generate and, for the cameras beside the perspective one, k_generate_cam<CAM> (tu_misc.hip): one row per PtCameraType. The perspective job launches the plain kernel.
using GenerateVariant = Variant<RenderConst, SobolTables, PathSoA, uint32_t *, uint32_t *, DevCounters *>;
static const GenerateVariant &generate_variant(uint32_t camera_type) {
    static const GenerateVariant t[3] = {{k_generate, "k_generate"}, {k_generate_cam<PT_CAMERA_ORTHOGRAPHIC>, symbol("k_generate_cam", (int)PT_CAMERA_ORTHOGRAPHIC)},
                                         {k_generate_cam<PT_CAMERA_ENVIRONMENT>, symbol("k_generate_cam", (int)PT_CAMERA_ENVIRONMENT)}};
    return t[camera_type];   // (check_camera: <= 2)
}

template <int MAXL, int DIFF> void launch_shade(pt_scene *sc, const RenderConst &rc, const LightGrid &grid, const ShadeJob &job, uint32_t upper) {
    const int mode = rc.volpath ? 3 : sc->ds.n_textures > 0 ? 2 : (general_geometry(sc) || rc.halton.enabled) ? 1 : 0;   // kern_shade.h: k_shade MODE
    launch(sc, shade_variant<MAXL, DIFF>(mode), blocks_for(upper, PT_SHADE_BLOCKS_PER_CU), dim3(256), sc->ds, rc, g_tabs, grid, sc->ps, job);   // persistent blocks: the LDS Sobol' table is staged once per block
}

// ---- shade classes (kernels.h: kNumClasses). One row per class: the launch kind its statistics go by, what runs on its queue, and for the surface classes the k_shade
// family <MAXL, DIFF> that does. The specular class is a surface class of the path integrator; volpath has none, and its queue serves the exit points of subsurface chains that
// wait for their traced shadow / MIS rays (k_bssrdf, stage B).
enum ClassKind { kSurface, kMiss, kMedium, kSpecularOrStageB };
struct ClassInfo { const char *stat; ClassKind kind; void (*launch)(pt_scene *, const RenderConst &, const LightGrid &, const ShadeJob &, uint32_t); };
constexpr ClassInfo kClasses[kNumClasses] = {
    {"shade_matte", kSurface, launch_shade<1, 1>}, {"shade_1lobe", kSurface, launch_shade<1, 0>}, {"shade_2lobe", kSurface, launch_shade<2, 0>}, {"shade_manylobe", kSurface, launch_shade<5, 0>},
    {"shade_miss", kMiss, nullptr}, {"shade_medium", kMedium, nullptr}, {"shade_specular", kSpecularOrStageB, launch_shade<1, 2>},
    {"shade_metal", kSurface, launch_shade<1, 3>}, {"shade_plastic", kSurface, launch_shade<2, 4>}, {"shade_uber", kSurface, launch_shade<5, 5>}, {"shade_sss", kSurface, launch_shade<1, 6>}};

// THE statement of class folding: the class in whose queue, and by whose kernel, a render shades the vertices of class c; -1 when the scene has none. The path integrator
// shades every class in its own queue; the volumetric router (k_medium_route) folds the specular class into class 1 and the lobe-set classes into their lobe-count class.
static int shaded_in(const pt_scene *sc, int c, bool volpath) { return !sc->class_used[c] ? -1 : !volpath ? c : c == kSpecClass ? 1 : (int)class_general((uint32_t)c); }
static bool class_launched(const pt_scene *sc, int q, bool volpath) { for (int c = 0; c < kNumClasses; ++c) if (shaded_in(sc, c, volpath) == q) return true; return false; }
// The workspace serves both integrators: a class has a queue when either launches it, and matte and the three service classes always (4 dead / escaped paths, 5 medium
// vertices, 6 also the waiting exit points of volpath)
static bool class_has_queue(const pt_scene *sc, int c) { return c == 0 || kClasses[c].kind != kSurface || class_launched(sc, c, false) || class_launched(sc, c, true); }
// queues of one path index each: ext[2] + shade[2][classes with a queue] + shadow + mis (+ probe[2])
// (in units of `capacity` entries: ext x 2, the ray queue's three entries per path, under PT_TRACE_SPLIT=1 the single-kind launches' MIS and shadow queues, probe x 2, the classes')
static size_t n_queues(const pt_scene *sc) { size_t n = 2 + 3 + (g_trace_split ? 2 : 0) + (sc->has_bssrdf ? 2 : 0); for (int c = 0; c < kNumClasses; ++c) n += class_has_queue(sc, c) ? 2 : 0; return n; }

// any: 0 closest hit, 1 any hit (rays of job.sub[0]); 2 mixed: the queues of job.sub[0..2] in one launch (n_upper covers all three)
int launch_trace(pt_scene *sc, int any, TraceJob job, uint32_t n_upper, bool probe) {
    if (n_upper == 0) return PT_OK;
    const uint32_t knob = job.sub[0].kind == 4 ? 0 : (job.sub[0].kind & 3);
    job.refill_min = (probe && !g_refill_from_env) ? 24u : g_refill_min[knob]; job.leaf_quorum = g_leaf_quorum[knob];   // (probe chains: 24 measured best on C5, 16: +1.6 %)
    if (sc->ds.n_instances > 0 && !g_refill_from_env) job.refill_min = 8;   // rays through instanced scenes are long (S4: 200 node visits): idle lanes are refilled early (measured 24 -> 8: +9 %)
    const uint32_t waves = (n_upper + 63) / 64, blocks = std::min<uint32_t>((waves + 3) / 4, sc->spill_waves / 4);
    const int mode = (sc->ds.tri_alpha || sc->ds.tri_shadow_alpha) ? 2 : sc->ds.n_spheres > 0 ? 1 : sc->ds.n_instances > 0 ? 3 : 0;  // kern_trace.h: k_trace MODE
    job.inst_quorum = g_inst_quorum;
    if (sc->quad_walk_only && (g_trace_exact || sc->exact_walk_only)) return fail(PT_ERR_UNSUPPORTED, "the two-wide (exact) walk addresses 2^25 records / packets: this scene has the production walk only");
    // production: the four-wide records, through 64-bit addresses when records + packets lie beyond 4 GB; pt_set_trace_exact(1): the two-wide walk with the reference's node-visit counter
    const int quadk = (g_trace_exact || sc->exact_walk_only) ? 0 : sc->pool_big ? 2 : 1;
#ifdef PT_TRACE_UTIL
    hipLaunchKernelGGL(k_trace_util_fold, dim3(1), dim3(1), 0, sc->stream, sc->dc, job.sub[0].kind & 3u, 0u, 1);
#endif
    launch(sc, trace_variant(any, mode, probe, quadk), dim3(blocks), dim3(kTraceBlock), sc->ds, job);
#ifdef PT_TRACE_UTIL
    hipLaunchKernelGGL(k_trace_util_fold, dim3(1), dim3(1), 0, sc->stream, sc->dc, job.sub[0].kind & 3u, blocks * (kTraceBlock / 64), 0);
#endif
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

int ensure_workspace(pt_scene *sc, size_t capacity, size_t film_px) {
    if (!sc->stream) HIP_TRY(hipStreamCreate(&sc->stream));
    if (!sc->qc) {
        int st;
        if ((st = sc->dalloc(&sc->qc, 1))) return st;
        if ((st = sc->dalloc(&sc->dc, 1))) return st;
        sc->spill_waves = (uint32_t)g_num_cus * g_trace_waves_per_cu;  // resident persistent waves (LDS: 5 KB per wave)
        if ((st = sc->dalloc(&sc->spill, (size_t)sc->spill_waves * 64 * kSpillWords))) return st;
        if ((st = sc->dalloc(&sc->d_filter, 256))) return st;
        if (sc->has_bssrdf && (st = sc->dalloc(&sc->probe_ring, (size_t)sc->spill_waves * 64 * kProbeRing * 3))) return st;
    }
    if (capacity > sc->capacity) {
        // the present workspace goes first (its memory is needed for the larger one); from here to the last allocation the scene HAS no workspace: a failure
        // leaves capacity 0 and every pointer null, so the next render allocates afresh instead of running on a freed slab behind the old capacity
        auto drop = [&]() {
            if (sc->slab) hipFree(sc->slab); if (sc->qbuf) hipFree(sc->qbuf); if (sc->ext_slab) hipFree(sc->ext_slab); if (sc->bss_slab) hipFree(sc->bss_slab);
            sc->slab = nullptr; sc->qbuf = nullptr; sc->ext_slab = nullptr; sc->bss_slab = nullptr; sc->ext_capacity = 0; sc->capacity = 0;
        };
        auto oom = [&](const char *what, hipError_t e) { (void)hipGetLastError(); drop(); return fail(PT_ERR_OUT_OF_MEMORY, std::string(what) + ": " + hipGetErrorString(e)); };
        drop();
        size_t bytes = capacity * (size_t)kPathBytes + 4096;
        hipError_t e = hipMalloc(&sc->slab, bytes);
        if (e != hipSuccess) { sc->slab = nullptr; return oom("path-state slab", e); }
        char *p = (char *)sc->slab;   // hipMalloc returns 256-byte aligned memory; every record array starts on a 64-byte line
        PathSoA &ps = sc->ps;
        ps.core = (float *)p; p += capacity * (size_t)PathSoA::kCoreWords * 4;
        ps.nee = (float *)p; p += capacity * (size_t)PathSoA::kNeeWords * 4;
        ps.mis = (float *)p; p += capacity * (size_t)PathSoA::kMisWords * 4;
        ps.ray = (float *)p; p += capacity * (size_t)PathSoA::kRayWords * 4;
        ps.hit = (float *)p; p += capacity * (size_t)PathSoA::kHitWords * 4;
        if (sc->has_bssrdf) {
            e = hipMalloc(&sc->bss_slab, capacity * (size_t)kBssBytes);
            if (e != hipSuccess) { sc->bss_slab = nullptr; return oom("BSSRDF probe state", e); }
            BssSoA &bs = sc->bs;
            float4 *bp = (float4 *)sc->bss_slab;
            bs.probe = bp; bp += capacity * (size_t)BssSoA::kProbeQuads; bs.frame = bp; bp += capacity * (size_t)BssSoA::kFrameQuads; bs.coef = bp;
        }
        // (after the path state, so that a pass too large for the device's memory is reported as that)
        if (capacity > kMaxRayQueuePaths) { drop(); return fail(PT_ERR_INVALID_ARG, "more than 2^29 paths in one pass: a ray-queue entry keeps the path id beside the ray's kind"); }
        e = hipMalloc((void **)&sc->qbuf, n_queues(sc) * capacity * 4);
        if (e != hipSuccess) { sc->qbuf = nullptr; return oom("queues", e); }
        uint32_t *qp = sc->qbuf;
        for (int i = 0; i < 2; ++i) { sc->q.ext[i] = qp; qp += capacity; }
        for (int i = 0; i < 2; ++i) for (int c = 0; c < kNumClasses; ++c) { sc->q.shade[i][c] = nullptr; if (class_has_queue(sc, c)) { sc->q.shade[i][c] = qp; qp += capacity; } }
        sc->q.rays = qp; qp += 3 * capacity;
        sc->q.shadow = sc->q.mis = nullptr;
        if (g_trace_split) { sc->q.shadow = qp; qp += capacity; sc->q.mis = qp; qp += capacity; }
        sc->q.probe[0] = sc->q.probe[1] = nullptr;
        if (sc->has_bssrdf) { sc->q.probe[0] = qp; qp += capacity; sc->q.probe[1] = qp; }
        sc->capacity = capacity;
    }
    if (film_px > sc->film_px) {
        if (sc->film_rgbw) hipFree(sc->film_rgbw);
        sc->film_rgbw = nullptr; sc->film_px = 0;
        if (hipError_t e = hipMalloc((void **)&sc->film_rgbw, film_px * 16); e != hipSuccess) { (void)hipGetLastError(); sc->film_rgbw = nullptr; return fail(PT_ERR_OUT_OF_MEMORY, std::string("device film: ") + hipGetErrorString(e)); }
        sc->film_px = film_px;
    }
    return PT_OK;
}

// SpatialLightDistribution::new's voxel counts (lightdistrib.rs:112-128)
void spatial_voxels(const pt_scene *sc, uint32_t nvox[3]) {
    float diag[3] = {sc->ds.wb_max[0] - sc->ds.wb_min[0], sc->ds.wb_max[1] - sc->ds.wb_min[1], sc->ds.wb_max[2] - sc->ds.wb_min[2]};
    int me = (diag[0] > diag[1] && diag[0] > diag[2]) ? 0 : (diag[1] > diag[2] ? 1 : 2);
    float bmax = diag[me];
    for (int i = 0; i < 3; ++i) {
        float v = std::round(diag[i] / bmax * 64.0f);
        uint32_t nv = (v > 0.0f) ? (uint32_t)v : 0u;  // `as usize` saturates, NaN -> 0
        nvox[i] = std::max<uint32_t>(1u, nv);
    }
}
constexpr size_t kEagerGridEntries = (size_t)1 << 25;   // voxels x lights up to which PT_LS_SPATIAL precomputes every voxel

// The light distributions of n voxels (k_light_grid_contrib: 128 Halton points x every light each, lightdistrib.rs:151-228; k_light_grid_finish: their CDFs): of all
// of them in order, or of those listed in `cells`, whose blocks (`stride` floats each, at func) are then published in cell_ptr
static void light_grid_cells(pt_scene *sc, const LightGrid &g, size_t n, float *func, float *cdf, float *fint, const uint32_t *cells, size_t stride, unsigned long long *cell_ptr) {
    const size_t total = n * g.n_lights;
    sc->begin("light_grid", total);
    launch(sc, "k_light_grid_contrib", k_light_grid_contrib, dim3((unsigned)((total + 255) / 256)), dim3(256), sc->ds, g.nvox[0], g.nvox[1], g.nvox[2], func, cells, cells ? n : 0, stride);
    hipLaunchKernelGGL(k_light_grid_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sc->stream, g.n_lights, n, func, cdf, fint, cells, stride, cell_ptr);
    sc->end();
}

int ensure_light_grid(pt_scene *sc, int requested, int &effective) {
    effective = requested;
    if (requested == PT_LS_UNIFORM || sc->n_lights == 1) effective = PT_LS_UNIFORM;  // lightdistrib.rs:21
    if (requested > PT_LS_SPATIAL_LAZY) effective = PT_LS_SPATIAL;
    if (effective == PT_LS_SPATIAL) {   // the form is the library's choice (include/mi355pt.h: PtLightStrategy)
        uint32_t nv[3]; spatial_voxels(sc, nv);
        effective = (size_t)nv[0] * nv[1] * nv[2] * std::max(1u, sc->n_lights) <= kEagerGridEntries ? PT_LS_SPATIAL_EAGER : PT_LS_SPATIAL_LAZY;
    }
    LightGrid &g = sc->grid[effective];
    if (sc->grid_ready[effective]) return PT_OK;
    g.strategy = effective >= PT_LS_SPATIAL ? (int)PT_LS_SPATIAL : effective; g.n_lights = sc->n_lights; g.nvox[0] = g.nvox[1] = g.nvox[2] = 1;
    g.cell_ptr = nullptr; g.zero_block = 0; g.missing = nullptr;
    const uint32_t nl = sc->n_lights;
    if (nl == 0) { g.strategy = PT_LS_UNIFORM; g.func = g.cdf = g.func_int = nullptr; sc->grid_ready[effective] = true; return PT_OK; }
    if (effective == PT_LS_UNIFORM || effective == PT_LS_POWER) {
        std::vector<float> func(nl, 1.0f), cdf; float fi;
        if (effective == PT_LS_POWER) {  // compute_light_power_distribution (integrator.rs:239-247): Light::power().y() per light
            std::vector<float> area(nl);
            HIP_TRY(hipMemcpy(area.data(), sc->ds.light_area, nl * sizeof(float), hipMemcpyDeviceToHost));
            const float wr = sc->ds.world_radius;
            for (uint32_t i = 0; i < nl; ++i) {
                const PtLight &L = sc->host_lights[i];
                RGB c(L.L[0], L.L[1], L.L[2]), p(0.0f);
                switch (L.type) {
                case PT_LIGHT_DIFFUSE_AREA: p = c * area[i] * kPi; break;                                  // diffuse.rs:82-84
                case PT_LIGHT_DISTANT: p = c * kPi * wr * wr; break;                                      // distant.rs:47-50
                case PT_LIGHT_POINT: p = c * 4.0f * kPi; break;                                           // point.rs:44-46
                case PT_LIGHT_SPOT: p = c * 2.0f * kPi * (1.0f - 0.5f * (L.cos_falloff_start + L.cos_total_width)); break;  // spot.rs:64-66
                case PT_LIGHT_INFINITE: {                                                                  // infinite.rs:103-109
                    p = RGB(sc->env_texel0[0], sc->env_texel0[1], sc->env_texel0[2]) * wr * wr * kPi; break;   // env_texel0 = PtSceneDesc.env_power_lookup
                }
                default: break;
                }
                func[i] = p.y();
            }
        }
        dist1d(func, cdf, fi);
        int st;
        if ((st = sc->upload(&g.func, func.data(), nl))) return st;
        if ((st = sc->upload(&g.cdf, cdf.data(), nl + 1))) return st;
        if ((st = sc->upload(&g.func_int, &fi, 1))) return st;
    } else if (effective == PT_LS_SPATIAL_LAZY) {   // voxels filled on first touch (lazy_light_fill, called from run_pass)
        spatial_voxels(sc, g.nvox);
        pt_scene::LazyGrid &z = sc->lazy;
        z.ncell = (size_t)g.nvox[0] * g.nvox[1] * g.nvox[2];
        z.stride = ((size_t)4 + nl + nl + 1 + 3) & ~(size_t)3;   // {func_int, -, -, -} func[nl] cdf[nl + 1], whole quads
        int st;
        if ((st = sc->dalloc(&z.cell_ptr, z.ncell))) return st;
        if ((st = sc->dalloc(&z.zero_block, z.stride))) return st;
        if ((st = sc->dalloc(&z.req_flag, z.ncell))) return st;
        if ((st = sc->dalloc(&z.req_list, z.ncell))) return st;
        if ((st = sc->dalloc(&z.req_count, 2))) return st;
        z.missing = z.req_count + 1;
        HIP_TRY(hipMemset(z.zero_block, 0, z.stride * 4));
        HIP_TRY(hipMemset(z.req_flag, 0, z.ncell * 4));
        HIP_TRY(hipMemset(z.req_count, 0, 8));
        std::vector<unsigned long long> init(z.ncell, (unsigned long long)z.zero_block);
        HIP_TRY(hipMemcpy(z.cell_ptr, init.data(), z.ncell * 8, hipMemcpyHostToDevice));
        g.func = g.cdf = g.func_int = nullptr;
        g.cell_ptr = z.cell_ptr; g.zero_block = (unsigned long long)z.zero_block; g.missing = z.missing;
    } else {  // SpatialLightDistribution::new (lightdistrib.rs:112-128), every voxel precomputed on device
        spatial_voxels(sc, g.nvox);
        size_t ncell = (size_t)g.nvox[0] * g.nvox[1] * g.nvox[2];
        if (ncell * nl > ((size_t)1 << 31)) return fail(PT_ERR_UNSUPPORTED, "PT_LS_SPATIAL_EAGER: voxels x lights > 2^31 (PT_LS_SPATIAL picks the first-touch form for such scenes)");
        float *func, *cdf, *fint; int st;
        if ((st = sc->dalloc(&func, ncell * nl))) return st;
        if ((st = sc->dalloc(&cdf, ncell * (nl + 1)))) return st;
        if ((st = sc->dalloc(&fint, ncell))) return st;
        light_grid_cells(sc, g, ncell, func, cdf, fint, nullptr, 0, nullptr);
        HIP_TRY(hipGetLastError());
        g.func = func; g.cdf = cdf; g.func_int = fint;
    }
    sc->grid_ready[effective] = true;
    return PT_OK;
}

// The 16x16 tiles of the sample bounds (integrator.rs:277-279): the grid tile_rank / tile_world and the tile lists index, row major
void tile_grid(const PtRenderParams *rp, uint32_t *ntx, uint32_t *nty) {
    const int32_t dx = rp->sample_bounds[2] - rp->sample_bounds[0], dy = rp->sample_bounds[3] - rp->sample_bounds[1];
    *ntx = (uint32_t)((dx + 15) / 16); *nty = (uint32_t)((dy + 15) / 16);
}

void fill_render_const(const PtRenderParams *rp, RenderConst &rc) {
    std::memset(&rc, 0, sizeof rc);
    std::memcpy(rc.sample_bounds, rp->sample_bounds, 16);
    std::memcpy(rc.pixel_bounds, rp->pixel_bounds, 16);
    std::memcpy(rc.crop, rp->cropped_pixel_bounds, 16);
    int32_t dx = rp->sample_bounds[2] - rp->sample_bounds[0], dy = rp->sample_bounds[3] - rp->sample_bounds[1];
    tile_grid(rp, &rc.ntx, &rc.nty);
    // SobolSampler::new (sobol.rs:42-44)
    int32_t v = std::max(dx, dy); v--; v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16; v++;
    rc.sobol.resolution = v; rc.sobol.log2_resolution = 31 - __builtin_clz((uint32_t)v);
    rc.sobol.sb_min[0] = rp->sample_bounds[0]; rc.sobol.sb_min[1] = rp->sample_bounds[1];
    if (rp->sampler_type == PT_SAMPLER_HALTON) {   // HaltonSampler::new (halton.rs:62-110), kMaxResolution = 128
        rc.halton.enabled = 1; rc.halton.at_center = rp->sample_at_pixel_center ? 1u : 0u;
        const int32_t res[2] = {dx, dy};
        for (int i = 0; i < 2; ++i) {
            const uint32_t base = i == 0 ? 2u : 3u;
            uint32_t scale = 1, e = 0;
            while ((int64_t)scale < (int64_t)std::min(res[i], 128)) { scale *= base; e++; }
            rc.halton.base_scale[i] = scale; rc.halton.base_exp[i] = e;
        }
        rc.halton.stride = rc.halton.base_scale[0] * rc.halton.base_scale[1];
        auto mult_inverse = [](int64_t a, int64_t n) {   // extended_gcd + mod_ (halton.rs:19-35)
            int64_t x0 = 1, x1 = 0, aa = a, bb = n;      // iterative form of the same recurrence: x with a*x = gcd (mod n)
            while (bb != 0) { const int64_t q = aa / bb; int64_t t = aa - q * bb; aa = bb; bb = t; t = x0 - q * x1; x0 = x1; x1 = t; }
            return ((x0 % n) + n) % n;
        };
        rc.halton.mult_inv[0] = (uint32_t)mult_inverse(rc.halton.base_scale[1], rc.halton.base_scale[0]);
        rc.halton.mult_inv[1] = (uint32_t)mult_inverse(rc.halton.base_scale[0], rc.halton.base_scale[1]);
    }
    std::memcpy(rc.raster_to_camera.m, rp->raster_to_camera, 64);
    std::memcpy(rc.camera_to_world.m, rp->camera_to_world, 64);
    rc.lens_radius = rp->lens_radius; rc.focal_distance = rp->focal_distance;
    rc.camera_type = rp->camera_type;
    rc.inv_sqrt_spp = 1.0f / std::sqrt((float)rp->spp);
    if (rp->camera_type == PT_CAMERA_ENVIRONMENT) {   // no raster_to_camera (the field is not read), no dx_camera: RenderConst::full_res in its place. environment.rs:38-39: `full_resolution.x as Float`
        rc.raster_to_camera = M4{};
        rc.dx_camera[0] = (float)rp->full_resolution[0]; rc.dx_camera[1] = (float)rp->full_resolution[1];
    } else {   // dx_camera / dy_camera. PerspectiveCamera::new (perspective.rs:64-70): differences of transformed POINTS; OrthographicCamera::new (orthographic.rs:55-56):
               // raster_to_camera on the VECTORS (1,0,0) and (0,1,0)
        const bool ortho = rp->camera_type == PT_CAMERA_ORTHOGRAPHIC;
        const V3 p2t = xf_point(rc.raster_to_camera, V3(0.0f, 0.0f, 0.0f));
        const V3 dx = ortho ? xf_vector(rc.raster_to_camera, V3(1.0f, 0.0f, 0.0f)) : xf_point(rc.raster_to_camera, V3(1.0f, 0.0f, 0.0f)) - p2t;
        const V3 dy = ortho ? xf_vector(rc.raster_to_camera, V3(0.0f, 1.0f, 0.0f)) : xf_point(rc.raster_to_camera, V3(0.0f, 1.0f, 0.0f)) - p2t;
        rc.dx_camera[0] = dx.x; rc.dx_camera[1] = dx.y; rc.dx_camera[2] = dx.z;
        rc.dy_camera[0] = dy.x; rc.dy_camera[1] = dy.y; rc.dy_camera[2] = dy.z;
    }
    rc.max_depth = rp->max_depth; rc.rr_threshold = rp->rr_threshold;
    rc.volpath = rp->integrator == PT_INTEGRATOR_VOLPATH ? 1u : 0u; rc.camera_medium = rc.volpath ? rp->camera_medium : PT_NONE;
    rc.filter_radius[0] = rp->filter_radius[0]; rc.filter_radius[1] = rp->filter_radius[1];
    rc.max_sample_luminance = rp->max_sample_luminance;
    rc.film_w = (uint32_t)(rp->cropped_pixel_bounds[2] - rp->cropped_pixel_bounds[0]);
    rc.film_h = (uint32_t)(rp->cropped_pixel_bounds[3] - rp->cropped_pixel_bounds[1]);
    rc.spp = rp->spp;
    rc.tile_world = rp->tile_world ? rp->tile_world : 1; rc.tile_rank = rp->tile_rank;
}

__global__ void k_reset(QCounters *qc, uint32_t mask, int cur) {
    // mask bit0: next ext + next shade queues; bit1: the ray queue (+ shadow + mis); bit2: trace heads; bit3: current ext + shade
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int nxt = 1 - cur;
    if (mask & 1u) { qc->ext[nxt] = 0; qc->probe[nxt] = 0; for (int c = 0; c < kNumClasses; ++c) qc->shade[nxt][c] = 0; }
    if (mask & 2u) { qc->rays = 0; qc->shadow = 0; qc->mis = 0; }
    if (mask & 4u) { for (int i = 0; i < 4; ++i) qc->head[i] = 0; }
    if (mask & 8u) { qc->ext[cur] = 0; qc->probe[cur] = 0; for (int c = 0; c < kNumClasses; ++c) qc->shade[cur][c] = 0; }
}

// Samples per pass when the caller leaves the choice to the library (PtRenderParams.spp_per_pass = 0): the device's free memory and what the scene's workspace holds and
// costs per path, handed to the one rule (pass_budget.h: pass_size_for) with the integrator's budget (host_common.h: kPathPassBudget; libmi355ao and libmi355aov pass their own)
uint32_t choose_pass_size(const pt_scene *sc, uint32_t n_pix_slots, uint32_t spp, uint32_t share, bool volpath, const PassBudget &budget) {
    // per path: the five state records, the queues that exist, the probe state of scenes with subsurface materials and -- volpath through material-less shells -- the
    // 128-byte chain record (PathSoA::ext, allocated after the main slab: left out of this sum, a shell scene asked for ~1.4x its budget)
    const size_t workspace = (size_t)kPathBytes + 4u * n_queues(sc) + (sc->has_bssrdf ? (size_t)kBssBytes : 0u)
                             + ((volpath && sc->has_null_material) ? 4u * (size_t)PathSoA::kExtWords : 0u);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
    return pass_size_for(free_b, sc->capacity * workspace, workspace + budget.extra_bytes_per_path, budget, n_pix_slots, spp, share);
}

// First-touch voxels of PT_LS_SPATIAL_LAZY. touch: the vertices of one queue name their voxels; fill: the voxels named since the last fill are computed and published.
int lazy_light_touch(pt_scene *sc, const RenderConst &rc, const LightGrid &grid, const uint32_t *queue, const uint32_t *count, uint32_t n_upper, uint32_t kind) {
    const pt_scene::LazyGrid &z = sc->lazy;
    if (!grid.cell_ptr || n_upper == 0) return PT_OK;
    sc->begin("light_touch", n_upper);
    launch(sc, touch_variant(general_geometry(sc)), blocks_for(n_upper, 16u), dim3(256), sc->ds, grid, sc->ps, queue, count, kind, rc.max_depth, z.req_flag, z.req_list, z.req_count);
    sc->end();
    return PT_OK;
}
int lazy_light_fill(pt_scene *sc, const LightGrid &grid) {
    if (!grid.cell_ptr) return PT_OK;
    pt_scene::LazyGrid &z = sc->lazy;
    uint32_t n_new = 0;
    HIP_TRY(hipMemcpyAsync(&n_new, z.req_count, 4, hipMemcpyDeviceToHost, sc->stream));
    HIP_TRY(hipStreamSynchronize(sc->stream));
    if (n_new == 0) return PT_OK;
    if (n_new > z.ncell) return fail(PT_ERR_HIP, "light grid: more voxels requested than the grid holds");
    const uint32_t nl = grid.n_lights;
    // in batches of at most 2^31 (voxel, light) pairs per launch and 1 GiB of blocks per allocation
    const size_t per_batch = std::max<size_t>(1, std::min<size_t>(((size_t)1 << 31) / std::max(1u, nl), ((size_t)1 << 28) / z.stride));
    for (size_t first = 0; first < n_new; first += per_batch) {
        const size_t n = std::min<size_t>(per_batch, n_new - first);
        // blocks live as long as the scene (their addresses are published in cell_ptr): carved from slabs of >= 64 MB, so that a long render that keeps
        // touching a few new voxels per iteration makes a handful of allocations instead of one per iteration
        const size_t need = n * z.stride;
        if (need > z.arena_left) {
            const size_t slab = std::max<size_t>(need, (size_t)16 << 20);   // floats
            if (int st = sc->dalloc(&z.arena, slab)) return st;
            z.arena_left = slab;
        }
        float *blocks = z.arena; z.arena += need; z.arena_left -= need;
        light_grid_cells(sc, grid, n, blocks, nullptr, nullptr, z.req_list + first, z.stride, z.cell_ptr);
    }
    HIP_TRY(hipMemsetAsync(z.req_count, 0, 4, sc->stream));
    HIP_TRY(hipGetLastError());
    z.filled += n_new;
    return PT_OK;
}

// The text behind a status a kernel raised (QCounters::error; the largest code wins when several were raised)
const char *device_error_text(uint32_t code) {
    switch (code) {
    case PT_ERR_STACK_OVERFLOW: return "BVH traversal stack overflow: a ray needed more than 96 pending entries in the four-wide production walk / 64 in the two-wide exact walk (the reference's 64-entry stack, accelerators/bvh.rs:722, has no check)";
    case PT_ERR_PROBE_CHAIN: return "BSSRDF probe chain with more than 2^32 - 1 intersections";
    case PT_ERR_SOBOL_DIMENSIONS: return "a path asked for sampler dimension >= 1024 (Sobol') / 1000 (Halton): the reference panics there (samplers/sobol.rs:69-73)";
    case PT_ERR_UNSUPPORTED: return "a hit's material class has no shade queue in this render (internal: k_route)";
    default: return "error raised on the device";
    }
}
// The queue counters as the stream has left them; a status a kernel raised meanwhile fails the call (run_pass at the start of every iteration, libmi355ao after every pass)
int sync_queue_counters(pt_scene *sc, QCounters &h) {
    HIP_TRY(hipMemcpyAsync(&h, sc->qc, sizeof h, hipMemcpyDeviceToHost, sc->stream));
    HIP_TRY(hipStreamSynchronize(sc->stream));
    if (h.error) return fail((int)h.error, device_error_text(h.error));
    return PT_OK;
}

// ---- one pass. An iteration consumes the queue set `cur` and fills the other one: trace, route, touch, probe, shade per class, reset (run_pass below). Its steps see it as
// an Iter: the queue sizes the host read at its start, and what the pass fixed (fin: the film kernel ends the paths, there is no miss class).
// n_rays: this iteration's rays of every kind -- the ray queue the vertices shaded last filled, which names their continuation rays (the n_ext entries of `ext`) once more;
// the camera rays of the first iteration are in `ext` alone.
struct Iter { pt_scene *sc; const RenderConst &rc; const LightGrid &grid; bool fin, profile_exact; int index, cur; uint32_t n_ext, n_resolve, n_rays, n_probe, n_stage_b; };

// A shading job (ShadeJob / BssrdfJob) with the outputs all of them share: its queue, the next iteration's continuation-ray queue, miss queue (none when the film kernel
// ends the paths) and the queue of class `self` (stage B of a volpath vertex), the ray queue, the error word and the counters.
template <class Job> Job shading_job(const Iter &it, const uint32_t *queue, const uint32_t *count, int self) {
    pt_scene *sc = it.sc; QCounters *qc = sc->qc; const int nxt = 1 - it.cur;
    Job j{}; j.queue = queue; j.count = count;
    j.ext_next = sc->q.ext[nxt]; j.ext_next_count = &qc->ext[nxt];
    if (!it.fin) { j.shade_next0 = sc->q.shade[nxt][kMissClass]; j.shade_next0_count = &qc->shade[nxt][kMissClass]; }
    j.self_next = sc->q.shade[nxt][self]; j.self_next_count = &qc->shade[nxt][self];
    j.rays = sc->q.rays; j.rays_count = &qc->rays;
    j.error = &qc->error; j.counters = sc->dc;
    return j;
}

// The rays of one kind: their queue, where a ray lies (`ray`, ray_words apart) and the counter slot (TraceSub::kind). The caller adds where the hit goes.
TraceSub trace_sub(uint32_t *queue, uint32_t *count, const float *ray, int ray_words, float tmax, uint32_t kind) {
    TraceSub s{}; s.queue = queue; s.count = count; s.ray = (const float4 *)ray; s.ray_stride = ray_words / 4; s.scalar_tmax = tmax; s.kind = kind; return s;
}
// The continuation rays of queue set `cur` -> hit record (Scene::intersect); `camera`: a pass's first rays, counted as camera rays (kind 3)
TraceSub extend_sub(pt_scene *sc, int cur, bool camera) {
    PathSoA &ps = sc->ps;
    TraceSub ext = trace_sub(sc->q.ext[cur], &sc->qc->ext[cur], ps.ray, PathSoA::kRayWords, INFINITY, camera ? 3 : 0);
    ext.out_hit = (float4 *)ps.hit; ext.out_hit_stride = PathSoA::kHitWords / 4; ext.out_hit2 = (float4 *)ps.hit + 1;   // {inst, t, packet, packet flags}
    return ext;
}
TraceJob trace_job(pt_scene *sc, int head) { TraceJob tj{}; tj.spill = sc->spill; tj.error = &sc->qc->error; tj.counters = sc->dc; tj.head = &sc->qc->head[head]; return tj; }
int traced(pt_scene *sc, const char *stat, int any, const TraceJob &tj, uint32_t n_upper, bool probe) {
    if (n_upper == 0) return PT_OK;   // (a launch kind with no work is not a launch: the per-launch averages of bench.py / rocprofv3 count real dispatches)
    sc->begin(stat, n_upper); const int st = launch_trace(sc, any, tj, n_upper, probe); sc->end();
    return st;
}

// trace: this iteration's continuation rays and the shadow / MIS rays of the vertices shaded in the previous one
static int trace_rays(const Iter &it) {
    pt_scene *sc = it.sc; QCounters *qc = sc->qc; PathSoA &ps = sc->ps; const RenderConst &rc = it.rc;
    const TraceSub ext = extend_sub(sc, it.cur, it.index == 0);   // (routed to the material classes next)
    // MIS rays of the previous vertex (closest hit, integrator.rs:215)
    TraceSub mis = trace_sub(sc->q.mis, &qc->mis, ps.mis, PathSoA::kMisWords, INFINITY, 1);
    mis.out_hit = (float4 *)&ps.mis_prim(0); mis.out_hit_stride = PathSoA::kMisWords / 4;
    mis.out_t = rc.volpath ? &ps.mis_t(0) : nullptr; mis.out_t_stride = PathSoA::kMisWords;
    const bool shells = rc.volpath && ps.ext != nullptr;   // the chains of VisibilityTester::tr / Scene::intersect_tr need every segment's full hit record
    if (shells) { mis.out_hit = (float4 *)ps.ext + 6; mis.out_hit_stride = PathSoA::kExtWords / 4; mis.out_hit2 = (float4 *)ps.ext + 7; mis.out_t = nullptr; }
    // shadow rays (any hit, light.rs:120-123). volpath: VisibilityTester::tr (light.rs:125-150) calls Scene::intersect, a closest-hit
    // query counted as one; without out_hit the primitive goes to out_word = nee.sh_prim, the slot `occluded` uses otherwise
    TraceSub sh = trace_sub(sc->q.shadow, &qc->shadow, ps.nee, PathSoA::kNeeWords, 1.0f - 0.0001f, 2);
    sh.out_word = &ps.occluded(0); sh.out_word_stride = PathSoA::kNeeWords; sh.any = rc.volpath ? 0u : 1u;
    if (shells) { sh.out_hit = (float4 *)ps.ext + 4; sh.out_hit_stride = PathSoA::kExtWords / 4; sh.out_hit2 = (float4 *)ps.ext + 5; }
    if (it.n_rays == it.n_ext || g_trace_split) {   // continuation rays only (the camera rays of the first iteration) / PT_TRACE_SPLIT=1: one launch per kind, each with its own work head
        auto one = [&](const char *stat, const TraceSub &sub, int head, int any, uint32_t n) { TraceJob tj = trace_job(sc, head); tj.sub[0] = sub; return traced(sc, stat, any, tj, n); };
        int st;
        uint32_t n_mis = 0, n_shadow = 0;
        if (it.n_rays != it.n_ext) {   // the single-kind launches read queues of plain path ids: the ray queue's MIS and shadow entries, scattered (the sizes: one more read of the counters)
            hipLaunchKernelGGL(k_split_rays, blocks_for(it.n_rays, 8u), dim3(256), 0, sc->stream, (const uint32_t *)sc->q.rays, (const uint32_t *)&qc->rays, sc->q.mis, &qc->mis, sc->q.shadow, &qc->shadow);
            QCounters h;
            if ((st = sync_queue_counters(sc, h))) return st;
            n_mis = h.mis; n_shadow = h.shadow;
        }
        if ((st = one(it.index == 0 ? "extend_camera" : "extend", ext, 0, 0, it.n_ext)) || (st = one("extend_mis", mis, 1, 0, n_mis))) return st;
        return one("shadow", sh, 2, (int)sh.any, n_shadow);
    }
    // the three ray kinds of this iteration in one launch: one tail of straggling rays instead of three, and the rays of a vertex side by side (the ray queue's order)
    TraceJob tj = trace_job(sc, 0);
    tj.sub[0] = ext; tj.sub[1] = mis; tj.sub[2] = sh;
    tj.sub[0].queue = sc->q.rays; tj.sub[0].count = &qc->rays;   // (TraceJob: the mixed launch's one queue)
    return traced(sc, "trace", 2, tj, it.n_rays);
}

// route: every hit goes to the shade queue of its material class. volpath: after medium sampling (volpath.rs:98-105), which may make the vertex a medium vertex
static void route_hits(const Iter &it) {
    pt_scene *sc = it.sc; QCounters *qc = sc->qc; const int cur = it.cur;
    if (it.n_ext == 0) return;
    sc->begin("route", it.n_ext);
    if (it.rc.volpath) {
        launch(sc, "k_medium_route", k_medium_route, blocks_for(it.n_ext, 8u), dim3(256), sc->ds, it.rc, g_tabs, sc->ps, sc->q.ext[cur], &qc->ext[cur], &qc->shade[cur][0],
               sc->q.shade[cur][0], sc->q.shade[cur][1], sc->q.shade[cur][2], sc->q.shade[cur][3], sc->q.shade[cur][4], sc->q.shade[cur][5], &qc->error);
    } else {
        RouteJob rj{}; rj.slot_map = ~0ull; rj.error = &qc->error; rj.drop_cls = it.fin ? (uint32_t)kMissClass : ~0u;   // (fin: escaped rays are dropped here, the film kernel ends them)
        int slot_of[kNumClasses]; std::fill(slot_of, slot_of + kNumClasses, -1);
        for (int c = 0; c < kNumClasses; ++c) {   // class c's nibble of slot_map names the staging queue ("slot") of the class it is shaded in; no hit is a medium vertex
            const int q = kClasses[c].kind == kMedium ? -1 : kClasses[c].kind == kMiss ? (it.fin ? -1 : c) : shaded_in(sc, c, false);
            if (q < 0) continue;
            if (slot_of[q] < 0) { slot_of[q] = (int)rj.n_slots; rj.cls_of_slot[rj.n_slots] = (uint32_t)q; rj.buf[rj.n_slots++] = sc->q.shade[cur][q]; }
            rj.slot_map = (rj.slot_map & ~(15ull << (4 * c))) | ((unsigned long long)slot_of[q] << (4 * c));
        }
        launch(sc, route_variant(rj.n_slots), blocks_for(it.n_ext, PT_ROUTE_BLOCKS_PER_CU), dim3(256), sc->ds, sc->q.ext[cur], &qc->ext[cur], sc->ps, &qc->shade[cur][0], rj);
    }
    sc->end();
}

// touch (first-touch light grids only): the vertices of every shade queue name their voxels, then the new ones are computed
static int touch_voxels(const Iter &it) {
    pt_scene *sc = it.sc;
    for (int c = 0; c < kNumClasses; ++c) {
        if (kClasses[c].kind == kMiss || !class_has_queue(sc, c)) continue;
        if (int st = lazy_light_touch(sc, it.rc, it.grid, sc->q.shade[it.cur][c], &sc->qc->shade[it.cur][c], it.n_ext + it.n_resolve + it.n_stage_b, kClasses[c].kind == kMedium ? 1u : 0u)) return st;
    }
    return lazy_light_fill(sc, it.grid);
}

// probe: subsurface probe chains (bssrdf.rs:367-402). Each lane of k_trace<.., PROBE> walks a whole chain, then k_bssrdf shades the vertex at the chain's exit point
static int probe_chains(const Iter &it) {
    pt_scene *sc = it.sc; QCounters *qc = sc->qc; PathSoA &ps = sc->ps; const int cur = it.cur;
    if (it.n_probe == 0) return PT_OK;
    TraceSub pr = trace_sub(sc->q.probe[cur], &qc->probe[cur], ps.ray, PathSoA::kRayWords, 1.0f - 0.0001f, 4);
    pr.out_hit = (float4 *)ps.hit; pr.out_hit_stride = PathSoA::kHitWords / 4; pr.out_hit2 = (float4 *)ps.hit + 1;
    TraceJob tj = trace_job(sc, 3); tj.sub[0] = pr; tj.bs = sc->bs; tj.ring = sc->probe_ring;
    int st;
    if ((st = traced(sc, "extend_probe", 0, tj, it.n_probe, true))) return st;
    // (first-touch light grids: the chains' exit points look their voxels up in k_bssrdf)
    if ((st = lazy_light_touch(sc, it.rc, it.grid, sc->q.probe[cur], &qc->probe[cur], it.n_probe, 2u)) || (st = lazy_light_fill(sc, it.grid))) return st;
    BssrdfJob bj = shading_job<BssrdfJob>(it, sc->q.probe[cur], &qc->probe[cur], kSpecClass);   // (self: under volpath the exit points wait for stage B in the specular class's queue)
    bj.bs = sc->bs;
    sc->begin("bssrdf", it.n_probe);
    launch(sc, bssrdf_variant(general_geometry(sc), it.rc.volpath), blocks_for(it.n_probe, PT_SHADE_BLOCKS_PER_CU), dim3(256), sc->ds, it.rc, g_tabs, it.grid, ps, bj);
    sc->end();
    return PT_OK;
}

// shade: the n (an upper bound unless the pass counts exactly) vertices in the queue of class c, by the kernel of the class's kind
static void shade_class(const Iter &it, int c, uint32_t n) {
    pt_scene *sc = it.sc; QCounters *qc = sc->qc; const RenderConst &rc = it.rc; const ClassInfo &ci = kClasses[c];
    if (n == 0) return;
    if (ci.kind == kSpecularOrStageB && rc.volpath) {   // exit-point vertices of subsurface chains in stage B (k_bssrdf put them here an iteration ago)
        if (!sc->has_bssrdf || !(sc->ds.has_grid || sc->ds.has_shells)) return;
        BssrdfJob bj = shading_job<BssrdfJob>(it, sc->q.shade[it.cur][c], &qc->shade[it.cur][c], c);
        bj.bs = sc->bs; bj.stage_b = 1u;
        sc->begin("bssrdf_stage_b", it.profile_exact ? n : 0);
        launch(sc, bssrdf_variant(general_geometry(sc), true), blocks_for(n, PT_SHADE_BLOCKS_PER_CU), dim3(256), sc->ds, rc, g_tabs, it.grid, sc->ps, bj);
        sc->end();
        return;
    }
    if (!class_launched(sc, c, rc.volpath != 0) || (ci.kind == kMiss && it.fin)) return;
    ShadeJob sj = shading_job<ShadeJob>(it, sc->q.shade[it.cur][c], &qc->shade[it.cur][c], c);
    sj.cls = (uint32_t)c;
    if ((c == 3 || c == kSssClass) && sc->has_bssrdf) { sj.probe_next = sc->q.probe[1 - it.cur]; sj.probe_next_count = &qc->probe[1 - it.cur]; sj.bs = sc->bs; }
    sc->begin(ci.stat, it.profile_exact ? n : 0);
    if (ci.kind == kMedium) launch(sc, "k_shade_medium", k_shade_medium, blocks_for(n, 8u), dim3(256), sc->ds, rc, g_tabs, it.grid, sc->ps, sj);
    else if (ci.kind == kMiss) launch(sc, miss_variant(general_geometry(sc), rc.volpath != 0), blocks_for(n, PT_MISS_BLOCKS_PER_CU), dim3(256), sc->ds, rc, sc->ps, sj);
    else ci.launch(sc, rc, it.grid, sj, n);
    sc->end();
}

// film: the pass's paths sanitised and splatted by k_film (kern_film.h) -- the passes whose paths the film kernel does not also end (volpath, PT_FILM_FINAL=0, libmi355ao)
int film_pass(pt_scene *sc, const RenderConst &rc) {
    sc->begin("film", rc.n_pix_slots * rc.s_count);
    launch(sc, "k_film", k_film, film_grid(rc), dim3(256), rc, sc->ps, sc->d_filter, sc->film_rgbw, sc->dc);
    sc->end();
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

static int run_pass(pt_scene *sc, RenderConst &rc, const LightGrid &grid, bool rp_profile_exact, int max_iterations) {
    const uint32_t total = rc.n_pix_slots * rc.s_count;
    QCounters *qc = sc->qc;   // (render_frame has zeroed the queue counters and put the pass's camera rays into ext[0])
    // The plain path integrator's paths are ended by the film kernel (k_film_final, kern_aux.h): no miss class, no k_shade_miss pass. Volpath keeps the pass (its
    // transmittance estimates draw sampler dimensions in iteration order).
    Iter it{sc, rc, grid, g_film_final && !rc.volpath, rp_profile_exact};
    const bool debug_iter = getenv("PT_DEBUG_ITER") != nullptr;
    auto reset = [&](uint32_t mask) { hipLaunchKernelGGL(k_reset, dim3(1), dim3(64), 0, sc->stream, qc, mask, it.cur); };
    int st;
    for (it.index = 0, it.cur = 0; it.index <= max_iterations; ++it.index, it.cur = 1 - it.cur) {   // a path needs <= max_depth + null-surface skips + probe segments iterations
        QCounters h;
        if ((st = sync_queue_counters(sc, h))) return st;
        if (it.index == max_iterations) return fail(PT_ERR_PROBE_CHAIN, "pass did not finish within " + std::to_string(max_iterations) + " wavefront iterations");
        const int cur = it.cur;
        if (debug_iter && it.index > 0 && it.index % 2048 == 0) {
            fprintf(stderr, "[iter %d] ext %u rays %u probe %u shade:", it.index, h.ext[cur], h.rays, h.probe[cur]);
            for (int c = 0; c < kNumClasses; ++c) fprintf(stderr, " %u", h.shade[cur][c]);
            fprintf(stderr, "\n");
        }
        it.n_ext = h.ext[cur]; it.n_resolve = h.shade[cur][kMissClass]; it.n_rays = it.index == 0 ? h.ext[cur] : h.rays; it.n_probe = h.probe[cur];
        // volpath with grid media: vertices that did their NEE set-up last iteration wait in their own shade class for stage B
        it.n_stage_b = 0;
        if (rc.volpath && (sc->ds.has_grid || sc->ds.has_shells)) for (int c = 0; c < kNumClasses; ++c) if (c != kMissClass) it.n_stage_b += h.shade[cur][c];
        if (it.n_ext == 0 && it.n_resolve == 0 && it.n_probe == 0 && it.n_stage_b == 0 && (!it.fin || it.n_rays == 0)) break;   // (fin: the last vertices' shadow / MIS rays are still to be traced)
        reset(4u | 1u);
        if ((st = trace_rays(it))) return st;
        route_hits(it);
        reset(2u);
        if ((st = touch_voxels(it)) || (st = probe_chains(it))) return st;
        uint32_t class_n[kNumClasses];
        if (rp_profile_exact) {  // exact per-class item counts for the statistics (costs one extra sync per iteration)
            QCounters h2;
            HIP_TRY(hipMemcpyAsync(&h2, qc, sizeof h2, hipMemcpyDeviceToHost, sc->stream));
            HIP_TRY(hipStreamSynchronize(sc->stream));
            for (int c = 0; c < kNumClasses; ++c) class_n[c] = h2.shade[cur][c];
        } else for (int c = 0; c < kNumClasses; ++c) class_n[c] = it.n_ext + it.n_resolve + it.n_stage_b;
        for (int c = 0; c < kNumClasses; ++c) shade_class(it, c, class_n[c]);
        HIP_TRY(hipGetLastError());
        reset(8u);
    }
    if (!it.fin) return film_pass(sc, rc);
    sc->begin("film", total);
    launch(sc, film_final_variant(general_geometry(sc)), film_grid(rc), dim3(256), sc->ds, rc, sc->ps, sc->d_filter, sc->film_rgbw, sc->dc);
    sc->end();
    HIP_TRY(hipGetLastError());
    return PT_OK;
}

void read_counters(pt_scene *sc) {
    DevCounters d;
    hipMemcpy(&d, sc->dc, sizeof d, hipMemcpyDeviceToHost);
    PtCounters &c = sc->counters;
    std::memset(&c, 0, sizeof c);
    c.camera_rays = d.camera_rays; c.intersect_tests = d.intersect_tests; c.shadow_tests = d.shadow_tests;
    c.bvh_nodes_visited = d.nodes; c.triangle_tests = d.tri_tests; c.sphere_tests = d.sphere_tests;
    c.zero_radiance_paths_num = d.zero_num; c.zero_radiance_paths_den = d.zero_den;
    for (int i = 0; i < 16; ++i) c.path_length_hist[i] = d.path_len[i];
    c.sanitized_nan = d.san_nan; c.sanitized_negative = d.san_neg; c.sanitized_infinite = d.san_inf;
    c.film_splats = d.splats; c.wavefront_stages = d.stages; c.reference_asserts = d.ref_asserts;
    for (int k = 0; k < kNumClasses; ++k) for (auto &s : sc->stats) if (s.name == kClasses[k].stat) { s.items = d.shade_items[k]; s.nodes = d.shade_bytes[k]; }
    static const char *kn[5] = {"extend", "extend_mis", "shadow", "extend_camera", "extend_probe"};
    for (int k = 0; k < 5; ++k) for (auto &s : sc->stats) if (s.name == kn[k]) { s.nodes = d.k_nodes[k]; s.tris = d.k_tris[k]; if (k == 4) s.items = d.k_rays[k]; }   // probe chains: items = segments traced
    for (auto &s : sc->stats) if (s.name == "trace") { s.nodes = d.k_nodes[0] + d.k_nodes[1] + d.k_nodes[2]; s.tris = d.k_tris[0] + d.k_tris[1] + d.k_tris[2]; }   // the mixed launches: all three kinds
    if (!g_trace_split) {   // what the mixed launches did per ray kind (no time of their own: launches = 0)
        for (int k = 0; k < 3; ++k) if (d.k_rays[k]) { bool have = false; for (auto &s : sc->stats) have = have || s.name == kn[k];
            if (!have) { Stat s2{std::string("trace:") + kn[k]}; s2.items = d.k_rays[k]; s2.nodes = d.k_nodes[k]; s2.tris = d.k_tris[k]; sc->stats.push_back(s2); } }
    }
    for (auto &s : sc->stats) if (s.name == "bssrdf") { s.items = d.bss_items; s.nodes = d.bss_bytes; }
#ifdef PT_TRACE_UTIL
    fprintf(stderr, "[trace-util] kernel saw leaf_quorum = %llu, refill_min = %llu (last launch)\n", d.dbg[0], d.dbg[1]);
    for (int k = 0; k < 4; ++k) if (d.tail[5 + 2 * k])
        fprintf(stderr, "[trace-util] %-14s wave slots busy %.1f %% of launch span x resident waves (the rest: launch ramp + tail after the queue drained)\n", kn[k], 100.0 * (double)d.tail[4 + 2 * k] / (double)d.tail[5 + 2 * k]);
    if (d.tail[2]) fprintf(stderr, "[trace-util] all trace launches: transform step %.3e wave iterations, %.1f %% lanes active, %.1f %% of the waves' cycles; record step (fetch + node / leaf + pop) %.1f %% of the cycles\n",
                           (double)d.tail[12], d.tail[12] ? 100.0 * (double)d.tail[13] / (64.0 * (double)d.tail[12]) : 0.0, 100.0 * (double)d.tail[14] / (double)d.tail[2], 100.0 * (double)d.tail[15] / (double)d.tail[2]);
    if (d.tail[2]) fprintf(stderr, "[trace-util] instance entries tried %.4e, turned away by the object's root test %.4e (%.1f %%), left with a hit %.4e (%.1f %%); stack entries written beyond the LDS ones %.4e\n",
                           (double)d.util2[4], (double)d.util2[5], d.util2[4] ? 100.0 * (double)d.util2[5] / (double)d.util2[4] : 0.0, (double)d.util2[6], d.util2[4] ? 100.0 * (double)d.util2[6] / (double)d.util2[4] : 0.0, (double)d.util2[7]);
    if (d.tail[2]) fprintf(stderr, "[trace-util] record step by part, %% of the waves' cycles: loads issued + waited for %.1f, node branch %.1f, leaf branch %.1f, pops %.1f\n",
                           100.0 * (double)d.util2[0] / (double)d.tail[2], 100.0 * (double)d.util2[1] / (double)d.tail[2], 100.0 * (double)d.util2[2] / (double)d.tail[2], 100.0 * (double)d.util2[3] / (double)d.tail[2]);
    for (int k = 0; k < 4; ++k)
        fprintf(stderr, "[trace-util] %-14s node phase: %.3e wave iterations, %.1f %% lanes active; leaf phase: %.3e iterations, %.1f %% lanes active\n", kn[k], (double)d.regions[4 * k],
                d.regions[4 * k] ? 100.0 * (double)d.regions[4 * k + 1] / (64.0 * (double)d.regions[4 * k]) : 0.0, (double)d.regions[4 * k + 2], d.regions[4 * k + 2] ? 100.0 * (double)d.regions[4 * k + 3] / (64.0 * (double)d.regions[4 * k + 2]) : 0.0);
#endif
#ifdef PT_REGION_PROFILE
    {
        static const char *rn[16] = {"0 loop/queue read", "1 resolve", "2 resolve env le", "3 load ray/hit + fill_hit + Le", "4 sobol window", "5 light choice",
                                     "6 light sample_li", "7 bsdf f/pdf + shadow ray", "8 MIS bsdf sample + store", "9 MIS light pdf_li", "10 bsdf build", "11 continuation sample + RR",
                                     "12 state write-back", "13 queue push/flush", "14 tail", "15 prologue"};
        unsigned long long tot = 0; for (int i = 0; i < 16; ++i) tot += d.regions[i];
        for (int i = 0; i < 16; ++i) fprintf(stderr, "[region] %-34s %6.2f %%  %.3e cycles\n", rn[i], tot ? 100.0 * (double)d.regions[i] / (double)tot : 0.0, (double)d.regions[i]);
    }
#endif
}

// ---- the render frame (host_common.h): what every integrator's render does before, around and after its passes
// The camera of a PtRenderParams, for every entry point that takes one (the renders through check_spp, the parity entries themselves): host arithmetic, before the device is touched
int check_camera(const PtRenderParams *rp) {
    if (rp->camera_type > PT_CAMERA_ENVIRONMENT) return fail(PT_ERR_INVALID_ARG, "camera_type " + std::to_string(rp->camera_type) + ": PT_CAMERA_PERSPECTIVE (0), PT_CAMERA_ORTHOGRAPHIC (1) and PT_CAMERA_ENVIRONMENT (2) run here");
    if (rp->camera_type == PT_CAMERA_ENVIRONMENT && (rp->full_resolution[0] <= 0 || rp->full_resolution[1] <= 0)) return fail(PT_ERR_INVALID_ARG, "the environment camera takes its angles over full_resolution, which must be > 0");
    return PT_OK;
}
int check_spp(const PtRenderParams *rp) { if (int st = check_camera(rp)) return st; return rp->spp == 0 ? fail(PT_ERR_INVALID_ARG, "spp must be > 0") : PT_OK; }   // (every render's first check: the camera rides with it)
// The range [first, first + n) of a job of rp->spp samples per pixel (pt_render_samples, pt_ao_render_samples, pt_multi_render_samples): host arithmetic, the sum in 64 bits
int check_sample_range(const PtRenderParams *rp, uint32_t first, uint32_t n) {
    if (n == 0) return fail(PT_ERR_INVALID_ARG, "n_samples must be > 0");
    if ((uint64_t)first + n > rp->spp) return fail(PT_ERR_INVALID_ARG, "sample range [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + n) + ") exceeds the job's spp = " + std::to_string(rp->spp));
    return PT_OK;
}
// 16x16 tiles of rank rc.tile_rank among rc.tile_world (tile t belongs to rank t % world)
uint32_t tile_slots(const RenderConst &rc) { const uint32_t ntiles = rc.ntx * rc.nty; return rc.tile_rank < ntiles ? (ntiles - rc.tile_rank + rc.tile_world - 1) / rc.tile_world : 0; }

// A tile list of the C ABI (pt_render_tiles, pt_tiles_select): strictly ascending -- so no tile twice: film_slot accumulates a thread's own pixel in registers, which is only
// right when no two slots name one pixel --, every entry inside the grid of n_grid tiles, and an array when n > 0. Host arithmetic.
int check_tile_list(const uint32_t *tiles, uint32_t n, uint64_t n_grid, const char *what) {
    if (n > 0 && !tiles) return fail(PT_ERR_INVALID_ARG, std::string(what) + ": null tile list");
    for (uint32_t i = 0; i < n; ++i) {
        if (tiles[i] >= n_grid) return fail(PT_ERR_INVALID_ARG, std::string(what) + ": tile " + std::to_string(tiles[i]) + " is outside the grid of " + std::to_string(n_grid) + " tiles");
        if (i > 0 && tiles[i] <= tiles[i - 1]) return fail(PT_ERR_INVALID_ARG, std::string(what) + ": the tile list must be strictly ascending (entry " + std::to_string(i) + ")");
    }
    return PT_OK;
}

// What every render checks before it touches the device, the re-bind to the scene's device, and rc (incl. n_tile_slots / n_pix_slots; 0: this rank owns no tile)
int frame_geometry(pt_scene *sc, const PtRenderParams *rp, RenderConst &rc) {
    if (int st = check_spp(rp)) return st;
    if (!(rp->filter_radius[0] > 0.0f) || !(rp->filter_radius[1] > 0.0f)) return fail(PT_ERR_INVALID_ARG, "filter radius must be > 0");
    if (rp->tile_world > 1 && rp->tile_rank >= rp->tile_world) return fail(PT_ERR_INVALID_ARG, "tile_rank >= tile_world");
    if (sc->device != g_device) { int bst = bind_device(sc->device); if (bst) return bst; }
    fill_render_const(rp, rc);
    if (rc.film_w == 0 || rc.film_h == 0 || rc.ntx == 0 || rc.nty == 0) return fail(PT_ERR_INVALID_ARG, "empty film or sample bounds");
    if (rc.sobol.log2_resolution > 25) return fail(PT_ERR_INVALID_ARG, "sample bounds exceed the 2^25 Sobol' pixel grid");
    rc.n_tile_slots = tile_slots(rc);
    rc.n_pix_slots = rc.n_tile_slots * 256u;
    return PT_OK;
}
// The pass size S an integrator asked for or chose, for a call that renders n_samples sample numbers: capped at them; 0 when this rank owns no tile
int frame_pass_size(const RenderConst &rc, uint32_t S, uint32_t n_samples, uint32_t *S_out) {
    S = rc.n_pix_slots ? std::min(S, n_samples) : 0;
    if ((size_t)rc.n_pix_slots * S > ((size_t)1 << 31)) return fail(PT_ERR_INVALID_ARG, "pass too large: pixel slots x samples per pass > 2^31 paths (lower spp_per_pass)");
    *S_out = S;
    return PT_OK;
}

int add_device_film(const float *d_film, size_t film_px, float *film_xyzw) {   // host film += device film, element by element in index order
    std::vector<float> host(film_px * 4);
    HIP_TRY(hipMemcpy(host.data(), d_film, film_px * 16, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < film_px * 4; ++i) film_xyzw[i] += host[i];
    return PT_OK;
}
// The film's way out: k_film_finish adds the render's sums (sc->film_rgbw) to the caller's device film, or to a zeroed temporary that is then added to the host film
int deliver_film(pt_scene *sc, size_t film_px, float *film_xyzw, int film_is_device) {
    float *dst = film_xyzw; DevTmp film_tmp;
    if (!film_is_device) {
        HIP_TRY(film_tmp.alloc(&dst, film_px * 16));
        HIP_TRY(hipMemsetAsync(dst, 0, film_px * 16, sc->stream));
    }
    sc->begin("film_finish", film_px);
    launch(sc, "k_film_finish", k_film_finish, dim3((unsigned)((film_px + 255) / 256)), dim3(256), sc->film_rgbw, dst, film_px);
    sc->end();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(sc->stream));
    return film_is_device ? PT_OK : add_device_film(dst, film_px, film_xyzw);
}

// Sample numbers [first, first + n_samples) in passes of S, between the geometry function (rc, S) and the caller's film. `prepare`: what the integrator needs besides the
// workspace; `pass`: the camera rays of rc.s_count samples from rc.s_begin, waiting in ext[0], to their splats in sc->film_rgbw; `finish`: what it checks after the
// last one. A rank that owns no tile leaves zeroed counters and no stats.
int render_frame(pt_scene *sc, const PtRenderParams *rp, RenderConst &rc, uint32_t S, uint32_t first, uint32_t n_samples, float *film_xyzw, int film_is_device,
                 const FrameStep &prepare, const FrameStep &pass, const FrameStep &finish) {
    const size_t film_px = (size_t)rc.film_w * rc.film_h;
    sc->profile = rp->profile != 0;
    sc->drop_timings();
    sc->stats.clear();
    sc->counters = PtCounters{};
    if (rc.n_pix_slots == 0) return PT_OK;
    int st;
    if ((st = ensure_workspace(sc, (size_t)rc.n_pix_slots * S, film_px)) || (st = prepare())) return st;
    HIP_TRY(hipMemcpyAsync(sc->d_filter, rp->filter_table, 256 * 4, hipMemcpyHostToDevice, sc->stream));
    HIP_TRY(hipMemsetAsync(sc->film_rgbw, 0, film_px * 16, sc->stream));
    HIP_TRY(hipMemsetAsync(sc->dc, 0, sizeof(DevCounters), sc->stream));
    HIP_TRY(hipMemsetAsync(sc->qc, 0, sizeof(QCounters), sc->stream));
    for (uint32_t s0 = first, end = first + n_samples; s0 < end; s0 += S) {
        rc.s_begin = s0; rc.s_count = std::min(S, end - s0);
        HIP_TRY(hipMemsetAsync(sc->qc, 0, offsetof(QCounters, error), sc->stream));
        sc->begin("generate", (uint64_t)rc.n_pix_slots * rc.s_count);   // SamplerIntegrator::render's camera rays (integrator.rs:331-340): every integrator's pass starts from them
        launch(sc, generate_variant(rc.camera_type), blocks_for(rc.n_pix_slots * rc.s_count, PT_GEN_BLOCKS_PER_CU), dim3(256), rc, g_tabs, sc->ps, sc->q.ext[0], &sc->qc->ext[0], sc->dc);
        sc->end();
        if ((st = pass())) return st;
    }
    if (finish && (st = finish())) return st;
    if ((st = deliver_film(sc, film_px, film_xyzw, film_is_device))) return st;
    sc->resolve_timings();
    read_counters(sc);
    return PT_OK;
}

}  // namespace pth

extern "C" {

// The path integrators' geometry -- ONE function for pt_render and pt_pass_size, so that the size pt_pass_size reports is the size of a render that would be accepted
// (the two had drifted apart): the frame's checks, what path / volpath take, and *S_out = samples per pixel per wavefront pass (0 when this rank owns no tile).
// `n_samples`: how many of the job's rp->spp sample numbers the call renders (pt_render_samples; rp->spp for pt_render and pt_pass_size) -- the pass size is capped at it and
// the library's choice makes equal passes over it, while rc keeps the JOB's spp (rc.inv_sqrt_spp, the differential scale). `n_listed` (pt_render_tiles): the call renders
// that many listed tiles instead of the rank's share -- the tile slots are the list's entries (rc.tile_list, set once the list is on the device).
static int render_geometry(pt_scene *sc, const PtRenderParams *rp, uint32_t n_samples, RenderConst &rc, uint32_t *S_out, const uint32_t *n_listed = nullptr) {
    if (int st = frame_geometry(sc, rp, rc)) return st;
    if (n_listed) { rc.n_tile_slots = *n_listed; rc.n_pix_slots = rc.n_tile_slots * 256u; }
    if (rp->max_depth > 254) return fail(PT_ERR_INVALID_ARG, "maxdepth must be <= 254 (the bounce count of a path is kept in 8 bits)");
    if (rc.volpath) {   // VolPathIntegrator (volpath.rs): what this back end takes
        if (sc->has_bssrdf && sc->ds.n_media >= 0xffffu) return fail(PT_ERR_UNSUPPORTED, "volpath: subsurface materials with more than 65534 media");
        if (rp->camera_medium != PT_NONE && rp->camera_medium >= sc->ds.n_media) return fail(PT_ERR_INVALID_ARG, "camera_medium out of range");
    }
    uint32_t S = rp->spp_per_pass;
    if (S == 0 && rc.n_pix_slots > 0) S = choose_pass_size(sc, rc.n_pix_slots, n_samples, 1, rc.volpath != 0);
    return frame_pass_size(rc, S, n_samples, S_out);
}

int pt_pass_size(pt_scene *sc, const PtRenderParams *rp, uint32_t *spp_per_pass) {
    if (!sc || !rp || !spp_per_pass) return fail(PT_ERR_INVALID_ARG, "null argument");
    RenderConst rc; uint32_t S = 0;
    if (int st = render_geometry(sc, rp, rp->spp, rc, &S)) return st;
    *spp_per_pass = reported_pass_size(S, rp);
    return PT_OK;
}

int pt_render(pt_scene *sc, const PtRenderParams *rp, float *film_xyzw, int film_is_device) {   // the whole job: sample numbers [0, spp)
    if (!sc || !rp || !film_xyzw) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int st = check_spp(rp)) return st;
    return pt_render_samples(sc, rp, 0, rp->spp, film_xyzw, film_is_device);
}

// Sample numbers [first, first + n) of the job `rp` describes. Sample k of a pixel is a function of the pixel and k alone (k_generate: rc.s_begin + sl), the film is added
// to, and everything that depends on the job's sample count -- the differential scale -- reads rp->spp: the range only sets the pass loop's bounds.
// `tiles` != NULL (pt_render_tiles): on *n_listed checked tiles (check_tile_list) instead of the rank's share.
static int render_range(pt_scene *sc, const PtRenderParams *rp, uint32_t first, uint32_t n_samples, const uint32_t *tiles, const uint32_t *n_listed, float *film_xyzw, int film_is_device) {
    RenderConst rc; uint32_t S = 0;
    if (int gst = render_geometry(sc, rp, n_samples, rc, &S, n_listed)) return gst;
    if (n_listed && *n_listed > 0) {   // the list goes to the scene's device buffer (the device is bound by now); the render's stream carries it before the first launch
        const size_t n = *n_listed;
        if (!sc->stream) HIP_TRY(hipStreamCreate(&sc->stream));
        if (n > sc->tile_list_cap) {
            if (sc->tile_list) hipFree(sc->tile_list);
            sc->tile_list = nullptr; sc->tile_list_cap = 0;
            if (hipError_t e = hipMalloc((void **)&sc->tile_list, n * 4); e != hipSuccess) { (void)hipGetLastError(); sc->tile_list = nullptr; return fail(PT_ERR_OUT_OF_MEMORY, std::string("tile list: ") + hipGetErrorString(e)); }
            sc->tile_list_cap = n;
        }
        HIP_TRY(hipMemcpyAsync(sc->tile_list, tiles, n * 4, hipMemcpyHostToDevice, sc->stream));
        rc.tile_list = sc->tile_list;
    }
    int max_iterations = 1 << 20;   // wavefront iterations per pass. TEST HOOK (env PT_TEST_MAX_ITERATIONS, read at every call): a smaller cap, so that the PT_ERR_PROBE_CHAIN return of a pass that does not end can be tested
    if (const char *e = getenv("PT_TEST_MAX_ITERATIONS")) { const int v = atoi(e); if (v > 0) max_iterations = v; }
    struct CapReset { ~CapReset() { t_max_blocks = ~0u; } } cap_reset;   // TEST HOOK (env PT_TEST_MAX_BLOCKS): see blocks_for; the cap holds for this call alone
    if (const char *e = getenv("PT_TEST_MAX_BLOCKS")) { const int v = atoi(e); if (v > 0) t_max_blocks = (uint32_t)v; }
    int eff = 0;
    auto lazy_grid = [&]() { return sc->grid[eff].cell_ptr != nullptr; };   // first-touch voxels (PT_LS_SPATIAL_LAZY)
    auto prepare = [&]() {
        if (rc.volpath && sc->has_null_material && sc->ext_capacity < sc->capacity) {   // the shells' chain state (PathSoA::ext)
            if (sc->ext_slab) { hipFree(sc->ext_slab); sc->ext_slab = nullptr; sc->ext_capacity = 0; }
            if (hipMalloc(&sc->ext_slab, sc->capacity * (size_t)PathSoA::kExtWords * 4) != hipSuccess) { (void)hipGetLastError(); return fail(PT_ERR_OUT_OF_MEMORY, "volpath: chain state of material-less shells"); }
            sc->ext_capacity = sc->capacity;
        }
        sc->ps.ext = (rc.volpath && sc->has_null_material) ? (float *)sc->ext_slab : nullptr;
        if (int st = ensure_light_grid(sc, (int)rp->light_strategy, eff)) return st;
        if (lazy_grid()) {   // a render that failed half way may have named voxels it never computed -- start from a clean request list
            HIP_TRY(hipMemsetAsync(sc->lazy.req_flag, 0, sc->lazy.ncell * 4, sc->stream));
            HIP_TRY(hipMemsetAsync(sc->lazy.req_count, 0, 8, sc->stream));
        }
        return (int)PT_OK;
    };
    auto pass = [&]() { return run_pass(sc, rc, sc->grid[eff], rp->profile >= 2, max_iterations); };
    auto finish = [&]() {   // a vertex that looked up a voxel nobody had computed: cannot happen (k_light_touch names every voxel first)
        uint32_t missing = 0;
        if (!lazy_grid()) return (int)PT_OK;
        HIP_TRY(hipMemcpyAsync(&missing, sc->lazy.missing, 4, hipMemcpyDeviceToHost, sc->stream));
        HIP_TRY(hipStreamSynchronize(sc->stream));
        if (missing) { HIP_TRY(hipMemset(sc->lazy.missing, 0, 4)); return fail(PT_ERR_HIP, "internal: " + std::to_string(missing) + " light-distribution lookups hit a voxel that had not been computed"); }
        return (int)PT_OK;
    };
    return render_frame(sc, rp, rc, S, first, n_samples, film_xyzw, film_is_device, prepare, pass, finish);
}

int pt_render_samples(pt_scene *sc, const PtRenderParams *rp, uint32_t first, uint32_t n_samples, float *film_xyzw, int film_is_device) {
    if (!sc || !rp || !film_xyzw) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int rst = check_sample_range(rp, first, n_samples)) return rst;   // (before the device is touched)
    return render_range(sc, rp, first, n_samples, nullptr, nullptr, film_xyzw, film_is_device);
}

int pt_tile_grid(const PtRenderParams *rp, uint32_t *ntx, uint32_t *nty) {
    if (!rp || !ntx || !nty) return fail(PT_ERR_INVALID_ARG, "null argument");
    tile_grid(rp, ntx, nty);
    return PT_OK;
}

// pt_render_samples on listed tiles. The list replaces the shard rule in the one place the kernels derive a slot's tile (slot_tile, kern_film.h); an empty list is a
// rank that owns no tile: PT_OK, nothing launched, zeroed counters.
int pt_render_tiles(pt_scene *sc, const PtRenderParams *rp, uint32_t first, uint32_t n_samples, const uint32_t *tiles, uint32_t n_tiles, float *film_xyzw, int film_is_device) {
    if (!sc || !rp || !film_xyzw) return fail(PT_ERR_INVALID_ARG, "null argument");
    if (int rst = check_sample_range(rp, first, n_samples)) return rst;   // (all of this before the device is touched)
    if (rp->tile_world > 1) return fail(PT_ERR_INVALID_ARG, "pt_render_tiles: the tile list replaces the shard rule, params->tile_world must be 0 or 1");
    uint32_t ntx = 0, nty = 0; tile_grid(rp, &ntx, &nty);
    if (int lst = check_tile_list(tiles, n_tiles, (uint64_t)ntx * nty, "pt_render_tiles")) return lst;
    return render_range(sc, rp, first, n_samples, tiles, &n_tiles, film_xyzw, film_is_device);
}

int pt_film_resolve(const float *xyzw, uint32_t n, float scale, float *rgb) {  // film.rs:217-258 (host arithmetic)
    if (!xyzw || !rgb) return fail(PT_ERR_INVALID_ARG, "null argument");
    for (uint32_t i = 0; i < n; ++i) film_resolve_pixel(xyzw + 4 * (size_t)i, scale, rgb + 3 * (size_t)i);
    return PT_OK;
}

int pt_get_counters(const pt_scene *sc, PtCounters *out) {
    if (!sc || !out) return fail(PT_ERR_INVALID_ARG, "null argument");
    *out = sc->counters;
    return PT_OK;
}
int pt_get_kernel_stats(const pt_scene *sc, PtKernelStat *out, uint32_t max_entries, uint32_t *n_out) {
    if (!sc || !out || !n_out) return fail(PT_ERR_INVALID_ARG, "null argument");
    uint32_t n = (uint32_t)std::min<size_t>(max_entries, sc->stats.size());
    for (uint32_t i = 0; i < n; ++i) {
        std::memset(&out[i], 0, sizeof out[i]);
        std::snprintf(out[i].name, sizeof out[i].name, "%s", sc->stats[i].name.c_str());
        std::snprintf(out[i].kernel, sizeof out[i].kernel, "%s", sc->stats[i].kernel.c_str());
        out[i].launches = sc->stats[i].launches; out[i].total_ms = sc->stats[i].ms; out[i].items = sc->stats[i].items;
        out[i].bvh_nodes = sc->stats[i].nodes; out[i].triangle_tests = sc->stats[i].tris;
    }
    *n_out = n;
    return PT_OK;
}

}  // extern "C"
