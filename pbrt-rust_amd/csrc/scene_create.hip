// scene_create.hip -- pt_scene_create / destroy / bvh read-back: the plan of scene_plan.h (checks, accelerators, derived tables), then uploads (host_common.h has the map).
#include "host_common.h"

#include <memory>

namespace {
// BVHAccel::new with SplitMethod::HLBVH on the device (gpu_bvh.hip); plan_build's other builder is the host's SAH (bvh.rs:145-198, the reference's tree)
PtStatus hlbvh_builder(const std::vector<pth::PrimBound> &pb, uint32_t maxp, std::vector<PtBVHNode> &nodes, std::vector<uint32_t> &ordered, std::string &msg) {
    const char *text = "HLBVH build failed";
    if (!pth::build_hlbvh_gpu(pb, maxp, nodes, ordered, &text)) return PT_OK;
    msg = text;
    return PT_ERR_HIP;
}
// The uploads of one scene: the first failure sticks and skips the rest.
struct Uploader {
    pt_scene *sc; int st = PT_OK;
    template <class T> void operator()(const T **field, const T *src, size_t count) { if (!st) st = sc->upload(field, src, count); }
    template <class T> void operator()(const T **field, const std::vector<T> &v) { (*this)(field, v.data(), v.size()); }
};
}  // namespace

extern "C" {

// plan_validate, ensure_device, plan_build (scene_plan.h: every refusal and every derived table, host only), then uploads, the record / packet pool and three small
// kernels: past `new pt_scene()` only an allocation, a copy or a kernel can fail.
int pt_scene_create(const PtSceneDesc *d, pt_scene **out) {
    if (!d || !out) return fail(PT_ERR_INVALID_ARG, "null argument");
    std::string msg;
    int st = plan_validate(*d, msg);
    if (st) return fail(st, msg);
    if ((st = ensure_device())) return st;
    ScenePlan plan;
    if ((st = plan_build(*d, PlanOptions{g_shade_specialise, g_test_pool_pad_records}, d->split_method == PT_SPLIT_HLBVH ? AccelBuilder(hlbvh_builder) : AccelBuilder(sah_builder), plan, msg))) return fail(st, msg);
    for (const std::string &w : plan.warnings) fprintf(stderr, "mi355pt: %s\n", w.c_str());

    std::unique_ptr<pt_scene, void (*)(pt_scene *)> owner(new pt_scene(), pt_scene_destroy);
    pt_scene *sc = owner.get();
    DeviceScene &ds = sc->ds;
    sc->device = g_device;
    sc->nodes = std::move(plan.nodes); sc->ordered = std::move(plan.ordered);
    sc->exact_walk_only = plan.exact_walk_only; sc->quad_walk_only = plan.quad_walk_only; sc->pool_big = plan.pool_big;
    std::copy(plan.class_used, plan.class_used + kNumClasses, sc->class_used);
    sc->has_null_material = plan.has_null_material; sc->has_bssrdf = plan.has_bssrdf;
    sc->n_lights = d->n_lights;
    if (d->n_lights) sc->host_lights.assign(d->lights, d->lights + d->n_lights);
    if (d->env_texels) { sc->env_w = d->env_width; sc->env_h = d->env_height; for (int k = 0; k < 3; ++k) sc->env_texel0[k] = d->env_power_lookup[k]; }

    // ---- uploads: the plan's tables, and the caller's arrays straight from the descriptor
    Uploader up{sc};
    up(&ds.wide, plan.wide); ds.root_ref = plan.root_ref; ds.root_ref4 = plan.root_ref4; ds.n_nodes = (uint32_t)sc->nodes.size();
    for (int k = 0; k < 3; ++k) { ds.root_min[k] = sc->nodes[0].bmin[k]; ds.root_max[k] = sc->nodes[0].bmax[k]; }
    up(&ds.instances, plan.instances); ds.n_instances = (uint32_t)plan.instances.size();
    up(&ds.P, d->P, 3 * (size_t)d->n_vertices);
    if (d->N) up(&ds.N, d->N, 3 * (size_t)d->n_vertices);
    if (d->S) up(&ds.S, d->S, 3 * (size_t)d->n_vertices);
    if (d->UV) up(&ds.UV, d->UV, 2 * (size_t)d->n_vertices);
    up(&ds.indices, d->indices, 3 * (size_t)d->n_triangles); ds.n_triangles = d->n_triangles;
    {
        std::vector<uint8_t> fl(d->n_triangles, 0);
        if (d->tri_flags) fl.assign(d->tri_flags, d->tri_flags + d->n_triangles);
        for (auto &f : fl) { if (!d->N) f &= ~PT_TRI_HAS_N; if (!d->S) f &= ~PT_TRI_HAS_S; if (!d->UV) f &= ~PT_TRI_HAS_UV; }
        up(&ds.tri_flags, fl);
    }
    up(&ds.prim_shape, d->prim_shape, d->n_prims); up(&ds.prim_material, d->prim_material, d->n_prims); up(&ds.prim_light, d->prim_light, d->n_prims);
    ds.n_prims = d->n_prims;
    up(&ds.materials, d->materials, d->n_materials); ds.n_materials = d->n_materials;
    if (d->n_media && d->media) {   // participating media (volpath only)
        up(&ds.media, d->media, d->n_media); ds.n_media = d->n_media;
        for (uint32_t i = 0; i < d->n_media; ++i)
            if (d->media[i].type == PT_MEDIUM_GRID) up(&plan.grid_aux[i].density, d->media[i].density, (size_t)d->media[i].nx * d->media[i].ny * d->media[i].nz);
        up(&ds.grid_aux, plan.grid_aux); ds.has_grid = plan.has_grid ? 1u : 0u;
        if (d->prim_medium_inside && d->prim_medium_outside) { up(&ds.prim_med_in, d->prim_medium_inside, d->n_prims); up(&ds.prim_med_out, d->prim_medium_outside, d->n_prims); }
    }
    ds.has_shells = sc->has_null_material ? 1u : 0u;
    up(&ds.spheres, d->spheres, d->n_spheres); ds.n_spheres = d->n_spheres;
    up(&ds.lights, d->lights, d->n_lights); ds.n_lights = d->n_lights;
    up(&ds.mat_class, plan.mat_class);
    {
        std::vector<DevBssTable> bt(d->n_bssrdf_tables);
        for (uint32_t i = 0; i < d->n_bssrdf_tables; ++i) {
            const PtBSSRDFTable &t = d->bssrdf_tables[i];
            bt[i].n_rho = (int)t.n_rho; bt[i].n_radius = (int)t.n_radius;
            if (!t.rho_samples || !t.radius_samples || !t.profile || !t.rhoeff || !t.profile_cdf) continue;   // unreferenced slot
            up(&bt[i].rho_samples, t.rho_samples, t.n_rho); up(&bt[i].radius_samples, t.radius_samples, t.n_radius);
            up(&bt[i].profile, t.profile, (size_t)t.n_rho * t.n_radius);
            up(&bt[i].rhoeff, t.rhoeff, t.n_rho);
            up(&bt[i].profile_cdf, t.profile_cdf, (size_t)t.n_rho * t.n_radius);
        }
        up(&ds.bss_tables, bt); ds.n_bss_tables = d->n_bssrdf_tables;
    }
    if (d->n_textures) {   // textures: nodes as given + one postfix program per node
        up(&ds.textures, d->textures, d->n_textures); ds.n_textures = d->n_textures;
        up(&ds.tex_prog_offset, plan.tex_prog_offset); up(&ds.tex_prog, plan.tex_prog);
        for (uint32_t i = 0; i < d->n_images; ++i) {
            const PtImage &im = d->images[i];
            if (!im.texels || im.n_levels == 0 || im.n_levels > 16) continue;   // unreferenced slot
            const uint32_t last = im.n_levels - 1;
            up(&plan.images[i].texels, im.texels, plan.images[i].level_offset[last] + (size_t)std::max(1u, im.width >> last) * std::max(1u, im.height >> last) * im.channels);
        }
        up(&ds.images, plan.images);
        if (d->ewa_weight_lut) up(&ds.ewa_lut, d->ewa_weight_lut, 128);
        auto any_mask = [&](const int32_t *a) { if (!a) return false; for (uint32_t i = 0; i < d->n_triangles; ++i) if (a[i] >= 0) return true; return false; };
        if (any_mask(d->tri_alpha)) up(&ds.tri_alpha, d->tri_alpha, d->n_triangles);
        if (any_mask(d->tri_shadow_alpha)) up(&ds.tri_shadow_alpha, d->tri_shadow_alpha, d->n_triangles);
    }
    up(&ds.infinite_lights, plan.infinite_lights); ds.n_infinite = (uint32_t)plan.infinite_lights.size();
    up(&ds.env_u, &plan.env_u, 1);
    if (d->env_texels) {
        ds.env_w = d->env_width; ds.env_h = d->env_height;
        up(&ds.env_texels, d->env_texels, 3 * (size_t)ds.env_w * ds.env_h);
        up(&ds.env_func, d->env_importance, 4 * (size_t)ds.env_w * ds.env_h); up(&ds.env_cdf, plan.env_cdf); up(&ds.env_func_int, plan.env_func_int);
        up(&ds.env_marg_func, plan.env_func_int); up(&ds.env_marg_cdf, plan.env_marg_cdf); ds.env_marg_int = plan.env_marg_int;
    }
    for (int k = 0; k < 3; ++k) { ds.wb_min[k] = plan.wb_min[k]; ds.wb_max[k] = plan.wb_max[k]; ds.world_center[k] = plan.world_center[k]; }
    ds.world_radius = plan.world_radius;
    const uint32_t *d_ordered = nullptr, *d_last = nullptr, *d_head = nullptr;
    up(&d_ordered, plan.packet_refs); up(&d_head, plan.light_head);
    if (up.st) return up.st;

    // ---- the four-wide records and the packets share ONE allocation, so that the production traversal addresses both with 32-bit quad indices from one
    // base (records of 8 quads, packets of 3; < 64 GB): [pad][records][packets + 2] (scene_plan.h)
    const uint32_t n_packets = (uint32_t)plan.packet_refs.size(), n_leaves = (uint32_t)plan.leaf_last.size();
    uint8_t *pool = nullptr; float *area = nullptr; float4 *lrec = nullptr;
    if ((st = sc->dalloc(&pool, plan.pool_bytes))) return st;
    // (record 0 is read as a dummy by the leaf lanes of k_trace<.., 2>, which aim their five node-only loads at it: with the test hook's pad in front of the pool that is pad memory)
    if (plan.pad_bytes && hipMemset(pool, 0, plan.pad_bytes) != hipSuccess) return fail(PT_ERR_HIP, "memset of the pool pad");
    if (hipMemcpy(pool + plan.pad_bytes, plan.quad.data(), plan.quad_bytes - plan.pad_bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(PT_ERR_HIP, "upload of the four-wide records");
    TriPacket *leaf = reinterpret_cast<TriPacket *>(pool + plan.quad_bytes);
    ds.quad = reinterpret_cast<const QuadNode *>(pool); ds.leaf_off = (uint32_t)(plan.quad_bytes / 16); ds.pool_quads = (uint32_t)(plan.pool_bytes / 16);
    if (hipMemset(leaf, 0, ((size_t)n_packets + 2) * sizeof(TriPacket)) != hipSuccess) return fail(PT_ERR_HIP, "memset");
    if ((st = sc->dalloc(&area, std::max<uint32_t>(1, d->n_lights)))) return st;
    if ((st = sc->dalloc(&lrec, 6 * (size_t)std::max<uint32_t>(1, d->n_lights)))) return st;
    up(&d_last, plan.leaf_last);
    if (up.st) return up.st;
    // ---- leaf triangle packets, leaf ends, light areas and records (device)
    hipLaunchKernelGGL(k_build_packets, dim3((n_packets + 255) / 256), dim3(256), 0, 0, ds, d_ordered, n_packets, leaf);
    ds.leaf = leaf;
    hipLaunchKernelGGL(k_mark_leaf_ends, dim3((n_leaves + 255) / 256), dim3(256), 0, 0, leaf, d_last, n_leaves);
    if (d->n_lights) hipLaunchKernelGGL(k_light_area, dim3((d->n_lights + 255) / 256), dim3(256), 0, 0, ds, d_head, area, lrec);
    ds.light_area = area; ds.light_rec = lrec;
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return fail(PT_ERR_HIP, "scene preparation kernels failed");
    *out = owner.release();
    return PT_OK;
}

void pt_scene_destroy(pt_scene *sc) {
    if (!sc) return;
    if (sc->device != g_device) bind_device(sc->device);
    for (void *p : sc->allocs) hipFree(p);
    if (sc->slab) hipFree(sc->slab);
    if (sc->qbuf) hipFree(sc->qbuf);
    if (sc->bss_slab) hipFree(sc->bss_slab);
    if (sc->ext_slab) hipFree(sc->ext_slab);
    if (sc->film_rgbw) hipFree(sc->film_rgbw);
    if (sc->tile_list) hipFree(sc->tile_list);
    sc->drop_timings();
    for (auto e : sc->event_pool) hipEventDestroy(e);
    if (sc->stream) hipStreamDestroy(sc->stream);
    delete sc;
}

int pt_scene_bvh_info(const pt_scene *sc, uint32_t *n_nodes, uint32_t *n_prims) {
    if (!sc || !n_nodes || !n_prims) return fail(PT_ERR_INVALID_ARG, "null argument");
    *n_nodes = (uint32_t)sc->nodes.size(); *n_prims = (uint32_t)sc->ordered.size();
    return PT_OK;
}
int pt_scene_bvh_read(const pt_scene *sc, PtBVHNode *nodes, uint32_t *ordered) {
    if (!sc || !nodes || !ordered) return fail(PT_ERR_INVALID_ARG, "null argument");
    std::memcpy(nodes, sc->nodes.data(), sc->nodes.size() * sizeof(PtBVHNode));
    std::memcpy(ordered, sc->ordered.data(), sc->ordered.size() * 4);
    return PT_OK;
}

}  // extern "C"
