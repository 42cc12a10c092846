// scene_plan.hip -- plan_validate / plan_build: the checks of a PtSceneDesc and the tables pt_scene_create derives from it, host arithmetic only (scene_plan.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include "scene_plan.h"
#include "dev_bsdf.h"      // disney_has_bssrdf
#include "dev_texture.h"   // kTexStack

namespace pth {

// Shade class of a material: by the number of BxDFs the material can produce, decided from its constant parameters (a textured parameter can take any value).
uint8_t material_class(const PtMaterial &m, bool specialise, bool untextured) {
    // `specialise`: hand out the classes of the lobe-SET kernels (metal, plastic-like, uber; kernels.h; PT_SHADE_SPECIALISE != 0) -- textured scenes too since round 6 (ADVICE r5:
    // one texture anywhere used to send every metal / plastic / uber vertex of the scene to the general kernels); the smooth-subsurface class in untextured scenes only
    auto textured = [&](int slot) { return m.tex[slot] >= 0; };
    auto black = [](const float c[3]) { return !(c[0] > 0.0f) && !(c[1] > 0.0f) && !(c[2] > 0.0f); };   // .clamps(0, inf).is_black()
    switch (m.type) {
    case PT_MAT_MATTE: return 0;
    case PT_MAT_MIRROR: return (uint8_t)kSpecClass;
    case PT_MAT_METAL: return specialise ? (uint8_t)kMetalClass : 1;
    case PT_MAT_SUBSTRATE: return 1;
    case PT_MAT_GLASS:   // glass.rs:57-92: one FresnelSpecular lobe when both roughnesses are 0, else up to two microfacet lobes
        if (textured(PT_MP_U_ROUGHNESS) || textured(PT_MP_V_ROUGHNESS)) return 2;
        return (m.u_roughness == 0.0f && m.v_roughness == 0.0f) ? (uint8_t)kSpecClass : 2;
    case PT_MAT_PLASTIC: return specialise ? (uint8_t)kPlasticClass : 2;
    case PT_MAT_UBER: {   // uber.rs:40-106: without specular reflection / transmission and fully opaque it is Lambertian + microfacet
        const bool opaque = !textured(PT_MP_OPACITY) && m.opacity[0] >= 1.0f && m.opacity[1] >= 1.0f && m.opacity[2] >= 1.0f;
        const bool no_spec = !textured(PT_MP_KR) && !textured(PT_MP_KT) && black(m.kr) && black(m.kt);
        if (opaque && no_spec) return specialise ? (uint8_t)kPlasticClass : 2;
        return specialise ? (uint8_t)kUberClass : 3;
    }
    case PT_MAT_SUBSURFACE:   // constant zero roughness: one FresnelSpecular lobe + the BSSRDF (subsurface.rs:84-109)
        if (specialise && untextured && m.u_roughness == 0.0f && m.v_roughness == 0.0f && !textured(PT_MP_U_ROUGHNESS) && !textured(PT_MP_V_ROUGHNESS)) return (uint8_t)kSssClass;
        return 3;
    default: return 3;
    }
}

void dist1d(const std::vector<float> &func, std::vector<float> &cdf, float &func_int) {
    size_t n = func.size();
    cdf.assign(n + 1, 0.0f);
    for (size_t i = 1; i < n + 1; ++i) cdf[i] = cdf[i - 1] + func[i - 1] / (float)n;
    func_int = cdf[n];
    if (func_int == 0.0f) { for (size_t i = 1; i < n + 1; ++i) cdf[i] = (float)i / (float)n; }
    else { for (size_t i = 1; i < n + 1; ++i) cdf[i] /= func_int; }
}

PrimBound transform_bounds(const float m[16], const float lo[3], const float hi[3]) {
    M4 t; std::memcpy(t.m, m, 64);
    const int corner[8][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 1, 1}, {1, 1, 0}, {1, 0, 1}, {1, 1, 1}};
    PrimBound out;
    for (int c = 0; c < 8; ++c) {
        V3 p = xf_point(t, V3(corner[c][0] ? hi[0] : lo[0], corner[c][1] ? hi[1] : lo[1], corner[c][2] ? hi[2] : lo[2]));
        const float pc[3] = {p.x, p.y, p.z};
        for (int k = 0; k < 3; ++k) { out.lo[k] = c ? std::fmin(out.lo[k], pc[k]) : pc[k]; out.hi[k] = c ? std::fmax(out.hi[k], pc[k]) : pc[k]; }
    }
    return out;
}

PtStatus sah_builder(const std::vector<PrimBound> &prims, uint32_t max_node_prims, std::vector<PtBVHNode> &nodes, std::vector<uint32_t> &ordered, std::string &) {
    build_sah_bvh(prims, max_node_prims, nodes, ordered);
    return PT_OK;
}

namespace {

PtStatus fail(std::string &msg, PtStatus code, const char *text) { msg = text; return code; }

bool instanced(const PtSceneDesc &d) { return d.n_instances > 0 && d.top_refs && d.n_top > 0; }
int tex_children(const PtTexture &t) {
    return (t.type == PT_TEX_MIX) ? 3 : (t.type == PT_TEX_SCALE || t.type == PT_TEX_CHECKERBOARD2D || t.type == PT_TEX_CHECKERBOARD3D || t.type == PT_TEX_DOTS) ? 2 : 0;
}

// One postfix program per texture node (children before parent): prog[off[r] .. off[r + 1]) evaluates node r on a value stack of at most kTexStack entries.
PtStatus tex_programs(const PtSceneDesc &d, std::vector<uint32_t> &off, std::vector<uint32_t> &prog, std::string &msg) {
    off.assign(d.n_textures + 1, 0); prog.clear();
    for (uint32_t r = 0; r < d.n_textures; ++r) {
        off[r] = (uint32_t)prog.size();
        // iterative post-order; the value-stack depth is tracked to validate kTexStack
        struct Fr { int node; int next; };
        std::vector<Fr> st{{(int)r, 0}};
        int depth = 0, max_depth = 0; size_t guard = 0;
        while (!st.empty()) {
            Fr &f = st.back();
            const int nchild = tex_children(d.textures[f.node]);
            if (f.next < nchild) { const int c = d.textures[f.node].child[f.next++]; st.push_back({c, 0}); if (++guard > 4096 || st.size() > 64) return fail(msg, PT_ERR_INVALID_ARG, "texture graph too deep or cyclic"); continue; }
            prog.push_back((uint32_t)f.node);
            depth += 1 - nchild; max_depth = std::max(max_depth, depth + nchild);
            st.pop_back();
        }
        if (max_depth > kTexStack) return fail(msg, PT_ERR_UNSUPPORTED, "texture expression needs a deeper value stack than kTexStack");
    }
    off[d.n_textures] = (uint32_t)prog.size();
    return PT_OK;
}

void prim_bound(const PtSceneDesc &d, uint32_t i, PrimBound &out) {
    const uint32_t idx = d.prim_shape[i] & 0x3fffffffu;
    if ((d.prim_shape[i] >> 30) == PT_SHAPE_SPHERE) {  // Shape::world_bound = transform_bounds(object_bound) (shape.rs:23-25, sphere.rs:53-57)
        const PtSphere &S = d.spheres[idx];
        const float lo[3] = {-S.radius, -S.radius, S.z_min}, hi[3] = {S.radius, S.radius, S.z_max};
        out = transform_bounds(S.object_to_world, lo, hi);
        return;
    }
    // Triangle::world_bound (triangle.rs:130-134)
    const float *a = d.P + 3 * (size_t)d.indices[3 * idx], *b = d.P + 3 * (size_t)d.indices[3 * idx + 1], *c = d.P + 3 * (size_t)d.indices[3 * idx + 2];
    for (int k = 0; k < 3; ++k) { out.lo[k] = std::fmin(std::fmin(a[k], b[k]), c[k]); out.hi[k] = std::fmax(std::fmax(a[k], b[k]), c[k]); }
}

// The two-wide and four-wide records of one accelerator and its packet order, appended to the plan's; references are offset by the bases it starts at.
void append_accel(ScenePlan &plan, uint32_t pad_records, const std::vector<PtBVHNode> &nn, const std::vector<uint32_t> &refs, uint32_t &root_ref, uint32_t &root_ref4) {
    std::vector<WideNode> &wide = plan.wide; std::vector<QuadNode> &quad = plan.quad;
    const uint32_t wbase = (uint32_t)wide.size(), pbase = (uint32_t)plan.packet_refs.size();
    std::vector<uint32_t> wide_id(nn.size(), 0);
    uint32_t n_int = 0;
    for (size_t i = 0; i < nn.size(); ++i) { if (nn[i].n_prims == 0) wide_id[i] = wbase + n_int++; else plan.leaf_last.push_back(pbase + nn[i].offset + nn[i].n_prims - 1); }
    auto ref_of = [&](uint32_t i) { return nn[i].n_prims ? (kLeafBit | (pbase + nn[i].offset)) : wide_id[i]; };
    wide.resize(wbase + n_int);
    for (size_t i = 0; i < nn.size(); ++i) {
        if (nn[i].n_prims) continue;
        WideNode &w = wide[wide_id[i]];
        const PtBVHNode &l = nn[i + 1], &r = nn[nn[i].offset];
        w.lmin[0] = l.bmin[0]; w.lmin[1] = l.bmin[1]; w.lmin[2] = l.bmin[2]; w.lmax0 = l.bmax[0];
        w.lmax12[0] = l.bmax[1]; w.lmax12[1] = l.bmax[2]; w.rmin01[0] = r.bmin[0]; w.rmin01[1] = r.bmin[1];
        w.rmin2 = r.bmin[2]; w.rmax[0] = r.bmax[0]; w.rmax[1] = r.bmax[1]; w.rmax[2] = r.bmax[2];
        w.left_ref = ref_of((uint32_t)i + 1); w.right_ref = ref_of(nn[i].offset);
        w.meta = nn[i].axis; w.pad = 0;
    }
    // four-wide records of the same tree (dev_scene.h: QuadNode): two binary levels per record, emitted depth first
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<uint32_t> todo;   // binary interior nodes that root a record, in emission order (their record = quad[qbase + position])
    std::vector<uint32_t> quad_id(nn.size(), PT_NONE);
    auto qref_of = [&](uint32_t i) { return nn[i].n_prims ? (kLeafBit | (pbase + nn[i].offset)) : quad_id[i]; };
    const uint32_t qbase = (uint32_t)quad.size();
    if (!nn.empty() && nn[0].n_prims == 0) {
        // pre-order numbering: a record's interior grandchildren root the next records, left to right
        std::vector<uint32_t> stack{0};
        while (!stack.empty()) {
            const uint32_t i = stack.back(); stack.pop_back();
            quad_id[i] = pad_records + qbase + (uint32_t)todo.size(); todo.push_back(i);   // (test hook: unused records in front of the pool, host_device.hip)
            uint32_t kids[4]; int nk = 0;
            for (uint32_t c : {(uint32_t)i + 1u, (uint32_t)nn[i].offset}) {
                if (nn[c].n_prims) continue;
                kids[nk++] = c + 1u; kids[nk++] = nn[c].offset;
            }
            for (int k = nk - 1; k >= 0; --k) if (nn[kids[k]].n_prims == 0) stack.push_back(kids[k]);
        }
    }
    quad.resize(qbase + todo.size());
    for (size_t t = 0; t < todo.size(); ++t) {
        const uint32_t i = todo[t];
        QuadNode &q = quad[qbase + t];
        for (int a = 0; a < 3; ++a) for (int k = 0; k < 4; ++k) { q.lo[a][k] = inf; q.hi[a][k] = -inf; }
        for (int k = 0; k < 4; ++k) q.ref[k] = PT_NONE;
        q.pad[0] = q.pad[1] = q.pad[2] = 0;
        const uint32_t c2[2] = {i + 1u, (uint32_t)nn[i].offset};
        uint32_t axes[3] = {nn[i].axis, 0u, 0u};
        auto put = [&](int slot, uint32_t n) {
            for (int a = 0; a < 3; ++a) { q.lo[a][slot] = nn[n].bmin[a]; q.hi[a][slot] = nn[n].bmax[a]; }
            q.ref[slot] = qref_of(n);
        };
        for (int side = 0; side < 2; ++side) {
            const uint32_t c = c2[side];
            if (nn[c].n_prims) put(2 * side, c);
            else { axes[1 + side] = nn[c].axis; put(2 * side, c + 1u); put(2 * side + 1, nn[c].offset); }
        }
        // order word: for each of the eight sign octants o = nx | ny << 1 | nz << 2, three bits at 3 o: bit 0 = the ray is negative along N's
        // axis (the right pair comes first), bit 1 = along L's (slot 1 before slot 0), bit 2 = along R's (slot 3 before slot 2)
        q.meta = 0;
        for (uint32_t o = 0; o < 8; ++o) q.meta |= (((o >> axes[0]) & 1u) | (((o >> axes[1]) & 1u) << 1) | (((o >> axes[2]) & 1u) << 2)) << (3u * o);
    }
    root_ref4 = nn.empty() ? 0u : qref_of(0);
    plan.packet_refs.insert(plan.packet_refs.end(), refs.begin(), refs.end());
    root_ref = ref_of(0);
}

}  // namespace


PtStatus plan_validate(const PtSceneDesc &d, std::string &msg) {
    if (d.n_prims == 0 || !d.prim_shape || !d.prim_material || !d.prim_light) return fail(msg, PT_ERR_INVALID_ARG, "scene has no primitives");
    if (d.n_triangles && (!d.P || !d.indices)) return fail(msg, PT_ERR_INVALID_ARG, "triangle arrays missing");
    if (d.n_spheres && !d.spheres) return fail(msg, PT_ERR_INVALID_ARG, "sphere array missing");
    const bool inst = instanced(d);
    if (d.n_instances && !inst) return fail(msg, PT_ERR_INVALID_ARG, "instances given without top_refs");
    // A count whose array is NULL. (Objects count with instancing only and images with textures only, as they are read; n_media with a NULL `media` keeps meaning
    // "no media", here as in the oracle. The last two rows: an environment map needs its importance image and a size.)
    const struct { uint64_t count; const void *array; const char *text; } arrays[] = {
        {d.n_materials, d.materials, "materials array missing"},
        {d.n_lights, d.lights, "lights array missing"},
        {d.n_textures, d.textures, "textures array missing"},
        {d.n_textures ? d.n_images : 0u, d.images, "images array missing"},
        {inst ? d.n_objects : 0u, d.objects, "objects array missing"},
        {inst ? d.n_instances : 0u, d.instances, "instances array missing"},
        {d.n_bssrdf_tables, d.bssrdf_tables, "bssrdf_tables array missing"},
        {d.env_texels ? 1u : 0u, d.env_importance, "env_texels without env_importance"},
        {d.env_texels ? 1u : 0u, (d.env_width && d.env_height) ? d.env_texels : nullptr, "env_texels with a zero env_width or env_height"},
    };
    for (const auto &a : arrays) if (a.count && !a.array) return fail(msg, PT_ERR_INVALID_ARG, a.text);
    for (uint32_t i = 0; i < 3 * d.n_triangles; ++i) if (d.indices[i] >= d.n_vertices) return fail(msg, PT_ERR_INVALID_ARG, "vertex index out of range");
    for (uint32_t i = 0; i < d.n_prims; ++i) {
        uint32_t s = d.prim_shape[i];
        const uint32_t kind = s >> 30, idx = s & 0x3fffffffu;
        if (!((kind == PT_SHAPE_TRIANGLE && idx < d.n_triangles) || (kind == PT_SHAPE_SPHERE && idx < d.n_spheres))) return fail(msg, PT_ERR_INVALID_ARG, "primitive shape reference out of range");
        if (d.prim_material[i] != PT_NONE && d.prim_material[i] >= d.n_materials) return fail(msg, PT_ERR_INVALID_ARG, "material index out of range");
        if (d.prim_light[i] != PT_NONE && d.prim_light[i] >= d.n_lights) return fail(msg, PT_ERR_INVALID_ARG, "light index out of range");
    }
    for (uint32_t i = 0; i < d.n_materials; ++i) {
        const PtMaterial &m = d.materials[i];
        if (m.type != PT_MAT_SUBSURFACE) continue;
        if (!d.bssrdf_tables || m.bssrdf_table >= d.n_bssrdf_tables) return fail(msg, PT_ERR_INVALID_ARG, "subsurface material without a BSSRDF table");
        const PtBSSRDFTable &t = d.bssrdf_tables[m.bssrdf_table];
        if (t.n_rho < 2 || t.n_radius < 2 || !t.rho_samples || !t.radius_samples || !t.profile || !t.rhoeff || !t.profile_cdf) return fail(msg, PT_ERR_INVALID_ARG, "incomplete BSSRDF table");
    }
    for (uint32_t i = 0; i < d.n_textures; ++i) {
        const PtTexture &t = d.textures[i];
        if (t.type > PT_TEX_DOTS) return fail(msg, PT_ERR_UNSUPPORTED, "texture type not implemented");
        for (int k = 0; k < 3; ++k) if (t.child[k] >= (int32_t)d.n_textures) return fail(msg, PT_ERR_INVALID_ARG, "texture child index out of range");
        if (t.type == PT_TEX_IMAGEMAP) {
            if (!d.images || t.image >= d.n_images) return fail(msg, PT_ERR_INVALID_ARG, "image texture without an image");
            const PtImage &im = d.images[t.image];
            auto pow2 = [](uint32_t v) { return v && !(v & (v - 1)); };
            if (!pow2(im.width) || !pow2(im.height) || !im.texels || (im.channels != 1 && im.channels != 3) || im.n_levels == 0 || im.n_levels > 16)
                return fail(msg, PT_ERR_INVALID_ARG, "PtImage must be a power-of-two MIPMap pyramid with 1 or 3 channels");
            if (t.wrap > PT_WRAP_BLACK) return fail(msg, PT_ERR_UNSUPPORTED, "ImageWrap::Clamp is not implemented");
            if (!t.trilinear && !d.ewa_weight_lut) return fail(msg, PT_ERR_INVALID_ARG, "EWA image texture without ewa_weight_lut");
        }
        if (tex_children(t) == 2 && (t.child[0] < 0 || t.child[1] < 0)) return fail(msg, PT_ERR_INVALID_ARG, "texture node needs two children");
        if (t.type == PT_TEX_MIX && (t.child[0] < 0 || t.child[1] < 0 || t.child[2] < 0)) return fail(msg, PT_ERR_INVALID_ARG, "mix texture needs three children");
    }
    for (const int32_t *arr : {d.tri_alpha, d.tri_shadow_alpha})
        if (arr) for (uint32_t i = 0; i < d.n_triangles; ++i) if (arr[i] >= (int32_t)d.n_textures) return fail(msg, PT_ERR_INVALID_ARG, "alpha-mask texture index out of range");
    for (uint32_t i = 0; i < d.n_materials; ++i) {
        const PtMaterial &m = d.materials[i];
        if (m.type > PT_MAT_DISNEY) return fail(msg, PT_ERR_INVALID_ARG, "unknown material type");
        if (m.type == PT_MAT_DISNEY) {   // disney.rs:741-836: BxDFs the parameters can produce; the shade class holds five
            const bool thin = m.disney_thin != 0;
            const float dw = (1.0f - m.disney[PT_DS_METALLIC]) * (1.0f - m.disney[PT_DS_SPECTRANS]);
            int n = 1 + (m.disney[PT_DS_CLEARCOAT] > 0.0f) + (m.disney[PT_DS_SPECTRANS] > 0.0f) + (thin ? 1 : 0);
            if (dw > 0.0f) n += (thin ? 2 : 1) + 1 + (m.disney[PT_DS_SHEEN] > 0.0f);
            if (n > 5) return fail(msg, PT_ERR_UNSUPPORTED, "disney material with more than 5 BxDFs");
            if (disney_has_bssrdf(m) && d.n_textures && m.tex[PT_MP_KD] >= 0) return fail(msg, PT_ERR_UNSUPPORTED, "disney: a textured color together with scatterdistance");
            if (disney_has_bssrdf(m) && (m.disney_scatter[0] <= 0.0f || m.disney_scatter[1] <= 0.0f || m.disney_scatter[2] <= 0.0f)) return fail(msg, PT_ERR_INVALID_ARG, "disney: scatterdistance must be positive in every channel");
        }
        if (m.type == PT_MAT_MIX) {   // mix.rs:25-50: two plain materials whose lobes fit the five-lobe shade class together
            auto lobes = [](const PtMaterial &q) { switch (q.type) { case PT_MAT_GLASS: return 2; case PT_MAT_PLASTIC: return 2; case PT_MAT_UBER: return 5; case PT_MAT_TRANSLUCENT: return 4; case PT_MAT_DISNEY: return 5; default: return 1; } };
            int total = 0;
            for (int k = 0; k < 2; ++k) {
                if (m.mix[k] >= d.n_materials) return fail(msg, PT_ERR_INVALID_ARG, "mix material index out of range");
                const PtMaterial &q = d.materials[m.mix[k]];
                if (q.type == PT_MAT_MIX || q.type == PT_MAT_SUBSURFACE || disney_has_bssrdf(q)) return fail(msg, PT_ERR_UNSUPPORTED, "mix of mix / subsurface materials");
                total += lobes(q);
            }
            if (total > 5) return fail(msg, PT_ERR_UNSUPPORTED, "mix material with more than 5 BxDFs");
        }
        for (int k = 0; k < 16; ++k) {   // (`> 0` without textures: a zero-initialised material names texture 0 in every slot)
            if (d.n_textures == 0 && m.tex[k] > 0) return fail(msg, PT_ERR_INVALID_ARG, "material references a texture but the scene has none");
            if (d.n_textures && m.tex[k] >= (int32_t)d.n_textures) return fail(msg, PT_ERR_INVALID_ARG, "material texture index out of range");
        }
    }
    for (uint32_t i = 0; i < d.n_lights; ++i) {
        const PtLight &L = d.lights[i];
        if (L.type == PT_LIGHT_DIFFUSE_AREA && L.prim >= d.n_prims) return fail(msg, PT_ERR_INVALID_ARG, "area light primitive out of range");
        if (L.type == PT_LIGHT_INFINITE && !d.env_texels) return fail(msg, PT_ERR_INVALID_ARG, "infinite light without env_texels");
    }
    if (d.split_method > PT_SPLIT_HLBVH) return fail(msg, PT_ERR_INVALID_ARG, "unknown split_method");
    // instancing: one BVH per multi-primitive object (api.rs:1692-1700), the top level over primitives and instances
    const uint32_t n_top = inst ? d.n_top : d.n_prims;
    if (inst) {
        for (uint32_t o = 0; o < d.n_objects; ++o)
            if (d.objects[o].n_prims == 0 || (uint64_t)d.objects[o].first_prim + d.objects[o].n_prims > d.n_prims) return fail(msg, PT_ERR_INVALID_ARG, "object primitive range out of bounds");
        for (uint32_t i = 0; i < d.n_instances; ++i) if (d.instances[i].object >= d.n_objects) return fail(msg, PT_ERR_INVALID_ARG, "instance object index out of range");
        for (uint32_t i = 0; i < n_top; ++i) {
            uint32_t r = d.top_refs[i];
            if ((r & PT_TOP_INSTANCE) ? ((r & ~PT_TOP_INSTANCE) >= d.n_instances) : (r >= d.n_prims)) return fail(msg, PT_ERR_INVALID_ARG, "top_refs entry out of range");
        }
    }
    if (d.nodes && d.n_nodes && d.ordered_prims) {   // an adopted top-level tree
        for (uint32_t i = 0; i < n_top; ++i) if (d.ordered_prims[i] >= n_top) return fail(msg, PT_ERR_INVALID_ARG, "ordered_prims entry out of range");
        for (uint32_t i = 0; i < d.n_nodes; ++i) {
            const PtBVHNode &n = d.nodes[i];
            // (an interior node's second child lies behind its first child's whole subtree -- the flattened tree is in pre-order, bvh.rs:662-703: a back edge would
            //  send the depth-first walks of plan_build, and the device's, round in circles)
            bool ok = n.n_prims ? ((uint64_t)n.offset + n.n_prims <= n_top) : (n.offset < d.n_nodes && n.offset > i + 1 && n.axis < 3);
            if (!ok) return fail(msg, PT_ERR_INVALID_ARG, "malformed BVH node");
        }
    }
    if (d.n_media && d.media) {   // participating media (volpath only)
        for (uint32_t i = 0; i < d.n_media; ++i) {
            const PtMedium &m = d.media[i];
            if (m.type > PT_MEDIUM_GRID) return fail(msg, PT_ERR_INVALID_ARG, "unknown medium type");
            if (m.type != PT_MEDIUM_GRID) continue;
            const size_t nvox = (size_t)m.nx * m.ny * m.nz;
            if (!m.density || nvox == 0 || nvox > ((size_t)1 << 31)) return fail(msg, PT_ERR_INVALID_ARG, "grid medium without a density grid");
            size_t k = 0;
            while (k < nvox && !(m.density[k] > 0.0f)) ++k;
            if (k == nvox) return fail(msg, PT_ERR_INVALID_ARG, "grid medium with no positive density");
        }
        if (d.prim_medium_inside && d.prim_medium_outside)
            for (uint32_t i = 0; i < d.n_prims; ++i)
                if ((d.prim_medium_inside[i] != PT_NONE && d.prim_medium_inside[i] >= d.n_media) || (d.prim_medium_outside[i] != PT_NONE && d.prim_medium_outside[i] >= d.n_media))
                    return fail(msg, PT_ERR_INVALID_ARG, "primitive medium index out of range");
    }
    std::vector<uint32_t> off, prog;
    return tex_programs(d, off, prog, msg);
}

PtStatus plan_build(const PtSceneDesc &d, const PlanOptions &opt, const AccelBuilder &build, ScenePlan &plan, std::string &msg) {
    PtStatus st;
    // ---- accelerators: one BVH per multi-primitive object (api.rs:1692-1700) + the top-level BVH (adopted or built)
    const bool inst = instanced(d);
    const uint32_t n_top = inst ? d.n_top : d.n_prims;
    const uint32_t maxp = d.max_node_prims ? d.max_node_prims : 4;
    struct ObjAccel { std::vector<PtBVHNode> nodes; std::vector<uint32_t> ordered; };
    std::vector<ObjAccel> obj(inst ? d.n_objects : 0);
    for (uint32_t o = 0; o < obj.size(); ++o) {
        const PtObject &O = d.objects[o];
        if (O.n_prims == 1) continue;
        std::vector<PrimBound> pb(O.n_prims);
        for (uint32_t i = 0; i < O.n_prims; ++i) prim_bound(d, O.first_prim + i, pb[i]);
        if ((st = build(pb, maxp, obj[o].nodes, obj[o].ordered, msg))) return st;
        for (auto &e : obj[o].ordered) e += O.first_prim;
    }
    auto top_ref = [&](uint32_t pos) { return inst ? d.top_refs[pos] : pos; };
    if (d.nodes && d.n_nodes && d.ordered_prims) {
        plan.nodes.assign(d.nodes, d.nodes + d.n_nodes);
        plan.ordered.assign(d.ordered_prims, d.ordered_prims + n_top);
        // The four-wide walk never tests the boxes of a record's collapsed children nor the root's: sound when every child's box lies inside its parent's, as in
        // every tree a union of primitive bounds builds. An adopted tree that is not nested is walked two-wide, box by box, like the reference does.
        for (uint32_t i = 0; i < d.n_nodes && !plan.exact_walk_only; ++i) {
            const PtBVHNode &n = plan.nodes[i];
            if (n.n_prims) continue;
            for (uint32_t c : {i + 1u, (uint32_t)n.offset}) for (int k = 0; k < 3; ++k)
                if (!(plan.nodes[c].bmin[k] >= n.bmin[k] && plan.nodes[c].bmax[k] <= n.bmax[k])) plan.exact_walk_only = true;
        }
    } else {
        std::vector<PrimBound> pb(n_top);
        for (uint32_t i = 0; i < n_top; ++i) {
            const uint32_t r = top_ref(i);
            if (!(r & PT_TOP_INSTANCE)) { prim_bound(d, r, pb[i]); continue; }
            // TransformedPrimitive::world_bound = prim_to_world.motion_bounds(inner bound) (primitive.rs:53-55, transform.rs:1564-1567)
            const PtInstance &I = d.instances[r & ~PT_TOP_INSTANCE];
            const PtObject &O = d.objects[I.object];
            PrimBound inner;
            if (O.n_prims == 1) prim_bound(d, O.first_prim, inner);
            else for (int k = 0; k < 3; ++k) { inner.lo[k] = obj[I.object].nodes[0].bmin[k]; inner.hi[k] = obj[I.object].nodes[0].bmax[k]; }
            pb[i] = transform_bounds(I.instance_to_world, inner.lo, inner.hi);
        }
        if ((st = build(pb, maxp, plan.nodes, plan.ordered, msg))) return st;
    }
    // ---- traversal records and the packet order of every accelerator: [top level][object 0][object 1]...
    {
        std::vector<uint32_t> top_order(n_top);
        for (uint32_t i = 0; i < n_top; ++i) top_order[i] = top_ref(plan.ordered[i]);
        append_accel(plan, opt.pool_pad_records, plan.nodes, top_order, plan.root_ref, plan.root_ref4);
    }
    std::vector<uint32_t> obj_root(obj.size(), 0), obj_root4(obj.size(), 0);
    for (size_t o = 0; o < obj.size(); ++o) {
        if (d.objects[o].n_prims == 1) {  // single primitive: a one-packet "leaf" without a BVH
            obj_root[o] = obj_root4[o] = kLeafBit | (uint32_t)plan.packet_refs.size();
            plan.leaf_last.push_back((uint32_t)plan.packet_refs.size());
            plan.packet_refs.push_back(d.objects[o].first_prim);
        } else append_accel(plan, opt.pool_pad_records, obj[o].nodes, obj[o].ordered, obj_root[o], obj_root4[o]);
    }
    plan.instances.resize(inst ? d.n_instances : 0);
    for (size_t i = 0; i < plan.instances.size(); ++i) {
        const PtInstance &I = d.instances[i]; DevInstance &D = plan.instances[i];
        std::memcpy(D.world_to_instance, I.world_to_instance, 64); std::memcpy(D.instance_to_world, I.instance_to_world, 64);
        D.single = d.objects[I.object].n_prims == 1; D.root_ref = obj_root[I.object]; D.root_ref4 = obj_root4[I.object];
        for (int k = 0; k < 3; ++k) { D.root_min[k] = D.single ? 0.0f : obj[I.object].nodes[0].bmin[k]; D.root_max[k] = D.single ? 0.0f : obj[I.object].nodes[0].bmax[k]; }
        bool ident = true;
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) ident = ident && I.instance_to_world[4 * r + c] == ((r == c) ? 1.0f : 0.0f);
        D.identity = ident;
    }
    // The production walk addresses records and packets as 16-byte quads of one pool (< 2^31 of each, < 64 GB together). The two-wide walk of pt_set_trace_exact
    // packs a skipped-entry count above 25-bit references: a larger scene has no exact walk (launch_trace refuses it) and its two-wide records are released.
    if (plan.quad.size() + opt.pool_pad_records >= ((size_t)1 << 28) || plan.packet_refs.size() >= ((size_t)1 << 31) - 2) return fail(msg, PT_ERR_UNSUPPORTED, "scene exceeds 2^28 four-wide BVH records / 2^31 packets");
    if (plan.wide.size() > (size_t)kRefMask || plan.packet_refs.size() > (size_t)kRefMask) { plan.quad_walk_only = true; plan.wide.clear(); plan.wide.shrink_to_fit(); }
    // an adopted tree that is not nested can only be walked two-wide, a scene beyond 2^25 records only four-wide: together no walk is left (such a scene
    // used to be accepted here and then failed at every traversal launch)
    if (plan.exact_walk_only && plan.quad_walk_only) return fail(msg, PT_ERR_UNSUPPORTED, "adopted BVH whose child boxes do not nest inside their parents' (needs the two-wide walk) in a scene beyond 2^25 records / packets (has the four-wide walk only)");
    if (plan.exact_walk_only) plan.warnings.push_back("warning: the adopted BVH's child boxes do not nest inside their parents'; this scene is walked two-wide, box by box (slower than the four-wide production walk)");
    if (plan.wide.empty()) plan.wide.resize(1);
    if (plan.quad.empty()) plan.quad.resize(1);
    plan.pad_bytes = (size_t)opt.pool_pad_records * sizeof(QuadNode);
    plan.quad_bytes = plan.pad_bytes + plan.quad.size() * sizeof(QuadNode);
    plan.pool_bytes = plan.quad_bytes + (plan.packet_refs.size() + 2) * sizeof(TriPacket);
    if (plan.pool_bytes / 16 >= (size_t)0xfffffff0u) return fail(msg, PT_ERR_UNSUPPORTED, "scene exceeds 64 GB of traversal records + packets");
    plan.pool_big = plan.pool_bytes >= (size_t)0xE0000000u;   // (beyond what the buffer loads' 32-bit byte offsets reach: k_trace<.., 2>)
    // ---- materials and lights
    plan.mat_class.assign(std::max<uint32_t>(1, d.n_materials), 0);
    for (uint32_t i = 0; i < d.n_materials; ++i) {   // (the volumetric router folds the lobe-set classes back into the lobe-count ones -- kern_aux.h: k_medium_route)
        plan.mat_class[i] = material_class(d.materials[i], opt.shade_specialise, d.n_textures == 0); plan.class_used[plan.mat_class[i]] = true;
        if (d.materials[i].type == PT_MAT_SUBSURFACE || disney_has_bssrdf(d.materials[i])) plan.has_bssrdf = true;
    }
    for (uint32_t i = 0; i < d.n_prims; ++i) if (d.prim_material[i] == PT_NONE) plan.has_null_material = true;
    for (uint32_t i = 0; i < d.n_lights; ++i) if (d.lights[i].type == PT_LIGHT_INFINITE) plan.infinite_lights.push_back(i);
    plan.light_head.assign(std::max<uint32_t>(1, d.n_lights), 0u);
    for (uint32_t i = 0; i < d.n_lights; ++i) plan.light_head[i] = light_rec_head(d.lights[i].type);
    // ---- textures: the programs, and per image its level offsets
    if (d.n_textures) {
        if ((st = tex_programs(d, plan.tex_prog_offset, plan.tex_prog, msg))) return st;
        plan.images.resize(d.n_images);
        for (uint32_t i = 0; i < d.n_images; ++i) {
            const PtImage &im = d.images[i]; DevImage &out = plan.images[i];
            out.width = im.width; out.height = im.height; out.n_levels = im.n_levels; out.channels = im.channels;
            if (!im.texels || im.n_levels == 0 || im.n_levels > 16) continue;   // unreferenced slot
            size_t o = 0;
            for (uint32_t l = 0; l < im.n_levels; ++l) { out.level_offset[l] = (uint32_t)o; o += (size_t)std::max(1u, im.width >> l) * std::max(1u, im.height >> l) * im.channels; }
        }
    }
    // ---- media
    if (d.n_media && d.media) {
        plan.grid_aux.assign(d.n_media, DevGridAux{nullptr, 0.0f, 0.0f});
        for (uint32_t i = 0; i < d.n_media; ++i) {   // GridDensityMedium::new (grid.rs:40-72)
            const PtMedium &m = d.media[i];
            if (m.type != PT_MEDIUM_GRID) continue;
            // grid.rs:46-52: `sigma_t = (sigma_a + sigma_s)[0]`; a spectrally varying coefficient is reported with error!() and rendering goes on with the first channel
            for (int k = 1; k < 3; ++k) if (m.sigma_a[k] + m.sigma_s[k] != m.sigma_a[0] + m.sigma_s[0]) { plan.warnings.push_back("GridDensityMedium requires spectrally uniform attenuation coefficient (medium " + std::to_string(i) + ": using channel 0, as grid.rs:46-52 does)"); break; }
            const size_t nvox = (size_t)m.nx * m.ny * m.nz;
            float maxd = 0.0f;
            for (size_t k = 0; k < nvox; ++k) maxd = std::fmax(maxd, m.density[k]);
            plan.grid_aux[i].sigma_t = m.sigma_a[0] + m.sigma_s[0]; plan.grid_aux[i].inv_max_density = 1.0f / maxd;
            plan.has_grid = true;
        }
        plan.class_used[kMediumClass] = true;
    }
    // ---- environment map: Distribution2D::new (sampling.rs:100-117) over the importance image
    if (d.env_texels) {
        const size_t nu = 2 * (size_t)d.env_width, nv = 2 * (size_t)d.env_height;
        plan.env_cdf.resize(nv * (nu + 1)); plan.env_func_int.resize(nv);
        std::vector<float> row, c;
        for (size_t v = 0; v < nv; ++v) {
            row.assign(d.env_importance + v * nu, d.env_importance + (v + 1) * nu);
            dist1d(row, c, plan.env_func_int[v]);
            std::copy(c.begin(), c.end(), plan.env_cdf.begin() + v * (nu + 1));
        }
        dist1d(plan.env_func_int, plan.env_marg_cdf, plan.env_marg_int);
    }
    // ---- the environment light's uniform block: the first infinite light's transforms; the tables of a 1 x 1 map, copied from the arrays above
    std::memset(&plan.env_u, 0, sizeof plan.env_u);
    plan.env_u.light = PT_NONE;
    if (!plan.infinite_lights.empty()) {
        const PtLight &L = d.lights[plan.infinite_lights[0]];
        plan.env_u.light = plan.infinite_lights[0];
        std::copy(L.world_to_light, L.world_to_light + 16, plan.env_u.world_to_light); std::copy(L.light_to_world, L.light_to_world + 16, plan.env_u.light_to_world);
    }
    if (d.env_texels && d.env_width == 1 && d.env_height == 1) {
        EnvUniform &e = plan.env_u;
        std::copy(d.env_texels, d.env_texels + 3, e.texel0);
        std::copy(plan.env_marg_cdf.begin(), plan.env_marg_cdf.begin() + 3, e.marg_cdf); e.marg_int = plan.env_marg_int;
        for (int v = 0; v < 2; ++v) {
            e.row_int[v] = plan.env_func_int[v];
            std::copy(plan.env_cdf.begin() + 3 * v, plan.env_cdf.begin() + 3 * v + 3, e.row_cdf[v]);
            std::copy(d.env_importance + 2 * v, d.env_importance + 2 * v + 2, e.row_func[v]);
        }
    }
    // ---- world bound = root node bounds (bvh.rs:697-703); Light::preprocess -> bounding sphere (bounds.rs:516-524)
    bool inside = true;
    for (int k = 0; k < 3; ++k) {
        plan.wb_min[k] = plan.nodes[0].bmin[k]; plan.wb_max[k] = plan.nodes[0].bmax[k];
        plan.world_center[k] = (plan.wb_min[k] + plan.wb_max[k]) * (1.0f / 2.0f);
        inside = inside && plan.world_center[k] >= plan.wb_min[k] && plan.world_center[k] <= plan.wb_max[k];
    }
    const float dx = plan.wb_max[0] - plan.world_center[0], dy = plan.wb_max[1] - plan.world_center[1], dz = plan.wb_max[2] - plan.world_center[2];
    plan.world_radius = inside ? std::sqrt(dx * dx + dy * dy + dz * dz) : 0.0f;
    return PT_OK;
}

}  // namespace pth
