// check_plan.cpp -- a stand-alone check of the scene plan (csrc/scene_plan.h) on the CPU: every refusal of plan_validate / plan_build that a toy scene can provoke,
// the two- and four-wide traversal records against the binary tree they are made from, and the derived tables against formulas written out here.
// Built from scene_plan.hip + host_bvh.cpp, host code only (tests/test_abi_and_host.py); argv[1] = the path of scene_plan.hip, whose refusal texts are counted.
// Exit status 0 = every check passed.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <set>
#include <sstream>
#include "scene_plan.h"
#include "dev_texture.h"   // kTexStack

using namespace pth;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond, ...) do { ++g_checked; if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
static void translation(float m[16], float x, float y, float z) { std::memcpy(m, kIdentity, 64); m[3] = x; m[7] = y; m[11] = z; }

// A scene that owns its arrays; desc() points a PtSceneDesc at them.
struct Toy {
    std::vector<float> P, N, UV, env_texels, env_importance, lut, texels, density;
    std::vector<uint32_t> indices, prim_shape, prim_material, prim_light, top_refs, med_in, med_out, ordered;
    std::vector<uint8_t> tri_flags;
    std::vector<int32_t> tri_alpha;
    std::vector<PtSphere> spheres;
    std::vector<PtMaterial> materials;
    std::vector<PtLight> lights;
    std::vector<PtTexture> textures;
    std::vector<PtImage> images;
    std::vector<PtObject> objects;
    std::vector<PtInstance> instances;
    std::vector<PtMedium> media;
    std::vector<PtBSSRDFTable> tables;
    std::vector<PtBVHNode> nodes;
    float bss[2 + 2 + 4 + 2 + 4] = {0.1f, 0.9f, 0.0f, 1.0f, 0.5f, 0.25f, 0.5f, 0.25f, 0.3f, 0.7f, 0.5f, 1.0f, 0.5f, 1.0f};
    uint32_t env_w = 0, env_h = 0, max_node_prims = 4, split_method = PT_SPLIT_SAH;

    PtSceneDesc desc() {
        PtSceneDesc d; std::memset(&d, 0, sizeof d);
        d.n_vertices = (uint32_t)P.size() / 3; d.P = P.data(); d.N = N.empty() ? nullptr : N.data(); d.UV = UV.empty() ? nullptr : UV.data();
        d.n_triangles = (uint32_t)indices.size() / 3; d.indices = indices.data(); d.tri_flags = tri_flags.empty() ? nullptr : tri_flags.data();
        d.n_spheres = (uint32_t)spheres.size(); d.spheres = spheres.data();
        d.n_prims = (uint32_t)prim_shape.size(); d.prim_shape = prim_shape.data(); d.prim_material = prim_material.data(); d.prim_light = prim_light.data();
        d.n_materials = (uint32_t)materials.size(); d.materials = materials.data();
        d.n_lights = (uint32_t)lights.size(); d.lights = lights.data();
        if (env_w) { d.env_width = env_w; d.env_height = env_h; d.env_texels = env_texels.data(); d.env_importance = env_importance.data(); d.env_power_lookup[0] = 1.0f; }
        d.max_node_prims = max_node_prims; d.split_method = split_method;
        if (!nodes.empty()) { d.n_nodes = (uint32_t)nodes.size(); d.nodes = nodes.data(); d.ordered_prims = ordered.data(); }
        if (!instances.empty()) { d.n_objects = (uint32_t)objects.size(); d.objects = objects.data(); d.n_instances = (uint32_t)instances.size(); d.instances = instances.data(); d.n_top = (uint32_t)top_refs.size(); d.top_refs = top_refs.data(); }
        for (size_t i = 0; i < tables.size(); ++i) { tables[i].rho_samples = bss; tables[i].radius_samples = bss + 2; tables[i].profile = bss + 4; tables[i].rhoeff = bss + 8; tables[i].profile_cdf = bss + 10; }
        d.n_bssrdf_tables = (uint32_t)tables.size(); d.bssrdf_tables = tables.empty() ? nullptr : tables.data();
        d.n_textures = (uint32_t)textures.size(); d.textures = textures.empty() ? nullptr : textures.data();
        d.tri_alpha = tri_alpha.empty() ? nullptr : tri_alpha.data();
        for (auto &im : images) im.texels = texels.data();
        d.n_images = (uint32_t)images.size(); d.images = images.empty() ? nullptr : images.data(); d.ewa_weight_lut = lut.empty() ? nullptr : lut.data();
        for (auto &m : media) if (m.type == PT_MEDIUM_GRID) m.density = density.data();
        if (!media.empty()) { d.n_media = (uint32_t)media.size(); d.media = media.data(); d.prim_medium_inside = med_in.data(); d.prim_medium_outside = med_out.data(); }
        return d;
    }
    void add_triangle(const float v[9], uint32_t material) {
        const uint32_t base = (uint32_t)P.size() / 3, tri = (uint32_t)indices.size() / 3;
        P.insert(P.end(), v, v + 9);
        for (uint32_t k = 0; k < 3; ++k) indices.push_back(base + k);
        add_prim(PT_SHAPE_REF(PT_SHAPE_TRIANGLE, tri), material);
    }
    void add_prim(uint32_t shape, uint32_t material) { prim_shape.push_back(shape); prim_material.push_back(material); prim_light.push_back(PT_NONE); }
};

static PtMaterial plain_material(uint32_t type) {
    PtMaterial m; std::memset(&m, 0, sizeof m);
    m.type = type; m.kd[0] = m.kd[1] = m.kd[2] = 0.5f; m.eta = 1.5f;
    for (int k = 0; k < 16; ++k) m.tex[k] = -1;
    return m;
}
static PtTexture texture_node(uint32_t type, int c0 = -1, int c1 = -1, int c2 = -1) {
    PtTexture t; std::memset(&t, 0, sizeof t);
    t.type = type; t.child[0] = c0; t.child[1] = c1; t.child[2] = c2; t.value[0] = t.value[1] = t.value[2] = 0.5f; t.su = t.sv = 1.0f; t.trilinear = 1; t.max_anisotropy = 8.0f;
    return t;
}

struct Rng {   // a 64-bit LCG: the seeded triangles
    uint64_t s;
    float next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (float)((s >> 40) & 0xffffffu) / 16777216.0f; }
};
static Toy random_triangles(uint32_t n, uint64_t seed, uint32_t maxp) {
    Toy t; t.max_node_prims = maxp; t.materials.push_back(plain_material(PT_MAT_MATTE));
    Rng r{seed};
    for (uint32_t i = 0; i < n; ++i) {
        float v[9]; const float c[3] = {10.0f * r.next(), 10.0f * r.next(), 10.0f * r.next()};
        for (int k = 0; k < 9; ++k) v[k] = c[k % 3] + r.next();
        t.add_triangle(v, 0);
    }
    return t;
}

// The valid scene with every feature: four top-level triangles with N and UV, a sphere and a disk, a two-triangle object and a one-triangle object instanced once each
// (the second with an identity matrix), an imagemap -> scale -> mix texture chain, an alpha mask, a subsurface material with a two-by-two table, a homogeneous and a
// 2 x 2 x 2 grid medium, a 2 x 1 environment map.
static Toy valid_scene(uint32_t maxp = 4) {
    Toy t; t.max_node_prims = maxp;
    t.materials = {plain_material(PT_MAT_MATTE), plain_material(PT_MAT_SUBSURFACE), plain_material(PT_MAT_MATTE)};
    t.materials[0].tex[PT_MP_KD] = 4; t.materials[1].bssrdf_table = 0;
    Rng r{7};
    for (uint32_t i = 0; i < 7; ++i) {   // triangles 0-3: top level; 4, 5: object 0; 6: object 1
        float v[9]; const float c[3] = {4.0f * r.next(), 4.0f * r.next(), 4.0f * r.next()};
        for (int k = 0; k < 9; ++k) v[k] = c[k % 3] + r.next();
        if (i == 4) {   // (the sphere and the disk sit between the top-level triangles and the objects' in the primitive list)
            t.add_prim(PT_SHAPE_REF(PT_SHAPE_SPHERE, 0), 1); t.add_prim(PT_SHAPE_REF(PT_SHAPE_SPHERE, 1), 2);
        }
        t.add_triangle(v, i == 0 ? 0 : 2);
    }
    t.N.assign(t.P.size(), 0.0f); for (size_t i = 2; i < t.N.size(); i += 3) t.N[i] = 1.0f;
    t.UV.assign(t.P.size() / 3 * 2, 0.25f);
    t.tri_flags.assign(7, PT_TRI_HAS_N | PT_TRI_HAS_UV);
    t.tri_alpha.assign(7, -1); t.tri_alpha[0] = 0;
    PtSphere s; std::memset(&s, 0, sizeof s);
    translation(s.object_to_world, 6, 1, 2); translation(s.world_to_object, -6, -1, -2);
    s.radius = 1.5f; s.z_min = -1.5f; s.z_max = 1.0f; s.theta_min = 3.14159265f; s.theta_max = 0.8410687f; s.phi_max = 6.2831853f; s.kind = PT_QUADRIC_SPHERE;
    t.spheres.push_back(s);
    translation(s.object_to_world, -3, 0, 1); translation(s.world_to_object, 3, 0, -1);
    s.radius = 2.0f; s.z_min = s.z_max = 0.5f; s.kind = PT_QUADRIC_DISK; s.inner_radius = 0.25f;
    t.spheres.push_back(s);
    t.objects = {PtObject{6, 2}, PtObject{8, 1}};
    t.instances.resize(2);
    t.instances[0].object = 0; translation(t.instances[0].instance_to_world, 0, 8, 0); translation(t.instances[0].world_to_instance, 0, -8, 0);
    t.instances[1].object = 1; std::memcpy(t.instances[1].instance_to_world, kIdentity, 64); std::memcpy(t.instances[1].world_to_instance, kIdentity, 64);
    t.top_refs = {0, 1, 2, 3, 4, 5, PT_TOP_INSTANCE | 0u, PT_TOP_INSTANCE | 1u};
    t.textures = {texture_node(PT_TEX_CONSTANT), texture_node(PT_TEX_IMAGEMAP), texture_node(PT_TEX_SCALE, 0, 1), texture_node(PT_TEX_CONSTANT), texture_node(PT_TEX_MIX, 2, 3, 0)};
    PtImage im; std::memset(&im, 0, sizeof im); im.width = im.height = 2; im.n_levels = 2; im.channels = 3;
    t.images.push_back(im); t.texels.assign(2 * 2 * 3 + 3, 0.5f);
    t.tables.resize(1); t.tables[0].n_rho = 2; t.tables[0].n_radius = 2;
    PtMedium m; std::memset(&m, 0, sizeof m);
    for (int k = 0; k < 3; ++k) { m.sigma_a[k] = 0.25f; m.sigma_s[k] = 0.75f; }
    m.type = PT_MEDIUM_HOMOGENEOUS; std::memcpy(m.world_to_medium, kIdentity, 64); t.media.push_back(m);
    m.type = PT_MEDIUM_GRID; m.nx = m.ny = m.nz = 2; m.sigma_a[0] = 0.5f; m.sigma_a[1] = m.sigma_a[2] = 0.5f; t.media.push_back(m);
    t.density = {0.0f, 0.5f, 2.5f, 1.0f, 0.0f, 0.125f, 0.75f, 2.0f};
    t.med_in.assign(t.prim_shape.size(), PT_NONE); t.med_out.assign(t.prim_shape.size(), PT_NONE); t.med_in[4] = 1; t.med_out[5] = 0;
    t.env_w = 2; t.env_h = 1; t.env_texels = {1, 1, 1, 2, 2, 2}; t.env_importance = {1, 3, 0.5f, 0.5f, 0, 0, 0, 0};
    PtLight L; std::memset(&L, 0, sizeof L);
    L.type = PT_LIGHT_INFINITE; std::memcpy(L.light_to_world, kIdentity, 64); std::memcpy(L.world_to_light, kIdentity, 64); t.lights.push_back(L);
    L.type = PT_LIGHT_DIFFUSE_AREA; L.prim = 1; L.L[0] = L.L[1] = L.L[2] = 1.0f; t.lights.push_back(L); t.prim_light[1] = 1;
    return t;
}

static PtStatus build(const PtSceneDesc &d, ScenePlan &plan, std::string &msg, uint32_t pad = 0) {
    PtStatus st = plan_validate(d, msg);
    if (st) return st;
    PlanOptions opt; opt.pool_pad_records = pad;
    return plan_build(d, opt, sah_builder, plan, msg);
}

// ---- refusals: one defect each in a copy of the valid scene; the expected status and text are the parent driver's (scene_create.hip before the plan unit)
struct Refusal { const char *text; PtStatus status; std::function<void(Toy &)> before; std::function<void(PtSceneDesc &)> after; bool adopt; };
static const char *kLimits[] = {   // refusals no toy scene reaches: 2^28 records / 2^31 packets (one text), the 64 GB pool, "not nested" beyond 2^25 records
    "scene exceeds 2^28 four-wide BVH records / 2^31 packets",
    "scene exceeds 64 GB of traversal records + packets",
    "adopted BVH whose child boxes do not nest inside their parents' (needs the two-wide walk) in a scene beyond 2^25 records / packets (has the four-wide walk only)"};
static const char *kNotRefusals[] = {   // the other string literals of the plan unit: its warnings
    "warning: the adopted BVH's child boxes do not nest inside their parents'; this scene is walked two-wide, box by box (slower than the four-wide production walk)",
    "GridDensityMedium requires spectrally uniform attenuation coefficient (medium ", ": using channel 0, as grid.rs:46-52 does)"};

static std::vector<Refusal> refusals() {
    const PtStatus A = PT_ERR_INVALID_ARG, U = PT_ERR_UNSUPPORTED;
    auto disney = [](Toy &t) -> PtMaterial & { t.materials[2] = plain_material(PT_MAT_DISNEY); return t.materials[2]; };
    std::vector<Refusal> r = {
        {"scene has no primitives", A, nullptr, [](PtSceneDesc &d) { d.n_prims = 0; }},
        {"triangle arrays missing", A, nullptr, [](PtSceneDesc &d) { d.P = nullptr; }},
        {"sphere array missing", A, nullptr, [](PtSceneDesc &d) { d.spheres = nullptr; }},
        {"instances given without top_refs", A, nullptr, [](PtSceneDesc &d) { d.top_refs = nullptr; }},
        // new with the plan unit: a count whose array is NULL used to be dereferenced
        {"materials array missing", A, nullptr, [](PtSceneDesc &d) { d.materials = nullptr; }},
        {"lights array missing", A, nullptr, [](PtSceneDesc &d) { d.lights = nullptr; }},
        {"textures array missing", A, nullptr, [](PtSceneDesc &d) { d.textures = nullptr; }},
        {"images array missing", A, nullptr, [](PtSceneDesc &d) { d.images = nullptr; }},
        {"objects array missing", A, nullptr, [](PtSceneDesc &d) { d.objects = nullptr; }},
        {"instances array missing", A, nullptr, [](PtSceneDesc &d) { d.instances = nullptr; }},
        {"bssrdf_tables array missing", A, nullptr, [](PtSceneDesc &d) { d.bssrdf_tables = nullptr; }},
        {"env_texels without env_importance", A, nullptr, [](PtSceneDesc &d) { d.env_importance = nullptr; }},
        {"env_texels with a zero env_width or env_height", A, nullptr, [](PtSceneDesc &d) { d.env_height = 0; }},
        // the parent's
        {"vertex index out of range", A, [](Toy &t) { t.indices[5] = 1000; }},
        {"primitive shape reference out of range", A, [](Toy &t) { t.prim_shape[4] = PT_SHAPE_REF(PT_SHAPE_SPHERE, 2); }},
        {"material index out of range", A, [](Toy &t) { t.prim_material[2] = 3; }},
        {"light index out of range", A, [](Toy &t) { t.prim_light[2] = 2; }},
        {"subsurface material without a BSSRDF table", A, [](Toy &t) { t.materials[1].bssrdf_table = 1; }},
        {"incomplete BSSRDF table", A, [](Toy &t) { t.tables[0].n_rho = 1; }},
        {"texture type not implemented", U, [](Toy &t) { t.textures[3].type = PT_TEX_DOTS + 1; }},
        {"texture child index out of range", A, [](Toy &t) { t.textures[3].child[2] = 5; }},
        {"image texture without an image", A, [](Toy &t) { t.textures[1].image = 1; }},
        {"PtImage must be a power-of-two MIPMap pyramid with 1 or 3 channels", A, [](Toy &t) { t.images[0].width = 3; }},
        {"ImageWrap::Clamp is not implemented", U, [](Toy &t) { t.textures[1].wrap = PT_WRAP_BLACK + 1; }},
        {"EWA image texture without ewa_weight_lut", A, [](Toy &t) { t.textures[1].trilinear = 0; }},
        {"texture node needs two children", A, [](Toy &t) { t.textures[2].child[1] = -1; }},
        {"mix texture needs three children", A, [](Toy &t) { t.textures[4].child[2] = -1; }},
        {"alpha-mask texture index out of range", A, [](Toy &t) { t.tri_alpha[3] = 5; }},
        {"unknown material type", A, [](Toy &t) { t.materials[2].type = PT_MAT_DISNEY + 1; }},
        {"disney material with more than 5 BxDFs", U, [=](Toy &t) { PtMaterial &m = disney(t); m.disney_thin = 1; m.disney[PT_DS_CLEARCOAT] = 1; m.disney[PT_DS_SPECTRANS] = 0.5f; m.disney[PT_DS_SHEEN] = 1; }},
        {"disney: a textured color together with scatterdistance", U, [=](Toy &t) { PtMaterial &m = disney(t); m.disney_scatter[0] = m.disney_scatter[1] = m.disney_scatter[2] = 1; m.tex[PT_MP_KD] = 0; }},
        {"disney: scatterdistance must be positive in every channel", A, [=](Toy &t) { PtMaterial &m = disney(t); m.disney_scatter[0] = m.disney_scatter[2] = 1; }},
        {"mix material index out of range", A, [](Toy &t) { t.materials[2].type = PT_MAT_MIX; t.materials[2].mix[0] = 3; }},
        {"mix of mix / subsurface materials", U, [](Toy &t) { t.materials[2].type = PT_MAT_MIX; t.materials[2].mix[0] = 1; }},
        {"mix material with more than 5 BxDFs", U, [](Toy &t) { t.materials.push_back(plain_material(PT_MAT_UBER)); t.materials[2].type = PT_MAT_MIX; t.materials[2].mix[0] = t.materials[2].mix[1] = 3; }},
        {"material references a texture but the scene has none", A, [](Toy &t) { t.textures.clear(); t.tri_alpha.clear(); }},
        {"material texture index out of range", A, [](Toy &t) { t.materials[2].tex[PT_MP_KS] = 5; }},
        {"area light primitive out of range", A, [](Toy &t) { t.lights[1].prim = 9; }},
        {"infinite light without env_texels", A, nullptr, [](PtSceneDesc &d) { d.env_texels = nullptr; }},
        {"unknown split_method", A, [](Toy &t) { t.split_method = PT_SPLIT_HLBVH + 1; }},
        {"object primitive range out of bounds", A, [](Toy &t) { t.objects[1].n_prims = 2; }},
        {"instance object index out of range", A, [](Toy &t) { t.instances[1].object = 2; }},
        {"top_refs entry out of range", A, [](Toy &t) { t.top_refs[6] = PT_TOP_INSTANCE | 2u; }},
        {"ordered_prims entry out of range", A, [](Toy &t) { t.ordered[0] = 8; }, nullptr, true},
        {"malformed BVH node", A, [](Toy &t) { for (auto &n : t.nodes) if (!n.n_prims) { n.offset = 0; break; } }, nullptr, true},
        {"unknown medium type", A, [](Toy &t) { t.media[0].type = PT_MEDIUM_GRID + 1; }},
        {"grid medium without a density grid", A, [](Toy &t) { t.media[1].nz = 0; }},
        {"grid medium with no positive density", A, [](Toy &t) { t.density.assign(8, 0.0f); }},
        {"primitive medium index out of range", A, [](Toy &t) { t.med_out[0] = 2; }},
        // a three-node cycle 5 -> 6 -> 7 -> 5, and a chain scale(c, scale(c, ...)) seven deep: its value stack holds eight entries
        {"texture graph too deep or cyclic", A, [](Toy &t) { t.textures.push_back(texture_node(PT_TEX_SCALE, 6, 0)); t.textures.push_back(texture_node(PT_TEX_SCALE, 7, 0)); t.textures.push_back(texture_node(PT_TEX_SCALE, 5, 0)); }},
        {"texture expression needs a deeper value stack than kTexStack", U, [](Toy &t) { for (int k = 0; k < 7; ++k) t.textures.push_back(texture_node(PT_TEX_SCALE, 0, k ? 4 + k : 0)); }},
    };
    return r;
}

static Toy adopted_scene(uint32_t maxp = 4) {   // the valid scene with its own top-level tree handed back in
    Toy t = valid_scene(maxp); ScenePlan p; std::string msg;
    CHECK(build(t.desc(), p, msg) == PT_OK, "%s", msg.c_str());
    t.nodes = p.nodes; t.ordered = p.ordered;
    return t;
}

// every string literal of a source file outside its comments and #include lines
static std::vector<std::string> string_literals(const char *path) {
    std::vector<std::string> out;
    std::ifstream in(path); std::string line;
    while (std::getline(in, line)) {
        if (line.find("#include") != std::string::npos) continue;
        bool in_str = false; std::string cur;
        for (size_t i = 0; i < line.size(); ++i) {
            if (!in_str && line[i] == '/' && i + 1 < line.size() && line[i + 1] == '/') break;
            if (line[i] == '"') { if (in_str) out.push_back(cur); cur.clear(); in_str = !in_str; continue; }
            if (in_str) cur += line[i];
        }
    }
    return out;
}

static void check_refusals(const char *plan_source) {
    const std::vector<Refusal> table = refusals();
    for (const Refusal &r : table) {
        Toy t = r.adopt ? adopted_scene() : valid_scene();
        if (r.before) r.before(t);
        PtSceneDesc d = t.desc();
        if (r.after) r.after(d);
        ScenePlan plan; std::string msg;
        const PtStatus st = build(d, plan, msg);
        CHECK(st == r.status && msg == r.text, "expected %d \"%s\", got %d \"%s\"", (int)r.status, r.text, (int)st, msg.c_str());
    }
    // the table lists every refusal text of the plan unit, or the text is one of the limits no toy scene reaches
    std::set<std::string> listed, limits(std::begin(kLimits), std::end(kLimits)), other(std::begin(kNotRefusals), std::end(kNotRefusals)), in_source;
    for (const Refusal &r : table) listed.insert(r.text);
    CHECK(listed.size() == table.size(), "a refusal is listed twice");
    const std::vector<std::string> lits = string_literals(plan_source);
    CHECK(!lits.empty(), "no string literal read from %s", plan_source);
    for (const std::string &s : lits) {
        if (other.count(s)) continue;
        in_source.insert(s);
        CHECK(listed.count(s) || limits.count(s), "refusal \"%s\" of %s is neither provoked here nor named as a limit", s.c_str(), plan_source);
    }
    for (const std::string &s : listed) CHECK(in_source.count(s), "listed refusal \"%s\" is not in %s", s.c_str(), plan_source);
    for (const std::string &s : limits) CHECK(in_source.count(s), "limit \"%s\" is not in %s", s.c_str(), plan_source);
    CHECK(in_source.size() == listed.size() + limits.size(), "%zu refusal texts in the source, %zu provoked + %zu limits", in_source.size(), listed.size(), limits.size());
    std::printf("refusals: %zu provoked, %zu limits named, %zu texts in %s\n", listed.size(), limits.size(), in_source.size(), plan_source);
}

// ---- records
using Leaves = std::vector<uint32_t>;   // leaf references (kLeafBit | first packet) in the order a walk meets them
static bool neg(uint32_t octant, uint32_t axis) { return (octant >> axis) & 1u; }

// the reference's walk (bvh.rs:705-814) without a ray: the near child first, near = the second child when the ray is negative along the split axis
static void binary_walk(const std::vector<PtBVHNode> &nn, uint32_t i, uint32_t octant, uint32_t pbase, Leaves &out) {
    if (nn[i].n_prims) { out.push_back(kLeafBit | (pbase + nn[i].offset)); return; }
    const uint32_t first = neg(octant, nn[i].axis) ? nn[i].offset : i + 1, second = neg(octant, nn[i].axis) ? i + 1 : nn[i].offset;
    binary_walk(nn, first, octant, pbase, out); binary_walk(nn, second, octant, pbase, out);
}
static void wide_walk(const ScenePlan &p, uint32_t ref, uint32_t octant, Leaves &out) {
    if (ref & kLeafBit) { out.push_back(ref); return; }
    const WideNode &w = p.wide[ref];
    const bool n = neg(octant, w.meta & 0xffu);
    wide_walk(p, n ? w.right_ref : w.left_ref, octant, out); wide_walk(p, n ? w.left_ref : w.right_ref, octant, out);
}
// the four slots in the order the order word gives for the octant (kern_trace.h: bit 0 = the right pair first, bit 1 = slot 1 before slot 0, bit 2 = slot 3 before slot 2)
static void quad_walk(const ScenePlan &p, uint32_t pad, uint32_t ref, uint32_t octant, Leaves &out) {
    if (ref & kLeafBit) { out.push_back(ref); return; }
    const QuadNode &q = p.quad[ref - pad];
    const uint32_t o3 = (q.meta >> (3u * octant)) & 7u;
    const int l0 = (o3 & 2u) ? 1 : 0, r0 = (o3 & 4u) ? 3 : 2;
    const int left[2] = {l0, l0 ^ 1}, right[2] = {r0, r0 == 3 ? 2 : 3};
    int order[4];
    for (int k = 0; k < 2; ++k) { order[k] = (o3 & 1u) ? right[k] : left[k]; order[2 + k] = (o3 & 1u) ? left[k] : right[k]; }
    for (int k = 0; k < 4; ++k) if (q.ref[order[k]] != PT_NONE) quad_walk(p, pad, q.ref[order[k]], octant, out);
}
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// The four-wide records of one tree against its binary nodes: slots 0, 1 = the children of the left child (or the left child itself, a leaf, in slot 0), slots 2, 3 the
// same of the right child; every filled slot's box is its node's, bit for bit; every other slot is +inf / -inf with PT_NONE; records are numbered in pre-order.
static void check_quad_records(const ScenePlan &p, const std::vector<PtBVHNode> &nn, uint32_t i, uint32_t ref, uint32_t pad, uint32_t pbase, uint32_t &next_record, const char *what) {
    CHECK(ref == next_record, "%s: record of node %u is %u, pre-order says %u", what, i, ref, next_record);
    ++next_record;
    const QuadNode &q = p.quad[ref - pad];
    const float inf = std::numeric_limits<float>::infinity();
    uint32_t node_of[4] = {PT_NONE, PT_NONE, PT_NONE, PT_NONE};
    const uint32_t side[2] = {i + 1, nn[i].offset};
    for (int s = 0; s < 2; ++s) {
        if (nn[side[s]].n_prims) node_of[2 * s] = side[s];
        else { node_of[2 * s] = side[s] + 1; node_of[2 * s + 1] = nn[side[s]].offset; }
    }
    for (int k = 0; k < 4; ++k) {
        if (node_of[k] == PT_NONE) {
            CHECK(q.ref[k] == PT_NONE, "%s: node %u slot %d should be empty", what, i, k);
            for (int a = 0; a < 3; ++a) CHECK(q.lo[a][k] == inf && q.hi[a][k] == -inf, "%s: node %u empty slot %d has a box", what, i, k);
            continue;
        }
        const PtBVHNode &c = nn[node_of[k]];
        for (int a = 0; a < 3; ++a) CHECK(same_bits(q.lo[a][k], c.bmin[a]) && same_bits(q.hi[a][k], c.bmax[a]), "%s: node %u slot %d: box differs from node %u's", what, i, k, node_of[k]);
        if (c.n_prims) CHECK(q.ref[k] == (kLeafBit | (pbase + c.offset)), "%s: node %u slot %d: leaf reference %08x", what, i, k, q.ref[k]);
        else { CHECK(!(q.ref[k] & kLeafBit), "%s: node %u slot %d: an interior node with a leaf reference", what, i, k); check_quad_records(p, nn, node_of[k], q.ref[k], pad, pbase, next_record, what); }
    }
    CHECK(q.pad[0] == 0 && q.pad[1] == 0 && q.pad[2] == 0, "%s: pad words", what);
}

// one tree of the plan: both record sets walk its leaves in the binary walk's order for every sign octant; the records mirror the nodes
static void check_tree(const ScenePlan &p, const std::vector<PtBVHNode> &nn, uint32_t root_ref, uint32_t root_ref4, uint32_t pad, uint32_t pbase, uint32_t &next_record, const char *what) {
    for (uint32_t o = 0; o < 8; ++o) {
        Leaves b, w, q;
        binary_walk(nn, 0, o, pbase, b); wide_walk(p, root_ref, o, w); quad_walk(p, pad, root_ref4, o, q);
        CHECK(b == w, "%s octant %u: the two-wide walk meets %zu leaves in another order than the binary walk's %zu", what, o, w.size(), b.size());
        CHECK(b == q, "%s octant %u: the four-wide walk meets %zu leaves in another order than the binary walk's %zu", what, o, q.size(), b.size());
    }
    if (nn[0].n_prims) CHECK(root_ref4 == (kLeafBit | (pbase + nn[0].offset)) && root_ref == root_ref4, "%s: a root leaf's references", what);
    else check_quad_records(p, nn, 0, root_ref4, pad, pbase, next_record, what);
}
static void expect_leaf_last(const std::vector<PtBVHNode> &nn, uint32_t pbase, Leaves &out) {
    for (const PtBVHNode &n : nn) if (n.n_prims) out.push_back(pbase + n.offset + n.n_prims - 1);
}
static PrimBound triangle_bound(const Toy &t, uint32_t tri) {
    PrimBound b;
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = std::numeric_limits<float>::infinity(); b.hi[k] = -b.lo[k];
        for (int v = 0; v < 3; ++v) { const float x = t.P[3 * t.indices[3 * tri + v] + k]; b.lo[k] = std::fmin(b.lo[k], x); b.hi[k] = std::fmax(b.hi[k], x); }
    }
    return b;
}

static void check_records() {
    bool saw_root_leaf = false, saw_two_leaves = false, saw_collapsed = false, saw_full = false;
    for (uint32_t maxp : {1u, 4u}) for (uint32_t n : {1u, 2u, 3u, 4u, 5u, 300u}) {
        Toy t = random_triangles(n, 1000 + n, maxp);
        char what[64]; std::snprintf(what, sizeof what, "%u triangles, maxnodeprims %u", n, maxp);
        for (uint32_t pad : {0u, 5u}) {
            ScenePlan p; std::string msg;
            CHECK(build(t.desc(), p, msg, pad) == PT_OK, "%s: %s", what, msg.c_str());
            uint32_t next = pad;
            check_tree(p, p.nodes, p.root_ref, p.root_ref4, pad, 0, next, what);
            const size_t interior = (size_t)std::count_if(p.nodes.begin(), p.nodes.end(), [](const PtBVHNode &x) { return x.n_prims == 0; });
            CHECK(p.quad.size() == std::max<size_t>(1, next - pad) && p.wide.size() == std::max<size_t>(1, interior), "%s: %zu four-wide, %zu two-wide records", what, p.quad.size(), p.wide.size());
            Leaves last; expect_leaf_last(p.nodes, 0, last);
            CHECK(p.leaf_last == last, "%s: leaf_last", what);
            CHECK(p.packet_refs == p.ordered && p.packet_refs.size() == n, "%s: the packet order is the tree's primitive order", what);
            CHECK(p.pad_bytes == pad * sizeof(QuadNode) && p.quad_bytes == p.pad_bytes + p.quad.size() * sizeof(QuadNode) && p.pool_bytes == p.quad_bytes + (n + 2) * sizeof(TriPacket) && !p.pool_big, "%s: pool sizes", what);
            saw_root_leaf |= p.nodes[0].n_prims != 0;
            if (!p.nodes[0].n_prims) for (const QuadNode &q : p.quad) {
                const int filled = (q.ref[0] != PT_NONE) + (q.ref[1] != PT_NONE) + (q.ref[2] != PT_NONE) + (q.ref[3] != PT_NONE);
                saw_two_leaves |= filled == 2 && q.ref[1] == PT_NONE && q.ref[3] == PT_NONE; saw_collapsed |= filled == 3; saw_full |= filled == 4;
            }
        }
        // with pad records in front of the pool every record reference moves by the pad and no packet reference moves
        ScenePlan a, b; std::string msg;
        build(t.desc(), a, msg, 0); build(t.desc(), b, msg, 5);
        CHECK(a.quad.size() == b.quad.size() && a.packet_refs == b.packet_refs && a.leaf_last == b.leaf_last, "%s: pad changes sizes", what);
        CHECK(a.wide.size() == b.wide.size() && std::memcmp(a.wide.data(), b.wide.data(), a.wide.size() * sizeof(WideNode)) == 0 && a.root_ref == b.root_ref, "%s: pad moves the two-wide records", what);
        auto moved = [](uint32_t r0, uint32_t r5) { return (r0 == PT_NONE || (r0 & kLeafBit)) ? r5 == r0 : r5 == r0 + 5; };
        CHECK(moved(a.root_ref4, b.root_ref4), "%s: root_ref4 with pad", what);
        if (!a.nodes[0].n_prims)   // (a root leaf has no record: the pool then starts with one unused, zeroed record)
            for (size_t i = 0; i < a.quad.size() && i < b.quad.size(); ++i) for (int k = 0; k < 4; ++k) CHECK(moved(a.quad[i].ref[k], b.quad[i].ref[k]), "%s: record %zu slot %d with pad", what, i, k);
    }
    CHECK(saw_root_leaf && saw_two_leaves && saw_collapsed && saw_full, "shapes reached: root leaf %d, two leaf slots %d, one collapsed side %d, full record %d", saw_root_leaf, saw_two_leaves, saw_collapsed, saw_full);

    // the instanced scene: [top level][object 0: a tree over two triangles][object 1: one packet without a tree]
    for (uint32_t maxp : {1u, 4u}) for (uint32_t pad : {0u, 5u}) {
        Toy t = valid_scene(maxp); ScenePlan p; std::string msg;
        char what[64]; std::snprintf(what, sizeof what, "instanced scene, maxnodeprims %u, pad %u", maxp, pad);
        CHECK(build(t.desc(), p, msg, pad) == PT_OK, "%s: %s", what, msg.c_str());
        uint32_t next = pad;
        check_tree(p, p.nodes, p.root_ref, p.root_ref4, pad, 0, next, what);
        const uint32_t n_top = (uint32_t)t.top_refs.size();
        Leaves last; expect_leaf_last(p.nodes, 0, last);
        for (uint32_t i = 0; i < n_top; ++i) CHECK(p.packet_refs[i] == t.top_refs[p.ordered[i]], "%s: top-level packet %u", what, i);
        // object 0: its own SAH tree over its two triangles' bounds, appended behind the top level
        std::vector<PrimBound> pb = {triangle_bound(t, 4), triangle_bound(t, 5)};
        std::vector<PtBVHNode> on; std::vector<uint32_t> oo;
        build_sah_bvh(pb, maxp, on, oo);
        const DevInstance &I0 = p.instances[0], &I1 = p.instances[1];
        const size_t top_interior = (size_t)std::count_if(p.nodes.begin(), p.nodes.end(), [](const PtBVHNode &x) { return x.n_prims == 0; });
        if (!on[0].n_prims) CHECK(I0.root_ref == top_interior && I0.root_ref4 == next, "%s: object 0's roots %u %u are not behind the top level's records (%zu, %u)", what, I0.root_ref, I0.root_ref4, top_interior, next);
        check_tree(p, on, I0.root_ref, I0.root_ref4, pad, n_top, next, what);
        expect_leaf_last(on, n_top, last);
        for (uint32_t k = 0; k < 2; ++k) CHECK(p.packet_refs[n_top + k] == 6 + oo[k], "%s: object 0's packet %u", what, k);
        for (int k = 0; k < 3; ++k) CHECK(same_bits(I0.root_min[k], on[0].bmin[k]) && same_bits(I0.root_max[k], on[0].bmax[k]), "%s: object 0's root box", what);
        CHECK(!I0.single && !I0.identity, "%s: instance 0 is a translated two-primitive object", what);
        // object 1: a single primitive
        CHECK(I1.single && I1.identity && I1.root_ref == (kLeafBit | (n_top + 2)) && I1.root_ref4 == I1.root_ref, "%s: instance 1: single %u identity %u root %08x", what, I1.single, I1.identity, I1.root_ref);
        CHECK(p.packet_refs.size() == n_top + 3 && p.packet_refs[n_top + 2] == 8, "%s: object 1's packet", what);
        last.push_back(n_top + 2);
        CHECK(p.leaf_last == last, "%s: leaf_last", what);
        CHECK(std::memcmp(I0.instance_to_world, t.instances[0].instance_to_world, 64) == 0 && std::memcmp(I0.world_to_instance, t.instances[0].world_to_instance, 64) == 0, "%s: instance matrices", what);
        // the instance's box in the top-level tree: object 0's root box moved by the translation (0, 8, 0)
        for (const PtBVHNode &n : p.nodes) if (n.n_prims) for (uint32_t k = 0; k < n.n_prims; ++k) if (p.packet_refs[n.offset + k] == (PT_TOP_INSTANCE | 0u) && n.n_prims == 1)
            for (int a = 0; a < 3; ++a) CHECK(n.bmin[a] == on[0].bmin[a] + (a == 1 ? 8.0f : 0.0f) && n.bmax[a] == on[0].bmax[a] + (a == 1 ? 8.0f : 0.0f), "%s: the instance's world bound, axis %d", what, a);
    }
}

// ---- tables
static void post_order(const std::vector<PtTexture> &tx, int node, std::vector<uint32_t> &out) {
    const int n = tx[node].type == PT_TEX_MIX ? 3 : tx[node].type == PT_TEX_SCALE ? 2 : 0;
    for (int k = 0; k < n; ++k) post_order(tx, tx[node].child[k], out);
    out.push_back((uint32_t)node);
}

static void check_tables() {
    Toy t = valid_scene(); ScenePlan p; std::string msg;
    CHECK(build(t.desc(), p, msg) == PT_OK, "the valid scene: %s", msg.c_str());
    // texture programs: children before their parent, on a value stack of at most kTexStack entries
    CHECK(p.tex_prog_offset.size() == t.textures.size() + 1 && p.tex_prog_offset.back() == p.tex_prog.size(), "texture program offsets");
    for (size_t r = 0; r + 1 < p.tex_prog_offset.size(); ++r) {
        std::vector<uint32_t> want; post_order(t.textures, (int)r, want);
        const std::vector<uint32_t> got(p.tex_prog.begin() + p.tex_prog_offset[r], p.tex_prog.begin() + p.tex_prog_offset[r + 1]);
        CHECK(got == want, "texture %zu: its program is not the post-order of its tree", r);
        int depth = 0, deepest = 0;
        for (uint32_t node : got) { const int n = t.textures[node].type == PT_TEX_MIX ? 3 : t.textures[node].type == PT_TEX_SCALE ? 2 : 0; CHECK(depth >= n, "texture %zu: stack underflow", r); depth += 1 - n; deepest = std::max(deepest, depth); }
        CHECK(depth == 1 && deepest <= kTexStack, "texture %zu: final depth %d, deepest %d", r, depth, deepest);
    }
    const std::vector<uint32_t> mix_prog(p.tex_prog.begin() + p.tex_prog_offset[4], p.tex_prog.end());
    CHECK((mix_prog == std::vector<uint32_t>{0, 1, 2, 3, 0, 4}), "the mix texture's program");
    CHECK(p.images.size() == 1 && p.images[0].level_offset[0] == 0 && p.images[0].level_offset[1] == 12 && p.images[0].texels == nullptr && p.images[0].n_levels == 2, "image level offsets");
    // shade classes, flags, light list
    CHECK(p.mat_class.size() == 3 && p.mat_class[0] == 0 && p.mat_class[1] == 3 && p.mat_class[2] == 0, "shade classes %d %d %d", p.mat_class[0], p.mat_class[1], p.mat_class[2]);
    for (int c = 0; c < kNumClasses; ++c) CHECK(p.class_used[c] == (c == 0 || c == 3 || c == kMissClass || c == kMediumClass), "class_used[%d]", c);
    CHECK(p.has_bssrdf && !p.has_null_material && p.infinite_lights == std::vector<uint32_t>{0}, "has_bssrdf / has_null_material / infinite lights");
    CHECK(material_class(plain_material(PT_MAT_SUBSURFACE), true, true) == kSssClass && material_class(plain_material(PT_MAT_METAL), false, true) == 1 && material_class(plain_material(PT_MAT_METAL), true, false) == kMetalClass, "material_class");
    { Toy s = valid_scene(); s.prim_material[3] = PT_NONE; ScenePlan q; CHECK(build(s.desc(), q, msg) == PT_OK && q.has_null_material, "a primitive without a material"); }
    // environment map: the rows' and the marginal's Distribution1D
    {
        std::vector<float> cdf; float fint;
        dist1d({1.0f, 3.0f}, cdf, fint);
        CHECK(fint == 2.0f && cdf == (std::vector<float>{0.0f, 0.25f, 1.0f}), "dist1d of {1, 3}");
        dist1d({0.0f, 0.0f}, cdf, fint);
        CHECK(fint == 0.0f && cdf == (std::vector<float>{0.0f, 0.5f, 1.0f}), "dist1d of a zero function");
        const size_t nu = 4, nv = 2;
        std::vector<float> ints(nv);
        for (size_t v = 0; v < nv; ++v) {
            dist1d(std::vector<float>(t.env_importance.begin() + v * nu, t.env_importance.begin() + (v + 1) * nu), cdf, ints[v]);
            CHECK(std::equal(cdf.begin(), cdf.end(), p.env_cdf.begin() + v * (nu + 1)), "environment row %zu", v);
        }
        CHECK(p.env_cdf.size() == nv * (nu + 1) && p.env_func_int == ints, "environment row integrals");
        dist1d(ints, cdf, fint);
        CHECK(p.env_marg_cdf == cdf && p.env_marg_int == fint && fint == (1.25f + 0.0f) / 2.0f, "environment marginal");
    }
    // grid medium (grid.rs:40-72): sigma_t = (sigma_a + sigma_s)[0], 1 / the largest density; nothing for the homogeneous one
    CHECK(p.grid_aux.size() == 2 && p.has_grid && p.grid_aux[0].sigma_t == 0.0f && p.grid_aux[0].inv_max_density == 0.0f, "the homogeneous medium's grid constants");
    CHECK(p.grid_aux[1].sigma_t == 0.5f + 0.75f && p.grid_aux[1].inv_max_density == 1.0f / 2.5f && p.grid_aux[1].density == nullptr, "the grid medium's constants %g %g", p.grid_aux[1].sigma_t, p.grid_aux[1].inv_max_density);
    CHECK(p.warnings.empty(), "%zu warnings for the valid scene", p.warnings.size());
    { Toy s = valid_scene(); s.media[1].sigma_s[2] = 1.0f; ScenePlan q; CHECK(build(s.desc(), q, msg) == PT_OK && q.warnings.size() == 1 && q.warnings[0].find("medium 1") != std::string::npos, "the spectrally varying grid medium's warning"); }
    // world bound = the root's box; bounding sphere (bounds.rs:516-524): centre (min + max) / 2, radius |max - centre| when the centre lies inside
    float c[3], r2 = 0.0f;
    for (int k = 0; k < 3; ++k) {
        CHECK(same_bits(p.wb_min[k], p.nodes[0].bmin[k]) && same_bits(p.wb_max[k], p.nodes[0].bmax[k]), "world bound axis %d", k);
        c[k] = (p.nodes[0].bmin[k] + p.nodes[0].bmax[k]) / 2.0f;
        CHECK(p.world_center[k] == c[k], "world centre axis %d", k);
    }
    { const float dx = p.nodes[0].bmax[0] - c[0], dy = p.nodes[0].bmax[1] - c[1], dz = p.nodes[0].bmax[2] - c[2]; r2 = dx * dx + dy * dy + dz * dz; }
    CHECK(p.world_radius == std::sqrt(r2) && p.world_radius > 0.0f, "world radius %g", p.world_radius);
    // the root's box holds the sphere's and the disk's transformed object bounds
    CHECK(p.nodes[0].bmax[0] >= 7.5f && p.nodes[0].bmin[0] <= -5.0f && p.nodes[0].bmax[1] >= 8.0f, "the root box misses a quadric or the instance");
    // the adopted tree: the same plan as the built one; a tree whose boxes do not nest is walked two-wide and says so
    Toy a = adopted_scene(); ScenePlan pa;
    CHECK(build(a.desc(), pa, msg) == PT_OK && !pa.exact_walk_only && pa.warnings.empty(), "the adopted tree: %s", msg.c_str());
    CHECK(pa.nodes.size() == p.nodes.size() && std::memcmp(pa.nodes.data(), p.nodes.data(), p.nodes.size() * sizeof(PtBVHNode)) == 0 && pa.ordered == p.ordered, "the adopted tree is kept as given");
    CHECK(pa.quad.size() == p.quad.size() && std::memcmp(pa.quad.data(), p.quad.data(), p.quad.size() * sizeof(QuadNode)) == 0 && pa.packet_refs == p.packet_refs && pa.leaf_last == p.leaf_last, "the adopted tree's records");
    a.nodes[1].bmax[0] = a.nodes[0].bmax[0] + 1.0f;
    ScenePlan pn;
    CHECK(build(a.desc(), pn, msg) == PT_OK && pn.exact_walk_only && !pn.quad_walk_only && pn.warnings.size() == 1, "the adopted tree that does not nest");
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: check_plan <path of scene_plan.hip>\n"); return 2; }
    { Toy t = valid_scene(); ScenePlan p; std::string msg; CHECK(build(t.desc(), p, msg) == PT_OK, "the valid scene is refused: %s", msg.c_str()); }
    check_refusals(argv[1]);
    check_records();
    check_tables();
    std::printf("scene plan: %d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
