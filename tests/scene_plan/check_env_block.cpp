// check_env_block.cpp -- a stand-alone check, on the CPU, of what the scene plan (csrc/scene_plan.h) prepares for the shade kernels' light sampling: the environment
// light's uniform block (dev_scene.h: EnvUniform) and every light's record header (light_rec_head). Built from scene_plan.hip + host_bvh.cpp, host code only
// (tests/test_env_light_plan.py). Exit status 0 = every check passed.
#include <cstdio>
#include <cstring>
#include <vector>
#include "scene_plan.h"

using namespace pth;

static int g_failed = 0, g_checked = 0;
#define CHECK(cond, ...) do { ++g_checked; if (!(cond)) { ++g_failed; std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
// two different non-identity matrices (a rotation with a translation, and roughly its inverse: the plan copies the light's matrices, it does not invert them)
static const float kRot[16] = {0.8f, -0.6f, 0.0f, 0.25f, 0.168f, 0.224f, -0.96f, -1.5f, 0.576f, 0.768f, 0.28f, 3.0f, 0, 0, 0, 1};
static const float kRotInv[16] = {0.8f, 0.168f, 0.576f, -1.676f, -0.6f, 0.224f, 0.768f, -1.818f, 0.0f, -0.96f, 0.28f, -2.28f, 0, 0, 0, 1};

struct Toy {
    std::vector<float> P, env_texels, env_importance;
    std::vector<uint32_t> indices, prim_shape, prim_material, prim_light;
    std::vector<PtSphere> spheres;
    std::vector<PtMaterial> materials;
    std::vector<PtLight> lights;
    uint32_t env_w = 0, env_h = 0;
    Toy() {
        PtMaterial m; std::memset(&m, 0, sizeof m);
        m.type = PT_MAT_MATTE; m.kd[0] = m.kd[1] = m.kd[2] = 0.5f; m.eta = 1.5f;
        for (int k = 0; k < 16; ++k) m.tex[k] = -1;
        materials.push_back(m);
    }
    PtSceneDesc desc() {
        PtSceneDesc d; std::memset(&d, 0, sizeof d);
        d.n_vertices = (uint32_t)P.size() / 3; d.P = P.data();
        d.n_triangles = (uint32_t)indices.size() / 3; d.indices = indices.data();
        d.n_spheres = (uint32_t)spheres.size(); d.spheres = spheres.data();
        d.n_prims = (uint32_t)prim_shape.size(); d.prim_shape = prim_shape.data(); d.prim_material = prim_material.data(); d.prim_light = prim_light.data();
        d.n_materials = (uint32_t)materials.size(); d.materials = materials.data();
        d.n_lights = (uint32_t)lights.size(); d.lights = lights.data();
        if (env_w) { d.env_width = env_w; d.env_height = env_h; d.env_texels = env_texels.data(); d.env_importance = env_importance.data(); d.env_power_lookup[0] = 1.0f; }
        d.max_node_prims = 4; d.split_method = PT_SPLIT_SAH;
        return d;
    }
    uint32_t add_triangle(float x) {
        const uint32_t base = (uint32_t)P.size() / 3, tri = (uint32_t)indices.size() / 3;
        const float v[9] = {x, 0, 0, x + 1, 0, 0.5f, x, 1, 1};
        P.insert(P.end(), v, v + 9);
        for (uint32_t k = 0; k < 3; ++k) indices.push_back(base + k);
        return add_prim(PT_SHAPE_REF(PT_SHAPE_TRIANGLE, tri));
    }
    uint32_t add_prim(uint32_t shape) { prim_shape.push_back(shape); prim_material.push_back(0); prim_light.push_back(PT_NONE); return (uint32_t)prim_shape.size() - 1; }
    void add_light(uint32_t type, uint32_t prim = 0) {
        PtLight L; std::memset(&L, 0, sizeof L);
        L.type = type; L.L[0] = 1.0f; L.L[1] = 2.0f; L.L[2] = 3.0f; L.prim = prim;
        std::memcpy(L.light_to_world, kIdentity, 64); std::memcpy(L.world_to_light, kIdentity, 64);
        if (type == PT_LIGHT_DIFFUSE_AREA) prim_light[prim] = (uint32_t)lights.size();
        lights.push_back(L);
    }
    void set_env(uint32_t w, uint32_t h, float scale) {   // unequal texels and an importance image with unequal entries in every row
        env_w = w; env_h = h;
        env_texels.clear(); env_importance.clear();
        for (uint32_t i = 0; i < 3 * w * h; ++i) env_texels.push_back(scale * (0.25f + 0.125f * (float)i));
        for (uint32_t i = 0; i < 4 * w * h; ++i) env_importance.push_back(scale * (0.5f + 0.375f * (float)((i * 5u) % 7u)));
    }
};

static bool build(Toy &t, ScenePlan &plan) {
    PtSceneDesc d = t.desc(); std::string msg;
    PtStatus st = plan_validate(d, msg);
    if (!st) st = plan_build(d, PlanOptions{}, sah_builder, plan, msg);
    CHECK(st == PT_OK, "the scene is refused: %s", msg.c_str());
    return st == PT_OK;
}
static bool all_zero(const void *p, size_t n) { const unsigned char *b = (const unsigned char *)p; for (size_t i = 0; i < n; ++i) if (b[i]) return false; return true; }

// one light of every kind; the infinite light rotated; a constant environment (1 x 1 map, 2 x 2 importance image)
static Toy every_kind() {
    Toy t;
    t.add_triangle(0.0f);                                   // prim 0: a plain triangle
    const uint32_t tri = t.add_triangle(3.0f);              // prim 1: a triangle light
    PtSphere s; std::memset(&s, 0, sizeof s);
    std::memcpy(s.object_to_world, kIdentity, 64); std::memcpy(s.world_to_object, kIdentity, 64);
    s.radius = 1.5f; s.z_min = -1.5f; s.z_max = 1.5f; s.theta_min = 3.14159265f; s.theta_max = 0.0f; s.phi_max = 6.2831853f; s.kind = PT_QUADRIC_SPHERE;
    t.spheres.push_back(s);
    const uint32_t sph = t.add_prim(PT_SHAPE_REF(PT_SHAPE_SPHERE, 0));   // prim 2: a sphere light
    t.add_light(PT_LIGHT_POINT); t.add_light(PT_LIGHT_DIFFUSE_AREA, tri); t.add_light(PT_LIGHT_SPOT); t.add_light(PT_LIGHT_INFINITE);
    t.add_light(PT_LIGHT_DIFFUSE_AREA, sph); t.add_light(PT_LIGHT_DISTANT);
    std::memcpy(t.lights[3].light_to_world, kRot, 64); std::memcpy(t.lights[3].world_to_light, kRotInv, 64);
    t.set_env(1, 1, 1.0f);
    return t;
}

int main() {
    {   // record headers: bits 12-15 the type, 0x400 for the delta lights (point, spot, distant), nothing else (k_light_area adds a triangle's bits below 0x400)
        Toy t = every_kind(); ScenePlan p;
        if (build(t, p)) {
            const uint32_t want[6] = {0x2400u, 0x0000u, 0x4400u, 0x3000u, 0x0000u, 0x1400u};
            CHECK(p.light_head.size() == 6, "%zu headers for 6 lights", p.light_head.size());
            for (size_t i = 0; i < 6 && i < p.light_head.size(); ++i) CHECK(p.light_head[i] == want[i], "light %zu (type %u): header %#x, expected %#x", i, t.lights[i].type, p.light_head[i], want[i]);
            CHECK(kLrecDelta == 0x400u && kLrecTypeShift == 12 && kLrecValid == 0x100u && kLrecDegenerate == 0x200u, "the header's bit layout");
            // the block: the infinite light's matrices bit for bit, the 1 x 1 map's tables = the plan's own arrays
            const EnvUniform &e = p.env_u;
            CHECK(e.light == 3, "the block names light %u", e.light);
            CHECK(std::memcmp(e.world_to_light, t.lights[3].world_to_light, 64) == 0 && std::memcmp(e.light_to_world, t.lights[3].light_to_world, 64) == 0, "the block's matrices");
            CHECK(std::memcmp(e.world_to_light, e.light_to_world, 64) != 0, "the two matrices of the rotated light are one and the same");
            CHECK(std::memcmp(e.texel0, t.env_texels.data(), 12) == 0, "texel 0");
            CHECK(p.env_marg_cdf.size() == 3 && p.env_cdf.size() == 6 && p.env_func_int.size() == 2, "the plan's tables of a 2 x 2 importance image: %zu %zu %zu", p.env_marg_cdf.size(), p.env_cdf.size(), p.env_func_int.size());
            CHECK(std::memcmp(e.marg_cdf, p.env_marg_cdf.data(), 12) == 0 && std::memcmp(&e.marg_int, &p.env_marg_int, 4) == 0, "the marginal's cdf and integral");
            CHECK(std::memcmp(e.row_int, p.env_func_int.data(), 8) == 0, "the rows' integrals (the marginal's function)");
            CHECK(std::memcmp(e.row_cdf, p.env_cdf.data(), 24) == 0, "the conditional rows' cdfs");
            CHECK(std::memcmp(e.row_func, t.env_importance.data(), 16) == 0, "the conditional rows' functions");
            CHECK(e.marg_int > 0.0f && e.row_cdf[0][1] != e.row_cdf[1][1] && e.marg_cdf[1] != 0.5f, "the toy importance image is uniform: the comparison says little");
        }
    }
    for (int shape = 0; shape < 3; ++shape) {   // 2 x 1, 1 x 2, 2 x 2 maps: beyond the register tables -- matrices as before, tables left zero
        Toy t = every_kind(); ScenePlan p;
        t.set_env(shape == 1 ? 1 : 2, shape == 0 ? 1 : 2, 1.0f);
        if (build(t, p)) {
            const EnvUniform &e = p.env_u;
            CHECK(e.light == 3 && std::memcmp(e.world_to_light, kRotInv, 64) == 0 && std::memcmp(e.light_to_world, kRot, 64) == 0, "a %u x %u map: the block's light and matrices", t.env_w, t.env_h);
            CHECK(all_zero(e.texel0, sizeof e.texel0) && all_zero(e.marg_cdf, sizeof e.marg_cdf) && e.marg_int == 0.0f && all_zero(e.row_int, sizeof e.row_int) && all_zero(e.row_cdf, sizeof e.row_cdf) && all_zero(e.row_func, sizeof e.row_func),
                  "a %u x %u map: tables filled for a map they cannot hold", t.env_w, t.env_h);
        }
    }
    {   // two infinite lights: the block serves the first (the second keeps its PtLight); a black constant environment: integrals 0, the uniform cdf of Distribution1D::new
        Toy t = every_kind(); ScenePlan p;
        t.add_light(PT_LIGHT_INFINITE);
        t.set_env(1, 1, 0.0f);
        if (build(t, p)) {
            CHECK(p.infinite_lights == (std::vector<uint32_t>{3, 6}) && p.env_u.light == 3 && std::memcmp(p.env_u.light_to_world, kRot, 64) == 0, "two infinite lights: the block's light is %u", p.env_u.light);
            CHECK(p.light_head.size() == 7 && p.light_head[6] == 0x3000u, "the second infinite light's header");
            CHECK(p.env_u.marg_int == 0.0f && p.env_u.marg_cdf[1] == 0.5f && p.env_u.marg_cdf[2] == 1.0f && p.env_u.row_cdf[1][1] == 0.5f && p.env_u.row_int[0] == 0.0f, "the black environment's tables");
        }
    }
    {   // no infinite light, no map
        Toy t; ScenePlan p;
        t.add_triangle(0.0f); t.add_light(PT_LIGHT_POINT);
        if (build(t, p)) {
            CHECK(p.env_u.light == PT_NONE, "a scene without an infinite light: the block names light %u", p.env_u.light);
            CHECK(all_zero(p.env_u.world_to_light, sizeof(EnvUniform) - sizeof(uint32_t)), "a scene without an environment: the block is not zero");
            CHECK(p.light_head == std::vector<uint32_t>{0x2400u}, "the point light's header");
        }
    }
    {   // no light at all: one (unused) header, so that the upload is never empty
        Toy t; ScenePlan p;
        t.add_triangle(0.0f);
        if (build(t, p)) CHECK(p.light_head == std::vector<uint32_t>{0u} && p.env_u.light == PT_NONE, "a scene without lights");
    }
    std::printf("env block and light headers: %d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
