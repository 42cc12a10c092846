// scene_plan.h -- the host-only half of pt_scene_create: the checks of the caller's PtSceneDesc and every table the kernels read that is not one of the caller's own
// arrays. No HIP runtime call, no pt_scene, none of the driver's globals: the unit is built and checked without a device (tests/scene_plan/check_plan.cpp).
#pragma once
#include <functional>
#include <string>
#include <vector>
#include "kernels.h"
#include "host_bvh.h"

namespace pth {
using namespace ptd;   // the device-side records and constants (dev_scene.h, kernels.h)

// Shade class of a material = the kernel its vertices are shaded by (kernels.h: kNumClasses).
uint8_t material_class(const PtMaterial &m, bool specialise, bool untextured);
// Distribution1D::new on the host (sampling.rs:12-34) for the uniform / power strategies and the env map.
void dist1d(const std::vector<float> &func, std::vector<float> &cdf, float &func_int);
// Bounds3f of the eight transformed corners of [lo, hi] (transform.rs:592-605): a quadric's and an instance's world bound.
PrimBound transform_bounds(const float m[16], const float lo[3], const float hi[3]);

struct PlanOptions {
    bool shade_specialise = true;      // hand out the lobe-set shade classes (PT_SHADE_SPECIALISE)
    uint32_t pool_pad_records = 0;     // TEST HOOK: unused records in front of the record / packet pool (PT_TEST_POOL_PAD_RECORDS)
};
// BVHAccel::new over primitive bounds: PT_OK, or a status with `msg` set (pt_scene_create: host SAH or the device's HLBVH, by split_method).
using AccelBuilder = std::function<PtStatus(const std::vector<PrimBound> &prims, uint32_t max_node_prims, std::vector<PtBVHNode> &nodes, std::vector<uint32_t> &ordered, std::string &msg)>;
PtStatus sah_builder(const std::vector<PrimBound> &prims, uint32_t max_node_prims, std::vector<PtBVHNode> &nodes, std::vector<uint32_t> &ordered, std::string &msg);

struct ScenePlan {
    // the top-level tree (adopted or built) and its primitive order: what pt_scene keeps for pt_scene_bvh_read
    std::vector<PtBVHNode> nodes;
    std::vector<uint32_t> ordered;
    bool exact_walk_only = false, quad_walk_only = false, pool_big = false;   // (host_common.h: pt_scene)
    // Traversal records (dev_scene.h: WideNode, QuadNode) and the packet order of every accelerator, concatenated: [top level][object 0][object 1]... ;
    // references inside an accelerator are offset by its bases (and record references of `quad` by the pad records in front of the pool).
    std::vector<WideNode> wide;             // released (one dummy record) when quad_walk_only
    std::vector<QuadNode> quad;             // at least one record
    uint32_t root_ref = 0, root_ref4 = 0;
    std::vector<uint32_t> packet_refs;      // per packet: the primitive it is built from
    std::vector<uint32_t> leaf_last;        // per leaf: its last packet
    std::vector<DevInstance> instances;
    // the pool [pad records][records][packets + 2], in bytes (records of 8 quads, packets of 3; +2: a packet's fourth quad is loaded with it)
    size_t pad_bytes = 0, quad_bytes = 0, pool_bytes = 0;
    // materials, lights
    std::vector<uint8_t> mat_class;         // at least one entry
    bool class_used[kNumClasses] = {true, false, false, false, true, false, false, false, false, false, false};
    bool has_null_material = false, has_bssrdf = false;
    std::vector<uint32_t> infinite_lights;
    // textures: one postfix program per node (children before parent), tex_prog[tex_prog_offset[i] .. tex_prog_offset[i + 1]); per image its level offsets (texels: NULL, the caller's)
    std::vector<uint32_t> tex_prog_offset, tex_prog;
    std::vector<DevImage> images;
    // Distribution2D::new (sampling.rs:100-117) over env_importance: conditional cdf rows, their integrals (= the marginal's function), the marginal's cdf and integral
    std::vector<float> env_cdf, env_func_int, env_marg_cdf; float env_marg_int = 0.0f;
    // the environment light's wave-uniform block (dev_scene.h: EnvUniform) and every light's record header (light_rec_head: type and delta bit; k_light_area adds the triangle's bits)
    EnvUniform env_u;
    std::vector<uint32_t> light_head;       // at least one entry
    // GridDensityMedium::new (grid.rs:40-72) per medium: sigma_t, 1 / max density (density: NULL, the caller's)
    std::vector<DevGridAux> grid_aux; bool has_grid = false;
    // world bound = root node bounds (bvh.rs:697-703); Light::preprocess -> bounding sphere (bounds.rs:516-524)
    float wb_min[3] = {0, 0, 0}, wb_max[3] = {0, 0, 0}, world_center[3] = {0, 0, 0}, world_radius = 0.0f;
    std::vector<std::string> warnings;      // for the caller's stderr
};

// Every refusal that needs no accelerator. `msg` is set when the status is not PT_OK.
PtStatus plan_validate(const PtSceneDesc &d, std::string &msg);
// Accelerators and the tables above, for a descriptor plan_validate accepted; refuses what only the built trees show (record / packet / pool limits).
PtStatus plan_build(const PtSceneDesc &d, const PlanOptions &opt, const AccelBuilder &build, ScenePlan &plan, std::string &msg);

}  // namespace pth
