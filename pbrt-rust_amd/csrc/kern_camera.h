// kern_camera.h -- camera rays: camera_ray<CAM>, the staging of fresh paths and the generate kernel of the cameras beside the perspective one (k_generate_cam<CAM>,
// instantiated by tu_camera.hip). k_generate itself, the perspective job's kernel, is in kern_misc.h (tu_misc.hip): the two live in different code objects because the
// LDS layout of a kernel depends on the other kernels of its code object -- with k_generate_cam beside it k_generate was other instructions (profiles/r6/NOTES.md section 17).
#pragma once
#include "kern_common.h"
#include "kern_film.h"   // slot_to_pixel
// ---- camera rays -------------------------------------------------------------------------------------
// One function per camera kind (CAM: PtCameraType); what the kinds share is written once.
//   0  PerspectiveCamera::generate_ray_differential's main ray (perspective.rs:120-179)
//   1  OrthographicCamera's (orthographic.rs:100-121): origin raster_to_camera(pfilm), direction (0,0,1); with a lens, the point of the focal plane the ray
//      meets is seen from the lens sample
//   2  EnvironmentCamera::generate_ray (environment.rs:36-51): theta = PI * pfilm.y / full_resolution.y, phi = 2 PI * pfilm.x / full_resolution.x, in that
//      operation order, d = (sin theta cos phi, cos theta, sin theta sin phi) from the origin. The lens sample is drawn (dimensions 3 and 4) and unused.
// The direction is NOT normalised after camera_to_world: a scaled camera hands on a non-unit d, as the reference does.
template <int CAM>
PT_DEV void camera_ray(const RenderConst &rc, float pfx, float pfy, float time_u, P2 plens_u, V3 &o, V3 &d) {
    V3 ro(0.0f, 0.0f, 0.0f), rd;
    if constexpr (CAM == PT_CAMERA_ENVIRONMENT) {
        const float theta = kPi * pfy / rc.full_res(1);            // environment.rs:38
        const float phi = 2.0f * kPi * pfx / rc.full_res(0);       // environment.rs:39
        float st, ct, sp, cp;
        dm_sincosf(theta, st, ct); dm_sincosf(phi, sp, cp);
        rd = V3(st * cp, ct, st * sp);                             // environment.rs:40-44
    } else {
        V3 pcamera = xf_point(rc.raster_to_camera, V3(pfx, pfy, 0.0f));
        if constexpr (CAM == PT_CAMERA_ORTHOGRAPHIC) { ro = pcamera; rd = V3(0.0f, 0.0f, 1.0f); }   // orthographic.rs:104-106
        else rd = normalize(pcamera);
        if (rc.lens_radius > 0.0f) {                               // perspective.rs:131-141, orthographic.rs:109-121
            P2 dsk = concentric_sample_disk(plens_u);
            float lx = dsk.x * rc.lens_radius, ly = dsk.y * rc.lens_radius;
            float ft = rc.focal_distance / rd.z;
            V3 pfocus = ro + rd * ft;
            ro = V3(lx, ly, 0.0f);
            rd = normalize(pfocus - ro);
        }
    }
    (void)time_u;  // ray.time = lerp(time, open, close) has no effect without animated transforms
    // Transform::transform_ray (transform.rs:543-577)
    V3 oerr;
    V3 ow = xf_point_err(rc.camera_to_world, ro, oerr);
    V3 dw = xf_vector(rc.camera_to_world, rd);
    float l2 = length_squared(dw);
    if (l2 > 0.0f) { float dt = dot(vabs(dw), oerr) / l2; ow = ow + dw * dt; }
    o = ow; d = dw;
}

// A fresh path's core record (64 B) and ray record (32 B) are staged in LDS by the lane that computed them and written by the block
// TRANSPOSED: thread t stores quad (t & 3) of path (t >> 2), so every store instruction of a wave covers 1 KB of consecutive HBM
// (a lane writing its own record quad by quad strides 64 B between lanes: measured 2.5 TB/s against 3.6 TB/s for the old 4-byte arrays).
// meta = dimension 5 after the camera sample, bounces 0, flags: camera ray.
constexpr int kGenPlane = 257;   // quads per LDS plane (256 paths + 1: the four planes of a path land in different banks)
struct GenStage { float4 core[4 * kGenPlane]; float4 ray[2 * kGenPlane]; uint32_t alive[256]; };
PT_DEV void stage_path(GenStage &g, uint32_t t, float pfx, float pfy, V3 o, V3 d, uint64_t index, uint32_t medium) {
    g.core[0 * kGenPlane + t] = make_float4(0.0f, 0.0f, 0.0f, 1.0f);                                               // L, etascale
    g.core[1 * kGenPlane + t] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(5u | (PF_CAMERA_RAY << 24)));        // beta, meta
    g.core[2 * kGenPlane + t] = make_float4(__uint_as_float((uint32_t)index), __uint_as_float((uint32_t)(index >> 32)), pfx, pfy);
    g.core[3 * kGenPlane + t] = make_float4(__uint_as_float(medium), __uint_as_float(PT_NONE), 0.0f, 0.0f);        // medium (volpath: the camera's, perspective.rs:114), mis_medium
    g.ray[0 * kGenPlane + t] = make_float4(o.x, o.y, o.z, d.x); g.ray[1 * kGenPlane + t] = make_float4(d.y, d.z, 0.0f, 0.0f);
}
PT_DEV void flush_paths(const GenStage &g, const PathSoA &ps, uint32_t pid0, uint32_t t) {   // all 256 threads; pid0 = first path id of the block's batch
    float4 *core = reinterpret_cast<float4 *>(ps.core) + 4 * (size_t)pid0, *ray = reinterpret_cast<float4 *>(ps.ray) + 2 * (size_t)pid0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) { const uint32_t gq = j * 256u + t, p = gq >> 2, q = gq & 3u; if (g.alive[p]) core[gq] = g.core[q * kGenPlane + p]; }
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j) { const uint32_t gq = j * 256u + t, p = gq >> 1, q = gq & 1u; if (g.alive[p]) ray[gq] = g.ray[q * kGenPlane + p]; }
}

template <int CAM>
__global__ __launch_bounds__(256) void k_generate_cam(RenderConst rc, SobolTables tabs, PathSoA ps, uint32_t *q_ext, uint32_t *q_ext_count, DevCounters *counters) {
#include "kern_generate_body.h"
}
