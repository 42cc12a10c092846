// pass_budget.h -- the pass size a render chooses when the caller leaves it to the library (PtRenderParams.spp_per_pass = 0): host arithmetic, no HIP call, so that
// tests/pass_budget/check_pass_budget.cpp checks it without a device. choose_pass_size (render_loop.hip) is hipMemGetInfo plus pass_size_for; every integrator goes through it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace pth {

// What an integrator adds to the rule: the bytes per path it allocates besides the scene's workspace, the part of the device's memory a pass may take, and the most paths
// one pass may hold.
struct PassBudget { size_t extra_bytes_per_path; double mem_fraction; size_t max_paths; };

// As many paths in flight as the memory allows. Every wavefront iteration ends in a tail of straggling rays (~0.8 ms on S2, whatever the launch size), so fewer, larger
// iterations spend less of the render in tails: S2 at 1080p x 256 spp: 32 samples per pass 1267, 64: 1367, 128: 1439, 256: 1468 Msamples/s.
// free_b: the device's free memory; held_b: what the scene's present workspace holds (it is freed before a larger one is allocated, and a pass that fits it is always
// affordable); per_path: workspace + the integrator's extra; `share` = renders that will hold a workspace on this device at the same time (pt_multi_render with a device
// listed more than once). Returns samples per pixel per pass: 1 <= S <= n_samples, in passes of equal size.
inline uint32_t pass_size_for(size_t free_b, size_t held_b, size_t per_path, const PassBudget &b, uint32_t n_pix_slots, uint32_t n_samples, uint32_t share) {
    share = std::max(1u, share); per_path = std::max<size_t>(1, per_path); n_samples = std::max(1u, n_samples);
    const size_t afford = std::max(held_b / per_path, (size_t)((double)(free_b / share + held_b) * b.mem_fraction) / per_path);
    const size_t paths = std::min(afford, b.max_paths / share);
    const uint32_t S = (uint32_t)std::min<size_t>(n_samples, std::max<size_t>(1, paths / std::max(1u, n_pix_slots)));
    const uint32_t n_pass = (n_samples + S - 1) / S;
    return (n_samples + n_pass - 1) / n_pass;   // passes of equal size
}

}  // namespace pth
