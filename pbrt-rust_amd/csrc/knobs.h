// knobs.h -- every compile-time tuning constant of the library, with its measured default. `-DPT_X=value` (tools/build_variant.sh) overrides one for an
// A/B build. One line each: what it sets and where its sweep is on record; the measurement narratives stay beside the code they explain.
#pragma once

// ---- k_trace (kern_trace.h): traversal stack entries per lane kept in LDS (kernels.h: kLdsStack*); deeper entries spill to HBM
#ifndef PT_LDS_STACK
#define PT_LDS_STACK 10               // exact walk, triangle-only scenes: seven workgroups fit a CU's LDS (kernels.h; profiles/HISTORY.md, PT_TRACE_WAVES)
#endif
#ifndef PT_LDS_STACK_GENERAL
#define PT_LDS_STACK_GENERAL 12       // exact walk, scenes with instances: a marker entry per instance entered (kernels.h: C4 with 10, trace +2.3 %)
#endif
#ifndef PT_LDS_STACK_QUAD
#define PT_LDS_STACK_QUAD 15          // four-wide walk, up to three pushes per record: five waves per SIMD x 7 KB per wave (kernels.h)
#endif
#ifndef PT_LDS_STACK_QUAD_INST
#define PT_LDS_STACK_QUAD_INST 19     // four-wide walk of scenes with instances: four waves per SIMD share a CU's LDS (kernels.h; kern_trace.h: kWrayHbm)
#endif
// ---- k_trace: waves per SIMD the kernel is compiled for (kern_trace.h: trace_waves)
#ifndef PT_TRACE_WAVES
#define PT_TRACE_WAVES 6              // exact walk, triangle-only: 80 VGPRs, no scratch (profiles/HISTORY.md, PT_TRACE_WAVES)
#endif
#ifndef PT_TRACE_WAVES_INST
#define PT_TRACE_WAVES_INST 4         // exact walk, triangles + instances (profiles/HISTORY.md, PT_TRACE_WAVES_INST)
#endif
#ifndef PT_TRACE_WAVES_QUAD
#define PT_TRACE_WAVES_QUAD 5         // four-wide walk, triangle-only: eight quads of a record in flight per lane; x 7 KB of LDS stack per wave (kernels.h: kLdsStackQuad)
#endif
#ifndef PT_TRACE_WAVES_QUAD_INST
#define PT_TRACE_WAVES_QUAD_INST 4    // four-wide walk, triangles + instances: what a CU's LDS holds (kernels.h: kLdsStackQuadInst)
#endif
#ifndef PT_TRACE_WAVES_PROBE
#define PT_TRACE_WAVES_PROBE 1        // triangle-only probe-chain kernel: 125 VGPRs; four waves asked for measured slower (profiles/r5/NOTES.md)
#endif
// ---- k_trace: work distribution
#ifndef PT_TRACE_CHUNK
#define PT_TRACE_CHUNK 512            // queue entries a wave reserves per atomic (profiles/HISTORY.md, PT_TRACE_CHUNK)
#endif
#ifndef PT_TRACE_TAIL_ROUNDS
#define PT_TRACE_TAIL_ROUNDS 2        // scenes with instances: grid rounds before the queue's end within which the bites shrink; 0 = never (kern_trace.h: kTailBites)
#endif

// ---- k_shade (kern_shade.h: shade_waves): waves per SIMD
#ifndef PT_SHADE_WAVES
#define PT_SHADE_WAVES 1              // floor for the one-lobe kernels; the measured per-class values are in shade_waves (profiles/r3/NOTES.md)
#endif
#ifndef PT_P2_WAVES                   // the plastic-like two-lobe kernel of triangle-only scenes; the three are overridden together or not at all (kern_shade.h)
#define PT_P2_WAVES 3                 // waves per SIMD: 168 VGPRs + 80 B of scratch
#define PT_P2_DIMS 28u                // Sobol' dimensions staged in LDS
#define PT_P2_QCAP 512                // entries of its LDS queues: 51 KB per workgroup, three fit a CU
#endif
#ifndef PT_METAL_WAVES
#define PT_METAL_WAVES 3              // the metal-only one-lobe kernel of triangle-only scenes (kern_shade.h)
#endif
// ---- the other kernels: waves per SIMD
#ifndef PT_BSSRDF_WAVES
#define PT_BSSRDF_WAVES ((SPH || VOL) ? 1 : 3)   // k_bssrdf, in its template arguments: three in triangle-only scenes (kern_bssrdf.h: C5 41.1 -> 35.7 ms)
#endif
#ifndef PT_MISS_WAVES
#define PT_MISS_WAVES 1               // k_shade_miss (profiles/r3/NOTES.md: six waves spill)
#endif
#ifndef PT_FILM_WAVES
#define PT_FILM_WAVES 4               // k_film_final: 128 registers + 32 B of scratch (kern_aux.h: three to eight waves on C2)
#endif

// ---- render_loop.hip: blocks per CU of the persistent grids, and the largest pass
#ifndef PT_SHADE_BLOCKS_PER_CU
#define PT_SHADE_BLOCKS_PER_CU 24u    // k_shade: evens out the per-vertex cost differences (render_loop.hip: 8 -> 24, 80.1 -> 76.3 ms on C2)
#endif
#ifndef PT_GEN_BLOCKS_PER_CU
#define PT_GEN_BLOCKS_PER_CU 40u      // k_generate (render_loop.hip: 16 -> 40, 12.2 -> 11.7 ms on C2)
#endif
#ifndef PT_ROUTE_BLOCKS_PER_CU
#define PT_ROUTE_BLOCKS_PER_CU 3u     // k_route: what a CU's LDS holds of its staging queues (render_loop.hip)
#endif
#ifndef PT_MISS_BLOCKS_PER_CU
#define PT_MISS_BLOCKS_PER_CU 16u     // k_shade_miss: insensitive (render_loop.hip)
#endif
#ifndef PT_PASS_MAX_PATHS_LOG2
#define PT_PASS_MAX_PATHS_LOG2 29     // log2 of the most paths in flight in one pass (host_common.h: kPathPassBudget, the path integrators' budget of choose_pass_size)
#endif
