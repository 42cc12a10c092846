// kern_generate_body.h -- NOT a header: the body of the generate kernels (kern_misc.h), included once inside each kernel's braces with `CAM` (PtCameraType) in scope as a
// constant: k_generate defines it, k_generate_cam<CAM> has it as its template parameter. Everything but the camera_ray<CAM> calls is the same code for every camera.
// (Why not an inlined function template: blockDim and gridDim read inside a device function are not the uniform block size a kernel's own reads are to the compiler, and
// handed in as arguments they are loaded at another place; either way k_generate stops being the instructions it was -- profiles/r6/NOTES.md section 17.)
// Parameters in scope: RenderConst rc, SobolTables tabs, PathSoA ps, uint32_t *q_ext, uint32_t *q_ext_count, DevCounters *counters.
    // LDS copies of what every lane needs, folded by NIBBLE of the word they are indexed with (the XORs of lowdiscrepancy.rs:512-569 regrouped, as in the shade
    // kernels' Sobol' windows): the generator matrices of dimensions 0..4 (SobolTables::nib) and the two van-der-Corput matrices of m. A look-up per nibble
    // replaces a count-trailing-zeros step per set bit -- the kernel issued vector instructions 99.7 % of its cycles, two thirds of them in those bit loops.
    constexpr uint32_t kVdcNibbles = 13;   // 52 columns
    __shared__ uint32_t s_nib[kSobolNibbles * 5 * 16];
    __shared__ uint64_t s_vdc[2 * kVdcNibbles * 16];   // [M | MI][nibble][16]
    __shared__ LdsQueue<1024> s_q;
    __shared__ GenStage s_gen;
    lq_init(s_q);
    const uint32_t m = (uint32_t)rc.sobol.log2_resolution;
    sobol_stage_lds(s_nib, tabs.nib, 5u, threadIdx.x, blockDim.x);
    if (m > 0) for (uint32_t i = threadIdx.x; i < 2 * kVdcNibbles * 16; i += blockDim.x) {
        const uint32_t which = i / (kVdcNibbles * 16), e = i - which * (kVdcNibbles * 16), j = e >> 4, n = e & 15u;
        const uint64_t *col = (which ? tabs.vdc_inv : tabs.vdc) + (m - 1) * 52 + 4 * j;
        uint64_t v = 0;
        for (uint32_t b = 0; b < 4; ++b) if (n & (1u << b)) v ^= col[b];
        s_vdc[i] = v;
    }
    __syncthreads();
    const uint32_t total = rc.n_pix_slots * rc.s_count;
    const uint32_t stride = gridDim.x * blockDim.x;
    const uint32_t rounded = (total + 255u) & ~255u;   // whole blocks iterate together (block-level queue flushes)
    unsigned long long n_alive = 0;
    for (uint32_t pid = blockIdx.x * blockDim.x + threadIdx.x; pid < rounded; pid += stride) {
        bool alive = false;
        if (pid < total) {
            const uint32_t slot = pid % rc.n_pix_slots, sl = pid / rc.n_pix_slots;
            int32_t px, py;
            if (slot_to_pixel(rc, slot, px, py)) {
                const uint64_t sample = rc.s_begin + sl;
                if (rc.halton.enabled) {   // HaltonSampler: same GlobalSampler bookkeeping, its own index and dimensions (halton.rs:122-165)
                    const uint64_t index = halton_index_for_sample(rc.halton, px, py, sample);
                    const float fx = halton_sample_dimension(tabs, rc.halton, index, 0u), fy = halton_sample_dimension(tabs, rc.halton, index, 1u);
                    const float pfx = (float)px + fx, pfy = (float)py + fy;   // get_camera_sample: p_film = pixel + get_2d() (sampler.rs:170-180)
                    const float tm = halton_sample_dimension(tabs, rc.halton, index, 2u);
                    const P2 pl(halton_sample_dimension(tabs, rc.halton, index, 3u), halton_sample_dimension(tabs, rc.halton, index, 4u));
                    V3 o, d;
                    camera_ray<CAM>(rc, pfx, pfy, tm, pl, o, d);
                    stage_path(s_gen, threadIdx.x, pfx, pfy, o, d, index, rc.volpath ? rc.camera_medium : PT_NONE);
                    alive = true;
                } else {
                // sobol_interval_to_index (lowdiscrepancy.rs:512-543) through the nibble tables
                uint64_t index = 0;
                if (m != 0) {
                    index = sample << (m << 1);
                    uint64_t delta = 0;
                    for (uint64_t f = sample, j = 0; f != 0; f >>= 4, ++j) delta ^= s_vdc[j * 16 + (f & 15u)];
                    uint64_t b = ((uint64_t)((uint32_t)(px - rc.sobol.sb_min[0]) << m) | (uint64_t)(uint32_t)(py - rc.sobol.sb_min[1])) ^ delta;
                    for (uint32_t j = 0; b != 0; b >>= 4, ++j) index ^= s_vdc[kVdcNibbles * 16 + j * 16 + (b & 15u)];
                }
                // get_camera_sample (sampler.rs:170-180): pfilm = get_2d, time = get_1d, plens = get_2d
                const uint32_t v0 = sobol_bits_nib(s_nib, 5u * 16u, tabs.m32, index), v1 = sobol_bits_nib(s_nib + 16, 5u * 16u, tabs.m32 + 52, index), v2 = sobol_bits_nib(s_nib + 32, 5u * 16u, tabs.m32 + 104, index),
                               v3 = sobol_bits_nib(s_nib + 48, 5u * 16u, tabs.m32 + 156, index), v4 = sobol_bits_nib(s_nib + 64, 5u * 16u, tabs.m32 + 208, index);
                // sobol.rs:77-81: film dimensions are remapped to the pixel
                float fx = sobol_to_float(v0) * (float)rc.sobol.resolution + (float)rc.sobol.sb_min[0];
                fx = clampf(fx - (float)px, 0.0f, kOneMinusEps);
                float fy = sobol_to_float(v1) * (float)rc.sobol.resolution + (float)rc.sobol.sb_min[1];
                fy = clampf(fy - (float)py, 0.0f, kOneMinusEps);
                const float pfx = (float)px + fx, pfy = (float)py + fy;
                V3 o, d;
                camera_ray<CAM>(rc, pfx, pfy, sobol_to_float(v2), P2(sobol_to_float(v3), sobol_to_float(v4)), o, d);
                stage_path(s_gen, threadIdx.x, pfx, pfy, o, d, index, rc.volpath ? rc.camera_medium : PT_NONE);
                alive = true;
                }
            }
        }
        s_gen.alive[threadIdx.x] = alive ? 1u : 0u;
        __syncthreads();
        flush_paths(s_gen, ps, pid - threadIdx.x, threadIdx.x);   // (the queue flush below holds the barrier that protects s_gen for the next round)
        lq_push(s_q, pid, alive);
        lq_sync_flush(s_q, q_ext_count, q_ext, 256u, false);
        n_alive += alive ? 1ull : 0ull;
    }
    lq_sync_flush(s_q, q_ext_count, q_ext, 0u, true);
    counter_add(&counters->camera_rays, n_alive);
