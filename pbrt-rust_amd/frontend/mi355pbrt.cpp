// mi355pbrt -- command-line renderer: the drop-in for `pbrt-rust scene.pbrt` on this back end (main.rs + api.rs:1715-1748).
//   mi355pbrt scene.pbrt [--outfile out.pfm] [--device N] [--spp N] [--quiet] [--samples A:B] [--checkpoint FILE] [--preview-every N]
//                        [--adaptive T [--adaptive-step N] [--adaptive-min N]] [--aov FILE.exr] [--denoise FILE [--denoise-iterations N]]
// Parses with libmi355front.so, renders with libmi355pt.so (HIP; Integrator "ambientocclusion": libmi355ao.so), writes the film in the format the Film's "filename"
// extension names (exr -- the reference's default "pbrt.exr" -- png, tga, pfm: core/imageio.rs:42-60).
// The film lives on the device and is rendered in groups of samples (pt_render_samples); one group -- the whole job -- unless asked otherwise:
//   --samples A:B        sample numbers [A, B) of the job's spp only (0 <= A < B <= spp)
//   --checkpoint FILE    after every group (--preview-every N samples, else one wavefront pass) the raw XYZW sums + a header go to FILE; a FILE of this job found at the
//                        start is resumed from its `samples done`, one of another job is refused
//   --preview-every N    every N samples the outfile is written from the film so far (pt_film_resolve_device)
//   --adaptive T         adaptive sampling: two half films, rounds of --adaptive-step N samples (default 4) into each; after a round (once --adaptive-min N samples are
//                        done, default 0) the 16x16 tiles whose film footprint no longer meets a film tile with halves error > T stop for good (pt_film_halves_error,
//                        pt_tiles_select, pt_render_tiles), the others go on up to the job's spp. Not with --samples / --checkpoint (the state of an adaptive render is
//                        a sample count per tile, which neither holds) nor Integrator "ambientocclusion" (libmi355ao has no tile-list render).
//   --aov FILE.exr       the feature buffers a denoiser takes beside the image (libmi355aov.so), for the sample numbers the image is made of: one uncompressed FLOAT
//                        scan-line EXR with the channels N.X N.Y N.Z (normalised mean shading normal), Z (mean depth of the hits), albedo.B albedo.G albedo.R. Not with
//                        --adaptive (libmi355aov has no tile-list render).
//   --denoise FILE       the denoised image (libmi355dn.so: an edge-avoiding a-trous filter guided by the feature buffers) goes to FILE, in the format its extension names;
//                        the outfile still receives the unfiltered image. The sample numbers are rendered as two halves, [A, (A + B) / 2) and [(A + B) / 2, B), whose
//                        difference is the filter's noise estimate, so there must be two of them at least; the outfile's film is their sum. --denoise-iterations N: the
//                        filter's levels, 0..5 (default 5). Not with --adaptive (tiles hold different sample counts), --checkpoint (it holds one film) or
//                        --preview-every (the film so far is two halves).
#include "../../include/mi355front.h"
#include "../../include/mi355aov.h"
#include "../../include/mi355dn.h"
#include <hip/hip_runtime_api.h>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static const char *kUsage = "usage: mi355pbrt scene.pbrt [--outfile out.pfm] [--device N] [--spp N] [--quiet] [--samples A:B] [--checkpoint FILE] [--preview-every N]\n"
                            "                 [--adaptive T [--adaptive-step N] [--adaptive-min N]] [--aov FILE.exr] [--denoise FILE [--denoise-iterations N]]\n";
static int usage(const std::string &why = "") { if (!why.empty()) std::fprintf(stderr, "mi355pbrt: %s\n", why.c_str()); std::fputs(kUsage, stderr); return 2; }

// "A:B" with decimal A < B, both fitting 32 bits
static bool parse_range(const std::string &a, long long &lo, long long &hi) {
    const size_t c = a.find(':');
    if (c == std::string::npos || c == 0 || c + 1 >= a.size() || a.size() > 21) return false;
    for (size_t i = 0; i < a.size(); ++i) if (i != c && (a[i] < '0' || a[i] > '9')) return false;
    lo = std::atoll(a.substr(0, c).c_str()); hi = std::atoll(a.substr(c + 1).c_str());
    return lo < hi && hi <= 0xffffffffll;
}

int main(int argc, char **argv) {
    std::string scene, outfile, samples, checkpoint, aov, denoise; long long dn_iterations = -1; int device = 0, spp = 0; long long preview = 0; bool quiet = false;
    bool adaptive = false; float threshold = 0.0f; long long astep = 4, amin = 0;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "--outfile" && i + 1 < argc) outfile = argv[++i];
        else if (a == "--device" && i + 1 < argc) device = std::atoi(argv[++i]);
        else if (a == "--spp" && i + 1 < argc) spp = std::atoi(argv[++i]);
        else if (a == "--samples" && i + 1 < argc) samples = argv[++i];
        else if (a == "--checkpoint" && i + 1 < argc) checkpoint = argv[++i];
        else if (a == "--aov" && i + 1 < argc) aov = argv[++i];
        else if (a == "--denoise" && i + 1 < argc) denoise = argv[++i];
        else if (a == "--denoise-iterations" && i + 1 < argc) {
            char *end = nullptr; dn_iterations = std::strtoll(argv[++i], &end, 10);
            if (end == argv[i] || *end || dn_iterations < 0 || dn_iterations > 5) return usage("--denoise-iterations takes a number of levels 0..5");
        }
        else if (a == "--preview-every" && i + 1 < argc) { preview = std::atoll(argv[++i]); if (preview <= 0 || preview > 0xffffffffll) return usage("--preview-every takes a number of samples > 0"); }
        else if (a == "--adaptive" && i + 1 < argc) {
            char *end = nullptr; threshold = std::strtof(argv[++i], &end);
            if (end == argv[i] || *end || !(threshold >= 0.0f)) return usage("--adaptive takes an error threshold >= 0");
            adaptive = true;
        }
        else if (a == "--adaptive-step" && i + 1 < argc) { astep = std::atoll(argv[++i]); if (astep <= 0 || astep > 0xffffffffll) return usage("--adaptive-step takes a number of samples > 0"); }
        else if (a == "--adaptive-min" && i + 1 < argc) { amin = std::atoll(argv[++i]); if (amin < 0 || amin > 0xffffffffll) return usage("--adaptive-min takes a number of samples >= 0"); }
        else if (a == "--quiet") quiet = true;
        else if (a[0] != '-') scene = a;
        else return usage();
    }
    if (scene.empty()) return usage();
    if (adaptive && !samples.empty()) return usage("--adaptive with --samples: an adaptive render chooses its own sample ranges, tile by tile");
    if (adaptive && !checkpoint.empty()) return usage("--adaptive with --checkpoint: a checkpoint holds one sample count for the frame, an adaptive render one per tile");
    if (adaptive && !aov.empty()) return usage("--adaptive with --aov: the feature buffers have no tile-list render");
    if (adaptive && !denoise.empty()) return usage("--adaptive with --denoise: the filter takes one sample count for the frame, an adaptive render's tiles hold different ones");
    if (!checkpoint.empty() && !denoise.empty()) return usage("--checkpoint with --denoise: a checkpoint holds one film, a denoising run renders two halves");
    if (preview > 0 && !denoise.empty()) return usage("--preview-every with --denoise: a preview shows the film so far, which a denoising run keeps as two halves");
    if (dn_iterations >= 0 && denoise.empty()) return usage("--denoise-iterations without --denoise");
    long long lo = 0, hi = 0;
    if (!samples.empty() && !parse_range(samples, lo, hi)) return usage("--samples takes A:B with 0 <= A < B, got \"" + samples + "\"");
    ptf_scene *fs = nullptr;
    if (ptf_parse_file(scene.c_str(), &fs) != PT_OK) { std::fprintf(stderr, "mi355pbrt: %s\n", ptf_last_error()); return 1; }
    PtRenderParams rp = *ptf_render_params(fs);
    if (spp > 0) rp.spp = (uint32_t)spp;
    if (samples.empty()) hi = rp.spp;
    else if (hi > (long long)rp.spp) return usage("--samples " + samples + " goes beyond the job's " + std::to_string(rp.spp) + " samples per pixel");
    const uint32_t first = (uint32_t)lo, last = (uint32_t)hi;
    const bool dn = !denoise.empty();
    if (dn && last - first < 2) return usage("--denoise needs two samples per pixel at least: it renders them as two halves");
    const uint32_t mid = first + (last - first) / 2;   // --denoise: half A is [first, mid), half B [mid, last)
    if (outfile.empty()) {
        outfile = ptf_output_filename(fs);
    }
    const bool is_ao = rp.integrator == PT_INTEGRATOR_AO;   // Integrator "ambientocclusion" (libmi355ao.so)
    PtAOParams ao{}; if (is_ao) ptf_ao_params(fs, &ao);
    if (adaptive && is_ao) return usage("--adaptive with Integrator \"ambientocclusion\": the ambient-occlusion integrator has no tile-list render");
    const int w = rp.cropped_pixel_bounds[2] - rp.cropped_pixel_bounds[0], h = rp.cropped_pixel_bounds[3] - rp.cropped_pixel_bounds[1];
    if (w <= 0 || h <= 0) { std::fprintf(stderr, "mi355pbrt: empty film\n"); return 1; }
    const size_t npix = (size_t)w * h;
    std::vector<float> film(npix * 4, 0.0f), rgb(npix * 3);
    // a checkpoint of this job: continue after its samples (host work: a file of another job is refused before the device is touched)
    PtfCheckpointHeader ck{PTF_CHECKPOINT_MAGIC, 1u, (uint32_t)w, (uint32_t)h, rp.spp, first, 0u, 0u, ptf_params_hash(&rp, is_ao ? &ao : nullptr)};
    if (!checkpoint.empty()) {
        if (ptf_checkpoint_read(checkpoint.c_str(), &ck, &ck.samples_done, film.data()) != PT_OK) { std::fprintf(stderr, "mi355pbrt: %s\n", ptf_last_error()); return 1; }
        if (ck.samples_done > last - first) { std::fprintf(stderr, "mi355pbrt: checkpoint \"%s\" holds more samples than --samples asks for\n", checkpoint.c_str()); return 1; }
        if (ck.samples_done && !quiet) std::printf("resuming %s at sample %u of [%u, %u)\n", checkpoint.c_str(), first + ck.samples_done, first, last);
    }
    if (pt_init(device) != PT_OK) { std::fprintf(stderr, "mi355pbrt: %s\n", pt_last_error()); return 1; }
    const auto t0 = std::chrono::steady_clock::now();
    pt_scene *sc = nullptr;
    if (pt_scene_create(ptf_scene_desc(fs), &sc) != PT_OK) { std::fprintf(stderr, "mi355pbrt: %s\n", pt_last_error()); return 1; }
    const auto t1 = std::chrono::steady_clock::now();
    float *d_film = nullptr, *d_rgb = nullptr;
    if (hipMalloc((void **)&d_film, npix * 16) != hipSuccess || hipMalloc((void **)&d_rgb, npix * 12) != hipSuccess ||
        hipMemcpy(d_film, film.data(), npix * 16, hipMemcpyHostToDevice) != hipSuccess) { std::fprintf(stderr, "mi355pbrt: device film: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
    // the film so far -> outfile, resolved on the device
    auto write_out = [&]() {
        if (pt_film_resolve_device(sc, d_film, (uint32_t)npix, rp.scale, d_rgb, nullptr) != PT_OK) { std::fprintf(stderr, "mi355pbrt: %s\n", pt_last_error()); return false; }
        if (hipMemcpy(rgb.data(), d_rgb, npix * 12, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "mi355pbrt: reading the image back failed\n"); return false; }
        if (ptf_write_image(outfile.c_str(), w, h, rgb.data()) != PT_OK) { std::fprintf(stderr, "mi355pbrt: %s\n", ptf_last_error()); return false; }
        return true;
    };
    uint32_t group = last - first;   // samples per pt_render_samples call
    if (preview > 0) group = (uint32_t)std::min<long long>(preview, group);
    else if (!checkpoint.empty()) {
        const int pst = is_ao ? pt_ao_pass_size(sc, &rp, &ao, &group) : pt_pass_size(sc, &rp, &group);
        if (pst != PT_OK) { std::fprintf(stderr, "mi355pbrt: %s\n", pt_last_error()); return 1; }
    }
    unsigned long long camera_rays = 0;
    float *d_half_b = nullptr;   // --denoise: half B (d_film is half A until the halves are summed)
    if (dn && (hipMalloc((void **)&d_half_b, npix * 16) != hipSuccess || hipMemset(d_half_b, 0, npix * 16) != hipSuccess || hipDeviceSynchronize() != hipSuccess)) {
        std::fprintf(stderr, "mi355pbrt: device film: %s\n", hipGetErrorString(hipGetLastError())); return 1;
    }
    if (adaptive) {   // runtime.Scene.render_adaptive's loop: d_film is half A, d_half half B, the active set only shrinks
        const auto fail_pt = [&]() { std::fprintf(stderr, "mi355pbrt: %s\n", pt_last_error()); return 1; };
        uint32_t ntx = 0, nty = 0;
        if (pt_tile_grid(&rp, &ntx, &nty) != PT_OK) return fail_pt();
        const size_t n_film_tiles = (size_t)((w + 15) / 16) * ((h + 15) / 16);
        float *d_half = nullptr, *d_err = nullptr;
        if (hipMalloc((void **)&d_half, npix * 16) != hipSuccess || hipMalloc((void **)&d_err, n_film_tiles * 4) != hipSuccess || hipMemset(d_half, 0, npix * 16) != hipSuccess ||
            hipDeviceSynchronize() != hipSuccess) { std::fprintf(stderr, "mi355pbrt: device film: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
        std::vector<uint32_t> active((size_t)ntx * nty), kept(active.size());
        for (size_t i = 0; i < active.size(); ++i) active[i] = (uint32_t)i;
        unsigned long long tile_samples = 0; unsigned rounds = 0;
        for (uint32_t done = 0; done < rp.spp && !active.empty(); ++rounds) {
            uint32_t n_b = 0;
            for (float *half : {d_film, d_half}) {
                const uint32_t n = (uint32_t)std::min<long long>(astep, rp.spp - done);
                if (half == d_half) n_b = n;
                if (n == 0) continue;
                if (pt_render_tiles(sc, &rp, done, n, active.data(), (uint32_t)active.size(), half, 1) != PT_OK) return fail_pt();
                PtCounters c; pt_get_counters(sc, &c); camera_rays += c.camera_rays;
                done += n; tile_samples += (unsigned long long)n * active.size();
            }
            if (n_b > 0 && done >= (uint32_t)amin) {
                uint32_t n_kept = 0;
                if (pt_film_halves_error(sc, d_film, d_half, (uint32_t)w, (uint32_t)h, d_err, nullptr, nullptr) != PT_OK ||
                    pt_tiles_select(sc, &rp, d_err, threshold, active.data(), (uint32_t)active.size(), kept.data(), &n_kept) != PT_OK) return fail_pt();
                active.assign(kept.begin(), kept.begin() + n_kept);
            }
        }
        // A += B: the film is the sum of the halves (host arithmetic on the read-back halves, element by element)
        std::vector<float> half_b(npix * 4);
        if (hipMemcpy(film.data(), d_film, npix * 16, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(half_b.data(), d_half, npix * 16, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "mi355pbrt: reading the film back failed\n"); return 1; }
        for (size_t i = 0; i < film.size(); ++i) film[i] += half_b[i];
        if (hipMemcpy(d_film, film.data(), npix * 16, hipMemcpyHostToDevice) != hipSuccess) { std::fprintf(stderr, "mi355pbrt: writing the film back failed\n"); return 1; }
        (void)hipFree(d_half); (void)hipFree(d_err);
        if (!quiet) std::printf("adaptive: %llu of %llu tile-samples, %u rounds\n", tile_samples, (unsigned long long)ntx * nty * rp.spp, rounds);
    }
    for (uint32_t s = first + ck.samples_done; s < last && !adaptive; ) {
        const uint32_t n = std::min(group, (dn && s < mid ? mid : last) - s);
        float *const into = dn && s >= mid ? d_half_b : d_film;
        const int rst = is_ao ? pt_ao_render_samples(sc, &rp, &ao, s, n, into, 1) : pt_render_samples(sc, &rp, s, n, into, 1);
        if (rst != PT_OK) { std::fprintf(stderr, "mi355pbrt: %s\n", pt_last_error()); return 1; }
        PtCounters c; pt_get_counters(sc, &c); camera_rays += c.camera_rays;
        s += n; ck.samples_done = s - first;
        if (!checkpoint.empty()) {
            if (hipMemcpy(film.data(), d_film, npix * 16, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "mi355pbrt: reading the film back failed\n"); return 1; }
            if (ptf_checkpoint_write(checkpoint.c_str(), &ck, film.data()) != PT_OK) { std::fprintf(stderr, "mi355pbrt: %s\n", ptf_last_error()); return 1; }
        }
        if (preview > 0 && s < last && !write_out()) return 1;
    }
    const auto t2 = std::chrono::steady_clock::now();
    float *d_sums = nullptr;   // the feature sums of sample numbers [first, last), whatever groups (or earlier runs, --checkpoint) rendered the image's: for --denoise and --aov
    if (dn || !aov.empty()) {
        if (hipMalloc((void **)&d_sums, npix * 40) != hipSuccess || hipMemset(d_sums, 0, npix * 40) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { std::fprintf(stderr, "mi355pbrt: feature buffers: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
        const PtAOVBuffers d_planes{d_sums, d_sums + npix * 4, d_sums + npix * 8};
        if (pt_aov_render_samples(sc, &rp, first, last - first, &d_planes, 1) != PT_OK) { std::fprintf(stderr, "mi355pbrt: %s\n", pt_last_error()); return 1; }
    }
    if (dn) {   // the filter reads the halves; then A += B: the outfile's film (host arithmetic on the read-back halves, element by element)
        const PtAOVBuffers d_planes{d_sums, d_sums + npix * 4, d_sums + npix * 8};
        PtDenoiseParams dp; pt_denoise_default_params(&dp);
        if (dn_iterations >= 0) dp.iterations = (uint32_t)dn_iterations;
        dp.scale = rp.scale;
        if (pt_denoise(sc, &dp, d_film, d_half_b, &d_planes, (uint32_t)w, (uint32_t)h, d_rgb, 1) != PT_OK) { std::fprintf(stderr, "mi355pbrt: %s\n", pt_last_error()); return 1; }
        if (hipMemcpy(rgb.data(), d_rgb, npix * 12, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "mi355pbrt: reading the denoised image back failed\n"); return 1; }
        if (ptf_write_image(denoise.c_str(), w, h, rgb.data()) != PT_OK) { std::fprintf(stderr, "mi355pbrt: %s\n", ptf_last_error()); return 1; }
        std::vector<float> half_b(npix * 4);
        if (hipMemcpy(film.data(), d_film, npix * 16, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(half_b.data(), d_half_b, npix * 16, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "mi355pbrt: reading the film back failed\n"); return 1; }
        for (size_t i = 0; i < film.size(); ++i) film[i] += half_b[i];
        if (hipMemcpy(d_film, film.data(), npix * 16, hipMemcpyHostToDevice) != hipSuccess) { std::fprintf(stderr, "mi355pbrt: writing the film back failed\n"); return 1; }
        (void)hipFree(d_half_b);
    }
    if (!write_out()) return 1;
    if (!aov.empty()) {
        std::vector<float> sums(npix * 10, 0.0f), res(npix * 7);
        if (hipMemcpy(sums.data(), d_sums, npix * 40, hipMemcpyDeviceToHost) != hipSuccess) { std::fprintf(stderr, "mi355pbrt: reading the feature buffers back failed\n"); return 1; }
        const PtAOVBuffers planes{sums.data(), sums.data() + npix * 4, sums.data() + npix * 8};
        float *albedo = res.data(), *normal = res.data() + npix * 3, *depth = res.data() + npix * 6;
        if (pt_aov_resolve(&planes, (uint32_t)npix, albedo, normal, depth) != PT_OK) { std::fprintf(stderr, "mi355pbrt: %s\n", pt_last_error()); return 1; }
        const char *names[7] = {"N.X", "N.Y", "N.Z", "Z", "albedo.B", "albedo.G", "albedo.R"};   // (byte-wise sorted, as the format stores them)
        const float *data[7] = {normal, normal + 1, normal + 2, depth, albedo + 2, albedo + 1, albedo};
        const uint32_t strides[7] = {3, 3, 3, 1, 3, 3, 3};
        if (ptf_write_exr_channels(aov.c_str(), w, h, 7, names, data, strides) != PT_OK) { std::fprintf(stderr, "mi355pbrt: %s\n", ptf_last_error()); return 1; }
    }
    if (!quiet) {
        const double ts = std::chrono::duration<double>(t1 - t0).count(), tr = std::chrono::duration<double>(t2 - t1).count();
        std::printf("%s: %dx%d, %u spp, %llu camera rays, scene %.2f s, render %.3f s (%.1f Msamples/s) -> %s\n", scene.c_str(), w, h, rp.spp,
                    camera_rays, ts, tr, (double)camera_rays / tr / 1e6, outfile.c_str());
    }
    (void)hipFree(d_film); (void)hipFree(d_rgb); (void)hipFree(d_sums);
    pt_scene_destroy(sc); ptf_scene_destroy(fs);
    return 0;
}
