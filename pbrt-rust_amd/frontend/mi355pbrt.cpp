// mi355pbrt -- command-line renderer: the drop-in for `pbrt-rust scene.pbrt` on this back end (main.rs + api.rs:1715-1748). The command line: kUsage below.
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
// What needs no device -- the flags, what they refuse, the sample numbers of a run and the render calls of its loop -- is cli_plan.h; this file is the device work.
#include "cli_plan.h"
#include "../../include/mi355aov.h"
#include "../../include/mi355dn.h"
#include <hip/hip_runtime_api.h>
#include <chrono>
#include <cstdio>

static const char *kUsage = "usage: mi355pbrt scene.pbrt [--outfile out.pfm] [--device N] [--spp N] [--quiet] [--samples A:B] [--checkpoint FILE] [--preview-every N]\n"
                            "                 [--adaptive T [--adaptive-step N] [--adaptive-min N]] [--aov FILE.exr] [--denoise FILE [--denoise-iterations N]]\n";

// The one failure path: the text on stderr, exit status 1. pt_ok, ptf_ok and hip_ok are false after they reported a failed call of their kind.
static int die(const char *text) { std::fprintf(stderr, "mi355pbrt: %s\n", text); return 1; }
static int usage(const std::string &why) { if (!why.empty()) die(why.c_str()); std::fputs(kUsage, stderr); return 2; }
static bool pt_ok(int st) { return st == PT_OK || !die(pt_last_error()); }
static bool ptf_ok(int st) { return st == PT_OK || !die(ptf_last_error()); }
static bool hip_ok(hipError_t e, const char *text) { return e == hipSuccess || !die(text); }
static bool hip_failed(const char *what) { return !die((std::string(what) + ": " + hipGetErrorString(hipGetLastError())).c_str()); }   // (false)
static bool download(std::vector<float> &to, const float *d_from, const char *text) { return hip_ok(hipMemcpy(to.data(), d_from, to.size() * 4, hipMemcpyDeviceToHost), text); }

// Owners: whatever path leaves main, the device buffers go first, then the scene, then the parsed file.
struct Parsed { ptf_scene *p = nullptr; ~Parsed() { if (p) ptf_scene_destroy(p); } };
struct Scene { pt_scene *p = nullptr; ~Scene() { if (p) pt_scene_destroy(p); } };
struct DeviceBuffer {
    float *p = nullptr;
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    // `zero`: cleared, and the device waited for (the library renders on its own stream: the zeros must be there before it adds to them)
    bool alloc(const char *what, size_t bytes, bool zero) {
        if (hipMalloc((void **)&p, bytes) != hipSuccess) p = nullptr;
        return (p && (!zero || (hipMemset(p, 0, bytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess))) || hip_failed(what);
    }
};

struct Job {   // what the steps share
    const Options &o; const Plan &p;
    const PtAOParams *ao;                    // of Integrator "ambientocclusion" (libmi355ao.so), else null
    size_t npix;
    std::vector<float> film, rgb;            // on the host: the XYZW sums, a resolved image
    Scene sc;
    DeviceBuffer d_film, d_rgb, d_half_b;    // d_half_b: --adaptive and --denoise render two halves, and d_film is half A until sum_halves
    unsigned long long camera_rays = 0;
};

// A += B: the film is the sum of the halves (host arithmetic on the read-back halves, element by element)
static bool sum_halves(std::vector<float> &film, float *d_a, const float *d_b) {
    std::vector<float> half_b(film.size());
    if (!download(film, d_a, "reading the film back failed") || !download(half_b, d_b, "reading the film back failed")) return false;
    for (size_t i = 0; i < film.size(); ++i) film[i] += half_b[i];
    return hip_ok(hipMemcpy(d_a, film.data(), film.size() * 4, hipMemcpyHostToDevice), "writing the film back failed");
}

// the three planes in one array of feature sums: albedo and normal of 4 floats per pixel, depth of 2
static PtAOVBuffers feature_planes(float *sums, size_t npix) { return {sums, sums + npix * 4, sums + npix * 8}; }

// d_rgb -> an image file
static bool write_rgb(Job &j, const std::string &path, const char *text) {
    return download(j.rgb, j.d_rgb.p, text) && ptf_ok(ptf_write_image(path.c_str(), j.p.width, j.p.height, j.rgb.data()));
}

// the film so far -> outfile, resolved on the device
static bool write_out(Job &j) {
    return pt_ok(pt_film_resolve_device(j.sc.p, j.d_film.p, (uint32_t)j.npix, j.p.rp.scale, j.d_rgb.p, nullptr)) && write_rgb(j, j.o.outfile, "reading the image back failed");
}

// a checkpoint of this job: continue after its samples (host work: a file of another job is refused before the device is touched)
static bool resume(Job &j, PtfCheckpointHeader &ck) {
    const Options &o = j.o;
    if (!ptf_ok(ptf_checkpoint_read(o.checkpoint.c_str(), &ck, &ck.samples_done, j.film.data()))) return false;
    if (ck.samples_done > j.p.last - j.p.first) return !die(("checkpoint \"" + o.checkpoint + "\" holds more samples than --samples asks for").c_str());
    if (ck.samples_done && !o.quiet) std::printf("resuming %s at sample %u of [%u, %u)\n", o.checkpoint.c_str(), j.p.first + ck.samples_done, j.p.first, j.p.last);
    return true;
}

// runtime.Scene.render_adaptive's loop: d_film is half A, d_half_b half B, the active set only shrinks
static bool render_adaptive(Job &j) {
    const Options &o = j.o; const PtRenderParams &rp = j.p.rp; pt_scene *sc = j.sc.p;
    uint32_t ntx = 0, nty = 0;
    if (!pt_ok(pt_tile_grid(&rp, &ntx, &nty))) return false;
    DeviceBuffer d_err;   // an error per 16x16 film tile
    if (!d_err.alloc("device film", (size_t)((j.p.width + 15) / 16) * ((j.p.height + 15) / 16) * 4, false)) return false;
    std::vector<uint32_t> active((size_t)ntx * nty), kept(active.size());
    for (size_t i = 0; i < active.size(); ++i) active[i] = (uint32_t)i;
    unsigned long long tile_samples = 0; unsigned rounds = 0;
    for (uint32_t done = 0; done < rp.spp && !active.empty(); ++rounds) {
        uint32_t n_b = 0;
        for (float *half : {j.d_film.p, j.d_half_b.p}) {
            const uint32_t n = (uint32_t)std::min<long long>(o.astep, rp.spp - done);
            if (half == j.d_half_b.p) n_b = n;
            if (n == 0) continue;
            if (!pt_ok(pt_render_tiles(sc, &rp, done, n, active.data(), (uint32_t)active.size(), half, 1))) return false;
            PtCounters c; pt_get_counters(sc, &c); j.camera_rays += c.camera_rays;
            done += n; tile_samples += (unsigned long long)n * active.size();
        }
        if (n_b > 0 && done >= (uint32_t)o.amin) {
            uint32_t n_kept = 0;
            if (!pt_ok(pt_film_halves_error(sc, j.d_film.p, j.d_half_b.p, (uint32_t)j.p.width, (uint32_t)j.p.height, d_err.p, nullptr, nullptr)) ||
                !pt_ok(pt_tiles_select(sc, &rp, d_err.p, o.threshold, active.data(), (uint32_t)active.size(), kept.data(), &n_kept))) return false;
            active.assign(kept.begin(), kept.begin() + n_kept);
        }
    }
    if (!sum_halves(j.film, j.d_film.p, j.d_half_b.p)) return false;
    if (!o.quiet) std::printf("adaptive: %llu of %llu tile-samples, %u rounds\n", tile_samples, (unsigned long long)ntx * nty * rp.spp, rounds);
    return true;
}

// The render calls groups() lists, of --preview-every N samples each, else (--checkpoint) of one wavefront pass, else the whole run in one; after each its counters,
// the checkpoint and, unless it was the last, the preview.
static bool render_groups(Job &j, PtfCheckpointHeader &ck) {
    const Options &o = j.o; const Plan &p = j.p; pt_scene *sc = j.sc.p;
    uint32_t group = p.last - p.first;   // samples per pt_render_samples call
    if (o.preview > 0) group = (uint32_t)std::min<long long>(o.preview, group);
    else if (!o.checkpoint.empty() && !pt_ok(j.ao ? pt_ao_pass_size(sc, &p.rp, j.ao, &group) : pt_pass_size(sc, &p.rp, &group))) return false;
    for (const Group &g : groups(p, group, ck.samples_done)) {
        float *const into = g.half ? j.d_half_b.p : j.d_film.p;
        if (!pt_ok(j.ao ? pt_ao_render_samples(sc, &p.rp, j.ao, g.first, g.n, into, 1) : pt_render_samples(sc, &p.rp, g.first, g.n, into, 1))) return false;
        PtCounters c; pt_get_counters(sc, &c); j.camera_rays += c.camera_rays;
        ck.samples_done = g.first + g.n - p.first;
        if (!o.checkpoint.empty() && !(download(j.film, j.d_film.p, "reading the film back failed") && ptf_ok(ptf_checkpoint_write(o.checkpoint.c_str(), &ck, j.film.data())))) return false;
        if (o.preview > 0 && g.first + g.n < p.last && !write_out(j)) return false;
    }
    return true;
}

// the feature sums of sample numbers [first, last), whatever groups (or earlier runs, --checkpoint) rendered the image's: for --denoise and --aov
static bool render_features(Job &j, DeviceBuffer &d_sums) {
    if (!d_sums.alloc("feature buffers", j.npix * 40, true)) return false;
    const PtAOVBuffers d_planes = feature_planes(d_sums.p, j.npix);
    return pt_ok(pt_aov_render_samples(j.sc.p, &j.p.rp, j.p.first, j.p.last - j.p.first, &d_planes, 1));
}

// the filter reads the halves; then A += B: the outfile's film
static bool write_denoised(Job &j, float *d_sums) {
    const PtAOVBuffers d_planes = feature_planes(d_sums, j.npix);
    PtDenoiseParams dp; pt_denoise_default_params(&dp);
    if (j.o.dn_iterations >= 0) dp.iterations = (uint32_t)j.o.dn_iterations;
    dp.scale = j.p.rp.scale;
    return pt_ok(pt_denoise(j.sc.p, &dp, j.d_film.p, j.d_half_b.p, &d_planes, (uint32_t)j.p.width, (uint32_t)j.p.height, j.d_rgb.p, 1)) &&
           write_rgb(j, j.o.denoise, "reading the denoised image back failed") && sum_halves(j.film, j.d_film.p, j.d_half_b.p);
}

static bool write_aov(Job &j, const float *d_sums) {
    const size_t npix = j.npix;
    std::vector<float> sums(npix * 10, 0.0f), res(npix * 7);
    if (!download(sums, d_sums, "reading the feature buffers back failed")) return false;
    const PtAOVBuffers planes = feature_planes(sums.data(), npix);
    float *albedo = res.data(), *normal = res.data() + npix * 3, *depth = res.data() + npix * 6;
    if (!pt_ok(pt_aov_resolve(&planes, (uint32_t)npix, albedo, normal, depth))) return false;
    const char *names[7] = {"N.X", "N.Y", "N.Z", "Z", "albedo.B", "albedo.G", "albedo.R"};   // (byte-wise sorted, as the format stores them)
    const float *data[7] = {normal, normal + 1, normal + 2, depth, albedo + 2, albedo + 1, albedo};
    const uint32_t strides[7] = {3, 3, 3, 1, 3, 3, 3};
    return ptf_ok(ptf_write_exr_channels(j.o.aov.c_str(), j.p.width, j.p.height, 7, names, data, strides));
}

int main(int argc, char **argv) {
    Options o; Plan plan; std::string why;
    if (parse_options(argc, argv, o, why)) return usage(why);
    Parsed fs;
    if (!ptf_ok(ptf_parse_file(o.scene.c_str(), &fs.p))) return 1;
    const bool is_ao = ptf_render_params(fs.p)->integrator == PT_INTEGRATOR_AO;
    if (const int st = make_plan(o, *ptf_render_params(fs.p), is_ao, plan, why)) return st == 2 ? usage(why) : die(why.c_str());
    if (o.outfile.empty()) o.outfile = ptf_output_filename(fs.p);
    PtAOParams ao{}; if (is_ao) ptf_ao_params(fs.p, &ao);
    const size_t npix = (size_t)plan.width * plan.height;
    Job j{o, plan, is_ao ? &ao : nullptr, npix, std::vector<float>(npix * 4, 0.0f), std::vector<float>(npix * 3)};
    PtfCheckpointHeader ck{PTF_CHECKPOINT_MAGIC, 1u, (uint32_t)plan.width, (uint32_t)plan.height, plan.rp.spp, plan.first, 0u, 0u, ptf_params_hash(&plan.rp, j.ao)};
    if (!o.checkpoint.empty() && !resume(j, ck)) return 1;

    if (!pt_ok(pt_init(o.device))) return 1;
    const auto t0 = std::chrono::steady_clock::now();
    if (!pt_ok(pt_scene_create(ptf_scene_desc(fs.p), &j.sc.p))) return 1;
    const auto t1 = std::chrono::steady_clock::now();
    if (!j.d_film.alloc("device film", npix * 16, false) || !j.d_rgb.alloc("device film", npix * 12, false) ||
        !(hipMemcpy(j.d_film.p, j.film.data(), npix * 16, hipMemcpyHostToDevice) == hipSuccess || hip_failed("device film"))) return 1;
    if ((plan.denoise || o.adaptive) && !j.d_half_b.alloc("device film", npix * 16, true)) return 1;
    if (!(o.adaptive ? render_adaptive(j) : render_groups(j, ck))) return 1;
    const auto t2 = std::chrono::steady_clock::now();

    DeviceBuffer d_sums;
    if ((plan.denoise || !o.aov.empty()) && !render_features(j, d_sums)) return 1;
    if (plan.denoise && !write_denoised(j, d_sums.p)) return 1;
    if (!write_out(j)) return 1;
    if (!o.aov.empty() && !write_aov(j, d_sums.p)) return 1;
    if (!o.quiet) {
        const double ts = std::chrono::duration<double>(t1 - t0).count(), tr = std::chrono::duration<double>(t2 - t1).count();
        std::printf("%s: %dx%d, %u spp, %llu camera rays, scene %.2f s, render %.3f s (%.1f Msamples/s) -> %s\n", o.scene.c_str(), plan.width, plan.height, plan.rp.spp,
                    j.camera_rays, ts, tr, (double)j.camera_rays / tr / 1e6, o.outfile.c_str());
    }
    return 0;
}
