// cli_plan.h -- the host-only part of mi355pbrt's command line (mi355pbrt.cpp holds the description of the flags): the flags and what they refuse, the sample numbers a run
// renders, and the render calls of its loop. Plain arithmetic over include/mi355front.h and the standard library, no HIP: tests/cli_plan/check_cli_plan.cpp checks it
// without a device. parse_options and make_plan return 0, or the exit status with its message in `why`: 2 is a usage error (`why` may be empty: the usage text alone).
#ifndef MI355_CLI_PLAN_H
#define MI355_CLI_PLAN_H
#include "../../include/mi355front.h"
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

struct Options {
    std::string scene, outfile, samples, checkpoint, aov, denoise;
    long long lo = 0, hi = 0;   // --samples lo:hi (both 0 without it)
    long long dn_iterations = -1, preview = 0, astep = 4, amin = 0;
    int device = 0, spp = 0;
    bool quiet = false, adaptive = false;
    float threshold = 0.0f;
};

// "A:B" with decimal A < B, both fitting 32 bits
inline bool parse_range(const std::string &a, long long &lo, long long &hi) {
    const size_t c = a.find(':');
    if (c == std::string::npos || c == 0 || c + 1 >= a.size() || a.size() > 21) return false;
    for (size_t i = 0; i < a.size(); ++i) if (i != c && (a[i] < '0' || a[i] > '9')) return false;
    lo = std::atoll(a.substr(0, c).c_str()); hi = std::atoll(a.substr(c + 1).c_str());
    return lo < hi && hi <= 0xffffffffll;
}

// The flags, and everything that is refused before the scene file is looked for.
inline int parse_options(int argc, char **argv, Options &o, std::string &why) {
    const auto refuse = [&why](const char *text) { why = text; return 2; };
    why.clear();
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const auto count = [&](long long &v, long long least) { v = std::atoll(argv[++i]); return v >= least && v <= 0xffffffffll; };
        if (a == "--outfile" && i + 1 < argc) o.outfile = argv[++i];
        else if (a == "--device" && i + 1 < argc) o.device = std::atoi(argv[++i]);
        else if (a == "--spp" && i + 1 < argc) o.spp = std::atoi(argv[++i]);
        else if (a == "--samples" && i + 1 < argc) o.samples = argv[++i];
        else if (a == "--checkpoint" && i + 1 < argc) o.checkpoint = argv[++i];
        else if (a == "--aov" && i + 1 < argc) o.aov = argv[++i];
        else if (a == "--denoise" && i + 1 < argc) o.denoise = argv[++i];
        else if (a == "--denoise-iterations" && i + 1 < argc) {
            char *end = nullptr; o.dn_iterations = std::strtoll(argv[++i], &end, 10);
            if (end == argv[i] || *end || o.dn_iterations < 0 || o.dn_iterations > 5) return refuse("--denoise-iterations takes a number of levels 0..5");
        }
        else if (a == "--preview-every" && i + 1 < argc) { if (!count(o.preview, 1)) return refuse("--preview-every takes a number of samples > 0"); }
        else if (a == "--adaptive" && i + 1 < argc) {
            char *end = nullptr; o.threshold = std::strtof(argv[++i], &end);
            if (end == argv[i] || *end || !(o.threshold >= 0.0f)) return refuse("--adaptive takes an error threshold >= 0");
            o.adaptive = true;
        }
        else if (a == "--adaptive-step" && i + 1 < argc) { if (!count(o.astep, 1)) return refuse("--adaptive-step takes a number of samples > 0"); }
        else if (a == "--adaptive-min" && i + 1 < argc) { if (!count(o.amin, 0)) return refuse("--adaptive-min takes a number of samples >= 0"); }
        else if (a == "--quiet") o.quiet = true;
        else if (a[0] != '-') o.scene = a;
        else return 2;
    }
    if (o.scene.empty()) return 2;
    if (o.adaptive && !o.samples.empty()) return refuse("--adaptive with --samples: an adaptive render chooses its own sample ranges, tile by tile");
    if (o.adaptive && !o.checkpoint.empty()) return refuse("--adaptive with --checkpoint: a checkpoint holds one sample count for the frame, an adaptive render one per tile");
    if (o.adaptive && !o.aov.empty()) return refuse("--adaptive with --aov: the feature buffers have no tile-list render");
    if (o.adaptive && !o.denoise.empty()) return refuse("--adaptive with --denoise: the filter takes one sample count for the frame, an adaptive render's tiles hold different ones");
    if (!o.checkpoint.empty() && !o.denoise.empty()) return refuse("--checkpoint with --denoise: a checkpoint holds one film, a denoising run renders two halves");
    if (o.preview > 0 && !o.denoise.empty()) return refuse("--preview-every with --denoise: a preview shows the film so far, which a denoising run keeps as two halves");
    if (o.dn_iterations >= 0 && o.denoise.empty()) return refuse("--denoise-iterations without --denoise");
    if (!o.samples.empty() && !parse_range(o.samples, o.lo, o.hi)) { why = "--samples takes A:B with 0 <= A < B, got \"" + o.samples + "\""; return 2; }
    return 0;
}

// What is known once the scene is parsed: the job's parameters with --spp applied, the sample numbers [first, last) this run renders, the film's size.
struct Plan {
    PtRenderParams rp;
    uint32_t first, last, mid;   // --denoise: half A is [first, mid), half B [mid, last)
    bool denoise;
    int width, height;
};

inline int make_plan(const Options &o, const PtRenderParams &parsed, bool is_ao, Plan &p, std::string &why) {
    p.rp = parsed;
    if (o.spp > 0) p.rp.spp = (uint32_t)o.spp;
    const long long hi = o.samples.empty() ? (long long)p.rp.spp : o.hi;
    if (hi > (long long)p.rp.spp) { why = "--samples " + o.samples + " goes beyond the job's " + std::to_string(p.rp.spp) + " samples per pixel"; return 2; }
    p.first = (uint32_t)o.lo; p.last = (uint32_t)hi;
    p.denoise = !o.denoise.empty();
    if (p.denoise && p.last - p.first < 2) { why = "--denoise needs two samples per pixel at least: it renders them as two halves"; return 2; }
    p.mid = p.first + (p.last - p.first) / 2;
    if (o.adaptive && is_ao) { why = "--adaptive with Integrator \"ambientocclusion\": the ambient-occlusion integrator has no tile-list render"; return 2; }
    p.width = p.rp.cropped_pixel_bounds[2] - p.rp.cropped_pixel_bounds[0]; p.height = p.rp.cropped_pixel_bounds[3] - p.rp.cropped_pixel_bounds[1];
    if (p.width <= 0 || p.height <= 0) { why = "empty film"; return 1; }
    return 0;
}

// The render calls of the loop that is not adaptive: sample numbers [first, first + n) into the film (half 0) or, under --denoise from `mid` on, into half B (half 1).
// They cover [p.first + samples_done, p.last) in steps of at most group_size (>= 1) samples, none of which crosses `mid` under --denoise.
struct Group { uint32_t first, n; int half; };

inline std::vector<Group> groups(const Plan &p, uint32_t group_size, uint32_t samples_done) {
    std::vector<Group> g;
    for (uint32_t s = p.first + samples_done; s < p.last; s += g.back().n) {
        const int half = p.denoise && s >= p.mid;
        g.push_back({s, std::min(group_size, (p.denoise && !half ? p.mid : p.last) - s), half});
    }
    return g;
}
#endif
